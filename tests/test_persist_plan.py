"""The host-side plan of the persistent attention decoder (csrc/decoder_persist.h: cluster shape, passes, LDS budget, workspace layout)
through its six query entry points, against a table recorded before the plan was gathered in one place: every accept / refuse
decision, every workspace size and every cluster size must stay what it was.  CPU only (the emulator build runs the same host code).

    python tests/test_persist_plan.py --write       records tests/test_persist_plan.json from the library as built
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "test_persist_plan.json")
QUERIES = ["lvsr_attdec_persist_ws_bytes", "lvsr_attdec_stack2_persist_ws_bytes",
           "lvsr_attdec_bwd_persist_ws_bytes", "lvsr_attdec_bwd_persist_clusters",
           "lvsr_attdec_stack2_bwd_persist_ws_bytes", "lvsr_attdec_stack2_bwd_persist_clusters"]
FIELDS = ["Tp", "B", "D", "M", "K", "c", "prior_type", "phases", "group_rows"]
BASE = dict(Tp=100, B=16, D=256, M=256, K=10, c=100, prior_type=0, phases=3, group_rows=0)


def blocks():
    """[(class, argument block)]: the outcome classes of pd_pick / pd_pick_passes / pd_geom / pb_geom (WSJ-base dims unless named)."""
    out = [("base", {})]
    # LDS budget: where clusters of 16 stop fitting (clusters of 8 are tried then) and where clusters of 8 stop (the two-layer queries
    # show that edge at any knob), for three matcher widths
    out += [("lds", dict(Tp=t, M=m)) for m in (256, 384, 512)
            for t in (216, 224, 232, 248, 264, 280, 296, 312, 328, 344, 360, 376, 392, 408, 424, 440, 448, 456, 480, 512)]
    out += [("Tp", dict(Tp=t)) for t in (1, 13, 513)]
    # passes: 16 / 32 / 64 / 128 utterances are 1 / 2 / 4 / 8 launches of clusters of 16 (1 / 1 / 2 / 4 of clusters of 8)
    out += [("passes", dict(B=b)) for b in (1, 8, 17, 32, 33, 64, 128, 256, 264)]
    out += [("prior", dict(B=b, prior_type=p, K=k)) for b, p, k in ((64, 1, 10), (64, 2, 10), (64, 2, 0), (16, 1, 10), (16, 2, 10))]
    out += [("K", dict(K=k)) for k in (0, 3, 4, 5, 12, 16, 17)]
    out += [("c", dict(c=c, K=k)) for c, k in ((1, 10), (127, 10), (128, 10), (128, 0))]
    out += [("M", dict(M=512)), ("M", dict(M=513)), ("M", dict(M=300, D=128)), ("M", dict(M=256, D=128))]
    out += [("D", dict(D=d)) for d in (250, 257, 264, 300, 512, 513)] + [("D", dict(D=512, B=8))]
    # small decoders (the emulator tests' shapes); (3 D) % 4 != 0 is refused by the two-layer backward only
    out += [("smallD", dict(D=d, M=m, Tp=13, B=4)) for d, m in ((8, 12), (10, 12), (36, 40), (36, 100), (5, 7))]
    # own positions of the backward: at most 32 per work-group (16 in clusters for D > 256)
    out += [("nown", dict(D=d, Tp=t)) for d, t in ((128, 256), (128, 300), (512, 512), (264, 280))]
    out += [("nown", dict(D=64, M=64, Tp=t)) for t in (64, 100, 128, 140)]
    out += [("phases", dict(phases=p)) for p in (0, 1, 2, 7)] + [("group_rows", dict(group_rows=4))]
    out += [("stack", dict(B=17)), ("stack", dict(B=16, D=250))]
    return [(cls, dict(BASE, **kw)) for cls, kw in out]


def query(lib, block):
    args = lib.make("lvsr_attdec_args", L=5, E=64, **block)
    return [int(getattr(lib, "_" + q)(ctypes.byref(args))) for q in QUERIES]


def table(lib):
    rows = []
    lib.set_knob("max_cluster_wgs", 256)
    try:
        for dec_cluster in (0, 8, 16):
            lib.set_knob("dec_cluster", dec_cluster)
            for cls, block in blocks():
                rows.append([cls, dec_cluster] + [block[f] for f in FIELDS] + query(lib, block))
    finally:
        lib.set_knob("dec_cluster", 0)
        lib.set_knob("max_cluster_wgs", 0)
    return rows


def test_plan_equals_the_recorded_table():
    from emu import emu_lib
    with open(TABLE) as f:
        recorded = json.load(f)
    assert recorded["columns"] == ["class", "dec_cluster"] + FIELDS + QUERIES
    got = table(emu_lib())
    assert len(got) == len(recorded["rows"]) <= 400
    for g, r in zip(got, recorded["rows"]):
        assert g == r, dict(zip(recorded["columns"], zip(r, g)))


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "attention-lvcsr_amd")):
        sys.path.insert(0, p)
    from emu import emu_lib
    rows = table(emu_lib())
    with open(TABLE, "w") as f:
        f.write('{"columns": %s,\n "rows": [\n%s\n]}\n' % (json.dumps(["class", "dec_cluster"] + FIELDS + QUERIES),
                                                          ",\n".join(json.dumps(r) for r in rows)))
    n = len(["class", "dec_cluster"] + FIELDS)
    for cls in sorted({r[0] for r in rows}):          # per class and query: accepted / refused rows
        mine = [r for r in rows if r[0] == cls]
        print("%-10s %3d rows; accepted per query: %s" % (cls, len(mine), [sum(1 for r in mine if r[n + q] != 0) for q in range(len(QUERIES))]))
    print("%d rows, %d bytes" % (len(rows), os.path.getsize(TABLE)))
