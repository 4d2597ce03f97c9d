"""What time stamps cost next to the search, at the WSJ decode shape of tools/measure_recognize.py (256 utterances of 4-8 s, beam 16,
device FST language model, chunks of 64, one chunk in flight):

  * decode.recognize(timestamps=False) and (timestamps=True), wall clock, alternating, medians with the run-to-run spread;
  * the feature's parts per chunk: SpeechRecognizer.align_staged on the search's own contexts (`reuse_contexts`: the teacher-forced
    pass, lvsr_alignment_times, the copy) and with an encoder pass of its own — the difference is what sharing the contexts saves;
  * lvsr_alignment_times alone (device events over 50 launches) at (L, B, T') = (120, 64, 200), with its algorithmic bytes;
  * the only route there was before: analyze_batch(..., want_alignments=True), which copies the (L,B,T') weights and energies to the
    host, plus the same reduction in NumPy.

    python tools/measure_timestamps.py [--utts 256] [--reps 5] [--out profiles/timestamps_wsj.md] [--before plain.json]
    python tools/measure_timestamps.py --plain-only          # timestamps=False alone, one JSON line (runs on the parent commit too)

`--before`: the JSON line `--plain-only` printed on the parent commit, for the first row of the table.  Needs an MI355X."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "attention-lvcsr_amd"), os.path.join(REPO, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy
import torch

from measure_recognize import SEARCH, build, clock, event_time, waveforms


def numpy_times(W, cost, lo, hi):
    """the reduction of lvsr_alignment_times on the host: W (L,n) float32 -> (L,8) float64"""
    L, n = W.shape
    w = W.astype(numpy.float64)
    t = numpy.arange(n, dtype=numpy.float64)
    C = numpy.cumsum(W, axis=1, dtype=numpy.float32)
    out = numpy.zeros((L, 8))
    out[:, 0] = W.argmax(axis=1)
    out[:, 1] = W.max(axis=1)
    out[:, 2] = (w * t).sum(axis=1)
    out[:, 3] = numpy.sqrt(numpy.maximum((w * t * t).sum(axis=1) - out[:, 2] ** 2, 0.0))
    out[:, 4] = (C >= numpy.float32(lo) * C[:, -1:]).argmax(axis=1)
    out[:, 5] = (C >= numpy.float32(hi) * C[:, -1:]).argmax(axis=1)
    out[:, 6] = C[:, -1]
    out[:, 7] = cost
    return out


def kernel_alone(rec, L=120, B=64, Tp=200):
    """-> (microseconds per launch, algorithmic bytes) on softmax rows under a ragged label mask and ragged attended lengths"""
    from lvsr_amd.observables import alignment_times
    dev = rec.device
    g = torch.Generator(device="cpu").manual_seed(3)
    lengths = torch.randint(Tp // 2, Tp + 1, (B,), generator=g, dtype=torch.int32)
    labels = torch.randint(L // 2, L + 1, (B,), generator=g)
    W = torch.softmax(4.0 * torch.randn(L, B, Tp, generator=g), dim=2)
    mask = (torch.arange(L)[:, None] < labels[None, :]).float()
    costs = torch.rand(L, B, generator=g)
    W, mask, costs, lengths = W.to(dev), mask.to(dev), costs.to(dev), lengths.to(dev)
    out = torch.empty(L, B, 8, dtype=torch.float64, device=dev)
    us = event_time(lambda: alignment_times(rec.lib, W, mask, costs, out, lengths=lengths), reps=50)
    live = (mask.cpu() * lengths.cpu()[None, :].float()).sum().item()                 # weights the contract has the kernel read
    nbytes = 4 * live + L * B * (4 + 4 + 64) + 4 * B
    return us, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--beam", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--before", default=None)
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measure_timestamps.py needs an MI355X"
    from lvsr_amd import decode
    from lvsr_amd.frontend import FrontEnd
    dev = torch.device("cuda:0")
    wavs = waveforms(a.utts)
    fe = FrontEnd(device=dev).fit([wavs[i: i + a.batch] for i in range(0, min(len(wavs), 2 * a.batch), a.batch)])
    rec = build(dev, a.beam)
    kw = dict(beam_size=a.beam, batch=a.batch, sort=True, **SEARCH)
    per_utt = lambda ts: [t * 1e3 / a.utts for t in ts]
    if a.plain_only:
        for _ in range(2):
            rows = decode.recognize(rec, fe, wavs, **kw)
        wall = [clock(lambda: decode.recognize(rec, fe, wavs, **kw))[0] for _ in range(a.reps)]
        print(json.dumps(dict(plain_ms_per_utt=per_utt(wall), found=sum(1 for r in rows if r["recognized"]),
                              labels=sum(len(r["recognized"]) for r in rows))))
        return
    for _ in range(2):                                     # warm-up: workspaces and graphs of every chunk shape, both ways
        plain = decode.recognize(rec, fe, wavs, **kw)
        timed = decode.recognize(rec, fe, wavs, timestamps=True, **kw)
    assert all(p["recognized"] == t["recognized"] and (p["search_cost"] == t["search_cost"] or not p["recognized"]) for p, t in zip(plain, timed))
    found = sum(1 for r in plain if r["recognized"])
    nlabels = sum(len(r["recognized"]) for r in plain)
    wall = {False: [], True: []}
    for _ in range(a.reps):                                # alternating, so that a drift of the machine hits both
        for ts in (False, True):
            wall[ts].append(clock(lambda: decode.recognize(rec, fe, wavs, timestamps=ts, **kw))[0])
    # the parts, chunk by chunk, on the hypotheses of the searches
    plan = decode.recognize_plan([len(w) for w in wavs], a.batch, True)
    parts = dict(reuse=[], own=[], old=[])
    same = 0
    for _ in range(a.reps):
        t_reuse = t_own = t_old = 0.0
        for chunk in plan:
            x, mask, lengths = fe.batch([wavs[i] for i in chunk])
            best = [plain[i]["recognized"] for i in chunk]
            with rec._on_stream():
                rec.compute_contexts_staged(x, mask)
            t, new = clock(lambda: rec.align_staged(x, mask, lengths, best, reuse_contexts=True))
            t_reuse += t
            t_own += clock(lambda: rec.align_staged(x, mask, lengths, best))[0]
            # the route there was: features on the host, analyze_batch with the alignments copied out, NumPy
            host = x.cpu().numpy()
            cols = [j for j, b in enumerate(best) if b]
            recs, labs = [host[: lengths[j], j] for j in cols], [best[j] for j in cols]

            def old_route():
                out = rec.analyze_batch(recs, labs, want_alignments=True)
                return [numpy_times(o["groundtruth"]["weights"], 0.0, 0.1, 0.9) for o in out]
            t, old = clock(old_route)
            t_old += t
            same = sum(int((o[:, [0, 1]] == new[j][:, [0, 1]]).all()) for o, j in zip(old, cols))
        parts["reuse"].append(t_reuse)
        parts["own"].append(t_own)
        parts["old"].append(t_old)
    us, nbytes = kernel_alone(rec)
    med = lambda v: statistics.median(per_utt(v))
    rng = lambda v: "%.3f .. %.3f" % (min(per_utt(v)), max(per_utt(v)))
    lines = ["# Recognising with time stamps at the WSJ decode shape", "",
             "`python tools/measure_timestamps.py --utts %d --batch %d --beam %d --reps %d` on one MI355X: the utterances, network, language "
             "model and chunks of tools/measure_recognize.py (4-8 s of PCM each, 123 features, WSJ-base with the conditioned decode "
             "weights, device FST language model, one chunk of %d in flight).  %d of %d utterances find a hypothesis, %d labels in all "
             "(%.1f per hypothesis); hypotheses and costs are the same with and without time stamps."
             % (a.utts, a.batch, a.beam, a.reps, a.batch, found, a.utts, nlabels, nlabels / float(max(found, 1))), "",
             "| run | ms per utterance (median of %d) | min .. max |" % a.reps, "|---|---|---|"]
    if a.before:
        before = json.loads(open(a.before).read().strip().splitlines()[-1])["plain_ms_per_utt"]
        lines.append("| recognize(timestamps=False), parent commit (a process of its own, same call) | %.3f | %.3f .. %.3f |"
                     % (statistics.median(before), min(before), max(before)))
    lines += ["| recognize(timestamps=False) | %.3f | %s |" % (med(wall[False]), rng(wall[False])),
              "| recognize(timestamps=True) | %.3f | %s |" % (med(wall[True]), rng(wall[True])),
              "| align_staged on the search's contexts: teacher-forced pass, lvsr_alignment_times, copy | %.3f | %s |" % (med(parts["reuse"]), rng(parts["reuse"])),
              "| align_staged with an encoder pass of its own | %.3f | %s |" % (med(parts["own"]), rng(parts["own"])),
              "| before: analyze_batch(want_alignments=True) from host features + the reduction in NumPy | %.3f | %s |" % (med(parts["old"]), rng(parts["old"])),
              "",
              "Time stamps cost %+.3f ms per utterance (difference of the two medians; the larger spread of the two runs is %.3f).  The "
              "encoder pass that sharing the search's contexts saves is %.3f ms per utterance.  The peaks of the old route's NumPy "
              "reduction equal the kernel's for %d of %d utterances of the last chunk."
              % (med(wall[True]) - med(wall[False]), max(max(per_utt(wall[k])) - min(per_utt(wall[k])) for k in wall),
                 med(parts["own"]) - med(parts["reuse"]), same, len(cols)), "",
              "| kernel | shape | us per launch (device events, 50 launches) | algorithmic bytes | GB/s |", "|---|---|---|---|---|",
              "| lvsr_alignment_times | (L, B, T') = (120, 64, 200), ragged labels and attended lengths | %.1f | %.1f MB | %.0f |"
              % (us, nbytes / 1e6, nbytes / us / 1e3)]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
