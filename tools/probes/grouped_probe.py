#!/usr/bin/env python3
"""The grouped weight-gradient call of a training step, alone: capture its member list from one eager step of a workload, then time
the same call (same operands) through one or more builds of the library, HIP events around 6 calls after 2 warm-ups.

    python tools/probes/grouped_probe.py [workload [batch]] [name=path/to/liblvsr_hip.so ...]

Without libraries it times the built one.  Per build: all members in one call with the encoder's fork products (N = 6H) added as members,
the step's own members alone, and the fork products as direct lvsr_sgemm calls.  Printed: the member list with the cut of the built
library (lvsr_sgemm_tn_grouped_plan) and one line per build.  profiles/r09_grouped_probe.txt is its output for builds of csrc/gemm.hip
that differed in the cut and in the block -> unit map."""
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (REPO, os.path.join(REPO, "attention-lvcsr_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch                                                     # noqa: E402
from lvsr_amd import native, spec, synthetic                     # noqa: E402
from lvsr_amd.bricks.recognizer import SpeechRecognizer          # noqa: E402

FIELDS = ("A", "B", "C", "M", "N", "K", "lda", "ldb", "ldc", "beta")


class RawLib(object):
    """Another build of the library, by the prototypes of the built one's header (it may lack newer entry points)."""
    def __init__(self, path, functions):
        self.dll, self.functions = ctypes.CDLL(path), functions

    def call(self, name, *args):
        fn = getattr(self.dll, name)
        fn.restype, fn.argtypes = self.functions[name][0], self.functions[name][1]
        if fn(*args) != 0:
            raise native.NativeError("%s failed" % name)


def main(argv):
    words = [a for a in argv if "=" not in a]
    builds = [tuple(a.split("=", 1)) for a in argv if "=" in a]
    workload = words[0] if words else "wsj_base"
    factory, B, T, L = spec.WORKLOADS[workload]
    B = int(words[1]) if len(words) > 1 else B
    cfg = factory()
    dev = torch.device("cuda", 0)
    lib = native.get()
    rec = SpeechRecognizer(device=dev, params=synthetic.make_params(cfg, seed=10), lib=lib, net_config=cfg, use_graph=False)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in synthetic.make_batch(cfg, B, T, L, seed=1234).items()}
    calls, fork_calls, call = [], [], lib.call

    def recording(name, *args):
        if name == "lvsr_sgemm_tn_grouped":
            calls.append([{f: getattr(args[1][i], f) for f in FIELDS} for i in range(args[2])])
        elif name == "lvsr_sgemm" and args[1] == 1 and args[2] == 0 and args[4] % 6 == 0 and args[4] >= 1024 and args[5] >= 3000:      # X^T dxg -> (I, 6H)
            fork_calls.append(dict(A=args[7].value, lda=args[8], B=args[9].value, ldb=args[10], beta=args[11], C=args[12].value, ldc=args[13],
                                   M=args[3], N=args[4], K=args[5]))
        return call(name, *args)
    lib.call = recording
    rec.cost_and_gradients(batch, region=False)
    torch.cuda.synchronize()
    del lib.call
    rest = max(calls, key=len)
    forks = fork_calls
    members = rest + forks
    print("grouped calls of the step: %s members; fork products launched directly: %d" % ([len(c) for c in calls], len(forks)))
    cls = lib.structs["lvsr_gemm_desc"]

    def descs(ms):
        arr = (cls * len(ms))()
        for d, m in zip(arr, ms):
            for f in FIELDS:
                setattr(d, f, m[f])
        return arr
    ws = torch.empty(1 << 26, device=dev)
    ws2 = torch.empty(1 << 22, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ks, kc = (ctypes.c_int * len(members))(), (ctypes.c_int * len(members))()
    lib.call("lvsr_sgemm_tn_grouped_plan", descs(members), len(members), ws.numel() * 4, ks, kc)
    print("members (M, N, K, lda, ldb, aligned, fork) -> ksplit, kchunk of the built library")
    for m, s, c in zip(members, ks, kc):
        al = m["lda"] % 4 == 0 and m["ldb"] % 4 == 0 and m["A"] % 16 == 0 and m["B"] % 16 == 0
        print("  ", (m["M"], m["N"], m["K"], m["lda"], m["ldb"], int(al), int(m in forks)), "->", s, c)

    def timed(fn, reps=6):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3

    def group_us(v, ms):
        arr = descs(ms)
        return timed(lambda: v.call("lvsr_sgemm_tn_grouped", stream, arr, len(ms), ctypes.c_void_p(ws.data_ptr()), ws.numel() * 4))

    def forks_us(v):
        def fn():
            for m in forks:
                v.call("lvsr_sgemm", stream, 1, 0, m["M"], m["N"], m["K"], 1.0, ctypes.c_void_p(m["A"]), m["lda"], ctypes.c_void_p(m["B"]),
                       m["ldb"], 0.0, ctypes.c_void_p(m["C"]), m["ldc"], None, ctypes.c_void_p(ws2.data_ptr()), ws2.numel() * 4)
        return timed(fn) if forks else 0.0
    for name, path in [("built", None)] + builds:
        v = lib if path is None else RawLib(path, lib.functions)
        a, r, f = group_us(v, members), group_us(v, rest), forks_us(v)
        print("%-20s all-in-group %7.1f us | group without forks %7.1f + forks direct %6.1f = %7.1f" % (name, a, r, f, r + f), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
