#!/usr/bin/env python3
"""Overhead of adaptive weight noise (lvsr_amd/weight_noise.py) per training step, in one process on one GPU: interleaved
same-box pairs of the plain step and the noisy step (each its own recognizer and trainer, graphs captured during warm-up), on
WSJ-base (bench.py's training configuration and global batch) and on the TIMIT shapes at batch 1.  Writes a markdown record.

    python tools/probe_adaptive_noise.py [--pairs 8] [--steps 10] [--out profiles/r07_adaptive_noise.md]
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "attention-lvcsr_amd")]

import numpy  # noqa: E402
import torch  # noqa: E402

from bench import TRAIN_CONF  # noqa: E402
from lvsr_amd import spec, synthetic  # noqa: E402
from lvsr_amd.bricks.recognizer import SpeechRecognizer  # noqa: E402
from lvsr_amd.training import Trainer  # noqa: E402

NOISE = dict(model_cost_coefficient=0.1, init_sigma=1e-12)      # exp/timit/configs/nips_baseline.yaml, stages main / annealing


def leg(workload, B, pairs, steps, warmup):
    factory, B0, T, L = spec.WORKLOADS[workload]
    cfg = factory()
    B = B or B0                                                  # bench.py's per-GPU batch (weak scaling)
    dev = torch.device("cuda:0")
    params = synthetic.make_params(cfg, seed=10)
    batches = [{k: torch.from_numpy(v).to(dev) for k, v in synthetic.make_batch(cfg, B, T, L, seed=1234 + s).items()}
               for s in range(2)]
    runs = {}
    for name, kw in (("plain", {}), ("noisy", dict(adaptive_noise=NOISE, num_examples=3696))):
        rec = SpeechRecognizer(device=dev, params=params, net_config=cfg)
        runs[name] = Trainer(rec, distributed=False, **dict(TRAIN_CONF, **kw))
    for tr in runs.values():
        for s in range(warmup):
            tr.train_step(batches[s % 2])
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for p in range(pairs):
        order = ("plain", "noisy") if p % 2 == 0 else ("noisy", "plain")
        for name in order:
            tr = runs[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(steps):
                tr.train_step(batches[s % 2])
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
    stats = runs["noisy"].noise_stats()
    n = runs["plain"].rec.store.num_parameters()
    for tr in runs.values():
        tr.close()
    return dict(workload=workload, B=B, T=T, L=L, parameters=n, plain=times["plain"], noisy=times["noisy"], stats=stats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r07_adaptive_noise.md"))
    args = ap.parse_args()
    rows = [leg("wsj_base", None, args.pairs, args.steps, args.warmup), leg("timit_tiny", 1, args.pairs, args.steps, args.warmup)]
    lines = ["# Adaptive weight noise: step time with and without (tools/probe_adaptive_noise.py)", "",
             "Interleaved same-box pairs (%d pairs x %d steps after %d warm-up steps per trainer), one process, one MI355X; "
             "bench.py's step rules (momentum + AdaDelta, max_norm 1.0); noise settings of nips_baseline.yaml (c = 0.1, "
             "init_sigma = 1e-12).  Median of the pairs." % (args.pairs, args.steps, args.warmup), "",
             "| workload | batch | parameters | plain ms/step | noisy ms/step | noisy / plain | target |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        p, q = float(numpy.median(r["plain"])), float(numpy.median(r["noisy"]))
        ratio = float(numpy.median(numpy.array(r["noisy"]) / numpy.array(r["plain"])))
        target = "<= 1.03: %s" % ("met" if ratio <= 1.03 else "MISSED") if r["workload"] == "wsj_base" else "-"
        lines.append("| %s | %d | %d | %.3f | %.3f | %.4f | %s |" % (r["workload"], r["B"], r["parameters"], p, q, ratio, target))
    lines += ["", "Per-pair ms/step (plain, noisy):", ""]
    for r in rows:
        lines.append("- %s: %s" % (r["workload"], ", ".join("(%.3f, %.3f)" % pq for pq in zip(r["plain"], r["noisy"]))))
        lines.append("  last noisy step: %s" % ", ".join("%s %.6g" % kv for kv in sorted(r["stats"].items())))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
