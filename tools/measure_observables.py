#!/usr/bin/env python3
"""Cost of the training observables (lvsr_amd/observables.py) per training step, in one process on one GPU: interleaved pairs of
the step with observables off, on, and on without the per-parameter statistics (each its own recognizer and trainer, graphs
captured during warm-up), timed with HIP events, on WSJ-base with bench.py's training configuration.  Writes a markdown record.

    python tools/measure_observables.py [--pairs 8] [--steps 10] [--out profiles/r08_observables.md]

Under `rocprofv3 --kernel-trace --stats -- python tools/measure_observables.py --pairs 1 --steps 8` the obs_* rows of the kernel
statistics are the kernel times of the three entry points (tools/rocpd_stats.py).
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "attention-lvcsr_amd")]

import numpy  # noqa: E402
import torch  # noqa: E402

from bench import TRAIN_CONF  # noqa: E402
from lvsr_amd import spec, synthetic  # noqa: E402
from lvsr_amd.bricks.recognizer import SpeechRecognizer  # noqa: E402
from lvsr_amd.training import Trainer  # noqa: E402

LEGS = (("off", None), ("on", True), ("on, parameter_stats off", dict(parameter_stats=False)))


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs an MI355X"
    dev = torch.device("cuda:0")
    factory, B, T, L = spec.WORKLOADS["wsj_base"]
    cfg = factory()
    params = synthetic.make_params(cfg, seed=10)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in synthetic.make_batch(cfg, B, T, L, seed=1234).items()}
    runs = {}
    for name, obs in LEGS:
        rec = SpeechRecognizer(device=dev, params=params, net_config=cfg)
        runs[name] = Trainer(rec, distributed=False, observables=obs, **TRAIN_CONF)
    for tr in runs.values():
        for _ in range(args.warmup):
            tr.train_step(batch)
    times = {k: [] for k in runs}
    names = [n for n, _ in LEGS]
    for p in range(args.pairs):
        for name in names[p % 3:] + names[:p % 3]:                 # every leg takes every place in the order
            tr = runs[name]
            times[name].append(timed(lambda: tr.train_step(batch), args.steps))
    replayed = {}
    for name, tr in runs.items():
        regions = list(tr.rec._regions.values())
        replayed[name] = any(s["seen"] >= 3 for s in regions) and not any(s.get("bad") for s in regions) and not tr.step_was_skipped()
    obs = runs["on"].observables()
    n = runs["off"].rec.store.num_parameters()
    Tp = obs["max_attended_length"]
    lines = ["# Training observables: step time with and without (tools/measure_observables.py)", "",
             "WSJ-base (B = %d, T = %d, L = %d, T' = %d, %d parameters in %d tensors), bench.py's step rules; interleaved same-process "
             "runs (%d rounds x %d steps per leg after %d warm-up steps), HIP events, one MI355X.  Median of the rounds."
             % (B, T, L, Tp, n, len(runs["off"].rec.store.offsets), args.pairs, args.steps, args.warmup), "",
             "| observables | ms/step (median) | min | max | vs off | graph replayed |", "|---|---|---|---|---|---|"]
    base = float(numpy.median(times["off"]))
    for name in names:
        t = times[name]
        lines.append("| %s | %.3f | %.3f | %.3f | %+.3f ms (%+.2f %%) | %s |" % (name, numpy.median(t), min(t), max(t), numpy.median(t) - base,
                                                                           100 * (numpy.median(t) / base - 1), replayed[name]))
    lines += ["", "Per-round ms/step (%s):" % ", ".join(names), "",
              ", ".join("(%s)" % ", ".join("%.3f" % times[k][p] for k in names) for p in range(args.pairs)), "",
              "Last step with observables on: " + ", ".join("%s %.6g" % (k, v) for k, v in sorted(obs.items()) if not k.endswith("_stats")), ""]
    for tr in runs.values():
        tr.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
