"""GPU measurement: cost of the task-loss-estimation criteria at the WSJ-base shape (HIP events).

    python tools/measure_mse_criterion.py [--out FILE.md] [--steps 20] [--warmup 5]

Times lvsr_reward_gain and lvsr_reward_mse alone (mean of 100 back-to-back launches) and whole training steps (Trainer.train_step:
forward, backward and the optimiser as one replayed graph) of the same network under log_likelihood, mse_gain imitative, mse_gain
greedy and mse_reward greedy.  The greedy step contains a second decoder pass: the free-running generation of L + 10 labels."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "attention-lvcsr_amd"))
import numpy
import torch
from lvsr_amd import spec, synthetic
from lvsr_amd.native import ptr
from lvsr_amd.bricks.recognizer import SpeechRecognizer
from lvsr_amd.training import Trainer
import bench


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
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs an MI355X"
    dev = torch.device("cuda:0")
    factory, B, T, L = spec.WORKLOADS["wsj_base"]
    base = factory()
    V, eos = base["num_phonemes"], base["num_phonemes"] - 1
    batch_np = synthetic.make_batch(base, B, T, L, seed=1234)
    lines = ["# mse_gain / mse_reward at the WSJ-base shape (B = %d, T = %d, L = %d, V = %d), HIP events" % (B, T, L, V), ""]

    # ---- the two kernels alone: groundtruth = the batch's labels, prediction = a perturbed copy 10 longer
    rng = numpy.random.RandomState(1)
    pred = numpy.concatenate([batch_np["labels"], numpy.full((10, B), eos)]).astype(numpy.int64)
    flip = rng.rand(*pred.shape) < 0.2
    pred[flip] = rng.randint(V - 1, size=int(flip.sum()))
    pred[-1] = eos
    Lp = pred.shape[0]
    gt, pr = torch.from_numpy(batch_np["labels"]).to(dev), torch.from_numpy(pred).to(dev)
    rw, gn, pm = torch.empty(Lp, B, V, device=dev), torch.empty(Lp, B, V, device=dev), torch.empty(Lp, B, device=dev)
    r, cost, dl = torch.randn(Lp * B, V, device=dev), torch.empty(Lp, B, device=dev), torch.empty(Lp * B, V, device=dev)
    rec = SpeechRecognizer(device=dev, params=synthetic.make_params(base, seed=10), net_config=dict(base, criterion="mse_gain"))
    lib = rec.lib
    st = lambda: lib.stream_for(rw)
    gain = lambda: lib.call("lvsr_reward_gain", st(), ptr(gt), L, ptr(pr), Lp, B, eos, V, ptr(rw), ptr(gn), ptr(pm))
    mse = lambda mode: lib.call("lvsr_reward_mse", st(), mode, ptr(r), V, ptr(gn), ptr(rw), ptr(pr), ptr(pm), Lp, B, V, -5.0, ptr(cost),
                                ptr(dl), V)
    for fn in (gain, lambda: mse(0), lambda: mse(1)):
        timed(fn, 10)
    lines += ["| kernel (Lp = %d) | us per launch |" % Lp, "|---|---|",
              "| lvsr_reward_gain | %.1f |" % (1e3 * timed(gain, 100)),
              "| lvsr_reward_mse, mse_gain | %.1f |" % (1e3 * timed(lambda: mse(0), 100)),
              "| lvsr_reward_mse, mse_reward | %.1f |" % (1e3 * timed(lambda: mse(1), 100)), ""]
    del rec

    # ---- whole training steps
    batch = {k: torch.from_numpy(v).to(dev) for k, v in batch_np.items()}
    lines += ["| training step | ms per step |", "|---|---|"]
    for name, criterion, exploration in (("log_likelihood (same build; this criterion's path is the one the project had before)", "log_likelihood", "imitative"),
                                         ("mse_gain, imitative", "mse_gain", "imitative"), ("mse_gain, greedy", "mse_gain", "greedy"),
                                         ("mse_reward, greedy", "mse_reward", "greedy")):
        cfg = dict(base, criterion=criterion, min_reward=-5.0)
        rec = SpeechRecognizer(device=dev, params=synthetic.make_params(base, seed=10), net_config=cfg)
        tr = Trainer(rec, distributed=False, exploration=exploration, **bench.TRAIN_CONF)
        for _ in range(args.warmup):
            tr.train_step(batch)
        ms = timed(lambda: tr.train_step(batch), args.steps)
        skipped = tr.step_was_skipped()
        regions = [s for s in rec._regions.values()]
        replayed = any(s["seen"] >= 3 for s in regions) and not any(s.get("bad") for s in regions)
        lines.append("| %s | %.2f%s |" % (name, ms, "" if replayed and not skipped else " (graph replay: %s, skipped: %s)" % (replayed, skipped)))
        tr.close()
        del tr, rec
    lines += ["", "The greedy steps contain a second decoder pass: the free-running generation of L + 10 = %d labels with the argmax" % (L + 10),
              "emitter (five launches per label), then the teacher-forced pass over those %d labels instead of %d." % (L + 10, L), ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
