#!/usr/bin/env python3
"""The training loop end to end, minibatches from the host pipeline against minibatches assembled on the device, in one process on
one GPU: a seeded synthetic dataset at bench.py's WSJ-base shape (per-GPU batch, frame lengths drawn as the `ragged` leg draws
them, padded to one shape so that the step graph is reused), global CMVN statistics as the Kaldi recipe computes them; epochs of
the loop of lvsr_amd.main.train (train_step, then the per-step reads of the cost and the gradient norm) alternate between
(a) `Data.get_stream` and (b) `DeviceData.get_stream` on ONE recognizer and trainer; a host clock around each epoch, ending in a
device synchronise.  Beside them the step on a minibatch that already sits in HBM (what bench.py times), and lvsr_assemble_batch
alone under device events.  Writes a markdown record.

    python tools/measure_data_path.py [--utterances 512] [--rounds 4] [--features 123] [--out profiles/data_path_wsj_base.md] [knob=int ...]
"""
import argparse
import ctypes
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "attention-lvcsr_amd")]

KNOBS = [a for a in sys.argv[1:] if "=" in a and not a.startswith("--")]
sys.argv = [a for a in sys.argv if a not in KNOBS]

import numpy  # noqa: E402
import torch  # noqa: E402

from bench import TRAIN_CONF  # noqa: E402
from lvsr_amd import kaldi_io, native, spec, synthetic  # noqa: E402
from lvsr_amd.bricks.recognizer import SpeechRecognizer  # noqa: E402
from lvsr_amd.data import ArrayDataset, Data, DeviceData  # noqa: E402
from lvsr_amd.training import Trainer  # noqa: E402

COPY_TBS = 6.29          # TB/s, the device-to-device copy ceiling the microarchitecture guide measures on MI355X


def make_dataset(cfg, n, T, L, seed):
    """T_i ~ U{T/2..T}, L_i ~ U{L/2..L} with <eol> (synthetic.make_batch(ragged=True)'s draw), features ~ N(3, 2): CMVN has work to do."""
    d = spec.Dims(cfg)
    rng = numpy.random.RandomState(seed)
    t_len = rng.randint(max(1, T // 2), T + 1, size=n)
    l_len = rng.randint(max(2, L // 2), L + 1, size=n) - 1                      # <eol> is appended by the pipeline
    t_len[0], l_len[0] = T, L - 1
    recs = [(3.0 + 2.0 * rng.standard_normal((t, d.F))).astype(numpy.float32) for t in t_len]
    labs = [rng.randint(0, max(1, d.V - 1), size=l) for l in l_len]
    return ArrayDataset(recs, labs, num_characters=d.V, eos_label=cfg.get("eos_label"))


def epoch(trainer, stream):
    """The loop body of lvsr_amd.main.train: the step, then what the log row reads back.  -> (steps, seconds, summed train cost)"""
    torch.cuda.synchronize()
    t0, steps, total = time.perf_counter(), 0, 0.0
    for batch in stream:
        cm = trainer.train_step(batch)
        assert not trainer.step_was_skipped()
        total += float(cm.sum()) / int(batch["labels"].shape[1])
        trainer.gradient_norm(), trainer.gradient_threshold()
        steps += 1
    torch.cuda.synchronize()
    return steps, time.perf_counter() - t0, total


def kernel_time(lib, dev, F, B, T, L, n=64, reps=200, seed=3):
    """lvsr_assemble_batch alone: `reps` launches on preallocated outputs between two device events.  -> (us, bytes)"""
    rng = numpy.random.RandomState(seed)
    t_len = rng.randint(T // 2, T + 1, size=n)
    l_len = rng.randint(L // 2, L + 1, size=n)
    t_len[0], l_len[0] = T, L
    up = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(dev)
    frames = torch.randn((int(t_len.sum()), F), device=dev)
    labels = torch.ones(int(l_len.sum()), dtype=torch.int64, device=dev)
    foff = up(numpy.concatenate([[0], numpy.cumsum(t_len)]).astype(numpy.int64))
    loff = up(numpy.concatenate([[0], numpy.cumsum(l_len)]).astype(numpy.int64))
    pick = numpy.concatenate([[0], rng.permutation(n)[: B - 1]])
    index = up(pick.astype(numpy.int64))
    out = [torch.empty(s, dtype=t, device=dev) for s, t in (((T, B, F), torch.float32), ((T, B), torch.float32), ((L, B), torch.int64),
                                                           ((L, B), torch.float32))]
    args = lib.make("lvsr_batch_args", frames=frames, frame_off=foff, labels=labels, label_off=loff, index=index, n=n, B=B, T=T, L=L,
                    F=F, recordings=out[0], recordings_mask=out[1], out_labels=out[2], labels_mask=out[3])
    stream = lib.stream_for(out[0])
    for _ in range(10):
        lib.call("lvsr_assemble_batch", stream, ctypes.byref(args))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        lib.call("lvsr_assemble_batch", stream, ctypes.byref(args))
    e1.record()
    torch.cuda.synchronize()
    moved = 4 * F * (int(t_len[pick].sum()) + T * B) + 4 * T * B + 8 * int(l_len[pick].sum()) + 12 * L * B
    return e0.elapsed_time(e1) * 1e3 / reps, moved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=4, help="alternations of the two paths (at least 3)")
    ap.add_argument("--resident-steps", type=int, default=32)
    ap.add_argument("--features", type=int, default=None, help="feature width (default: the workload's; 123 = fbank with deltas)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "data_path_wsj_base.md"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs an MI355X"
    assert args.rounds >= 3 and args.utterances >= 512
    dev = torch.device("cuda:0")
    lib = native.get()
    lib.set_knobs(KNOBS)
    factory, B, T, L = spec.WORKLOADS["wsj_base"]
    cfg = factory() if args.features is None else dict(factory(), input_dim=args.features)
    ds = make_dataset(cfg, args.utterances, T, L, seed=77)
    data = Data({"train": ds}, batch_size=B, normalization=kaldi_io.compute_cmvn_stats(ds.recordings), pad_frames_to=T, pad_labels_to=L)
    t0 = time.perf_counter()
    ddata = DeviceData(data, device=dev, lib=lib)
    torch.cuda.synchronize()
    t_upload = time.perf_counter() - t0
    rec = SpeechRecognizer(device=dev, params=synthetic.make_params(cfg, seed=10), net_config=cfg)
    trainer = Trainer(rec, distributed=False, **TRAIN_CONF)
    # warm every shape on both paths (eager pass, capture, first replays)
    for source in (data, ddata):
        epoch(trainer, source.get_stream("train", shuffle=True, seed=0, num_examples=6 * B))
    rows = {"a": [], "b": []}
    for r in range(args.rounds):
        for name, source in (("a", data), ("b", ddata)) if r % 2 == 0 else (("b", ddata), ("a", data)):
            steps, sec, _ = epoch(trainer, source.get_stream("train", shuffle=True, seed=1 + r))
            rows[name].append(sec / steps * 1e3)
    # resident minibatch of the same shape: bench.py's way (no read-back), and with the per-step reads of the training loop
    resident = next(iter(ddata.get_stream("train", shuffle=True, seed=1)))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.resident_steps):
        trainer.train_step(resident)
    torch.cuda.synchronize()
    ms_resident = (time.perf_counter() - t0) / args.resident_steps * 1e3
    _, sec, _ = epoch(trainer, (resident for _ in range(args.resident_steps)))
    ms_resident_reads = sec / args.resident_steps * 1e3
    regions = list(rec._regions.values())
    replayed = any(s["seen"] >= 3 for s in regions) and not any(s.get("bad") for s in regions)
    d = spec.Dims(cfg)
    kern = [(F,) + kernel_time(lib, dev, F, B, T, L) for F in sorted({d.F, 40, 123})]
    a, b = numpy.asarray(rows["a"]), numpy.asarray(rows["b"])
    steps_per_epoch = -(-args.utterances // B)
    lines = ["# Data path of the training loop: host pipeline against device-resident dataset (tools/measure_data_path.py)", "",
             "WSJ-base network and step rules of bench.py; %d synthetic utterances, T_i ~ U{%d..%d} frames x F = %d, L_i ~ U{%d..%d} labels, "
             "float32 CMVN statistics, minibatches of %d padded to T = %d, L = %d (one shape, one step graph; replayed: %s); %d steps per "
             "epoch.  One process, one MI355X, one recognizer and trainer for both paths; epochs alternate a, b, b, a, ...; host clock "
             "around each epoch, ending in a device synchronise.  The loop is that of lvsr_amd.main.train: train_step, then the reads of "
             "the cost, the gradient norm and the clipping threshold." % (args.utterances, T // 2, T, d.F, L // 2, L, B, T, L, replayed,
                                                                         steps_per_epoch), "",
             "| path | ms/step (median of %d epochs) | min | max |" % args.rounds, "|---|---|---|---|",
             "| (a) host `Data.get_stream` (the baseline) | %.3f | %.3f | %.3f |" % (numpy.median(a), a.min(), a.max()),
             "| (b) `DeviceData.get_stream` | %.3f | %.3f | %.3f |" % (numpy.median(b), b.min(), b.max()),
             "| resident minibatch, same loop (with the per-step reads) | %.3f | | |" % ms_resident_reads,
             "| resident minibatch, no read-back (bench.py's way) | %.3f | | |" % ms_resident, "",
             "Per-epoch ms/step, (a): %s; (b): %s." % (", ".join("%.3f" % v for v in a), ", ".join("%.3f" % v for v in b)), "",
             "(b) - (a) = %+.3f ms/step (%+.1f %%); (b) - resident with reads = %+.3f ms/step." % (
                 numpy.median(b) - numpy.median(a), 100 * (numpy.median(b) / numpy.median(a) - 1), numpy.median(b) - ms_resident_reads), "",
             "Store: %.1f MB on the device (frames, labels, two offset tables), normalised and uploaded once in %.2f s." % (
                 ddata.nbytes("train") / 1e6, t_upload), "",
             "## lvsr_assemble_batch alone", "",
             "200 back-to-back launches on preallocated outputs between two device events (B = %d, T = %d, L = %d, utterances drawn as "
             "above); bytes = frames read + every output element written." % (B, T, L), "",
             "| F | us per launch | MB moved | GB/s | time at the guide's %.2f TB/s copy figure | bound |" % COPY_TBS, "|---|---|---|---|---|---|"]
    for F, us, moved in kern:
        ideal = moved / (COPY_TBS * 1e12) * 1e6
        lines.append("| %d | %.2f | %.2f | %.0f | %.2f us | %s |" % (F, us, moved / 1e6, moved / us / 1e3, ideal,
                                                                   "launch-bound" if us > 2 * ideal else "bandwidth-bound"))
    lines.append("")
    trainer.close()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
