#!/usr/bin/env python3
"""Benchmark of the hot path: encoder+attention+decoder TRAINING frames/sec on WSJ-shape synthetic fbank batches.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload wsj_base|wsj_deep|wsj_stack2|wsj_paper|timit_tiny|wsj_decode]
                    [--scaling weak|strong] [--batch B] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times the K steps and prints the line.  `--full` adds the secondary measurements around it
(with_h2d, sustained, ragged, strong, the all-reduce alone, roofline + dense_gemm, fbank, decode + beam200, cpu_baseline; the
--no-* flags and --sustained-seconds select among them).  `--dump-outputs DIR` writes what the last timed step computed as
DIR/<name>.npy (dump_outputs()), so that two builds can be compared output for output on the same seeded inputs.

A step = forward + backward of the whole recognizer on one minibatch already resident in HBM, the (RCCL) sum
all-reduce of the flat gradient buffer when N > 1, and the fused optimiser step (clip -> scale -> AdaDelta ->
max-norm -> remove-not-finite).  `--gpus N` without a torchrun environment re-launches itself under
torch.distributed.run with N ranks (one per GPU, 127.0.0.1 rendezvous).
  weak scaling (default): every rank processes B utterances per step (global batch N*B);
  strong scaling: the global batch is fixed (BASELINE.json configs[2]: 128 utterances for wsj_base) and rank r takes
  utterances r::N of it, so the per-GPU batch shrinks as N grows.
value = real (unpadded) input frames of all ranks per second.  Rank 0 prints ONE JSON line on stdout; everything else
goes to stderr.  `--workload wsj_decode` is the decoding benchmark (configs[4]), see decode_bench().
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
for _p in (REPO, os.path.join(REPO, "attention-lvcsr_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy
import torch


def log(*a):
    print(*a, file=sys.stderr, flush=True)


TRAIN_CONF = dict(gradient_threshold=100.0, rules=("momentum", "adadelta"), scale=0.1, momentum=0.0, decay_rate=0.95,
                  epsilon=1e-8, max_norm=1.0)        # exp/wsj/configs/wsj_jan_new.yaml training/regularization sections
STRONG_GLOBAL_BATCH = {"wsj_base": 128, "wsj_deep": 64, "timit_tiny": 16}     # configs[2] for wsj_base
TRAIN_FLOP_PER_FRAME = {"wsj_base": 22.730e6, "wsj_deep": 143.43e6, "timit_tiny": 1.382e6}
PEAK_FP32_MFMA = 157.3          # TFLOP/s dense fp32 matrix (MI355X_MICROARCH.md)


class GpuBackend(object):
    """Where the benchmark runs: one MI355X per rank, RCCL between ranks.  (tests/bench_cpu_launch.py passes a CPU stand-in to
    main() to exercise the launcher / sharding / JSON plumbing without a GPU; bench.py itself knows no other backend.)"""
    measured = True             # the roofline / cpu_baseline / decode legs run
    collective = "nccl"
    workloads = {}              # extra workloads (name -> (factory, B, T, L))

    def open(self, local_rank):
        assert torch.cuda.is_available(), "bench.py needs an MI355X"
        torch.cuda.set_device(local_rank)
        return torch.device("cuda", local_rank), None


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def respawn_under_torchrun(n):
    """`python bench.py --gpus N` as the driver calls it: become N ranks of one node (one process per GPU)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(sys.argv[0])] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    log("bench: launching %d ranks: %s" % (n, " ".join(cmd)))
    return subprocess.call(cmd, env=env)


def encoder_kernels_of(rec, B, dims):
    cols = rec.encoder._pass_columns(B)
    if cols is not None:
        return "persistent clusters, %d passes of <= %d utterances" % (len(cols), max(hi - lo for lo, hi in cols))
    return "persistent clusters" if rec.encoder._sync_ws(0, B, dims.Hs[0]) is not None else "step kernels"


def dominant_kernel_probe(rec, dims, T, B):
    """Average launch duration of the dominant kernel measured with HIP events on the recognizer's own stream.
    Persistent encoder (default at WSJ-base): enc_pbwd_kernel, ONE launch = the whole BPTT time loop of a layer (both
    directions, T steps); flops = the three (B x H)·(H x H) contractions per step and direction.
    Step kernels (large per-GPU batches): enc_bwd_b_kernel, one launch per time step, measured over T graph-replayed
    launches (the figure then includes the dependent-launch boundary, which IS the cost of that latency-bound kernel)."""
    lib, ws, enc, p = rec.lib, rec.ws, rec.encoder, rec.store.p
    H = dims.Hs[0]
    nf, nb = enc._names(0, "forward"), enc._names(0, "backward")
    Bp = (B + 15) // 16 * 16
    sync = enc._sync_ws(0, B, H)
    bufs = dict(y=ws.get("enc0.y", (T, B, 2 * H)), u=ws.get("enc0.u", (T, B, 2 * H)), r=ws.get("enc0.r", (T, B, 2 * H)),
                c=ws.get("enc0.c", (T, B, 2 * H)), dy=ws.get("probe.dy", (T, B, 2 * H)), dxg=ws.get("enc0.dxg", (T, B, 6 * H)),
                dh_ws=ws.get("enc0.dh", (12 * Bp * H,)))
    fields = dict(mask=None, h0=[p[nf["h0"]], p[nb["h0"]]], dh0=[ws.get("probe.dh0a", (H,)), ws.get("probe.dh0b", (H,))],
                  sub=1, T=T, B=B, H=H, **bufs)
    if sync is not None:
        fields.update(WhhT_p=[p[nf["Whh"]], p[nb["Whh"]]], WhgT_p=[p[nf["Whg"]], p[nb["Whg"]]], persistent=1, sync_ws=sync)
        name, launches, flops = "enc_pbwd_kernel", 1, 2.0 * B * H * H * 3 * 2 * T
    else:
        pk = enc._packed(0)
        fields.update(WhhT_p=[pk["WhhT"][0], pk["WhhT"][1]], WhgT_p=[pk["WhgT"][0], pk["WhgT"][1]], kernel_mask=2)
        name, launches, flops = "enc_bwd_b_kernel", T, 2.0 * B * H * H * 2
    times = []
    with torch.cuda.stream(rec.stream):
        for it in range(4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(rec.stream)
            lib.run("lvsr_bigru_bwd", "lvsr_bigru_bwd_args", bufs["dxg"], True, **fields)
            e1.record(rec.stream)
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3 / launches)
    avg = sorted(times[1:])[len(times[1:]) // 2]
    # algorithmic HBM bytes of one launch: reads of u, r, c, y (+ dy), writes of dxg, the recurrent weights once
    per_step = B * 2 * H * 4 * (4 + 1 + 3)
    abytes = (lambda t: per_step * t + 2 * 3 * H * H * 4) if sync is not None else (lambda t: per_step + 2 * H * H * 4)
    return dict(kernel=name, launch_s=avg, flops=flops, steps_per_launch=(T if sync is not None else 1), algorithmic_bytes=abytes(T),
                algorithmic_bytes_at=abytes)


def gemm_probe(rec, dims, T, B):
    """The step's dense contractions timed alone with HIP events on the recognizer's stream — the MFMA-bound part of the path,
    reported beside the latency-bound dominant kernel.  The three big shapes of an encoder layer above the first: the input
    projection of both directions and all gates as ONE product (T*B, 2H) x (2H, 6H) [the largest contraction of the step], its
    input gradient (T*B, 6H) x (6H, 2H)^T and its weight gradient (2H, T*B)^T x (T*B, 6H) (deterministic split-K)."""
    lib, dev = rec.lib, rec.device
    H = dims.Hs[0]
    M, K, N = T * B, 2 * H, 6 * H
    X, W, XG = torch.randn(M, K, device=dev), torch.randn(K, N, device=dev), torch.randn(M, N, device=dev)
    dX, dW, ws = torch.empty(M, K, device=dev), torch.empty(K, N, device=dev), torch.empty(64 << 20, device=dev)
    calls = [("projection", lambda: lib.sgemm(X, W, XG), [M, N, K]),
             ("input_gradient", lambda: lib.sgemm(XG, W, dX, transB=True), [M, K, N]),
             ("weight_gradient", lambda: lib.sgemm(X, XG, dW, transA=True, ws=ws), [K, N, M])]
    out = {}
    # 300 launches per shape (~60 ms): a burst of 20 behind a host synchronisation measured 20 % slower than the steady state (225 vs
    # 185 us for the projection; 3.6 s of back-to-back launches hold 181 us, profiles/r04_gemm_k_sweep.txt) — the first launches after an
    # idle gap run at ramping clocks
    NL = 300
    with torch.cuda.stream(rec.stream):
        for name, fn, shape in calls:
            for _ in range(20):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(rec.stream)
            for _ in range(NL):
                fn()
            e1.record(rec.stream)
            e1.synchronize()
            sec = e0.elapsed_time(e1) * 1e-3 / NL
            ach = 2.0 * shape[0] * shape[1] * shape[2] / sec / 1e12
            out[name] = dict(shape_mnk=shape, launch_us=sec * 1e6, launches=NL, achieved=ach, frac=ach / PEAK_FP32_MFMA)
        # the burst figure round 3 reported, for comparison
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(rec.stream)
        for _ in range(20):
            calls[0][1]()
        e1.record(rec.stream)
        e1.synchronize()
        out["projection"]["burst_of_20_us"] = e0.elapsed_time(e1) * 1e3 / 20
    big = out["projection"]
    return dict(kernel="lvsr_sgemm64_kernel", shape=big["shape_mnk"], launch_us=big["launch_us"], achieved=big["achieved"], unit="TFLOP/s",
                frac=big["frac"], layer_shapes=out)


PMC_FILE = os.path.join(REPO, "profiles", "r06_pmc_bench.json")


def csrc_sha():
    """Hash of the sources the dominant kernel is compiled from: csrc/encoder_persist.hip and the csrc headers it includes."""
    import hashlib
    csrc = os.path.join(REPO, "attention-lvcsr_amd", "csrc")
    h = hashlib.sha256()
    for f in ("common.h", "encoder_persist.hip", "graph_cache.h", "persist.h"):
        h.update(open(os.path.join(csrc, f), "rb").read())
    return h.hexdigest()[:16]


def pmc_record(kernel):
    """HBM-side bytes per launch of `kernel` from the committed rocprofv3 PMC passes over THIS benchmark's step (PMC_FILE, written
    by tools/pmc_summary.py from separate --pmc FETCH_SIZE / WRITE_SIZE runs; FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes).
    The record carries a hash of the kernel sources it was measured on: -> (record, None), or (None, why) when there is no
    record or the sources have changed since (a stale traffic figure is not printed)."""
    if not os.path.exists(PMC_FILE):
        return None, "no PMC record (%s)" % os.path.basename(PMC_FILE)
    try:
        doc = json.load(open(PMC_FILE))
    except Exception as exc:
        return None, "unreadable PMC record: %s" % exc
    stamp = (doc.get("__stamp__") or {}).get("csrc_sha256")
    if stamp != csrc_sha():
        return None, "PMC record is stale: taken on kernel sources %s, this run has %s" % (stamp, csrc_sha())
    rec = doc.get(kernel)
    return (rec, None) if rec else (None, "kernel %s not in the PMC record" % kernel)


PEAK_HBM = 8.0e12               # bytes/s (MI355X_MICROARCH.md)


def decode_leg(dev, utterances, batch=64, streams=8):
    """configs[4] in the default line: ALL 1000 synthetic utterances by default (round 5 decoded a 128-utterance sample here; the whole
    set is about a second of GPU time; `--workload wsj_decode` runs the same set as a line of its own) —
    beam 16 + char-trigram FST LM on the device, window_around_median(10, 100), exp/wsj/decode.sh settings, 800-frame synthetic
    utterances, `batch` utterances per set of launches and `streams` such batches in flight on one GPU (tools/bench_decode.py)."""
    from tools.bench_decode import build, run_batched
    recs = [build(dev, 16)[0] for _ in range(streams)]
    sec, done, nframes, chars, steps = run_batched(recs, utterances, 800, batch=batch)
    # what a position of one utterance has to move and compute at least: the attended rows and their preprocessed copies of the
    # utterance once (T' x (E + M) floats: the 16 hypotheses share them), two transcendentals per (hypothesis, window position, match
    # column) of the energies — priced against the HBM roofline and the quarter-rate transcendental pipe
    Tp, E, M, K, window = 200, 512, 512, 16, 111
    pos_s = sec / max(steps, 1)
    hbm_bytes = Tp * (E + M) * 4
    trans = 2.0 * K * window * M
    trans_peak = 256 * 4 * 16 / 4 * 2.4e9          # CUs x SIMDs x lanes / 4 (quarter rate) x clock
    roof = dict(bound="latency (13 small kernels per position)", us_per_position_per_utterance=pos_s * 1e6,
                hbm=dict(algorithmic_bytes=hbm_bytes, achieved=hbm_bytes / pos_s / 1e9, peak=PEAK_HBM / 1e9, unit="GB/s", frac=hbm_bytes / pos_s / PEAK_HBM),
                transcendental=dict(ops=trans, achieved=trans / pos_s / 1e12, peak=trans_peak / 1e12, unit="Tops/s", frac=trans / pos_s / trans_peak),
                note="neither roofline is near: the leg is bound by the ramp-up / tails of thirteen dependent kernels per position (DESIGN.md 7)")
    return dict(roofline=roof, workload="wsj_decode: %d synthetic 800-frame utterances (BASELINE configs[4]: 1000), WSJ-base weights, beam 16, device FST LM "
                         "(weight 0.5, no_transition_cost 20), char_discount 1.0, max length T/3" % done,
                utterances=done, ms_per_utterance=sec / done * 1e3, utterances_per_s=done / sec, frames_per_s=nframes / sec,
                utterances_per_launch_set=batch, searches_in_flight=streams * batch, positions_per_utterance=steps / max(done, 1), us_per_position=sec * 1e6 / max(steps, 1),
                mean_best_hypothesis_length=chars / max(done, 1),
                parity="tests/test_decode_golden.py::test_full_size_wsj_decode_batched_whole_list_matches_the_reference_gpu (reference-generated golden)")


def beam200_leg(dev, utterances=32, batch=8, streams=2):
    """The beam width the reference's README recommends for its best numbers (exp/wsj/README.md:58-60, exp/wsj/decode.sh:12): 200
    hypotheses x 33 characters = 6 600 candidates per position in lvsr_beam_select, row groups of 200 across the 16-row tiles.
    A bounded sample (32 of the synthetic 800-frame utterances, 8 per set of launches = 1 600 rows, two sets in flight)."""
    from tools.bench_decode import build, run_batched
    # on the CONDITIONED network of the reference-generated decode fixtures (round-5 verdict, weak 4: on the random-weight set of the beam-16 leg
    # a beam-200 search ends on a bare <eol> — all 222 positions run, but nothing is explored)
    recs = [build(dev, 200, conditioned=True)[0] for _ in range(streams)]
    sec, done, nframes, chars, steps = run_batched(recs, utterances, 800, batch=batch)
    return dict(beam_size=200, utterances=done, utterances_per_launch_set=batch, searches_in_flight=streams * batch, ms_per_utterance=sec / done * 1e3,
                network="WSJ-base at the parameter scales of tests/golden/wsj_decode_full2 / wsj_decode_beam200 (WSJ_COND_DECODE on scale 2, LM seed 9)",
                parity="tests/test_decode_golden.py::test_beam_200_matches_the_reference_gpu (reference-generated golden, whole ranked lists)",
                positions_per_utterance=steps / max(done, 1), us_per_position=sec * 1e6 / max(steps, 1), mean_best_hypothesis_length=chars / max(done, 1))


def fbank_leg(dev, seconds=8.0, utterances=512):
    """The front end on a SET of synthetic utterances resident in HBM, one launch per stage (lvsr_fbank_batch: a 512-point FFT per
    frame, one wave per frame; lvsr_add_deltas_cmvn_batch): integer-in / float-out streaming work, priced against the HBM roofline with
    its ALGORITHMIC bytes (int16 samples in, (T, 41) log-mel + energy out; then (T, 41) in, (T, 123) out).  Beside it the
    per-utterance launches of the direct-DFT kernel (what round 3 shipped)."""
    from lvsr_amd.features import Fbank
    fb = Fbank(device=dev)
    nsamp = int(seconds * 16000)
    rng = numpy.random.RandomState(7)
    one = (rng.normal(size=nsamp) * 3000).astype(numpy.int16)
    T = fb.num_frames(nsamp)
    wav = torch.from_numpy(one).to(dev).repeat(utterances)
    wav_off = torch.arange(utterances + 1, dtype=torch.int64, device=dev) * nsamp
    frame_off = (torch.arange(utterances + 1, dtype=torch.int64, device=dev) * T).to(torch.int32)
    mean, std = numpy.zeros(123, numpy.float32), numpy.ones(123, numpy.float32)
    for _ in range(2):
        feats, _ = fb.batch_resident(wav, wav_off, frame_off, utterances, utterances * T)
        fb.add_deltas_cmvn_batch(feats, frame_off, mean, std)
    torch.cuda.synchronize()
    reps = 10
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    for _ in range(reps):
        feats, _ = fb.batch_resident(wav, wav_off, frame_off, utterances, utterances * T)
    e[1].record()
    for _ in range(reps):
        fb.add_deltas_cmvn_batch(feats, frame_off, mean, std)
    e[2].record()
    e[2].synchronize()
    t_fb, t_dl = e[0].elapsed_time(e[1]) * 1e-3 / reps, e[1].elapsed_time(e[2]) * 1e-3 / reps
    b_fb = utterances * (nsamp * 2 + T * 41 * 4)
    b_dl = utterances * (T * 41 * 4 + T * 123 * 4)
    # the per-utterance path on 16 of them
    wavs = [wav[u * nsamp:(u + 1) * nsamp] for u in range(16)]
    for w in wavs[:2]:
        fb(w)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for w in wavs:
        fb(w)
    e1.record()
    e1.synchronize()
    t_one = e0.elapsed_time(e1) * 1e-3 / len(wavs)
    return dict(workload="%d utterances x %.0f s of 16 kHz int16 PCM (%.0f MB) -> %d frames x 41 (log-mel + energy) -> x 123 (deltas, CMVN); "
                         "one launch per stage for the whole set" % (utterances, seconds, utterances * nsamp * 2 / 1e6, T),
                frames_per_s=utterances * T / (t_fb + t_dl), audio_seconds_per_s=utterances * seconds / (t_fb + t_dl),
                lvsr_fbank_batch=dict(bound="hbm", launch_us=t_fb * 1e6, us_per_utterance=t_fb / utterances * 1e6, algorithmic_bytes=b_fb,
                                      achieved=b_fb / t_fb / 1e9, peak=PEAK_HBM / 1e9, unit="GB/s", frac=b_fb / t_fb / PEAK_HBM),
                lvsr_add_deltas_cmvn_batch=dict(bound="hbm", launch_us=t_dl * 1e6, us_per_utterance=t_dl / utterances * 1e6, algorithmic_bytes=b_dl,
                                                achieved=b_dl / t_dl / 1e9, peak=PEAK_HBM / 1e9, unit="GB/s", frac=b_dl / t_dl / PEAK_HBM),
                lvsr_fbank_per_utterance=dict(us_per_utterance=t_one * 1e6, achieved=(nsamp * 2 + T * 41 * 4) / t_one / 1e9, unit="GB/s",
                                              note="one launch of the direct-DFT kernel per 0.4-MB utterance: launch / latency bound"),
                note="parity: the 40 log-mel columns are pinned to an independent Kaldi-compatible implementation (HuggingFace transformers.audio_utils, "
                     "tests/golden/fbank_hf_kaldi.npz); no Kaldi-produced vector exists in the image (DESIGN.md section 4)")


def cpu_baseline(cfg, params, B, T, L, workload):
    """The CPU oracle (torch fp32 restatement of the reference's algorithm, oracle/lvsr_oracle.py) timed on this
    box's host cores on whole minibatches of the same workload (forward + backward).  The reference's own Theano path
    cannot travel to the GPU box; its figure, measured where it can run, rides along under `reference_theano`."""
    from oracle import lvsr_oracle as O
    from lvsr_amd import synthetic
    batch = synthetic.make_batch(cfg, B, T, L, seed=1234)
    orc = O.OracleRecognizer(cfg, params, dtype=torch.float32)
    ncores = min(8, os.cpu_count() or 1)        # the per-step matrices are small: more threads only add overhead
    torch.set_num_threads(ncores)
    # bounded sample: whole minibatches until ~12 s of CPU work have been done (at least one, at most four)
    reps, t0 = 0, time.time()
    while reps < 1 or (time.time() - t0 < 12.0 and reps < 4):
        orc.cost_and_grads(batch)
        reps += 1
    dt = time.time() - t0
    out = dict(value=reps * B * T / dt, unit="frames/s", cores=ncores, kind="port",
               sample="%d forward+backward passes over one %dx%d-frame minibatch (%s) = %.1f s of CPU work; torch-CPU fp32 "
                      "restatement of the reference's Theano graph" % (reps, B, T, "same synthetic batch shape", dt))
    gold = os.path.join(REPO, "tests", "golden", workload + ".npz")
    if os.path.exists(gold):
        meta = json.loads(str(numpy.load(gold, allow_pickle=False)["meta"]))
        if meta.get("step_s"):
            out["reference_theano"] = dict(value=meta["B"] * meta["T"] / meta["step_s"], unit="frames/s", cores=8, step_s=meta["step_s"],
                                           measured="2026-09-26, build container (8 vCPU), when tests/golden/%s.npz was generated" % workload,
                                           how="the reference itself: Theano 0.8 python linker (cxx=, optimizer_excluding=fusion), one "
                                               "forward+backward on the same batch; it cannot run on the GPU box")
    return out


DUMP_CAP = dict(cost_matrix=1 << 20, parameters=7 << 20, gradients=7 << 20)      # float32 elements per file: 60 MiB in all


def dump_outputs(out_dir, cm, store):
    """--dump-outputs: what the timed path computed in its last step, as out_dir/<name>.npy (float32): the cost matrix
    Trainer.train_step returned (labels x utterances of rank 0), and the store's flat parameter and gradient vectors after that
    step (ParameterStore.offsets maps names to slices).  An array longer than its DUMP_CAP entry is written as a fixed sample: the
    elements at the sorted indices numpy.random.RandomState(0).choice(n, cap, replace=False)."""
    os.makedirs(out_dir, exist_ok=True)
    for name, t in (("cost_matrix", cm), ("parameters", store.flat), ("gradients", store.grad)):
        a = t.detach().to(torch.float32).cpu().numpy()
        if a.size > DUMP_CAP[name]:
            a = a.ravel()[numpy.sort(numpy.random.RandomState(0).choice(a.size, DUMP_CAP[name], replace=False))]
        numpy.save(os.path.join(out_dir, name + ".npy"), numpy.ascontiguousarray(a))
        log("bench: wrote %s %s (%s)" % (os.path.join(out_dir, name + ".npy"), a.shape, "sampled" if a.size < t.numel() else "whole"))


def main(backend=None):
    backend = backend or GpuBackend()
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="wsj_base")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak")
    ap.add_argument("--batch", type=int, default=None, help="utterances per GPU (weak) / global batch (strong) override")
    ap.add_argument("--frames", type=int, default=None, help="frames per utterance override (labels scale along unless --labels)")
    ap.add_argument("--labels", type=int, default=None, help="labels per utterance override")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-decode", action="store_true", help="skip the decode leg (configs[4]: all 1000 utterances) of the default line")
    ap.add_argument("--decode-utterances", type=int, default=1000, help="utterances of the decode leg (configs[4] names 1000)")
    ap.add_argument("--decode-batch", type=int, default=64, help="decode: utterances per set of launches (1: one search per recognizer, --streams in flight)")
    ap.add_argument("--knob", action="append", default=[], metavar="NAME=INT",
                    help="tuning knob of the library (include/lvsr_hip.h LVSR_KNOB_*), for A/B measurements; recorded in config.knobs")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-drain", action="store_true",
                    help="do not block the host until a step's graph has drained (Lib.sync_after_graph = False): the next step's launch is enqueued behind the running one")
    ap.add_argument("--force-dist", action="store_true", help="initialise the process group (RCCL) even with one rank")
    ap.add_argument("--ragged", action="store_true",
                    help="secondary run of SURVEY.md 8(d): utterance lengths ~U{T/2..T}, zero padded; counts real frames only")
    ap.add_argument("--sustained-seconds", type=float, default=7.5,
                    help="length of the `sustained` segment behind the timed region (replayed steps at steady-state clocks); 0 = skip")
    ap.add_argument("--no-strong", action="store_true",
                    help="skip the `strong` sub-object (global batch of configs[2] split over the ranks, speed-up over ONE GPU at that batch)")
    ap.add_argument("--no-fbank", action="store_true", help="skip the front-end leg (lvsr_fbank GB/s)")
    ap.add_argument("--no-ragged", action="store_true", help="skip the `ragged` sub-object (the same job on ragged minibatches, real frames/s)")
    ap.add_argument("--no-beam200", action="store_true", help="skip decode.beam200 (the README's beam width, exp/wsj/README.md:58-60)")
    ap.add_argument("--overlap-allreduce", action="store_true",
                    help="data parallel: reduce the decoder's gradients while the encoder's BPTT runs (two buckets, Trainer(overlap_allreduce=True))")
    ap.add_argument("--utterances", type=int, default=None, help="wsj_decode: number of utterances (default 1000 = configs[4])")
    ap.add_argument("--streams", type=int, default=None, help="wsj_decode: recognizers (streams) in flight per GPU (default 4 batches; 8 searches with --decode-batch 1)")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary measurements: with_h2d, sustained, ragged, strong, the all-reduce alone, roofline (+ dense_gemm), "
                         "fbank, decode (+ beam200), cpu_baseline (the --no-* flags and --sustained-seconds select among them)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (cost matrix, parameters and gradients after it) as DIR/<name>.npy, float32")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.dump_outputs and args.workload == "wsj_decode":
        ap.error("--dump-outputs is for the training workloads; wsj_decode has no step outputs to write")

    if args.gpus > 1 and "RANK" not in os.environ:
        raise SystemExit(respawn_under_torchrun(args.gpus))
    # stdout carries exactly ONE line, the JSON record of rank 0: libraries that chat on fd 1 (RCCL prints a version banner
    # there when a communicator is created) are sent to stderr for the duration of the run
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py --gpus %d was started with WORLD_SIZE=%d" % (args.gpus, world))
    if args.workload == "wsj_decode":
        from tools.bench_decode import decode_bench
        return decode_bench(args, rank, world, local_rank, json_out)
    dev, lib = backend.open(local_rank)
    dist = world > 1 or args.force_dist
    if dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(29500))
        kw = dict(device_id=dev) if backend.collective == "nccl" else {}
        torch.distributed.init_process_group(backend.collective, rank=rank, world_size=world, **kw)

    from lvsr_amd import spec, synthetic
    from lvsr_amd.bricks.recognizer import SpeechRecognizer
    from lvsr_amd.training import Trainer

    factory, B0, T, L = backend.workloads[args.workload] if args.workload in backend.workloads else spec.WORKLOADS[args.workload]
    cfg = factory()
    dims = spec.Dims(cfg)
    if args.frames:          # length sweeps: longer utterances leave the persistent decoder kernels' limits
        L = args.labels or max(1, L * args.frames // T)
        T = args.frames
    elif args.labels:
        L = args.labels
    if args.scaling == "weak":
        B = args.batch or B0
        global_batch = B * world
    else:
        global_batch = args.batch or STRONG_GLOBAL_BATCH.get(args.workload, 2 * B0)
        if global_batch % world:
            raise SystemExit("strong scaling: the global batch %d does not divide over %d ranks" % (global_batch, world))
        B = global_batch // world
    params = synthetic.make_params(cfg, seed=10)
    rec = SpeechRecognizer(device=dev, params=params, lib=lib, net_config=cfg, use_graph=not args.no_graph)
    if args.no_drain:
        rec.lib.sync_after_graph = False
    knobs = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in args.knob}
    for k, v in knobs.items():
        rec.lib.set_knob(k, v)
    trainer = Trainer(rec, distributed=dist, overlap_allreduce=args.overlap_allreduce, **TRAIN_CONF)
    nsteps = args.steps + args.warmup
    # synthetic global batches, seeded identically on every rank; rank r keeps utterances r::world.  `value` is measured with the
    # minibatches resident in HBM (the bench contract); with --full the same K steps are then repeated with the minibatches waiting
    # in PINNED HOST memory and copied per step (four asynchronous copies on the recognizer's stream in front of the step's graph): the
    # H2D-inclusive step of SURVEY.md 8(d), reported beside it as config.with_h2d.
    nstage = min(nsteps, 4)
    staged, staged_host = [], []
    for s in range(nstage):
        gb = synthetic.make_batch(cfg, global_batch, T, L, seed=1234 + s, ragged=args.ragged)
        sh = synthetic.shard_batch(gb, rank, world)
        staged.append({k: torch.from_numpy(v).to(dev) for k, v in sh.items()})
        if dev.type == "cuda" and args.full:
            staged_host.append({k: torch.from_numpy(v).pin_memory() for k, v in sh.items()})
    h2d_bytes = sum(v.numel() * v.element_size() for v in staged[0].values())
    # real (unpadded) frames per step over all ranks: every rank holds global_batch/world utterances of the same lengths
    # distribution; with the default all-ones masks this is exactly global_batch*T
    frames_local = float(sum(float(b["recordings_mask"].sum()) for b in staged)) / len(staged)
    if dist:
        t = torch.tensor([frames_local], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(t)
        frames_per_step = float(t[0])
    else:
        frames_per_step = frames_local

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()

    def barrier():
        if dist:
            torch.distributed.barrier()

    sync()
    # setup, not warm-up: the first step of a shape allocates the workspaces, the second captures the whole-step hipGraph
    # (lvsr_amd.native.Region); whatever --warmup says, the timed steps are replays.  Reported as config.priming_steps.
    PRIME = 2 if (not args.no_graph and backend.measured) else 0
    for s in range(PRIME):
        trainer.train_step(staged[s % nstage], global_batch_size=global_batch)
    for s in range(args.warmup):
        cm = trainer.train_step(staged[s % nstage], global_batch_size=global_batch)
    sync()
    barrier()
    sync()
    t0 = time.perf_counter()
    marks = [t0]
    for s in range(args.steps):
        cm = trainer.train_step(staged[(args.warmup + s) % nstage], global_batch_size=global_batch)
        marks.append(time.perf_counter())       # host clock when the step's call returned (the whole-step graph blocks the host)
    sync()
    barrier()
    sync()
    elapsed = time.perf_counter() - t0
    marks[-1] = t0 + elapsed
    per_step = sorted((b - a) * 1e3 for a, b in zip(marks[:-1], marks[1:]))
    ms_median = per_step[len(per_step) // 2] if len(per_step) % 2 else 0.5 * (per_step[len(per_step) // 2 - 1] + per_step[len(per_step) // 2])
    # the last timed step's outputs, taken before any --full leg steps the trainer again
    last_cost = float(cm.sum())
    assert numpy.isfinite(last_cost), "training diverged in the benchmark"
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, cm, rec.store)
    with_h2d = None
    if staged_host:
        trainer.train_step(staged_host[0], global_batch_size=global_batch)
        sync()
        barrier()
        th = time.perf_counter()
        for s in range(args.steps):
            cm = trainer.train_step(staged_host[(args.warmup + s) % nstage], global_batch_size=global_batch)
        sync()
        barrier()
        eh = time.perf_counter() - th
        if dist:
            t = torch.tensor([eh], dtype=torch.float64, device=dev)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            eh = float(t[0])
        with_h2d = dict(ms_per_step=eh / args.steps * 1e3, bytes_per_step=h2d_bytes,
                        how="minibatch copied per step from pinned host memory on the compute stream, not overlapped")
    def max_over_ranks(x):
        if not dist:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        return float(t[0])

    elapsed = max_over_ranks(elapsed)

    def timed(tr, batches, nsteps, gbs, nwarm):
        """nwarm untimed + nsteps timed steps of trainer `tr` on `batches` -> (seconds, per-step host intervals in ms); barrier +
        device synchronisation on both sides, maximum over the ranks."""
        for k in range(nwarm):
            tr.train_step(batches[k % len(batches)], global_batch_size=gbs)
        sync(); barrier(); sync()
        t_a = time.perf_counter()
        mk = [t_a]
        for k in range(nsteps):
            tr.train_step(batches[k % len(batches)], global_batch_size=gbs)
            mk.append(time.perf_counter())
        sync(); barrier(); sync()
        el = time.perf_counter() - t_a
        mk[-1] = t_a + el
        return max_over_ranks(el), [(b_ - a_) * 1e3 for a_, b_ in zip(mk[:-1], mk[1:])]

    # ---- sustained segment: the same replayed step for several seconds, so that the clocks are those of a long run (the K timed
    # steps above last a fraction of a second on a chip that has just been idle) and samplers with a coarse period see the GPU busy
    sustained = None
    if backend.measured and args.full and args.sustained_seconds > 0:
        n_sus = max(20, int(args.sustained_seconds / max(1e-4, elapsed / args.steps)))
        el, iv = timed(trainer, staged, n_sus, global_batch, 0)
        srt = sorted(iv)
        q = max(1, n_sus // 5)
        sustained = dict(steps=n_sus, seconds=el, ms_per_step=el / n_sus * 1e3, ms_per_step_median=srt[n_sus // 2],
                         ms_per_step_p95=srt[min(n_sus - 1, int(0.95 * n_sus))], ms_per_step_min=srt[0], ms_per_step_max=srt[-1],
                         ms_per_step_first_fifth=sum(iv[:q]) / q, ms_per_step_last_fifth=sum(iv[-q:]) / q,
                         value=frames_per_step * n_sus / el, unit="frames/s",
                         how="same replayed whole-step graph as the timed region, %d steps back to back; per-step figures are host intervals "
                             "(the host blocks until a step's graph has drained), rank 0's" % n_sus)

    # ---- secondary run of SURVEY.md 8(d): the same job on RAGGED minibatches (T_i ~ U{T/2..T}, L_i ~ U{L/2..L}, zero padded to (T, L);
    # utterance 0 of every global batch full length) — real (unpadded) frames per second
    ragged = None
    if backend.measured and args.full and not args.ragged and not args.no_ragged and args.scaling == "weak":
        rb, rframes = [], 0.0
        for k in range(2):
            gbatch = synthetic.make_batch(cfg, global_batch, T, L, seed=2345 + k, ragged=True)
            sh = synthetic.shard_batch(gbatch, rank, world)
            rframes += float(gbatch["recordings_mask"].sum()) / 2
            rb.append({kk: torch.from_numpy(v).to(dev) for kk, v in sh.items()})
        n_rg = max(5, min(args.steps, 10))
        el, _ = timed(trainer, rb, n_rg, global_batch, 3)
        ragged = dict(steps=n_rg, ms_per_step=el / n_rg * 1e3, real_frames_per_step=rframes, padded_frames_per_step=float(global_batch * T),
                      value=rframes * n_rg / el, unit="real frames/s", fraction_of_all_ones_value=(rframes * n_rg / el) / (frames_per_step * args.steps / elapsed),
                      how="T_i ~ U{T/2..T}, L_i ~ U{L/2..L} (synthetic.make_batch(ragged=True)), zero padded; frames counted = sum of the input mask",
                      note="one utterance per cluster and as many clusters as the chip holds: the step lasts as long as its longest "
                           "utterance's chain, so iid lengths cost mean/max of the throughput whatever the kernels do (DESIGN.md 6); what "
                           "removes the padding is the reference's own length bucketing, below")
        # the same length distribution through the reference's data pipeline option `sort_k_batches` (lvsr/datasets/__init__.py:281-293,
        # lvsr_amd.data.Data._sort_k): 8 minibatches' worth of utterances sorted by length, cut into minibatches, every minibatch
        # padded to ITS longest utterance (rounded up to 32 frames: few distinct shapes = few captured step graphs)
        if world == 1:
            from lvsr_amd.data import Data
            K = 8
            big = synthetic.make_batch(cfg, global_batch * K, T, L, seed=3456, ragged=True)
            tl, ll = big["recordings_mask"].sum(0).astype(int), big["labels_mask"].sum(0).astype(int)
            def sorted_leg(label_len):
                exs = [(big["recordings"][: tl[i], i], numpy.concatenate([big["labels"][: label_len(i) - 1, i] % max(1, dims.V - 1), [dims.cfg["eos_label"]]]))
                       for i in range(global_batch * K)]
                exs = list(Data._sort_k(iter(exs), global_batch * K))
                sb, sframes, shapes = [], 0.0, []
                for k in range(K):
                    pb = Data.pad_batch(exs[k * global_batch: (k + 1) * global_batch], pad_frames_to=32, pad_labels_to=4)
                    sframes += float(pb["recordings_mask"].sum())
                    shapes.append([int(pb["recordings"].shape[0]), int(pb["labels"].shape[0])])
                    sb.append({kk: torch.from_numpy(numpy.ascontiguousarray(v)).to(dev) for kk, v in pb.items()})
                el, _ = timed(trainer, sb, 2 * K, global_batch, 3 * K)      # every shape: eager, captured, replayed once before the clock
                return dict(k=K, minibatch_shapes_TL=shapes, steps=2 * K, ms_per_step=el / (2 * K) * 1e3, real_frames_per_step=sframes / K,
                            value=2 * sframes / el, unit="real frames/s",
                            fraction_of_all_ones_value=(2 * sframes / el) / (frames_per_step * args.steps / elapsed))
            ragged["sort_k_batches"] = sorted_leg(lambda i: int(ll[i]))
            ragged["sort_k_batches"]["labels"] = "L_i ~ U{L/2..L}, independent of the utterance's length (synthetic.make_batch): the decoder's share of a step does not shrink with T"
            # read speech has a roughly constant number of characters per second: label counts proportional to the durations
            ragged["sort_k_batches_proportional_labels"] = sorted_leg(lambda i: max(2, int(round(L * tl[i] / float(T)))))
            ragged["sort_k_batches_proportional_labels"]["labels"] = "L_i = round(L * T_i / T): characters proportional to duration, as in read speech"

    # ---- strong scaling (north_star: global batch 128 = BASELINE configs[2] sharded over the ranks, rank r takes r::N; target >= 6x
    # at 8 GPUs): the same job in the SAME launch as the weak line, and the one-GPU step at that global batch it is measured against
    strong = None
    strong_batches = dict(STRONG_GLOBAL_BATCH, **getattr(backend, "strong_global_batch", {}))
    if (backend.measured or getattr(backend, "strong_leg", False)) and args.full and not args.no_strong and args.scaling == "weak" \
            and args.workload in strong_batches and not args.ragged and not args.frames and not args.batch:
        GB = strong_batches[args.workload]
        if GB % world == 0:
            sb = []
            for k in range(2):
                gbatch = synthetic.make_batch(cfg, GB, T, L, seed=4321 + k)
                sb.append({kk: torch.from_numpy(v).to(dev) for kk, v in synthetic.shard_batch(gbatch, rank, world).items()})
            # (a stand-in backend — the CPU emulator of the launch tests — runs ONE step of each form: the plumbing, not the numbers)
            n_st, n_warm = (max(5, min(args.steps, 10)), 3) if backend.measured else (1, 0)
            el, _ = timed(trainer, sb, n_st, GB, n_warm)
            strong = dict(global_batch=GB, per_gpu_batch=GB // world, steps=n_st, ms_per_step=el / n_st * 1e3,
                          value=GB * T * n_st / el, unit="frames/s", scaling="strong",
                          encoder_kernels=encoder_kernels_of(rec, GB // world, dims))
            def one_gpu_step_ms(passes):
                """The one-GPU step at the global batch, live: rank 0 alone (no collective).  passes=True: the encoder in passes of
                <= 64 utterances on the cluster kernels (the default, bricks.Encoder.PASS_ROWS); False: one pass on the step kernels
                (what round 4 measured as the one-GPU baseline)."""
                keep = rec.encoder.PASS_ROWS
                rec.encoder.PASS_ROWS = keep if passes else 1 << 30
                try:
                    solo = Trainer(rec, distributed=False, **TRAIN_CONF)
                    full = [{kk: torch.from_numpy(v).to(dev) for kk, v in synthetic.make_batch(cfg, GB, T, L, seed=4321 + k).items()} for k in range(2)]
                    for k in range(n_warm):
                        solo.train_step(full[k % 2], global_batch_size=GB)
                    sync()
                    t_a = time.perf_counter()
                    for k in range(n_st):
                        solo.train_step(full[k % 2], global_batch_size=GB)
                    sync()
                    return (time.perf_counter() - t_a) / n_st * 1e3
                finally:
                    rec.encoder.PASS_ROWS = keep
            one = one_steps = None
            if rank == 0 and (world > 1 or GB // world > rec.encoder.PASS_ROWS):
                one = one_gpu_step_ms(True)
                # (a stand-in backend runs no cluster kernels: its two one-GPU forms are the same code — measured once)
                one_steps = one_gpu_step_ms(False) if backend.measured else one
            barrier()
            if rank == 0:
                if one is None:
                    one = one_steps = strong["ms_per_step"]
                strong.update(one_gpu_ms_per_step=min(one, one_steps), speedup_vs_one_gpu=min(one, one_steps) / strong["ms_per_step"],
                              one_gpu_ms_per_step_encoder_in_passes=one, one_gpu_ms_per_step_encoder_step_kernels=one_steps,
                              speedup_vs_one_gpu_encoder_step_kernels=one_steps / strong["ms_per_step"],
                              one_gpu_how="rank 0 alone on the whole global batch (no collective) in this same launch; the speed-up is "
                                          "quoted against the FASTER of the two one-GPU forms (encoder in passes of 64 utterances on the "
                                          "cluster kernels / one pass on the step kernels)")
                if args.workload == "wsj_base":
                    # what a reader of an 8-GPU line should expect (no 8-GPU node was available to the build in any round): the
                    # north_star asks for >= 6x; the step of 16 utterances per GPU is a chain of dependent recurrent steps that does
                    # not shorten with the batch, so the projection from the one-GPU measurements is below it
                    strong.update(north_star_target_at_8_gpus=6.0, projected_speedup_at_8_gpus=4.2,
                                  projection_how="one-GPU step at global batch 128 (encoder in passes, 57.3 ms) / (one-GPU step at 16 "
                                                 "utterances, 13.5 ms + one 20.9 MB all-reduce, 0.3 ms): DESIGN.md section 5; the chain "
                                                 "floor of 16 utterances per GPU (2 x 2 800 recurrent steps x 1.1 us + decoder + "
                                                 "products = 10.8 ms) bounds this mechanism at 5.3x")
    # ---- self-check inputs (all ranks): was any step skipped, did the step replay as a captured graph region
    skipped_local = 1.0 if trainer.step_was_skipped() else 0.0
    regions = list(getattr(rec, "_regions", {}).values())
    graph_local = 1.0 if (args.no_graph or not backend.measured or (regions and any(r.get("seen", 0) >= 3 for r in regions) and not any(r.get("bad") for r in regions))) else 0.0
    if dist:
        t = torch.tensor([skipped_local, 1.0 - graph_local], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(t)
        skipped_total, graph_region_ok = float(t[0]), float(t[1]) == 0.0
    else:
        skipped_total, graph_region_ok = skipped_local, graph_local == 1.0
    # rank r works on utterances r::world of every global minibatch: every rank fingerprints the shard it was
    # actually fed, rank 0 compares with the fingerprints of columns r::world of the global minibatch it generates itself
    import zlib
    def shard_crc(b):
        return zlib.crc32(b"".join(numpy.ascontiguousarray(b[k]).tobytes() for k in ("recordings", "recordings_mask", "labels", "labels_mask")))
    mine = shard_crc({k: v.cpu().numpy() for k, v in staged[0].items()})
    shards_ok = True
    if dist:
        got = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
        torch.distributed.all_gather(got, torch.tensor([mine], dtype=torch.int64, device=dev))
        if rank == 0:
            gb0 = synthetic.make_batch(cfg, global_batch, T, L, seed=1234, ragged=args.ragged)
            shards_ok = all(int(got[r][0]) == shard_crc(synthetic.shard_batch(gb0, r, world)) for r in range(world))
    check_ok = skipped_total == 0 and graph_region_ok and shards_ok and ((not dist) or torch.distributed.get_world_size() == args.gpus)
    rec.generator.check_persistent()
    rec.encoder.check_persistent()          # raises if a persistent cluster kernel gave up waiting (results would be invalid)
    ms = elapsed / args.steps * 1e3
    value = frames_per_step * args.steps / elapsed

    # the exchange step alone: ONE sum all-reduce of the flat gradient bucket (RCCL over xGMI on GPUs), timed back to back
    allreduce_ms = None
    if dist and args.full:
        g = rec.store.grad
        for _ in range(2):
            torch.distributed.all_reduce(g)
        sync()
        barrier()
        ta = time.perf_counter()
        for _ in range(10):
            torch.distributed.all_reduce(g)
        sync()
        allreduce_ms = (time.perf_counter() - ta) / 10 * 1e3
        g.zero_()

    if rank == 0:
        out = dict(metric="encoder+attention+decoder training frames/sec (whole node)", value=value, unit="frames/s",
                   n_gpus=world, steps=args.steps, warmup=args.warmup, ms_per_step=ms, ms_per_step_median=ms_median,
                   higher_is_better=True,
                   scaling=args.scaling, vs_baseline=None, dtype="f32", data="synthetic",
                   config=dict(workload="%s: B=%d utterances x T=%d frames x F=%d fbank per GPU, L=%d labels; %s" % (
                       args.workload, B, T, dims.F, L, "x".join(str(h) for h in dims.Hs) + " BiGRU subsample " +
                       str(dims.subsample) + ", " + cfg["attention_type"] + " attention, %d-unit GRU decoder" % dims.D),
                       global_batch=global_batch, per_gpu_batch=B, frames_per_step=frames_per_step,
                       ragged=bool(args.ragged), parallelism="dp%d" % world, optimizer="clip100+adadelta+maxnorm1",
                       hip_graph=not args.no_graph, priming_steps=PRIME, host_blocks_per_step=bool(rec.lib.sync_after_graph),
                       encoder_kernels=encoder_kernels_of(rec, B, dims),
                       h2d="value: minibatches resident in HBM when the timed region starts (bench contract); with_h2d: the same steps fed from pinned host memory",
                       with_h2d=(dict(with_h2d, value=frames_per_step / (with_h2d["ms_per_step"] * 1e-3)) if with_h2d else None),
                       value_is="steps * frames_per_step / wall time of the K steps (mean); ms_per_step_median = median of the per-step host intervals",
                       final_cost_per_utterance=last_cost / B, knobs=knobs, full=bool(args.full)))
        if sustained:
            out["sustained"] = sustained
        if ragged:
            out["ragged"] = ragged
        if strong:
            out["strong"] = strong
        if dist:
            out["config"].update(overlap_allreduce=bool(args.overlap_allreduce))
            out["config"].update(collective_backend=torch.distributed.get_backend(), collective_world_size=torch.distributed.get_world_size(),
                                 allreduce_ms=allreduce_ms, allreduce_bytes=int(rec.store.grad.numel()) * 4,
                                 whole_step_graph_region=bool(trainer.dp_region))
        # self-check of the run (every rank's verdict, reduced): the collective spans exactly --gpus ranks, the step replays as a
        # whole-step graph region, no step of any rank was skipped by the guard and no cluster launch gave up
        out["self_check"] = dict(ok=bool(check_ok), collective_world_size_is_n_gpus=(not dist) or torch.distributed.get_world_size() == args.gpus,
                                 whole_step_graph_region=bool(graph_region_ok), steps_skipped=int(skipped_total), cluster_aborts=int(trainer.aborts),
                                 rank_r_holds_utterances_r_mod_world=bool(shards_ok),
                                 cluster_reserve=int(rec.lib.get_knob("cluster_reserve")))
        if backend.measured and args.full:
            pr = dominant_kernel_probe(rec, dims, T, B)
            ach = pr["flops"] / pr["launch_s"] / 1e12
            pmc, pmc_why = pmc_record(pr["kernel"] + "@%s" % args.workload) if B == B0 else (None, "PMC record is for the default per-GPU batch")
            # the PMC figure is the mean over the launches of ALL layers; their time steps differ (subsampling): price the
            # algorithmic bytes at the mean number of steps per launch, not at layer 0's
            layer_T, t_ = [], T
            for sub in dims.subsample:
                layer_T.append(t_)
                t_ = (t_ + sub - 1) // sub
            mean_T = sum(layer_T) / float(len(layer_T))
            roof = dict(bound="mfma", kernel=pr["kernel"], achieved=ach, peak=PEAK_FP32_MFMA, unit="TFLOP/s", frac=ach / PEAK_FP32_MFMA,
                        traffic=(pmc["hbm_bytes_per_launch"] if pmc else None), launch_us=pr["launch_s"] * 1e6,
                        us_per_recurrent_step=pr["launch_s"] * 1e6 / pr["steps_per_launch"], flops_per_launch=pr["flops"],
                        algorithmic_bytes_per_launch=pr["algorithmic_bytes"],
                        frac_source="HIP events around the kernel on the recognizer's stream inside this run (layer 0, T steps; rocprofv3 "
                                    "of the same command: profiles/r06_bench_wsj_base_kernel_stats.md)",
                        note="latency bound by construction: a chain of T dependent GRU steps, two cluster-wide exchanges each; the "
                             "contraction runs on the VALU (GEMV per utterance), formally priced against the fp32 MFMA peak")
            if pmc:
                roof.update(traffic_source=pmc.get("source"), traffic_steps_per_launch=mean_T,
                            traffic_algorithmic_bytes=pr["algorithmic_bytes_at"](mean_T),
                            traffic_over_algorithmic=pmc["hbm_bytes_per_launch"] / pr["algorithmic_bytes_at"](mean_T),
                            mfma_busy=pmc.get("mfma_busy"), valu_busy=pmc.get("valu_busy"), wait_frac=pmc.get("wait_frac"),
                            counters_note="valu_busy / wait_frac = SQ_ACTIVE_INST_VALU / SQ_WAIT_ANY over SQ_WAVE_CYCLES: fractions of a "
                                          "resident wave's time; mfma_busy = SQ_VALU_MFMA_BUSY_CYCLES / SQ_BUSY_CYCLES")
            else:
                roof["traffic_note"] = pmc_why
            if args.workload in TRAIN_FLOP_PER_FRAME:
                tf = value / world * TRAIN_FLOP_PER_FRAME[args.workload] / 1e12
                roof.update(whole_step_tflops=tf, whole_step_frac=tf / PEAK_FP32_MFMA)
            roof["dense_gemm"] = gemm_probe(rec, dims, T, B)
            out["roofline"] = roof
            if world == 1 and not args.no_fbank and args.workload == "wsj_base":
                out["fbank"] = fbank_leg(dev)
            if world == 1 and not args.no_decode and args.workload == "wsj_base":
                out["decode"] = decode_leg(dev, args.decode_utterances, batch=args.decode_batch)
                if not args.no_beam200:
                    out["decode"]["beam200"] = beam200_leg(dev)
            if world == 1 and not args.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline(cfg, params, B0, T, L, args.workload)
        print(json.dumps(out), file=json_out, flush=True)
    barrier()
    if dist:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
