"""What a decode chunk costs from waveforms: the hand-written glue of calls that existed before the device front end
(Fbank.batch -> add_deltas_cmvn_batch -> copy to the host -> slices -> SpeechRecognizer.beam_search_batch, which pads on the host and
uploads) against decode.recognize (FrontEnd.batch -> beam_search_staged).  WSJ decode shape: utterances of 4-8 s of 16 kHz PCM,
40 mel + energy with deltas = 123 features, the WSJ-base network with the conditioned weights of tools/bench_decode.py, device FST
language model, beam 16, chunks of 64.  Both paths decode the SAME chunks (decode.recognize_plan), one chunk in flight.

    python tools/measure_recognize.py [--utts 256] [--reps 5] [--out profiles/recognize_wsj.md]

Wall times are host clocks around work that ends in a device synchronise; the two kernels are timed with device events around
repeated launches, next to the bytes their algorithm has to move.  Needs an MI355X."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "attention-lvcsr_amd"), os.path.join(REPO, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy
import torch

SEARCH = dict(char_discount=1.0, round_to_inf=1e9, stop_on="optimistic_future_cost")


def build(device, beam):
    from bench_decode import WSJ_COND_DECODE
    from lvsr_amd import spec, synthetic, lm as LM
    from lvsr_amd.bricks.recognizer import SpeechRecognizer
    cfg = spec.wsj_base(prior=dict(type="window_around_median", before=10, after=100))
    cfg["input_dim"] = 123
    cfg["max_decoded_length_scale"] = 3.0
    rec = SpeechRecognizer(device=device, params=synthetic.make_params(cfg, seed=10, scale=2.0, scales=WSJ_COND_DECODE), net_config=cfg)
    fst, cmap = LM.char_ngram_fst(33, seed=9)
    rec.set_language_model(LM.DeviceFSTLanguageModel(fst, device, nn_char_map=cmap, no_transition_cost=20.0, weight=0.5))
    rec.init_beam_search(beam)
    return rec


def waveforms(n, seed=5):
    """n utterances of 4-8 s: noise under a slow envelope, so that frames differ and the statistics are sound"""
    rng = numpy.random.RandomState(seed)
    out = []
    for _ in range(n):
        m = int(rng.uniform(4.0, 8.0) * 16000)
        env = 1500.0 * (1.0 + 0.9 * numpy.sin(numpy.arange(m) / rng.uniform(2000.0, 9000.0)))
        out.append(numpy.clip(rng.randn(m) * env, -32000, 32000).astype(numpy.int16))
    return out


def glue_features(fe, wavs):
    fb = fe.fbank
    feats, foff = fb.batch(wavs)
    out = fb.add_deltas_cmvn_batch(feats, foff, mean=fe.mean, std=fe.std).cpu().numpy()
    off = foff.cpu().numpy()
    return [out[off[i]: off[i + 1]] for i in range(len(wavs))]


def glue_path(rec, fe, wavs, plan, contexts_only=False):
    results = [None] * len(wavs)
    for chunk in plan:
        recs = glue_features(fe, [wavs[i] for i in chunk])
        if contexts_only:
            with rec._on_stream():
                rec.compute_contexts_batch(recs)
            continue
        for i, r in zip(chunk, rec.beam_search_batch(recs, **SEARCH)):
            results[i] = r
    torch.cuda.synchronize()
    return results


def staged_path(rec, fe, wavs, plan, contexts_only=False):
    from lvsr_amd import decode
    if not contexts_only:
        rows = decode.recognize(rec, fe, wavs, beam_size=rec.beam_size, batch=len(plan[0]), sort=True, **SEARCH)
        torch.cuda.synchronize()
        return rows
    for chunk in plan:
        x, mask, _ = fe.batch([wavs[i] for i in chunk])
        with rec._on_stream():
            rec.compute_contexts_staged(x, mask)
    torch.cuda.synchronize()


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def event_time(fn, reps=50):
    """-> microseconds per call of fn (device events around `reps` launches, after a warm-up)"""
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def kernel_rows(fe, wavs):
    """the two new kernels alone at the chunk shape: (name, shape, microseconds, algorithmic bytes)"""
    from lvsr_amd.frontend import STATS_PARTS
    from lvsr_amd.native import ptr
    lib, dev = fe.lib, fe.device
    feats, foff, nfr = fe._static(wavs)
    n, total, longest, W = len(wavs), int(feats.shape[0]), max(nfr), fe.num_features
    T = (longest + 63) // 64 * 64
    x = torch.empty(T, n, W, device=dev)
    mask = torch.empty(T, n, device=dev)
    us_fb = event_time(lambda: lib.call("lvsr_frontend_batch", lib.stream_for(x), ptr(feats), ptr(foff), n, total, longest, fe.dim, 1,
                                        ptr(fe._mean), ptr(fe._istd), T, ptr(x), ptr(mask)))
    bytes_fb = 4 * (total * fe.dim + T * n * W + T * n)
    packed = fe.fbank.add_deltas_cmvn_batch(feats, foff)
    sums = torch.zeros(2 * W, dtype=torch.float64, device=dev)
    partials = torch.zeros(2 * W * STATS_PARTS, dtype=torch.float64, device=dev)
    us_fs = event_time(lambda: lib.call("lvsr_feature_stats", lib.stream_for(sums), ptr(packed), total, W, ptr(partials), ptr(sums), 1))
    bytes_fs = 4 * total * W
    return [("lvsr_frontend_batch", "%d utterances, %d frames, T = %d, dim %d -> x (%d, %d, %d)" % (n, total, T, fe.dim, T, n, W), us_fb, bytes_fb),
            ("lvsr_feature_stats", "(%d, %d) float32" % (total, W), us_fs, bytes_fs)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--beam", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measure_recognize.py needs an MI355X"
    from lvsr_amd import decode
    from lvsr_amd.frontend import FrontEnd
    dev = torch.device("cuda:0")
    wavs = waveforms(a.utts)
    fe = FrontEnd(device=dev).fit([wavs[i: i + a.batch] for i in range(0, min(len(wavs), 2 * a.batch), a.batch)])
    rec = build(dev, a.beam)
    plan = decode.recognize_plan([len(w) for w in wavs], a.batch, True)
    frames = sum(fe.num_frames(len(w)) for w in wavs)
    # warm-up: workspaces, graphs of every chunk shape, both paths; the two paths must agree before they are compared
    for _ in range(2):
        old = glue_path(rec, fe, wavs, plan)
        new = staged_path(rec, fe, wavs, plan)
    same = sum(1 for o, r in zip(old, new) if (isinstance(o, Exception) and r["recognized"] == []) or
               (not isinstance(o, Exception) and o[0][0] == r["recognized"] and o[1][0] == r["search_cost"]))
    found = sum(1 for o in old if not isinstance(o, Exception))
    wall = {"glue": [], "recognize": []}
    ctx = {"glue": [], "recognize": []}
    for _ in range(a.reps):          # alternating, so that a drift of the machine hits both
        for name, path in (("glue", glue_path), ("recognize", staged_path)):
            wall[name].append(clock(lambda: path(rec, fe, wavs, plan))[0])
            ctx[name].append(clock(lambda: path(rec, fe, wavs, plan, contexts_only=True))[0])
    lines = ["# From waveforms to hypotheses at the WSJ decode shape", "",
             "`python tools/measure_recognize.py --utts %d --batch %d --beam %d --reps %d` on one MI355X: %d utterances of 4-8 s "
             "(%d frames, %.0f per utterance), 123 features, WSJ-base with the conditioned decode weights and the device FST language "
             "model, one chunk of %d in flight, the same chunks on both paths (decode.recognize_plan, sorted by length).  "
             "%d of %d utterances find a hypothesis; best hypothesis and cost equal on both paths for %d of %d."
             % (a.utts, a.batch, a.beam, a.reps, a.utts, frames, frames / float(a.utts), a.batch, found, a.utts, same, a.utts), "",
             "| path | ms per utterance (median of %d) | min .. max | waveforms -> contexts, ms per utterance | search (the rest) |" % a.reps,
             "|---|---|---|---|---|"]
    med = {}
    for name, label in (("glue", "(a) glue: Fbank.batch, add_deltas_cmvn_batch, copy to host, beam_search_batch"),
                        ("recognize", "(b) decode.recognize")):
        w = [t * 1e3 / a.utts for t in wall[name]]
        c = [t * 1e3 / a.utts for t in ctx[name]]
        med[name] = statistics.median(w)
        lines.append("| %s | %.3f | %.3f .. %.3f | %.3f (%.3f .. %.3f) | %.3f |"
                     % (label, med[name], min(w), max(w), statistics.median(c), min(c), max(c), med[name] - statistics.median(c)))
    spread = max(max(wall[k]) - min(wall[k]) for k in wall) * 1e3 / a.utts
    lines += ["", "(b) - (a) = %+.3f ms per utterance; the larger run-to-run spread of the two paths is %.3f.  \"waveforms -> contexts\" is a "
              "run of its own that stops behind the encoder pass (synchronised); \"search\" is the whole minus that." % (med["recognize"] - med["glue"], spread), "",
              "| kernel | shape | us per launch (device events, 50 launches) | algorithmic bytes | GB/s |", "|---|---|---|---|---|"]
    for name, shape, us, nbytes in kernel_rows(fe, [wavs[i] for i in plan[0]]):
        lines.append("| %s | %s | %.1f | %.1f MB | %.0f |" % (name, shape, us, nbytes / 1e6, nbytes / us / 1e3))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
