#!/usr/bin/env python3
"""Cost of the decode report (lvsr_amd.decode.search as a whole: search + scoring of ground truth and best hypothesis), which
tools/bench_decode.py leaves out: wall clock around `decode.search` on WSJ-base with beam 16 and the device FST language model of
tools/bench_decode.build, over synthetic utterances (800 frames, ground truths of about 100 labels), one warm-up run discarded.

    python tools/measure_decode_report.py --legs default                      # batch=64, utterance-by-utterance scoring
    python tools/measure_decode_report.py --legs default,batched              # ... and batch=64, score_batch=64
    python tools/measure_decode_report.py --tree <checkout of another commit> --legs default --json a.json
    python tools/measure_decode_report.py --legs default,batched --before a.json --out profiles/r09_decode_report.md

`--tree`: import the package (and its built library) from another checkout — the parent commit's, for the leg "the same arguments
before this change"; `--before` puts that run's JSON next to this one's in the record.  Also times lvsr_utterance_stats alone
(HIP events) at the shapes of a scoring chunk.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--legs", default="default,batched")
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--labels", type=int, default=100)
    ap.add_argument("--beam", type=int, default=16)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--conditioned", action="store_true", help="the parameter scales of the full-size decode fixtures (long hypotheses)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--before", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path[:0] = [tree, os.path.join(tree, "attention-lvcsr_amd"), os.path.join(tree, "tools")]

    import numpy
    import torch
    import bench_decode
    from lvsr_amd import decode
    assert torch.cuda.is_available(), "this measurement needs an MI355X"
    dev = torch.device("cuda:0")
    rec, cfg = bench_decode.build(dev, args.beam, conditioned=args.conditioned)
    eos, V = rec.eos_label, cfg["num_phonemes"]
    utts = []
    for i in range(args.utts):
        rng = numpy.random.RandomState(1234 + i)
        x = rng.normal(size=(args.frames, 40)).astype(numpy.float32)
        n = args.labels + int(rng.randint(-10, 11))
        labels = [int(t) for t in rng.randint(0, V, size=n - 1)]
        utts.append((x, [t if t != eos else (t + 1) % V for t in labels] + [eos]))
    kw = dict(beam_size=args.beam, char_discount=1.0, round_to_inf=1e9, stop_on="optimistic_future_cost", batch=args.batch)
    leg_kw = dict(default={}, batched=dict(score_batch=args.batch))
    result = dict(tree=tree, utterances=args.utts, frames=args.frames, labels=args.labels, beam=args.beam, batch=args.batch,
                  conditioned=bool(args.conditioned), legs={})
    for leg in [l for l in args.legs.split(",") if l]:
        times = []
        for r in range(args.repeats + 1):                    # the first run is the warm-up: workspaces, captured graphs
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rep = decode.search(rec, utts, **dict(kw, **leg_kw[leg]))
            torch.cuda.synchronize()
            if r:
                times.append(time.perf_counter() - t0)
        rows = rep["per_utterance"]
        result["legs"][leg] = dict(seconds=times, median=float(numpy.median(times)), ms_per_utterance=1e3 * float(numpy.median(times)) / args.utts,
                                   cer=rep["cer"], hypotheses=sum(1 for r in rows if r["recognized"]),
                                   mean_hypothesis_length=float(numpy.mean([len(r["recognized"]) for r in rows])),
                                   mean_groundtruth_cost=float(numpy.mean([r["groundtruth_cost"] for r in rows])))
        print(json.dumps({leg: result["legs"][leg]}), flush=True)
    # the search alone (no scoring), for the share of the report
    if "batched" in result["legs"]:
        times = []
        for r in range(args.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(0, len(utts), args.batch):
                rec.beam_search_batch([u[0] for u in utts[i:i + args.batch]], char_discount=1.0, round_to_inf=1e9, stop_on="optimistic_future_cost")
            torch.cuda.synchronize()
            if r:
                times.append(time.perf_counter() - t0)
        result["search_only"] = dict(seconds=times, median=float(numpy.median(times)), ms_per_utterance=1e3 * float(numpy.median(times)) / args.utts)
        print(json.dumps(dict(search_only=result["search_only"])), flush=True)
        # lvsr_utterance_stats alone, HIP events: a chunk's alignment (L+1, B, T') with the ground truths' ragged mask
        from lvsr_amd import observables as OBS
        L, B, Tp = args.labels + 10, args.batch, args.frames // int(numpy.prod(rec.cfg["subsample"]))
        W = torch.softmax(torch.randn(L + 1, B, Tp, device=dev), dim=2)
        lens = torch.tensor([len(u[1]) for u in utts[:B]], device=dev)
        mask = (torch.arange(L, device=dev)[:, None] < lens[None, :]).float().contiguous()
        costs, out = torch.rand(L, B, device=dev), torch.zeros(B, 4, dtype=torch.float64, device=dev)
        lengths = torch.full((B,), Tp, dtype=torch.int32, device=dev)
        call = lambda: OBS.utterance_stats(rec.lib, W[1:], mask, costs, out, rec.ws, lengths=lengths)
        for _ in range(5):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(200):
            call()
        e1.record()
        torch.cuda.synchronize()
        result["utterance_stats_us"] = dict(L=L, B=B, Tp=Tp, us_per_call=1e3 * e0.elapsed_time(e1) / 200)
        print(json.dumps(dict(utterance_stats_us=result["utterance_stats_us"])), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    if args.out:
        before = json.load(open(args.before)) if args.before else None
        with open(args.out, "w") as f:
            f.write(record(result, before))


def record(now, before):
    legs = now["legs"]
    lines = ["# The decode report as a whole: search + scoring (tools/measure_decode_report.py)", "",
             "WSJ-base, beam %d, device FST language model (tools/bench_decode.build%s), %d synthetic utterances x %d frames, ground truths of "
             "about %d labels; wall clock around `decode.search`, one warm-up run discarded, %d timed runs per leg, one MI355X."
             % (now["beam"], ", conditioned weights" if now["conditioned"] else "", now["utterances"], now["frames"], now["labels"],
                len(next(iter(legs.values()))["seconds"])), "",
             "| leg | seconds (median) | runs | ms per utterance | hypotheses | mean hypothesis length |", "|---|---|---|---|---|---|"]

    def row(name, leg):
        lines.append("| %s | %.3f | %s | %.3f | %d | %.1f |" % (name, leg["median"], ", ".join("%.3f" % s for s in leg["seconds"]),
                                                              leg["ms_per_utterance"], leg["hypotheses"], leg["mean_hypothesis_length"]))
    a = before["legs"].get("default") if before else None
    if a:
        row("(a) batch=%d, scoring per utterance, parent commit" % now["batch"], a)
    if "default" in legs:
        row("(b) the same arguments, this commit", legs["default"])
    if "batched" in legs:
        row("(c) batch=%d, score_batch=%d" % (now["batch"], now["batch"]), legs["batched"])
    lines.append("")
    if "search_only" in now:
        s = now["search_only"]
        lines += ["The searches alone (`beam_search_batch` over the same chunks, no scoring): %.3f s (%s), %.3f ms per utterance."
                  % (s["median"], ", ".join("%.3f" % t for t in s["seconds"]), s["ms_per_utterance"]), ""]
    if a and "batched" in legs:
        lines += ["(a) / (c) = %.2f." % (a["median"] / legs["batched"]["median"])
                  + (" (b) / (a) = %.3f." % (legs["default"]["median"] / a["median"]) if "default" in legs else ""), ""]
    if "utterance_stats_us" in now:
        u = now["utterance_stats_us"]
        lines += ["`lvsr_utterance_stats` alone (both kernels, HIP events over 200 calls) on L = %d, B = %d, T' = %d: %.1f us per call."
                  % (u["L"], u["B"], u["Tp"], u["us_per_call"]), ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
