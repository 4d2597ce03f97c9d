"""Recognising with time stamps: SpeechRecognizer.align_batch / align_staged (one teacher-forced pass, lvsr_alignment_times, one small
copy), decode.recognize(timestamps=True), decode.align, and the host functions decode.token_times / group_words.

align_batch is held to the float64 NumPy reduction of the very alignment it reduced: `analyze_batch(..., want_alignments=True)` makes
the same launches on the same chunk, so the weights it copies out are the kernel's input bit for bit, and the rules are those of
tests/test_alignment_times_kernel.py's random fixtures.  The staged entry point and the drivers are then compared EXACTLY with
align_batch / align_staged on the same features (tests/test_recognize.py shows the staged features are the host path's bit for bit).
The tiny network and front end are those of tests/test_recognize.py.  Bodies run on the CPU emulator and, under `gpu`, on the device."""
import math

import numpy
import pytest
import torch
from numpy.testing import assert_allclose

from lvsr_amd import decode, synthetic
from lvsr_amd.bricks.recognizer import SpeechRecognizer
from lvsr_amd.frontend import FrontEnd

CFG = dict(input_dim=15, num_phonemes=8, dims_bidir=[4, 4], subsample=[1, 2], dim_dec=6, dim_matcher=8,
           attention_type="content_and_conv", conv_n=2, conv_num_filters=2, post_merge_dims=[6],
           post_merge_activation="maxout2", embed_outputs=False, data_prepend_eos=False, max_decoded_length_scale=4)
FBANK = dict(num_mel=4, use_energy=True)          # 5 static coefficients, 15 with deltas
FRAMES = [4, 10, 21, 38, 38]                      # five utterances: chunks of two leave a chunk of one
BEAM, BATCH = 3, 2
SEARCH = dict(char_discount=0.2, round_to_inf=1e9, stop_on="patience")
LABELS = [[1, 2, 7], [], [3, 0, 4, 4, 7], [5, 7], [6, 1, 2, 0, 3, 5, 7]]          # ragged, one empty (a short utterance's)
SHIFT, LENGTH, RATE = 160, 400, 16000.0


def _lib(device):
    if device == "cpu":
        from emu import emu_lib
        return emu_lib()
    from lvsr_amd import native
    return native.get()


def waveform(frames, i, rng):
    n = LENGTH + SHIFT * (frames - 1) + (37 * i) % SHIFT          # `frames` frames, with samples to spare behind the last one
    t = numpy.arange(n)
    amp = 300.0 * (1 + i) * (1.0 + 0.8 * numpy.sin(t / (150.0 + 40 * i)))
    return numpy.clip(rng.randn(n) * amp, -32000, 32000).astype(numpy.int16)


_made = {}


def setup(device):
    """-> dict(wavs, fe: the fitted front end, rec, stacked: a recognizer with dec_stack = 2, feats: host features), once per device"""
    key = str(device)
    if key in _made:
        return _made[key]
    lib = _lib(device)
    rng = numpy.random.RandomState(11)
    wavs = [waveform(f, i, rng) for i, f in enumerate(FRAMES)]
    fe = FrontEnd(device=device, lib=lib, fbank=FBANK)
    assert fe.num_features == 15 and [fe.num_frames(len(w)) for w in wavs] == FRAMES
    fe.fit([wavs[:2], wavs[2:]])
    rec = SpeechRecognizer(device=device, params=synthetic.make_params(CFG, seed=7, scale=2.0), lib=lib, net_config=CFG)
    rec.init_beam_search(BEAM)
    x, _, lengths = fe.batch(wavs)
    host = x.cpu().numpy()
    feats = [host[:n, i].copy() for i, n in enumerate(lengths)]
    _made[key] = dict(wavs=wavs, fe=fe, rec=rec, lib=lib, feats=feats)
    return _made[key]


def duration(frames):
    return ((frames - 1) * SHIFT + LENGTH) / RATE


# ---- the kernel test's rules, on alignments the network made ------------------------------------------------------------------------
def check_rows(rows8, W, lo, hi, what):
    """rows8 (L,8) against the float64 reduction of W (L,n) float32: peak and weight exact, moments within the bound of two float64
    summation orders, total within the float32 summation bound, quantile positions by the acceptance rule (module docstring of
    tests/test_alignment_times_kernel.py) -> how many positions differ from the float64 model's own"""
    L, n = W.shape
    assert rows8.shape == (L, 8) and rows8.dtype == numpy.float64, what
    U23, U52 = 2.0 ** -23, 2.0 ** -52
    differ = 0
    t = numpy.arange(n, dtype=numpy.float64)
    for l in range(L):
        g, w32 = rows8[l], W[l]
        w64 = w32.astype(numpy.float64)
        assert g[0] == int(numpy.argmax(w32)) and g[1] == float(w32.max()), (what, l, g)
        e1, e2 = (w64 * t).sum(), (w64 * t * t).sum()
        gam = n * U52
        assert abs(g[2] - e1) <= gam * e1, (what, l)
        x, d = max(e2 - e1 * e1, 0.0), 5 * gam * e2
        assert abs(g[3] - math.sqrt(x)) <= (d / math.sqrt(x) if x >= d and x > 0 else math.sqrt(d)) + 2 * U52 * math.sqrt(x), (what, l)
        C = numpy.cumsum(w64)
        assert abs(g[6] - C[-1]) <= n * U23 * C[-1], (what, l)
        tol = n * U23 * C[-1]
        for slot, q in ((4, lo), (5, hi)):
            k, thr = int(g[slot]), float(numpy.float32(q)) * C[-1]
            assert g[slot] == k and 0 <= k < n
            assert C[k] >= thr - tol and (k == 0 or C[k - 1] < thr + tol), (what, l, slot, k)
            differ += k != int(numpy.argmax(C >= thr))
        assert g[4] <= g[5]
    return differ


def run_align_batch(device, cfg):
    s = setup(device)
    feats = s["feats"]
    stacked = cfg is not CFG
    rec = SpeechRecognizer(device=device, params=synthetic.make_params(cfg, seed=7, scale=2.0), lib=s["lib"], net_config=cfg) if stacked else s["rec"]
    lo, hi = 0.1, 0.9
    # one analyze_batch call makes both passes: its ground-truth pass is align_batch's over `full` (every utterance has labels), its
    # prediction pass — over the gathered columns that have one — align_batch's over LABELS, whose second sequence is empty
    full = [l if l else [2, 7] for l in LABELS]
    ref = rec.analyze_batch(feats, full, [l or None for l in LABELS], want_alignments=True)
    differ = 0
    if not stacked:
        got = rec.align_batch(feats, full)
        for i, (rows8, r) in enumerate(zip(got, ref)):
            W = r["groundtruth"]["weights"]
            assert W.shape == (len(full[i]), rec.d.subsampled_length(FRAMES[i]))
            differ += check_rows(rows8, W, lo, hi, ("full", i))
            # float64 sums of at most seven float32 costs in two orders
            assert_allclose(rows8[:, 7].sum(), r["groundtruth"]["cost"], rtol=1e-14)
            if i in (0, 4):
                # `analyze` is the pass at batch 1 without padding: another float32 summation order.  Its logits (of order 1 to 10 here)
                # carry a few units of 2^-24 relative, 1e-6 absolute, and cost = logsumexp - logit inherits that absolutely: 1e-5, the
                # relative bar tests/test_decode_batched_scoring.py holds the summed costs to, on costs of order one
                cost = rec.analyze({"recordings": feats[i]}, numpy.asarray(full[i]))[0]
                assert_allclose(rows8[:, 7], cost.astype(numpy.float64), rtol=1e-5, atol=1e-5)
    got = rec.align_batch(feats, LABELS, quantiles=(0.25, 0.5))
    assert [g.shape for g in got] == [(len(l), 8) for l in LABELS] and got[1].dtype == numpy.float64
    for i, (rows8, r) in enumerate(zip(got, ref)):
        if LABELS[i]:
            differ += check_rows(rows8, r["prediction"]["weights"], 0.25, 0.5, ("ragged", i))
            assert_allclose(rows8[:, 7].sum(), r["prediction"]["cost"], rtol=1e-14)
    if not stacked:
        # a chunk of one; nothing but empty sequences; no utterance at all
        one = rec.align_batch(feats[2:3], LABELS[2:3])
        ref = rec.analyze_batch(feats[2:3], LABELS[2:3], want_alignments=True)
        differ += check_rows(one[0], ref[0]["groundtruth"]["weights"], lo, hi, "one")
        assert [g.shape for g in rec.align_batch(feats[:2], [[], []])] == [(0, 8), (0, 8)] and rec.align_batch([], []) == []
        with pytest.raises(ValueError, match="3 recordings, 2 label sequences"):
            rec.align_batch(feats[:3], LABELS[:2])
        with pytest.raises(ValueError, match="quantiles"):
            rec.align_batch(feats[:2], LABELS[:2], quantiles=(0.9, 0.1))
    print("%d quantile positions differ from the float64 model's" % differ)


def test_align_batch_emulated():
    run_align_batch("cpu", CFG)


def test_align_batch_stacked_decoder_emulated():
    run_align_batch("cpu", dict(CFG, dec_stack=2))


@pytest.mark.gpu
def test_align_batch_gpu(gpu_device):
    run_align_batch(gpu_device, CFG)


@pytest.mark.gpu
def test_align_batch_stacked_decoder_gpu(gpu_device):
    run_align_batch(gpu_device, dict(CFG, dec_stack=2))


# ---- align_staged = align_batch on the same features ----------------------------------------------------------------------------------
def same_arrays(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def run_align_staged(device):
    s = setup(device)
    fe, rec, wavs, feats = s["fe"], s["rec"], s["wavs"], s["feats"]
    want = rec.align_batch(feats, LABELS)
    x, mask, lengths = fe.batch(wavs)
    staged_names = []
    rec._t = lambda t, dtype, name: staged_names.append(name) or SpeechRecognizer._t(rec, t, dtype, name)
    try:
        got = rec.align_staged(x, mask, lengths, LABELS)
    finally:
        del rec._t
    assert same_arrays(got, want)
    assert "recordings" not in staged_names and "recordings_mask" not in staged_names          # the features are read where they are
    # refusals, in front of any launch
    calls = []
    lib = s["lib"]
    lib.call = lambda name, *a: calls.append(name) or type(lib).call(lib, name, *a)
    try:
        with pytest.raises(ValueError, match="align_staged: x must be a contiguous float32"):
            rec.align_staged(x.double(), mask, lengths, LABELS)
        with pytest.raises(ValueError, match="align_staged: 5 features per frame"):
            rec.align_staged(x[:, :, :5].contiguous(), mask, lengths, LABELS)
        with pytest.raises(ValueError, match="align_staged: mask"):
            rec.align_staged(x, mask[:, :4].contiguous(), lengths, LABELS)
        with pytest.raises(ValueError, match="5 utterances, 5 lengths, 4 label sequences"):
            rec.align_staged(x, mask, lengths, LABELS[:4])
        with pytest.raises(ValueError, match="quantiles"):
            rec.align_staged(x, mask, lengths, LABELS, quantiles=(-0.1, 0.5))
        if torch.device(device).type != "cpu":
            with pytest.raises(ValueError, match="lives on cpu"):
                rec.align_staged(x.cpu(), mask, lengths, LABELS)
        # contexts of other tensors are not reused
        rec.compute_contexts_staged(x, mask)
        del calls[:]
        with pytest.raises(ValueError, match="reuse_contexts"):
            rec.align_staged(x.clone(), mask, lengths, LABELS, reuse_contexts=True)
        assert calls == []
    finally:
        del lib.call
    assert same_arrays(rec.align_staged(x, mask, lengths, LABELS, reuse_contexts=True), want)


def test_align_staged_emulated():
    run_align_staged("cpu")


@pytest.mark.gpu
def test_align_staged_gpu(gpu_device):
    run_align_staged(gpu_device)


# ---- decode.recognize(timestamps=True) -------------------------------------------------------------------------------------------
def same_value(a, b):
    return a == b or (isinstance(a, float) and a != a and b != b)


def run_recognize(device):
    s = setup(device)
    fe, rec, wavs = s["fe"], s["rec"], s["wavs"]
    boundary = {0, 7}
    to_text = lambda labels: "".join(chr(97 + t) for t in labels)
    plain = decode.recognize(rec, fe, wavs, beam_size=BEAM, batch=BATCH, to_text=to_text, **SEARCH)
    timed = decode.recognize(rec, fe, wavs, beam_size=BEAM, batch=BATCH, to_text=to_text, timestamps=True, quantiles=(0.2, 0.8),
                             word_boundary=boundary, **SEARCH)
    plan = decode.recognize_plan([len(w) for w in wavs], BATCH, True)
    assert [len(c) for c in plan] == [2, 2, 1]
    assert all("tokens" not in r and "words" not in r for r in plain)
    for a, b in zip(plain, timed):
        assert set(b) == set(a) | {"tokens", "words"} and all(same_value(a[k], b[k]) for k in a), (a, b)
    found = 0
    for chunk in plan:
        x, mask, lengths = fe.batch([wavs[i] for i in chunk])
        rows8 = rec.align_staged(x, mask, lengths, [timed[i]["recognized"] for i in chunk], quantiles=(0.2, 0.8))
        for i, r8 in zip(chunk, rows8):
            row = timed[i]
            want = decode.token_times(r8, row["recognized"], [1, 2], SHIFT, LENGTH, RATE, FRAMES[i])
            assert row["tokens"] == want and len(row["tokens"]) == len(row["recognized"]), (i, row["tokens"], want)
            assert row["words"] == decode.group_words(want, boundary)
            for tok in row["tokens"]:
                assert 0.0 <= tok["start"] <= tok["end"] <= duration(FRAMES[i]) and 0.0 < tok["confidence"] <= 1.0
                assert 0.0 < tok["peak"] <= duration(FRAMES[i])
            found += bool(row["recognized"])
    assert found >= 3
    # no candidate: an utterance of two frames may not emit a single label (int(2 / 4) = 0), next to one that may
    rng = numpy.random.RandomState(5)
    rows = decode.recognize(rec, fe, [("none", waveform(2, 1, rng)), ("some", wavs[3])], beam_size=BEAM, batch=BATCH, timestamps=True,
                            word_boundary=boundary, **SEARCH)
    assert rows[0]["error"] == "CandidateNotFoundError" and rows[0]["recognized"] == [] and rows[0]["tokens"] == [] and rows[0]["words"] == []
    assert "error" not in rows[1] and len(rows[1]["tokens"]) == len(rows[1]["recognized"]) > 0


def test_recognize_timestamps_emulated():
    run_recognize("cpu")


@pytest.mark.gpu
def test_recognize_timestamps_gpu(gpu_device):
    run_recognize(gpu_device)


# ---- decode.align ---------------------------------------------------------------------------------------------------------------
def run_align(device):
    s = setup(device)
    fe, rec, wavs = s["fe"], s["rec"], s["wavs"]
    named = [("utt%d" % i, w) for i, w in enumerate(wavs)]
    by_order = {}
    for sort in (True, False):
        rows = decode.align(rec, fe, named, LABELS, batch=BATCH, word_boundary={0, 7}, sort=sort)
        by_order[sort] = rows
        assert [r["id"] for r in rows] == [n for n, _ in named] and [r["num_frames"] for r in rows] == FRAMES
        assert [[t["label"] for t in r["tokens"]] for r in rows] == LABELS
        for chunk in ([] if sort else decode.recognize_plan([len(w) for w in wavs], BATCH, sort)):
            x, mask, lengths = fe.batch([wavs[i] for i in chunk])
            for i, r8 in zip(chunk, rec.align_staged(x, mask, lengths, [LABELS[i] for i in chunk])):
                want = decode.token_times(r8, LABELS[i], [1, 2], SHIFT, LENGTH, RATE, FRAMES[i])
                assert rows[i]["tokens"] == want and rows[i]["words"] == decode.group_words(want, {0, 7})
                assert rows[i]["cost"] == float(r8[:, 7].sum())
        assert rows[1]["tokens"] == [] and rows[1]["cost"] == 0.0 and rows[1]["words"] == []
    # another chunking pads otherwise: another float32 order in the encoder, the same costs to the bar of run_align_batch
    assert_allclose([r["cost"] for r in by_order[True]], [r["cost"] for r in by_order[False]], rtol=1e-5, atol=1e-5)
    assert "words" not in decode.align(rec, fe, wavs[:1], LABELS[:1])[0]
    with pytest.raises(ValueError, match="5 waveforms, 4 transcripts"):
        decode.align(rec, fe, named, LABELS[:4])
    with pytest.raises(ValueError, match="'short'.*fewer than one frame"):
        decode.align(rec, fe, [("ok", wavs[1]), ("short", wavs[0][:399])], LABELS[:2])
    with pytest.raises(ValueError, match="5 features per frame, the recognizer takes 15"):
        decode.align(rec, FrontEnd(device=device, lib=s["lib"], fbank=FBANK, deltas=False), wavs[:2], LABELS[:2])


def test_align_emulated():
    run_align("cpu")


@pytest.mark.gpu
def test_align_gpu(gpu_device):
    run_align(gpu_device)


# ---- token_times and group_words: host arithmetic --------------------------------------------------------------------------------
def planted(peak, start, end, cost):
    return [peak, 0.5, peak + 0.25, 1.0, start, end, 1.0, cost]


def test_token_times():
    rows = [planted(0, 0, 1, 0.0), planted(3, 2, 4, math.log(4.0)), planted(9, 9, 9, 1.0)]
    # subsample [1, 2]: a position is two frames of 10 ms; 19 frames last (18 * 160 + 400) / 16000 = 0.205 s
    toks = decode.token_times(rows, [4, 0, 7], [1, 2], 160, 400, 16000.0, 19)
    assert [t["label"] for t in toks] == [4, 0, 7]
    assert_allclose([t["start"] for t in toks], [0.0, 0.04, 0.18], rtol=1e-12)
    assert_allclose([t["end"] for t in toks], [0.04, 0.10, 0.20], rtol=1e-12)
    assert_allclose([t["peak"] for t in toks], [0.01, 0.07, 0.19], rtol=1e-12)
    assert_allclose([t["confidence"] for t in toks], [1.0, 0.25, math.exp(-1.0)], rtol=1e-12)
    # subsample [2, 2]: four frames; position 9 would end at 0.40 s and peak at 0.38 s, the utterance (37 frames) ends at 0.385 s
    toks = decode.token_times(rows, [4, 0, 7], [2, 2], 160, 400, 16000.0, 37)
    assert_allclose([t["start"] for t in toks], [0.0, 0.08, 0.36], rtol=1e-12)
    assert_allclose([t["end"] for t in toks], [0.08, 0.20, 0.385], rtol=1e-12)
    assert_allclose([t["peak"] for t in toks], [0.02, 0.14, 0.38], rtol=1e-12)
    # clipped harder: 34 frames end at 0.355 s, inside position 8 — start, peak and end of the last token all stop there
    toks = decode.token_times(rows, [4, 0, 7], [2, 2], 160, 400, 16000.0, 34)
    assert toks[2]["start"] == toks[2]["peak"] == toks[2]["end"] == (33 * 160 + 400) / 16000.0
    # an mse criterion's cost is a squared error: no confidence
    toks = decode.token_times(rows, [4, 0, 7], [1, 2], 160, 400, 16000.0, 19, mse=True)
    assert all(set(t) == {"label", "start", "end", "peak"} for t in toks)
    assert decode.token_times(numpy.zeros((0, 8)), [], [1, 2], 160, 400, 16000.0, 19) == []
    with pytest.raises(ValueError, match="3 rows for 2 labels"):
        decode.token_times(rows, [4, 0], [1, 2], 160, 400, 16000.0, 19)


def test_group_words():
    SPACE, EOS = 0, 7
    tok = lambda label, start, end, conf=None: dict(dict(label=label, start=start, end=end, peak=(start + end) / 2),
                                                    **({} if conf is None else {"confidence": conf}))
    # leading, doubled and trailing boundaries
    seq = [tok(SPACE, 0.0, 0.1, 0.9), tok(3, 0.1, 0.2, 0.8), tok(4, 0.2, 0.3, 0.5), tok(SPACE, 0.3, 0.4, 0.9), tok(SPACE, 0.4, 0.5, 0.9),
           tok(5, 0.5, 0.6, 0.7), tok(SPACE, 0.6, 0.7, 0.2), tok(EOS, 0.7, 0.8, 0.1)]
    assert decode.group_words(seq, {SPACE, EOS}) == [dict(labels=[3, 4], start=0.1, end=0.3, confidence=0.5),
                                                     dict(labels=[5], start=0.5, end=0.6, confidence=0.7)]
    # no boundary at all: one word; boundaries only, nothing: no word
    assert decode.group_words(seq[1:3], {SPACE, EOS}) == [dict(labels=[3, 4], start=0.1, end=0.3, confidence=0.5)]
    assert decode.group_words(seq, set()) == [dict(labels=[0, 3, 4, 0, 0, 5, 0, 7], start=0.0, end=0.8, confidence=0.1)]
    assert decode.group_words([seq[0], seq[3]], {SPACE}) == [] and decode.group_words([], {SPACE}) == []
    # tokens of an mse criterion carry no confidence: neither do the words
    bare = [tok(3, 0.1, 0.2), tok(SPACE, 0.2, 0.3), tok(4, 0.3, 0.5), tok(5, 0.5, 0.6)]
    assert decode.group_words(bare, [SPACE]) == [dict(labels=[3], start=0.1, end=0.2), dict(labels=[4, 5], start=0.3, end=0.6)]
