"""SpeechRecognizer.analyze_batch and the decode driver's batched scoring (decode.search(score_batch=, nll_only=)): a chunk of
utterances scored in one ragged pass with the report's reductions on the device (lvsr_utterance_stats), against the float32 oracle,
against `analyze` of the same recognizer utterance by utterance, and against the per-utterance driver.  Every body runs on the CPU
emulator build and on the GPU."""
import numpy
import pytest
import torch
from numpy.testing import assert_allclose

from lvsr_amd import decode, error_rate as ER, synthetic
from lvsr_amd.bricks.recognizer import SpeechRecognizer

CONTENT = dict(input_dim=5, num_phonemes=6, dims_bidir=[4], dim_dec=5, dim_matcher=6, attention_type="content",
               post_merge_dims=None, embed_outputs=True, data_prepend_eos=False)                  # tests/test_error_rate_decode.py
CONV = dict(input_dim=5, num_phonemes=6, dims_bidir=[4, 4], subsample=[1, 2], dim_dec=5, dim_matcher=6, attention_type="content_and_conv",
            conv_n=2, conv_num_filters=3, post_merge_dims=None, embed_outputs=True, data_prepend_eos=False)
EOS = 5
STD_RTOL, PENALTY_RTOL = 2e-4, 1e-5         # the bars of tests/test_error_rate_decode.py on the reference's fixture


# Two float32 implementations of the same alignment differ by a few units of roundoff per weight (hardware exp and reciprocal on the
# GPU, another summation order at another batch size); the penalty adds up to (L - 1) T' differences of two cumulative sums of such
# weights: some 1e-7 to 1e-6 absolute at these sizes.  The fixture bar of 1e-5 relative is therefore a statement about penalties of
# order one (the fixture's own are 5.9 and 4.8), not about one of 0.03, which is the difference of cumulative sums that nearly
# cancel.  The parameters below give penalties above this on every ground truth, checked on the oracle's own alignments.
WELL_CONDITIONED = 0.5


def _lib(device):
    if device == "cpu":
        from emu import emu_lib
        return emu_lib()
    return None


def utterances():
    rng = numpy.random.RandomState(0)
    frames, labels = (9, 7, 12), ([1, 2, EOS], [3, EOS], [2, 4, 0, EOS])
    return [rng.normal(size=(t, 5)).astype(numpy.float32) for t in frames], [list(l) for l in labels]


# one shorter than its ground truth, one longer, one without
PREDICTIONS = [[1, EOS], [3, 1, 2, EOS], None]


def same_scores(got, cost, weights, cost_rtol):
    """an entry of analyze_batch against a cost vector and, unless `weights` is None, an (L,T') alignment"""
    assert got["length"] == len(cost)
    assert_allclose(got["cost"], float(numpy.asarray(cost, numpy.float64).sum()), rtol=cost_rtol)
    if weights is None:
        return
    assert_allclose(got["weights_std"], ER.weights_std(weights[:, None, :]), rtol=STD_RTOL)
    assert_allclose(got["monotonicity_penalty"], ER.monotonicity_penalty(weights[:, None, :]), rtol=PENALTY_RTOL)


# ---- analyze_batch against the oracle and against analyze ------------------------------------------------------------------
def run_analyze_batch(cfg, device):
    from oracle import lvsr_oracle as O
    params = synthetic.make_params(cfg, seed=1, scale=2.0)          # well-conditioned penalties, see WELL_CONDITIONED
    rec = SpeechRecognizer(device=device, params=params, lib=_lib(device), net_config=cfg)
    orc = O.OracleRecognizer(cfg, params, dtype=torch.float32)
    xs, gts = utterances()
    plain = rec.analyze_batch(xs, gts)
    full = rec.analyze_batch(xs, gts, PREDICTIONS, want_alignments=True)
    assert len(plain) == len(full) == 3
    padded = -(-max(len(x) for x in xs) // 64) * 64
    for i, (x, gt) in enumerate(zip(xs, gts)):
        cost, weights = orc.analyze(x, numpy.asarray(gt))
        Tp = weights.shape[1]
        assert ER.monotonicity_penalty(weights[:, None, :]) > WELL_CONDITIONED
        if cfg is CONV:
            assert Tp != len(x) and Tp != padded and Tp != padded // 2
        for res in (plain, full):
            assert res[i]["groundtruth"]["length"] == len(gt)
            same_scores(res[i]["groundtruth"], cost, weights, 1e-4)
        assert plain[i]["prediction"] is None and set(plain[i]["groundtruth"]) == {"cost", "weights_std", "monotonicity_penalty", "length"}
        g = full[i]["groundtruth"]
        assert g["weights"].shape == g["energies"].shape == (len(gt), Tp)
        assert (g["weights"].argmax(axis=1) == weights.argmax(axis=1)).all()
        pred = PREDICTIONS[i]
        if pred is None:
            assert full[i]["prediction"] is None
            continue
        # the prediction: the same recognizer's analyze(inputs, groundtruth, prediction), which the driver called before
        cost, weights, energies = rec.analyze({"recordings": x}, numpy.asarray(gt), numpy.asarray(pred))
        p = full[i]["prediction"]
        same_scores(p, cost, weights, 1e-5)
        assert p["weights"].shape == p["energies"].shape == (len(pred), Tp)
        assert (p["weights"].argmax(axis=1) == weights.argmax(axis=1)).all()
        assert_allclose(p["energies"], energies, rtol=1e-4, atol=1e-5)
    # an empty prediction counts as none (Theano's scan has no 0-length sequences, lvsr/main.py:816-817); all of them: one pass
    none = rec.analyze_batch(xs, gts, [[], None, []])
    assert all(r["prediction"] is None for r in none)
    assert [r["groundtruth"] for r in none] == [r["groundtruth"] for r in plain]
    with pytest.raises(ValueError):
        rec.analyze_batch(xs, gts[:2])


@pytest.mark.parametrize("cfg", [CONTENT, CONV], ids=["content", "conv_subsample"])
def test_analyze_batch_emulated(cfg):
    run_analyze_batch(cfg, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [CONTENT, CONV], ids=["content", "conv_subsample"])
def test_analyze_batch_gpu(gpu_device, cfg):
    run_analyze_batch(cfg, gpu_device)


def run_analyze_batch_mse(device):
    """mse_gain: the cost of a prediction is measured against the ground truth's rewards, as analyze(inputs, gt, pred) does.  (Costs
    only, here and with the language model: these networks' alignments are deltas, their penalty float32 noise around zero.)"""
    from test_mse_criterion import mse_cfg
    cfg = mse_cfg("mse_gain")
    rec = SpeechRecognizer(device=device, params=synthetic.make_params(cfg, seed=5), lib=_lib(device), net_config=cfg)
    xs, gts = utterances()
    got = rec.analyze_batch(xs, gts, PREDICTIONS)
    differs = []
    for i, (x, gt) in enumerate(zip(xs, gts)):
        cost, weights, _ = rec.analyze({"recordings": x}, numpy.asarray(gt))
        same_scores(got[i]["groundtruth"], cost, None, 1e-5)
        if PREDICTIONS[i] is None:
            assert got[i]["prediction"] is None
            continue
        cost, weights, _ = rec.analyze({"recordings": x}, numpy.asarray(gt), numpy.asarray(PREDICTIONS[i]))
        same_scores(got[i]["prediction"], cost, None, 1e-5)
        total = float(cost.sum())        # (on the emulator `cost` is a view of a workspace buffer: the next call overwrites it)
        own, _, _ = rec.analyze({"recordings": x}, numpy.asarray(PREDICTIONS[i]))
        differs.append(abs(float(own.sum()) - total) > 1e-3 * abs(total))
    assert any(differs)                  # not the cost of a prediction against itself: the ground truth went through


def test_analyze_batch_mse_emulated():
    run_analyze_batch_mse("cpu")


@pytest.mark.gpu
def test_analyze_batch_mse_gpu(gpu_device):
    run_analyze_batch_mse(gpu_device)


def run_analyze_batch_lm(device):
    """with the device language model of tests/test_lm.py's tiny_conv_lm_analyze fixture attached: the fused costs of analyze"""
    from conftest import load_golden
    from lvsr_amd import lm as LM
    z, meta = load_golden("tiny_conv_lm_analyze")
    cfg = meta["cfg"]
    V = cfg["num_phonemes"]
    rec = SpeechRecognizer(device=device, params=synthetic.make_params(cfg, seed=meta["param_seed"], scale=meta["scale"]), lib=_lib(device),
                           net_config=cfg)
    f = LM.ArcFST(start=int(z["arcs"][0][0]))
    for a, b, il, w in z["arcs"]:
        f.add_arc(int(a), int(b), int(il), float(w))
    f.isyms = dict([("<eps>", 0)] + [("c%d" % c, c + 1) for c in range(V)])
    lm_kw = dict(meta["lm"])
    kw = dict(nn_char_map={"c%d" % c: c for c in range(V)}, weight=lm_kw.pop("weight"), no_transition_cost=lm_kw.pop("no_transition_cost"),
              am_beta=lm_kw.pop("am_beta", 1.0), normalize_am_weights=lm_kw.pop("normalize_am_weights", True),
              normalize_lm_weights=lm_kw.pop("normalize_lm_weights", False), normalize_tot_weights=lm_kw.pop("normalize_tot_weights", False))
    # the fixture's two utterances (14 frames each) and the first 9 frames of one of them, with its label sequences
    labels = lambda u, j: [int(t) for t in z["an_u%d_%d_labels" % (u, j)]]
    xs = [z["x0"], z["x1"], z["x0"][:9]]
    gts, preds = [labels(0, 0), labels(1, 0), labels(0, 2)], [labels(0, 1), labels(1, 1), labels(1, 2)]
    without = rec.analyze_batch(xs, gts, preds)
    rec.set_language_model(LM.DeviceFSTLanguageModel(f, device, lib=rec.lib, **kw))
    got = rec.analyze_batch(xs, gts, preds)
    for i, x in enumerate(xs):
        cost, weights, _ = rec.analyze({"recordings": x}, numpy.asarray(gts[i]))
        same_scores(got[i]["groundtruth"], cost, None, 1e-5)
        cost, weights, _ = rec.analyze({"recordings": x}, numpy.asarray(gts[i]), numpy.asarray(preds[i]))
        same_scores(got[i]["prediction"], cost, None, 1e-5)
        assert abs(got[i]["groundtruth"]["cost"] - without[i]["groundtruth"]["cost"]) > 1e-3       # the language model went in


def test_analyze_batch_language_model_emulated():
    run_analyze_batch_lm("cpu")


@pytest.mark.gpu
def test_analyze_batch_language_model_gpu(gpu_device):
    run_analyze_batch_lm(gpu_device)


# ---- the driver ------------------------------------------------------------------------------------------------------------
# 9 and 7 frames search up to 3 and 2 labels; 2 frames: a search limit of 0, no candidate (CandidateNotFoundError)
DRIVER_CFG = dict(CONTENT, max_decoded_length_scale=3)
ROW_KEYS = ("groundtruth_cost", "recognized_cost", "weights_std", "monotonicity_penalty")


def driver_params():
    """(with the weights of tests/test_error_rate_decode.py no hypothesis ever ends; with these two utterances have one, and no
    alignment is a delta, whose penalty would be float32 noise around zero)"""
    return synthetic.make_params(DRIVER_CFG, seed=3, scale=4.0)


def driver_utterances():
    rng = numpy.random.RandomState(0)
    utts = [(rng.normal(size=(9, 5)).astype(numpy.float32), [1, 2, 5]), (rng.normal(size=(7, 5)).astype(numpy.float32), [3, 5])]
    return utts + [(rng.normal(size=(2, 5)).astype(numpy.float32), [4, 5])]


def run_driver(device):
    rec = SpeechRecognizer(device=device, params=driver_params(), lib=_lib(device), net_config=DRIVER_CFG)
    utts = driver_utterances()
    kw = dict(beam_size=3, char_discount=0.3, to_words=lambda ls: ["w%d" % l for l in ls if l != 5])
    seen, seen_batched = [], []
    rep = decode.search(rec, utts, report=seen.append, **kw)
    got = decode.search(rec, utts, batch=2, score_batch=2, report=seen_batched.append, **kw)
    rows, want = got["per_utterance"], rep["per_utterance"]
    assert [r["number"] for r in seen_batched] == [r["number"] for r in seen] == [0, 1, 2]
    assert want[2].get("error") == "CandidateNotFoundError" and want[0]["recognized"] and want[1]["recognized"]
    assert got["cer"] == rep["cer"] and got["wer"] == rep["wer"]
    for a, b in zip(rows, want):
        assert set(a) == set(b)
        for k in ("number", "groundtruth", "recognized", "char_errors", "cer", "word_errors", "wer", "error"):
            assert a.get(k) == b.get(k), k
        assert_allclose(a["search_cost"], b["search_cost"], rtol=1e-5, equal_nan=True)
        assert_allclose(a["groundtruth_cost"], b["groundtruth_cost"], rtol=1e-4)
        if "recognized_cost" in b:
            assert_allclose(a["recognized_cost"], b["recognized_cost"], rtol=1e-4)
        assert_allclose(a["weights_std"], b["weights_std"], rtol=STD_RTOL)
        assert_allclose(a["monotonicity_penalty"], b["monotonicity_penalty"], rtol=PENALTY_RTOL)
    for res in (rep, got):
        assert_allclose(res["nll_groundtruth"], numpy.mean([r["groundtruth_cost"] for r in res["per_utterance"]]), rtol=1e-12)
        assert_allclose(res["nll_recognized"], numpy.mean([r["recognized_cost"] for r in res["per_utterance"] if "recognized_cost" in r]),
                        rtol=1e-12)
    # one utterance at a time inside a scoring chunk, and a chunk larger than the set
    for extra in (dict(score_batch=2), dict(batch=2, score_batch=8)):
        other = decode.search(rec, utts, **dict(kw, **extra))
        assert [r["recognized"] for r in other["per_utterance"]] == [r["recognized"] for r in want]
        assert_allclose([r["groundtruth_cost"] for r in other["per_utterance"]], [r["groundtruth_cost"] for r in want], rtol=1e-4)

    # nll_only: no search is ever started, the rows lack the recognition keys; both scoring modes
    class NoSearch(SpeechRecognizer):
        def init_beam_search(self, beam_size):
            raise AssertionError("nll_only set up a search")

        def beam_search(self, inputs, **kwargs):
            raise AssertionError("nll_only started a search")

        def beam_search_batch(self, recordings, **kwargs):
            raise AssertionError("nll_only started a search")

    deaf = NoSearch(device=device, params=driver_params(), lib=_lib(device), net_config=DRIVER_CFG)
    for extra in (dict(), dict(score_batch=2)):
        seen_nll = []
        nll = decode.search(deaf, utts, nll_only=True, report=seen_nll.append, **dict(kw, **extra))
        assert [r["number"] for r in seen_nll] == [0, 1, 2]
        assert set(nll) == {"per_utterance", "nll_groundtruth"}
        for a, b in zip(nll["per_utterance"], want):
            assert set(a) == {"number", "groundtruth", "groundtruth_cost", "weights_std", "monotonicity_penalty"}
            assert_allclose(a["groundtruth_cost"], b["groundtruth_cost"], rtol=1e-4)
            assert_allclose(a["weights_std"], b["weights_std"], rtol=STD_RTOL)
            assert_allclose(a["monotonicity_penalty"], b["monotonicity_penalty"], rtol=PENALTY_RTOL)
        assert_allclose(nll["nll_groundtruth"], rep["nll_groundtruth"], rtol=1e-4)
    return rec, utts, kw, rep


def parent_rows(rec, utts, beam_size, char_discount, to_words):
    """The rows as the driver built them before it had `score_batch`: search, two `analyze` calls, the host reductions."""
    from lvsr_amd.search import CandidateNotFoundError
    rec.init_beam_search(beam_size)
    rows = []
    for number, (x, gt) in enumerate(utts):
        row = dict(number=number, groundtruth=[int(t) for t in gt])
        try:
            outputs, costs = rec.beam_search({"recordings": x}, char_discount=char_discount, round_to_inf=1e9, stop_on="patience")
            row.update(recognized=outputs[0], search_cost=costs[0])
        except CandidateNotFoundError:
            row.update(recognized=[], search_cost=float("nan"), error="CandidateNotFoundError")
        cost, weights, _ = rec.analyze({"recordings": x}, numpy.asarray(gt))
        row.update(groundtruth_cost=float(cost.sum()), weights_std=float(ER.weights_std(weights[:, None, :])),
                   monotonicity_penalty=float(ER.monotonicity_penalty(weights[:, None, :])))
        if row["recognized"]:
            row["recognized_cost"] = float(rec.analyze({"recordings": x}, numpy.asarray(gt), numpy.asarray(row["recognized"]))[0].sum())
        err = int(ER.edit_distance(row["groundtruth"], row["recognized"]))
        gw, rw = to_words(row["groundtruth"]), to_words(row["recognized"])
        werr = int(ER.edit_distance(gw, rw))
        row.update(char_errors=err, cer=err / float(len(gt)), word_errors=werr, wer=werr / float(max(1, len(gw))))
        rows.append(row)
    return rows


def run_driver_default_path(device):
    """score_batch = 0: the rows are the parent's, bit for bit (same calls in the same order)"""
    rec, utts, kw, rep = run_driver(device)
    want = parent_rows(rec, utts, **kw)
    assert len(rep["per_utterance"]) == len(want)
    for a, b in zip(rep["per_utterance"], want):
        assert list(a) and set(a) == set(b)
        for k in b:
            assert a[k] == b[k] or (k == "search_cost" and numpy.isnan(a[k]) and numpy.isnan(b[k])), k


def test_decode_batched_scoring_emulated():
    run_driver_default_path("cpu")


@pytest.mark.gpu
def test_decode_batched_scoring_gpu(gpu_device):
    run_driver_default_path(gpu_device)
