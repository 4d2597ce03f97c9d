"""The host side of the beam search (lvsr_amd/search.py, bricks/beam_state.py): which library entry points a whole search
issues, position by position; that a generator serves one search set at a time and says so; that a search in pieces is the
search in one call; the shape of `last_stats`.  The kernels themselves are pinned in test_beam_kernels.py."""
import pytest

from conftest import load_golden
from emu import emu_lib
from lvsr_amd import lm as LM
from lvsr_amd import synthetic
from lvsr_amd.bricks.recognizer import SpeechRecognizer
from lvsr_amd.search import CandidateNotFoundError

BEAM = 3


def _recognizer(case, device="cpu", lib=None):
    """-> (recognizer, the utterances of the fixture's ragged batch)."""
    z, meta = load_golden(case)
    params = synthetic.make_params(meta["cfg"], seed=meta["param_seed"], scale=meta["scale"])
    batch = synthetic.make_batch(meta["cfg"], meta["B"], meta["T"], meta["L"], seed=meta["batch_seed"], ragged=meta["ragged"])
    rec = SpeechRecognizer(device=device, params=params, lib=emu_lib() if lib is None and device == "cpu" else lib, net_config=meta["cfg"])
    rec.init_beam_search(BEAM)
    lens = [int(batch["recordings_mask"][:, u].sum()) for u in range(meta["B"])]
    assert len(set(lens)) > 1
    return rec, [batch["recordings"][:tl, u] for u, tl in enumerate(lens)]


def _with_device_lm(rec):
    fst, cmap = LM.char_ngram_fst(rec.d.V, seed=5)
    rec.set_language_model(LM.DeviceFSTLanguageModel(fst, rec.device, lib=rec.lib, nn_char_map=cmap, no_transition_cost=20.0, weight=0.5))
    return rec


def record_calls(rec, search):
    """Names of the entry points `search()` issues through the recognizer's library, in order."""
    lib, names = rec.lib, []

    def call(name, *args):
        names.append(name)
        return type(lib).call(lib, name, *args)
    lib.call = call
    try:
        search()
    finally:
        del lib.call
    return names


def split_positions(names):
    """-> (what runs before the first position, the launches of one position, how often they repeat to the end)."""
    first = names.index("lvsr_attdec_fwd")                       # pass A of position 0: nothing before the search uses the step kernel
    last = names.index("lvsr_beam_compact", first) + 1           # the launch that ends every position
    position, tail = names[first:last], names[first:]
    assert len(tail) % len(position) == 0 and tail == position * (len(tail) // len(position)), "positions differ"
    return names[:first], position, len(tail) // len(position)


# ---- the launches of a search: literals recorded from the code before the state object existed ----------------------------------
# two BiGRU layers, `preprocess`, the packed decoder weights | one layer (tiny_content_embed)
BEFORE = ['lvsr_pack_b_many', 'lvsr_copy2d_many', 'lvsr_sgemm', 'lvsr_bigru_fwd', 'lvsr_copy2d_many', 'lvsr_sgemm', 'lvsr_bigru_fwd',
          'lvsr_sgemm', 'lvsr_copy2d_many', 'lvsr_pack_b_many']
BEFORE_ONE_LAYER = ['lvsr_pack_b_many', 'lvsr_copy2d_many', 'lvsr_sgemm', 'lvsr_bigru_fwd', 'lvsr_sgemm', 'lvsr_copy2d_many', 'lvsr_pack_b_many']
MERGE_PACKS, LM_INITIAL = ['lvsr_pack_b_many'], ['lvsr_fst_lm_step']
CASES = {            # name: (before the first position, the launches of a position, positions launched)
    'single': (BEFORE, ['lvsr_attdec_fwd', 'lvsr_readout_step', 'lvsr_beam_select', 'lvsr_attdec_fwd', 'lvsr_beam_compact'], 13),
    'batch_of_one': (BEFORE + MERGE_PACKS,
                     ['lvsr_attdec_fwd', 'lvsr_readout_merge', 'lvsr_readout_step', 'lvsr_beam_select', 'lvsr_attdec_fwd', 'lvsr_beam_compact'], 13),
    'batch_of_three': (BEFORE + MERGE_PACKS,
                       ['lvsr_attdec_fwd', 'lvsr_readout_merge', 'lvsr_readout_step', 'lvsr_beam_select', 'lvsr_attdec_fwd', 'lvsr_beam_compact'], 13),
    'device_lm': (BEFORE + LM_INITIAL,
                  ['lvsr_attdec_fwd', 'lvsr_readout_step', 'lvsr_beam_select', 'lvsr_attdec_fwd', 'lvsr_fst_lm_step', 'lvsr_beam_compact'], 13),
    'device_lm_batch': (BEFORE + MERGE_PACKS + LM_INITIAL,
                        ['lvsr_attdec_fwd', 'lvsr_readout_merge', 'lvsr_readout_step', 'lvsr_beam_select', 'lvsr_attdec_fwd',
                         'lvsr_fst_lm_step_groups', 'lvsr_beam_compact'], 13),
    'lookup_feedback': (BEFORE_ONE_LAYER,
                        ['lvsr_attdec_fwd', 'lvsr_readout_step', 'lvsr_beam_select', 'lvsr_gather_rows', 'lvsr_sgemm', 'lvsr_sgemm',
                         'lvsr_attdec_fwd', 'lvsr_beam_compact'], 9),
    'stacked': (BEFORE,
                ['lvsr_attdec_fwd', 'lvsr_readout_step', 'lvsr_beam_select', 'lvsr_gather_rows', 'lvsr_gather_rows', 'lvsr_gather_rows',
                 'lvsr_gather_rows', 'lvsr_attdec_fwd', 'lvsr_attdec_fwd', 'lvsr_copy2d_many', 'lvsr_attdec_fwd', 'lvsr_beam_compact'], 13),
}


def _finds_nothing(rec, x):
    with pytest.raises(CandidateNotFoundError):
        rec.beam_search({"recordings": x})


def _case(name):
    if name == "single":
        rec, xs = _recognizer("tiny_conv_median")
        return rec, lambda: rec.beam_search({"recordings": xs[0]})
    if name == "batch_of_one":
        rec, xs = _recognizer("tiny_conv_median")
        return rec, lambda: rec.beam_search_batch(xs[:1])
    if name == "batch_of_three":
        rec, xs = _recognizer("tiny_conv_median")
        return rec, lambda: rec.beam_search_batch(xs)
    if name == "device_lm":
        rec, xs = _recognizer("tiny_conv_median")
        return _with_device_lm(rec), lambda: rec.beam_search({"recordings": xs[0]})
    if name == "device_lm_batch":
        rec, xs = _recognizer("tiny_conv_median")
        return _with_device_lm(rec), lambda: rec.beam_search_batch(xs[:2])
    if name == "lookup_feedback":
        rec, xs = _recognizer("tiny_content_embed")
        return rec, lambda: _finds_nothing(rec, xs[0])            # (as in the reference: the fixture records the error)
    if name == "stacked":
        rec, xs = _recognizer("tiny_conv_stack2")
        return rec, lambda: rec.beam_search({"recordings": xs[0]})
    raise KeyError(name)


CASE_NAMES = ["single", "batch_of_one", "batch_of_three", "device_lm", "device_lm_batch", "lookup_feedback", "stacked"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_a_search_issues_the_same_launches(name):
    rec, search = _case(name)
    before, position, count = split_positions(record_calls(rec, search))
    want_before, want_position, want_count = CASES[name]
    assert position == want_position
    assert before == want_before
    assert count == want_count


# ---- a generator serves one search set at a time, and an older one is refused ---------------------------------------------------
def run_refusal(device, lib):
    rec, xs = _recognizer("tiny_conv_median", device, lib)
    bs = rec._beam_search
    limits = [int(x.shape[0] / rec.max_decoded_length_scale) for x in xs]
    want = rec.beam_search({"recordings": xs[1]})
    a = bs.begin({"recordings": xs[0][:, None, :]}, rec.eos_label, limits[0], ignore_first_eol=rec.data_prepend_eos)
    bs.advance(a, 3, wait=True)
    b = bs.begin({"recordings": xs[1][:, None, :]}, rec.eos_label, limits[1], ignore_first_eol=rec.data_prepend_eos)
    with pytest.raises(RuntimeError, match="another search"):
        bs.advance(a, 3, wait=True)
    with pytest.raises(RuntimeError, match="another search"):
        bs.finish(a)
    with pytest.raises(RuntimeError, match="another search"):
        a.state.steps(1)
    while not bs.advance(b, 3, wait=True):
        pass
    outs, costs = bs.finish(b)
    assert [[int(t) for t in o] for o in outs] == want[0] and [float(c) for c in costs] == want[1]


def test_an_older_search_is_refused_and_the_newer_one_is_not_disturbed_emulated():
    run_refusal("cpu", None)


@pytest.mark.gpu
def test_an_older_search_is_refused_and_the_newer_one_is_not_disturbed_gpu(gpu_device):
    run_refusal(gpu_device, None)


# ---- the pieces are the whole; `last_stats` has one shape ---------------------------------------------------------------------
STAT_KEYS = {"positions", "finished", "done", "reused"}


def _check_stats(stats, n):
    per = stats["per_utterance"]
    assert len(per) == n and all(set(u) == STAT_KEYS and all(type(v) is int for v in u.values()) for u in per)
    assert stats["positions"] == max(u["positions"] for u in per) and stats["reused"] == sum(u["reused"] for u in per)
    assert all(0 < u["positions"] and u["done"] != 0 for u in per)


def test_search_in_pieces_equals_search_and_last_stats_has_one_shape():
    rec, xs = _recognizer("tiny_conv_median")
    bs = rec._beam_search
    limits = [int(x.shape[0] / rec.max_decoded_length_scale) for x in xs]
    whole = bs.search({"recordings": xs[0][:, None, :]}, rec.eos_label, limits[0], ignore_first_eol=rec.data_prepend_eos)
    stats = dict(bs.last_stats)
    _check_stats(stats, 1)
    assert stats["finished"] == stats["per_utterance"][0]["finished"] > 0 and stats["done"] == stats["per_utterance"][0]["done"]
    run = bs.begin({"recordings": xs[0][:, None, :]}, rec.eos_label, limits[0], ignore_first_eol=rec.data_prepend_eos)
    while not bs.advance(run, 3, wait=True):
        pass
    pieces = bs.finish(run)
    assert pieces[0] == whole[0] and pieces[1] == whole[1]              # tokens and costs, exactly
    assert bs.last_stats == stats
    one = bs.search_batch(xs[:1], rec.eos_label, limits[:1], ignore_first_eol=rec.data_prepend_eos)
    _check_stats(bs.last_stats, 1)
    assert len(one) == 1 and one[0][0] == whole[0]
    three = bs.search_batch(xs, rec.eos_label, limits, ignore_first_eol=rec.data_prepend_eos)
    _check_stats(bs.last_stats, 3)
    assert len(three) == 3 and three[0][0] == whole[0]
    assert len(set(u["positions"] for u in bs.last_stats["per_utterance"])) > 1, "the scenario needs searches of different lengths"
