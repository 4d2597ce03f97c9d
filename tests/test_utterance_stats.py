"""lvsr_utterance_stats (csrc/observables.hip): the decode report's per-utterance reductions — summed cost, weights_std,
monotonicity_penalty, label count — against what the reference's own expressions wrote (tests/golden/misc_reference.npz) and against
the float64 host functions of lvsr_amd.error_rate taken per column.  Every body runs on the CPU emulator build and on the GPU."""
import math

import numpy
import pytest
import torch
from numpy.testing import assert_allclose

from conftest import golden_path
from lvsr_amd import error_rate as ER
from lvsr_amd import native
from lvsr_amd import observables as OBS
from lvsr_amd.params import Workspace

U = 2.0 ** -24                     # unit roundoff of float32
U64 = 2.0 ** -53                   # ... of float64


def _lib(device):
    if device == "cpu":
        from emu import emu_lib
        return emu_lib()
    return native.get()


def call(lib, device, w, mask, costs, lengths=None, pad=3):
    """weights as the rows [1:] of an (L+1,B,T'+pad) buffer: ldw > T', the row in front of label 0 and the tail of every row are
    poisoned (NaN), so reading either shows"""
    L, B, Tp = w.shape
    full = torch.full((L + 1, B, Tp + pad), float("nan"), device=device)
    full[1:, :, :Tp] = torch.from_numpy(w)
    dev = lambda a, dt: None if a is None else torch.from_numpy(numpy.ascontiguousarray(a, dtype=dt)).to(device)
    out = torch.full((B, 4), 7.0, dtype=torch.float64, device=device)
    OBS.utterance_stats(lib, full[1:, :, :Tp], dev(mask, numpy.float32), dev(costs, numpy.float32), out, Workspace(torch.device(device)),
                        lengths=dev(lengths, numpy.int32))
    return out.cpu().numpy()


def restatement(w, mask, costs, lengths=None):
    """(B,4) from lvsr_amd.error_rate on every column alone, cut to the utterance's attended length, in float64"""
    L, B, Tp = w.shape
    m = numpy.ones((L, B)) if mask is None else mask.astype(numpy.float64)
    out = numpy.zeros((B, 4))
    for b in range(B):
        n = Tp if lengths is None else int(lengths[b])
        col, mb = w[:, b:b + 1, :n], m[:, b:b + 1]
        out[b] = [0.0 if costs is None else (mb[:, 0] * costs[:, b].astype(numpy.float64)).sum(), ER.weights_std(col, mb) * L,
                  ER.monotonicity_penalty(col, mb), mb.sum()]
    return out


# ---- test 1: the reference's own values -------------------------------------------------------------------------------------
def test_host_functions_per_utterance_add_up_to_the_reference():
    """the per-column sums of the float64 host functions are the reference's totals at the fixture bars: the restatement the kernel
    is held to below stays within them on its own"""
    z = numpy.load(golden_path("misc_reference"), allow_pickle=False)
    w, m = z["expr_weights"], z["expr_mask"]
    L = w.shape[0]
    plain, masked = restatement(w, None, None), restatement(w, m, None)
    assert_allclose(plain[:, 1].sum() / L, z["weights_std"], rtol=2e-4)
    assert_allclose(masked[:, 1].sum() / L, z["weights_std_masked"], rtol=2e-4)
    assert_allclose(plain[:, 2].sum(), z["monotonicity_penalty"], rtol=1e-5)
    assert_allclose(masked[:, 2].sum(), z["monotonicity_penalty_masked"], rtol=1e-5)


def run_golden(lib, device):
    z = numpy.load(golden_path("misc_reference"), allow_pickle=False)
    w, m = z["expr_weights"].astype(numpy.float32), z["expr_mask"].astype(numpy.float32)
    assert w.shape == (6, 3, 9) and 0 < m.sum() < m.size
    L = w.shape[0]
    plain, masked = call(lib, device, w, None, None), call(lib, device, w, m, None)
    assert_allclose(plain[:, 1].sum() / L, z["weights_std"], rtol=2e-4)
    assert_allclose(masked[:, 1].sum() / L, z["weights_std_masked"], rtol=2e-4)
    assert_allclose(plain[:, 2].sum(), z["monotonicity_penalty"], rtol=1e-5)
    assert_allclose(masked[:, 2].sum(), z["monotonicity_penalty_masked"], rtol=1e-5)
    assert (plain[:, 3] == L).all() and (masked[:, 3] == m.sum(axis=0)).all()
    assert (plain[:, 0] == 0).all()


def test_utterance_stats_reference_golden_emulated():
    run_golden(_lib("cpu"), "cpu")


@pytest.mark.gpu
def test_utterance_stats_reference_golden_gpu(gpu_device):
    run_golden(_lib(gpu_device), gpu_device)


# ---- test 2: against the float64 restatement, per utterance -----------------------------------------------------------------
def bounds(w, mask, lengths):
    """Worst-case deviation of the kernel from the float64 restatement, per utterance -> (std (B,), penalty (B,)).
    Penalty (float32, u = 2^-24), as tests/test_observables.py derives it for lvsr_alignment_stats: a scanned prefix of values that
    sum to at most 1 carries six rounded additions of the 64-lane scan, one for the carry, and the carry went through ceil(n/64)
    chunks: c = 7 + ceil(n/64) roundings of values <= 1.  A term max(C1 - C0, 0): both prefixes (2 c u) and the subtraction (u).  A row
    folds n such terms, each <= 1, with ceil(n/64) lane-strided additions and the six of the xor tree: (ceil(n/64) + 6) u n more.  So
    a row is off by at most n (3 c + 1) u.  Rows are converted to float64 exactly and added in float64: L u64 |total| more.
    Moments (float64, u64 = 2^-53) on both sides: a sum of n products in any order is off by at most (n + 1) u64 times the sum of
    the magnitudes, so E2 by g E2 and E1^2 by (2 g + u64) E1^2 <= 3 g E2 (E1^2 <= E2 for weights that sum to at most 1 + n u),
    g = (n + 1) u64; with the subtraction the radicand x is off by d <= 5 g E2 on each side, 10 g E2 between the two.
    |sqrt(max(x + d, 0)) - sqrt(x)| <= d / sqrt(x) where x >= d and <= sqrt(d) elsewhere; the square root itself and the float64
    additions of the rows: 2 L u64 |total|."""
    L, B, Tp = w.shape
    std, pen = numpy.zeros(B), numpy.zeros(B)
    for b in range(B):
        n = Tp if lengths is None else int(lengths[b])
        chunks = -(-n // 64)
        c = 7 + chunks
        pos = numpy.arange(n, dtype=numpy.float64)
        for l in range(L):
            if mask is not None and mask[l, b] == 0:
                continue
            if l >= 1:
                pen[b] += n * (3 * c + 1) * U
            a = w[l, b, :n].astype(numpy.float64)
            e1, e2 = (a * pos).sum(), (a * pos * pos).sum()
            x, d = max(e2 - e1 * e1, 0.0), 10 * (n + 1) * U64 * e2
            std[b] += d / math.sqrt(x) if x >= d and x > 0 else math.sqrt(d)
    return std, pen


def ragged_case(rng, L, B, Tp, null_mask, with_lengths):
    """Dirichlet rows (concentration 0.3: peaked, as alignments are) over each utterance's own attended length; behind it the
    buffer holds garbage when `with_lengths` (the kernel must not read it), zeros otherwise (what the attention writes)."""
    lengths = rng.randint(max(1, Tp // 2), Tp + 1, size=B)
    lengths[0] = Tp
    w = numpy.full((L, B, Tp), 0.25 if with_lengths else 0.0, numpy.float32)
    for b in range(B):
        w[:, b, :lengths[b]] = rng.dirichlet(numpy.full(lengths[b], 0.3), size=L)
    mask = None
    if not null_mask:
        mask = numpy.zeros((L, B), numpy.float32)
        for b in range(B):
            mask[: rng.randint(1, L + 1), b] = 1
        mask[:, 0] = 1
        mask[1:, B - 1] = 0              # one utterance of a single label: no penalty row
    return w, mask, lengths


SHAPES = [(L, 3, Tp) for L in (1, 5) for Tp in (9, 64, 65, 130)]


def run_case(lib, device, shape, with_costs):
    L, B, Tp = shape
    for with_lengths in (False, True):
        rng = numpy.random.RandomState(100 * L + Tp + int(with_costs))
        w, mask, lengths = ragged_case(rng, L, B, Tp, False, with_lengths)
        if not with_lengths:
            lengths = None
        costs = (rng.gamma(2.0, 2.0, size=(L, B))).astype(numpy.float32) if with_costs else None
        # a masked row reads nothing: poison its weights and its cost
        w[mask == 0] = numpy.nan
        if costs is not None:
            costs[mask == 0] = numpy.nan
        got = call(lib, device, w, mask, costs, lengths)
        w_clean, c_clean = numpy.nan_to_num(w), None if costs is None else numpy.nan_to_num(costs)
        want = restatement(w_clean, mask, c_clean, lengths)
        std_bound, pen_bound = bounds(w_clean, mask, lengths)
        scale = 2 * L * U64
        for b in range(B):
            print("%s lengths=%s b=%d: cost %.9g / %.9g, std %.12g (deviation %.3g, bound %.3g), penalty %.9g (deviation %.3g, bound %.3g), "
                  "labels %g" % (shape, with_lengths, b, got[b, 0], want[b, 0], got[b, 1], abs(got[b, 1] - want[b, 1]),
                                 std_bound[b] + scale * want[b, 1], got[b, 2], abs(got[b, 2] - want[b, 2]),
                                 pen_bound[b] + scale * want[b, 2], got[b, 3]))
        assert numpy.isfinite(got).all()
        # sums of at most five float32 values (times a mask of zeros and ones) in float64: exact whatever the order
        assert got[:, 0].tobytes() == want[:, 0].tobytes() and got[:, 3].tobytes() == want[:, 3].tobytes()
        assert (numpy.abs(got[:, 1] - want[:, 1]) <= std_bound + scale * want[:, 1]).all()
        assert (numpy.abs(got[:, 2] - want[:, 2]) <= pen_bound + scale * want[:, 2]).all()
        assert (got[:, 3] == mask.sum(axis=0)).all() and len(set(got[:, 3])) > 1 or L == 1
        if L == 1:
            assert (got[:, 2] == 0).all()
        else:
            assert got[0, 2] > 0 and got[0, 1] > 0
        if with_costs:
            assert (got[:, 0] > 0).all()
        else:
            assert (got[:, 0] == 0).all()
        again = call(lib, device, w, mask, costs, lengths)
        assert got.tobytes() == again.tobytes()


@pytest.mark.parametrize("with_costs", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_utterance_stats_emulated(shape, with_costs):
    run_case(_lib("cpu"), "cpu", shape, with_costs)


@pytest.mark.gpu
@pytest.mark.parametrize("with_costs", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_utterance_stats_gpu(gpu_device, shape, with_costs):
    run_case(_lib(gpu_device), gpu_device, shape, with_costs)


def test_utterance_stats_argument_checks():
    lib = _lib("cpu")
    w = torch.zeros(2, 1, 4)
    out = torch.zeros(1, 4, dtype=torch.float64)
    part = torch.zeros(6, dtype=torch.float64)
    p = native.ptr
    for args in [(None, 4, 2, 1, 4, None, None, None, p(part), p(out)),              # null weights
                 (p(w), 3, 2, 1, 4, None, None, None, p(part), p(out)),             # ldw < T'
                 (p(w), 4, 0, 1, 4, None, None, None, p(part), p(out)),             # L = 0
                 (p(w), 4, 2, 1, 4, None, None, None, p(part), None)]:              # null out
        with pytest.raises(native.NativeError):
            lib.call("lvsr_utterance_stats", lib.stream_for(out), *args)
