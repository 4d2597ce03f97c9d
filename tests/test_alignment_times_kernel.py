"""lvsr_alignment_times (csrc/observables.hip) called directly, against a float64 NumPy model of its contract (include/lvsr_hip.h).

Buffers: `out` sits between guard bands of a NaN bit pattern and is filled with it first; the weights behind each utterance's
attended length n_b, every weight of a masked row and the costs of rows that must not be read hold a NaN pattern too.  Every output
must be finite and the guards untouched: a row that was not written and a read of padding both show.

Exact fixtures: weights that are multiples of 2^-10 and sum to 1 (one-hot rows, two equal peaks, a plateau, mass on the last
position, multinomial counts): every float32 partial sum is exact whatever its order, so the peak, its weight, both quantile
positions and the total must equal the model EXACTLY; the moments (sums of exact float64 products, exact as well) to 1e-12 relative,
which leaves room for the one rounding of E1^2 — fused into the subtraction or not — because the fixtures keep E1^2 below 2000 times
the variance (asserted on the fixtures).

Random fixtures: float32 softmax rows, sharp and flat.  Peak and weight exact; the moments within n 2^-52 sum |terms|, the bound any
two float64 summation orders of exact terms meet (tests/test_frontend_kernels.py), carried through the square root as
tests/test_utterance_stats.py carries it; the total within n 2^-23 sum w of the float64 sum; a quantile position k is accepted iff
C64[k] >= thr - tol and (k == 0 or C64[k-1] < thr + tol), C64 the float64 running sum, thr = q C64[n-1], tol = n 2^-23 C64[n-1] (the
float32 summation bound, doubled for the rounded threshold product).  That rule is no hiding place: the rows whose position differs
from the float64 model's own may be at most 1 % of a case's random rows, and a plain NumPy float32 `cumsum` model must stay within
that share on the same rows.  Observed, on the emulator and on the device alike: 0 of the 576 quantile positions of every T' differ
from the float64 model's (0 %), and 0 of NumPy's float32 `cumsum` model's.

The bodies run on the CPU emulator (same sources) and, under the `gpu` marker, on the device."""
import itertools
import math

import numpy
import pytest
import torch

from lvsr_amd import observables as OBS
from lvsr_amd.native import NativeError, ptr

GUARD = 64                               # doubles of pattern in front of and behind `out`
PATTERN64 = 0x7FF8A5A5A5A5A5A5           # NaNs no kernel computes
PATTERN32 = 0x7FC5A5A5
TPS = [1, 2, 63, 64, 65, 129, 200]       # below, at and above one wave; a second and a fourth chunk
QUANTILES = [(0.1, 0.9), (0.5, 0.5), (0.0, 1.0)]


def _lib(device):
    if device == "cpu":
        from emu import emu_lib
        return emu_lib()
    from lvsr_amd import native
    return native.get()


def layouts(Tp):
    """(L, B, ldw, lengths or None, with_mask, with_costs): 4 rows per work-group do not divide 15; ldw > T' is a strided view"""
    for L, B, pad, ragged, with_mask, with_costs in itertools.product((1, 3), (1, 5), (0, 7), (False, True), (False, True), (False, True)):
        if not ragged:
            yield L, B, Tp + pad, None, with_mask, with_costs
        elif B == 5:
            yield L, B, Tp + pad, [Tp, 0, 1, max(1, Tp // 2), max(1, Tp - 1)], with_mask, with_costs
        else:
            for n in (0, 1, Tp):
                yield L, B, Tp + pad, [n], with_mask, with_costs


def make_mask(L, B):
    """zero rows, among them a whole zero column"""
    m = numpy.ones((L, B), numpy.float32)
    m[:, B - 1] = 0
    if L > 1:
        m[L - 1, 0] = 0
    if B > 1:
        m[0, 1 % B] = 0
    return m


def exact_row(rng, n, kind):
    """multiples of 2^-10 that sum to 1 over n positions"""
    w = numpy.zeros(n, numpy.float32)
    kind = kind % 6
    if n == 1 or kind == 0:                                  # one-hot, anywhere
        w[rng.randint(n)] = 1.0
    elif kind == 1:                                          # mass on the last position alone
        w[n - 1] = 1.0
    elif kind == 2:                                          # two equal peaks, apart: the tie goes to the smaller index
        p = rng.randint(0, max(1, n // 4))
        w[p] = w[n - 1 - rng.randint(0, max(1, n // 4))] = 0.5
        if w.sum() != 1.0:                                   # (n = 2 or 3: both draws met)
            w[:] = 0
            w[0] = w[n - 1] = 0.5
    elif kind == 3:                                          # a plateau of equal weights
        k = 1 << min(3, int(math.log2(n)))
        p = rng.randint(0, min(n - k, 8) + 1)
        w[p: p + k] = 1.0 / k
    elif kind == 4:                                          # most of the mass on the last position
        w[0], w[n - 1] = 0.25, 0.75
    else:                                                    # counts of 1024 draws (ties and zeros occur)
        w[:] = rng.multinomial(1024, rng.dirichlet(numpy.full(n, 0.5))) / 1024.0
    assert w.sum(dtype=numpy.float64) == 1.0 and ((w * 1024) == numpy.round(w * 1024)).all()
    return w


def random_row(rng, n, kind):
    """a float32 softmax row, sharp (an alignment that has formed) or flat (one that has not)"""
    e = rng.randn(n) * (8.0 if kind % 2 == 0 else 0.05)
    p = numpy.exp(e - e.max())
    return (p / p.sum()).astype(numpy.float32)


def make_case(rng, L, B, Tp, lengths, mask, with_costs, row_maker):
    """-> weights (L,B,T') with NaN pattern wherever the kernel must not read, costs (L,B) likewise or None"""
    w = numpy.full((L, B, Tp), numpy.nan, numpy.float32)
    w.view(numpy.uint32)[:] = PATTERN32
    costs = None
    if with_costs:
        costs = numpy.empty((L, B), numpy.float32)
        costs.view(numpy.uint32)[:] = PATTERN32
    for l in range(L):
        for b in range(B):
            n = Tp if lengths is None else lengths[b]
            if (mask is not None and mask[l, b] == 0) or n == 0:
                continue
            w[l, b, :n] = row_maker(rng, n, l * B + b + rng.randint(6))
            if with_costs:
                costs[l, b] = rng.gamma(2.0, 2.0)
    return w, costs


def call(lib, device, w, ldw, mask, costs, lengths, lo, hi):
    """-> (L,B,8) float64; the guards of `out` are checked here"""
    L, B, Tp = w.shape
    full = torch.full((L, B, ldw), PATTERN32, dtype=torch.int32).view(torch.float32)
    full[:, :, :Tp] = torch.from_numpy(w)
    full = full.to(device)
    dev = lambda a, dt: None if a is None else torch.from_numpy(numpy.ascontiguousarray(a, dtype=dt)).to(device)
    n = L * B * 8
    whole = torch.full((n + 2 * GUARD,), PATTERN64, dtype=torch.int64, device=device).view(torch.float64)
    out = whole[GUARD: GUARD + n].view(L, B, 8)
    OBS.alignment_times(lib, full[:, :, :Tp], dev(mask, numpy.float32), dev(costs, numpy.float32), out, lengths=dev(lengths, numpy.int32),
                        lo=lo, hi=hi)
    host = whole.cpu().numpy()
    bits = host.view(numpy.uint64)
    assert (bits[:GUARD] == PATTERN64).all() and (bits[GUARD + n:] == PATTERN64).all(), "a store outside `out`"
    got = host[GUARD: GUARD + n].reshape(L, B, 8).copy()
    assert numpy.isfinite(got).all(), "an unwritten row, or a read of padding / of a masked row"
    return got


def first_reaching(C, thr):
    return int(numpy.argmax(C >= thr))


def live_rows(L, B, Tp, mask, lengths):
    for l in range(L):
        for b in range(B):
            n = Tp if lengths is None else lengths[b]
            yield l, b, n, not ((mask is not None and mask[l, b] == 0) or n == 0)


# ---- exact fixtures ---------------------------------------------------------------------------------------------------------------
def run_exact(device, Tp):
    lib = _lib(device)
    rng = numpy.random.RandomState(1000 + Tp)
    checked = 0
    for (L, B, ldw, lengths, with_mask, with_costs), (lo, hi) in zip(layouts(Tp), itertools.cycle(QUANTILES)):
        mask = make_mask(L, B) if with_mask else None
        w, costs = make_case(rng, L, B, Tp, lengths, mask, with_costs, exact_row)
        got = call(lib, device, w, ldw, mask, costs, lengths, lo, hi)
        for l, b, n, live in live_rows(L, B, Tp, mask, lengths):
            g = got[l, b]
            if not live:
                assert (g == 0).all() and not numpy.signbit(g).any(), (l, b, g)
                continue
            w32 = w[l, b, :n]
            w64, t = w32.astype(numpy.float64), numpy.arange(n, dtype=numpy.float64)
            C = numpy.cumsum(w64)                                                # exact: multiples of 2^-10 up to 1
            assert C[-1] == 1.0
            e1, e2 = (w64 * t).sum(), (w64 * t * t).sum()                        # exact: multiples of 2^-10 below 2^16
            var = e2 - e1 * e1
            assert var == 0 or e1 * e1 <= 2000 * var, "an ill-conditioned fixture: 1e-12 would not cover the rounding of E1^2"
            thr = [numpy.float32(numpy.float32(q) * numpy.float32(C[-1])) for q in (lo, hi)]
            want = [int(numpy.argmax(w32)), float(w32.max()), e1, math.sqrt(max(var, 0.0)), first_reaching(C, thr[0]),
                    first_reaching(C, thr[1]), 1.0, float(costs[l, b]) if with_costs else 0.0]
            for k in (0, 1, 4, 5, 6, 7):
                assert g[k] == want[k], (Tp, L, B, ldw, lengths, l, b, k, g, want)
            for k in (2, 3):
                assert abs(g[k] - want[k]) <= 1e-12 * abs(want[k]), (Tp, L, B, l, b, k, g[k], want[k])
            assert g[4] <= g[5] <= n - 1
            if lo == 0.0:
                assert g[4] == 0
            if hi == 1.0:
                assert g[5] == numpy.nonzero(w32)[0][-1]                         # where the last of the mass sits
            checked += 1
    assert checked > 0


@pytest.mark.parametrize("Tp", TPS)
def test_exact_fixtures_emulated(Tp):
    run_exact("cpu", Tp)


@pytest.mark.gpu
@pytest.mark.parametrize("Tp", TPS)
def test_exact_fixtures_gpu(gpu_device, Tp):
    run_exact(gpu_device, Tp)


def test_ties_go_to_the_smaller_index_across_lanes_and_chunks():
    """equal maxima in one lane's two chunks (t, t + 64), in two lanes of a chunk, and on both ends of the row"""
    lib = _lib("cpu")
    for Tp, places in ((200, (70, 134)), (200, (134, 70, 198)), (65, (64, 0)), (129, (128, 63)), (64, (63, 31))):
        w = numpy.zeros((1, 1, Tp), numpy.float32)
        for p in places:
            w[0, 0, p] = 1.0 / 4
        rest = [t for t in range(2, Tp) if t not in places][: int(round((1.0 - w.sum()) * 16))]
        w[0, 0, rest] = 1.0 / 16                                                  # the rest of the mass, in pieces smaller than a peak
        assert w.sum() == 1.0
        got = call(lib, "cpu", w, Tp, None, None, None, 0.1, 0.9)
        assert got[0, 0, 0] == min(places) and got[0, 0, 1] == 0.25, (Tp, places, got)


# ---- random fixtures --------------------------------------------------------------------------------------------------------------
def run_random(device, Tp):
    lib = _lib(device)
    rng = numpy.random.RandomState(2000 + Tp)
    U23, U52 = 2.0 ** -23, 2.0 ** -52
    rows, differ, differ32 = 0, 0, 0
    for L, B, ldw, lengths, with_mask, with_costs in layouts(Tp):
        lo, hi = 0.1, 0.9
        mask = make_mask(L, B) if with_mask else None
        w, costs = make_case(rng, L, B, Tp, lengths, mask, with_costs, random_row)
        got = call(lib, device, w, ldw, mask, costs, lengths, lo, hi)
        if ldw > Tp and with_mask:                                               # two runs: the same bits
            assert got.tobytes() == call(lib, device, w, ldw, mask, costs, lengths, lo, hi).tobytes()
        for l, b, n, live in live_rows(L, B, Tp, mask, lengths):
            g = got[l, b]
            if not live:
                assert (g == 0).all(), (l, b, g)
                continue
            w32 = w[l, b, :n]
            w64, t = w32.astype(numpy.float64), numpy.arange(n, dtype=numpy.float64)
            assert g[0] == int(numpy.argmax(w32)) and g[1] == float(w32.max()), (Tp, L, B, l, b, g)
            assert g[7] == (float(costs[l, b]) if with_costs else 0.0)
            # moments: exact terms, two float64 orders
            e1, e2 = (w64 * t).sum(), (w64 * t * t).sum()
            gam = n * U52
            assert abs(g[2] - e1) <= gam * e1, (Tp, l, b, g[2], e1)
            # E2 is off by gam E2, E1^2 by (2 gam + gam^2) E1^2 <= 2.5 gam E2 (E1^2 <= (sum w) E2, sum w <= 1 + n 2^-24), the
            # subtraction's roundings on both sides by 2^-52 E2 <= gam E2: the radicand x by d <= 5 gam E2, and
            # |sqrt(max(x + d, 0)) - sqrt(x)| <= d / sqrt(x) where x >= d, <= sqrt(d) elsewhere; the roots' own roundings on top
            x, d = max(e2 - e1 * e1, 0.0), 5 * gam * e2
            bound3 = (d / math.sqrt(x) if x >= d and x > 0 else math.sqrt(d)) + 2 * U52 * math.sqrt(x)
            assert abs(g[3] - math.sqrt(x)) <= bound3, (Tp, l, b, g[3], math.sqrt(x), bound3)
            # the total and the quantile positions
            C = numpy.cumsum(w64)
            assert abs(g[6] - C[-1]) <= n * U23 * C[-1], (Tp, l, b, g[6], C[-1])
            tol = n * U23 * C[-1]
            C32 = numpy.cumsum(w32, dtype=numpy.float32)                         # the plain float32 model the seeds are chosen against
            for slot, q in ((4, lo), (5, hi)):
                k, thr = int(g[slot]), float(numpy.float32(q)) * C[-1]
                assert g[slot] == k and 0 <= k < n
                assert C[k] >= thr - tol and (k == 0 or C[k - 1] < thr + tol), (Tp, l, b, slot, k, C[k], thr, tol)
                differ += k != first_reaching(C, thr)
                differ32 += first_reaching(C32, numpy.float32(numpy.float32(q) * C32[-1])) != first_reaching(C, thr)
                rows += 1
            assert g[4] <= g[5]
    print("T' = %d: %d of %d quantile positions differ from the float64 model's (NumPy's float32 cumsum: %d)" % (Tp, differ, rows, differ32))
    assert rows > 0 and differ32 <= 0.01 * rows, "the fixtures themselves leave the 1 % share: choose other seeds"
    assert differ <= 0.01 * rows, (differ, rows)


@pytest.mark.parametrize("Tp", TPS)
def test_random_fixtures_emulated(Tp):
    run_random("cpu", Tp)


@pytest.mark.gpu
@pytest.mark.parametrize("Tp", TPS)
def test_random_fixtures_gpu(gpu_device, Tp):
    run_random(gpu_device, Tp)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def run_refusals(device):
    lib = _lib(device)
    w = torch.zeros(2, 1, 4, device=device)
    out = torch.zeros(2, 1, 8, dtype=torch.float64, device=device)
    ok = (ptr(w), 4, 2, 1, 4, None, None, None, 0.1, 0.9, ptr(out))
    lib.call("lvsr_alignment_times", lib.stream_for(out), *ok)
    change = lambda **kw: tuple(kw.get(name, v) for name, v in zip(("weights", "ldw", "L", "B", "Tp", "mask", "costs", "lengths", "lo", "hi", "out"), ok))
    for args in [change(weights=None), change(out=None), change(L=0), change(B=0), change(Tp=0), change(L=-1), change(ldw=3),
                 change(L=1 << 16, B=1 << 15),                                   # 2^31 rows
                 change(lo=-0.1), change(hi=1.5), change(lo=0.9, hi=0.1), change(lo=float("nan")), change(hi=float("nan"))]:
        with pytest.raises(NativeError, match="lvsr_alignment_times"):
            lib.call("lvsr_alignment_times", lib.stream_for(out), *args)


def test_refusals_emulated():
    run_refusals("cpu")


@pytest.mark.gpu
def test_refusals_gpu(gpu_device):
    run_refusals(gpu_device)
