"""The ten entry points of csrc/readout.hip called directly, each against a float64 NumPy restatement of the same operation, at the
shapes where these kernels can go wrong: vocabularies beyond one 64-lane trip of the row reductions, index lists beyond one
2048-entry chunk of the scatter, every column / contraction split of the per-row matrix-vector product of lvsr_readout_step,
padded row strides, optional (NULL) arguments, labels outside [0, V) and row counts that do not fill the last work-group.

Inputs carry 1e30 in their padding columns (a read past the width shows in the result), outputs are pre-filled with a sentinel
that must survive in theirs.  Every checker runs on the CPU emulator build and on the product library.

Bars (none of them comes from what the kernels give):
* logits / merged pre-activations: |got - ref64| <= 1e-5 * max(1, max |ref64| of the row) (check_argmax_emitter's rtol at the row
  maximum; an element-wise relative bar means nothing at a logit near zero);
* log-probabilities, costs, fusion outputs: rtol 2e-5, atol 1e-4 * max(1, 1e-7 * max |ref|) (run_fusion, tests/test_lm.py);
* dlogits, tanh forward / backward, scatter with beta = 0.3: atol 2e-6 * max(1, max |ref|) (the alignment-weights atol of
  tests/test_gpu_kernels.py; these values are bounded by their scale);
* integer, copy, selection and max operations and the scatter at beta 0 / 1: exact.
The weights of the lvsr_readout_step cases are drawn at scale 1 / sqrt(contraction depth), so that logits stay O(1) at every depth."""
import ctypes

import numpy
import pytest
import torch

from lvsr_amd import native
from lvsr_amd.native import ptr
from oracle import lm_oracle as LO

F32, F64, I64 = numpy.float32, numpy.float64, numpy.int64
SENT = -777.25            # the sentinel outputs are pre-filled with
POISON = 1e30             # the padding of inputs
WORST = {}                # what -> (largest error / bar seen, the error there): printed by every checker


# ---- comparators --------------------------------------------------------------------------------------------------------------
def _note(what, err, bar):
    ratio = numpy.max(err / bar) if numpy.size(err) else 0.0
    if what not in WORST or ratio > WORST[what][0]:
        WORST[what] = (float(ratio), float(numpy.max(err)) if numpy.size(err) else 0.0)
    return ratio


def report(family, device):
    """Print and forget the worst deviations of a family (`pytest -s` shows them next to their bars)."""
    for what in sorted(WORST):
        if what.startswith(family):
            ratio, err = WORST.pop(what)
            print("%-34s on %s: worst error %.3g = %.3g of its bar" % (what, device, err, ratio))


def close_logits(got, ref, what="logits"):
    ref = numpy.asarray(ref, F64)
    assert got.shape == ref.shape and numpy.isfinite(got).all(), what
    bar = 1e-5 * numpy.maximum(1.0, numpy.abs(ref).max(axis=-1, keepdims=True))
    err = numpy.abs(got - ref)
    assert _note(what, err, bar * numpy.ones_like(err)) <= 1.0, "%s: %g over a bar of %g" % (what, err.max(), bar.min())


def close_logp(got, ref, what="logp"):
    ref = numpy.asarray(ref, F64)
    assert got.shape == ref.shape and not numpy.isnan(got).any(), what
    atol = 1e-4 * max(1.0, 1e-7 * numpy.abs(ref).max()) if ref.size else 1e-4
    err, bar = numpy.abs(got - ref), atol + 2e-5 * numpy.abs(ref)
    assert _note(what, err, bar) <= 1.0, "%s: worst error / bar = %g" % (what, (err / bar).max())


def close_grad(got, ref, what="grad"):
    ref = numpy.asarray(ref, F64)
    assert got.shape == ref.shape and numpy.isfinite(got).all(), what
    bar = 2e-6 * max(1.0, numpy.abs(ref).max()) if ref.size else 2e-6
    err = numpy.abs(got - ref)
    assert _note(what, err, bar * numpy.ones_like(err)) <= 1.0, "%s: %g over a bar of %g" % (what, err.max(), bar)


def same_bits(got, ref, what="bits"):
    got, ref = numpy.ascontiguousarray(got), numpy.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    view = numpy.uint32 if got.dtype == F32 else got.dtype
    assert numpy.array_equal(got.view(view), ref.view(view)), what


def equal_classes(got, ref, what="classes"):
    assert numpy.array_equal(numpy.asarray(got, I64), numpy.asarray(ref, I64)), "%s: %s != %s" % (what, got, ref)


# ---- buffers --------------------------------------------------------------------------------------------------------------------
def dev(x, device):
    return None if x is None else torch.from_numpy(numpy.ascontiguousarray(x)).to(device)


def padded(a, ld, device, fill=POISON):
    """(n, w) array -> (n, ld) device tensor with `fill` in the padding columns."""
    a = numpy.asarray(a, F32)
    buf = numpy.full((a.shape[0], ld), fill, F32)
    buf[:, :a.shape[1]] = a
    return dev(buf, device)


def out_buf(n, ld, device, dtype=torch.float32, fill=SENT):
    return torch.full((n, ld), fill, dtype=dtype, device=device)


def take(t, w):
    """The (n, w) payload of an output buffer; its padding columns must still hold the sentinel."""
    a = t.cpu().numpy()
    assert (a[:, w:] == SENT).all(), "padding columns were written"
    return numpy.ascontiguousarray(a[:, :w])


def log_softmax64(x):
    x = numpy.asarray(x, F64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - numpy.log(numpy.exp(x - m).sum(axis=-1, keepdims=True))


def draw_uniforms(p, zero_last):
    """Uniforms in [0, 0.999] (the last row 0 if asked) for the inverse-CDF emitters, from the first seed at which every one of them is
    at least 1e-4 away from every boundary of the float64 CDF of `p` — so that no float32 running sum can excuse another class.
    -> uniforms (float32), the classes the float64 CDF picks."""
    cdf = numpy.cumsum(numpy.asarray(p, F64), axis=1)
    n = cdf.shape[0]
    for seed in range(1000):
        u = numpy.random.RandomState(seed).uniform(0.0, 0.999, n).astype(F32)
        if zero_last:
            u[-1] = 0.0
        if numpy.abs(cdf - u.astype(F64)[:, None]).min() >= 1e-4:
            break
    assert numpy.abs(cdf - u.astype(F64)[:, None]).min() >= 1e-4, "no seed keeps the uniforms clear of the CDF boundaries"
    assert (cdf[:, -1] > u).all()
    return u, (cdf > u.astype(F64)[:, None]).argmax(axis=1)


# ---- 1. lvsr_softmax_nll ------------------------------------------------------------------------------------------------------
NLL_V = (1, 2, 63, 64, 65, 129, 200, 2048)
NLL_N = (1, 4, 5, 9)
NLL_SCALE = 0.25


def nll_case(n, V):
    """Row 0: maximum in column 64 (the second trip of a lane; 100, so that a maximum taken over the first trip alone overflows the
    exponentials instead of cancelling), label V.  Row 1: maximum in column V - 1, label -1.  Row 2: +-80
    entries (exp needs the maximum subtracted).  Row 3: one entry of -1e4, label V - 1.  Further rows: plain.  Mask 0: row 4, or row 2
    when there are four rows."""
    rng = numpy.random.RandomState(1000 * n + V)
    x = rng.normal(0, 2, (n, V)).astype(F32)
    labels = rng.randint(0, V, n).astype(I64)
    mask = numpy.ones(n, F32)
    if V > 64:
        x[0, 64] = 100.0
    labels[0] = V
    if n > 1:
        x[1, V - 1] = 100.0
        labels[1] = -1
    if n > 2:
        x[2, 0] = 80.0
        if V > 1:
            x[2, V - 1] = -80.0
        if V > 2:
            x[2, V // 2] = 80.0
        mask[4 if n > 4 else 2] = 0.0
    if n > 3:
        x[3, V // 3] = -1e4
        labels[3] = V - 1
    return x, labels, mask


def nll_ref(x, labels, mask, scale, lse=None):
    """float64: cost (n), dlogits (n,V), neglogp (n,V).  `lse` overrides the log-sum-exp (negative control)."""
    x = x.astype(F64)
    n, V = x.shape
    logp = log_softmax64(x) if lse is None else x - lse[:, None]
    m = numpy.ones(n) if mask is None else mask.astype(F64)
    y = numpy.full(n, -1, I64) if labels is None else labels
    ok = (y >= 0) & (y < V)
    onehot = numpy.zeros((n, V))
    onehot[numpy.nonzero(ok)[0], y[ok]] = 1.0
    cost = numpy.where(ok, -logp[numpy.arange(n), numpy.where(ok, y, 0)], 0.0) * m
    return cost, (numpy.exp(logp) - onehot) * m[:, None] * scale, -logp


def call_nll(lib, device, x, labels, mask, scale, want=("cost", "dlogits", "neglogp")):
    n, V = x.shape
    ld, ldd, ldn = V + 3, V + 2, V + 1
    xd, yd, md = padded(x, ld, device), dev(labels, device), dev(mask, device)
    cost = out_buf(1, n + 2, device) if "cost" in want else None
    dl = out_buf(n, ldd, device) if "dlogits" in want else None
    nl = out_buf(n, ldn, device) if "neglogp" in want else None
    lib.call("lvsr_softmax_nll", lib.stream_for(xd), ptr(xd), ld, ptr(yd), ptr(md), n, V, ptr(cost), ptr(dl), ldd, float(scale), ptr(nl), ldn)
    return dict(cost=None if cost is None else take(cost, n)[0], dlogits=None if dl is None else take(dl, V),
                neglogp=None if nl is None else take(nl, V))


def run_softmax_nll(device, lib):
    for V in NLL_V:
        for n in NLL_N:
            x, labels, mask = nll_case(n, V)
            got = call_nll(lib, device, x, labels, mask, NLL_SCALE)
            cost, dl, nl = nll_ref(x, labels, mask, NLL_SCALE)
            close_logp(got["cost"], cost, "nll cost")
            close_logp(got["neglogp"], nl, "nll neglogp")
            close_grad(got["dlogits"], dl, "nll dlogits")
            if V > 64:
                assert x[0].argmax() == 64 and (n < 2 or x[1].argmax() == V - 1)
            # labels outside [0, V): no cost, the gradient is the softmax alone
            off = (labels < 0) | (labels >= V)
            assert off[0] and (got["cost"][off] == 0).all()
            if n > 2:       # a masked row: cost 0 and a gradient row of exactly 0
                off = mask == 0
                assert off.sum() == 1 and (got["cost"][off] == 0).all() and (got["dlogits"][off] == 0).all()
            # every optional argument NULL in turn: what is still written does not change by a bit
            for drop in ("cost", "dlogits", "neglogp"):
                rest = tuple(k for k in ("cost", "dlogits", "neglogp") if k != drop)
                part = call_nll(lib, device, x, labels, mask, NLL_SCALE, want=rest)
                assert part[drop] is None
                for k in rest:
                    same_bits(part[k], got[k], "nll %s without %s" % (k, drop))
            ones = call_nll(lib, device, x, labels, numpy.ones(n, F32), NLL_SCALE)
            nomask = call_nll(lib, device, x, labels, None, NLL_SCALE)
            nolab = call_nll(lib, device, x, None, mask, NLL_SCALE)
            none = call_nll(lib, device, x, numpy.full(n, -1, I64), mask, NLL_SCALE)
            for k in ("cost", "dlogits", "neglogp"):
                same_bits(nomask[k], ones[k], "nll %s, mask NULL" % k)
                same_bits(nolab[k], none[k], "nll %s, labels NULL" % k)
            same_bits(nomask["neglogp"], got["neglogp"], "nll neglogp, mask NULL")
            same_bits(nolab["neglogp"], got["neglogp"], "nll neglogp, labels NULL")
            assert (nolab["cost"] == 0).all()
            close_grad(nolab["dlogits"], nll_ref(x, None, mask, NLL_SCALE)[1], "nll dlogits")
            close_logp(nomask["cost"], nll_ref(x, labels, None, NLL_SCALE)[0], "nll cost")
    report("nll", device)


def test_softmax_nll_emulated():
    from emu import emu_lib
    run_softmax_nll("cpu", emu_lib())


@pytest.mark.gpu
def test_softmax_nll_gpu(gpu_device):
    run_softmax_nll(gpu_device, native.get())


def test_softmax_nll_control():
    """A log-sum-exp that leaves out class V - 1 (the row whose maximum sits there) is rejected."""
    x, labels, mask = nll_case(4, 200)
    x[3, 199] = 3.0                                  # row 3's label: a class with some mass
    cost, dl, nl = nll_ref(x, labels, mask, NLL_SCALE)
    as_f32 = lambda a: a.astype(F32)
    close_logp(as_f32(nl), nl), close_logp(as_f32(cost), cost), close_grad(as_f32(dl), dl)
    x64 = x.astype(F64)[:, :-1]
    m = x64.max(axis=1)
    short = m + numpy.log(numpy.exp(x64 - m[:, None]).sum(axis=1))
    wrong_cost, wrong_dl, wrong_nl = nll_ref(x, labels, mask, NLL_SCALE, lse=short)
    with pytest.raises(AssertionError):
        close_logp(as_f32(nl), wrong_nl)
    with pytest.raises(AssertionError):
        close_logp(as_f32(cost), wrong_cost)
    with pytest.raises(AssertionError):
        close_grad(as_f32(dl), wrong_dl)


# ---- 2. lvsr_scatter_add_rows, lvsr_gather_rows ---------------------------------------------------------------------------------
SCATTER_SHAPES = ((0, 3, 5), (1, 3, 5), (2047, 5, 257), (2048, 5, 33), (2049, 5, 300), (5000, 7, 300))
GRID_Y_MAX = 65535


def scatter_ref32(src, idx, nrows, dst0, beta):
    """The kernel's documented order in float32: the matching source rows added one by one in ascending row order, then beta * dst."""
    acc = numpy.zeros((nrows, src.shape[1]), F32)
    for r in range(len(idx)):
        if 0 <= idx[r] < nrows:
            acc[idx[r]] += src[r]
    return acc if beta == 0 else (F32(beta) * dst0 + acc).astype(F32)


def scatter_ref64(src, idx, nrows, dst0, beta):
    acc = numpy.zeros((nrows, src.shape[1]), F64)
    numpy.add.at(acc, idx[(idx >= 0) & (idx < nrows)], src.astype(F64)[(idx >= 0) & (idx < nrows)])
    return F64(F32(beta)) * dst0.astype(F64) + acc


def call_scatter(lib, device, src, idx, nrows, dst0, beta):
    n, width = src.shape
    lds, ldd = width + 2, width + 1
    sd, idd = padded(src, lds, device), dev(idx, device)
    dst = padded(dst0, ldd, device, fill=SENT)
    lib.call("lvsr_scatter_add_rows", lib.stream_for(dst), ptr(sd), lds, ptr(idd), n, nrows, width, ptr(dst), ldd, float(beta))
    return take(dst, width)


def scatter_case(n, nrows, width, all_equal=False):
    rng = numpy.random.RandomState(n + 7 * width)
    src = rng.normal(0, 1, (n, width)).astype(F32)
    idx = rng.randint(-1, nrows + 1, n).astype(I64)          # -1 and nrows occur and must be ignored
    if all_equal:
        idx[:] = 2
    elif n > 1:
        idx[0], idx[-1] = -1, nrows
    return src, idx, rng.normal(0, 1, (nrows, width)).astype(F32)


def run_scatter(device, lib):
    cases = [(s, False) for s in SCATTER_SHAPES] + [((2048, 5, 33), True)]      # every index equal: 2048 hits in one chunk
    for (n, nrows, width), all_equal in cases:
        src, idx, dst0 = scatter_case(n, nrows, width, all_equal)
        for beta in (0.0, 1.0) if all_equal else (0.0, 1.0, 0.3):
            start = numpy.full_like(dst0, numpy.nan) if beta == 0 else dst0        # beta = 0: dst is not read
            got = call_scatter(lib, device, src, idx, nrows, start, beta)
            same_bits(call_scatter(lib, device, src, idx, nrows, start, beta), got, "scatter: two runs")
            if beta in (0.0, 1.0):
                same_bits(got, scatter_ref32(src, idx, nrows, dst0, beta), "scatter n=%d beta=%g" % (n, beta))
            else:
                close_grad(got, scatter_ref64(src, idx, nrows, dst0, beta), "scatter beta=0.3")
    report("scatter", device)


def test_scatter_add_rows_emulated():
    from emu import emu_lib
    run_scatter("cpu", emu_lib())


@pytest.mark.gpu
def test_scatter_add_rows_gpu(gpu_device):
    run_scatter(gpu_device, native.get())


def test_scatter_add_rows_control():
    """Two source rows on either side of the 2048 seam swapped: the same multiset of addends in another order fails the bitwise bar."""
    n, nrows, width = 2049, 5, 300
    src, idx, dst0 = scatter_case(n, nrows, width)
    idx[2040:2049] = 3
    ref = scatter_ref32(src, idx, nrows, dst0, 1.0)
    same_bits(ref.copy(), ref)
    swapped = src.copy()
    swapped[[2047, 2048]] = src[[2048, 2047]]
    wrong = scatter_ref32(swapped, idx, nrows, dst0, 1.0)
    close_grad(ref, wrong.astype(F64))               # the same sum to rounding ...
    with pytest.raises(AssertionError):
        same_bits(ref, wrong)                        # ... but not the same bits


def run_gather(device, lib):
    nrows = 11
    for n in (1, 300):
        for width in (1, 256, 257, 600):
            rng = numpy.random.RandomState(n + width)
            table, bias = rng.normal(0, 1, (nrows, width)).astype(F32), rng.normal(0, 1, width).astype(F32)
            ldt, ldo = width + 3, width + 2
            td, bd = padded(table, ldt, device), dev(bias, device)
            lists = [[-1], [3], [nrows], [nrows - 1]] if n == 1 else [numpy.concatenate([[-1, nrows, 0, nrows - 1], rng.randint(-1, nrows + 1, n - 4)])]
            for idx in lists:
                idx = numpy.asarray(idx, I64)
                ok = (idx >= 0) & (idx < nrows)
                rows = numpy.where(ok[:, None], table[numpy.where(ok, idx, 0)], F32(0))
                idd = dev(idx, device)
                for b in (None, bd):
                    out = out_buf(n, ldo, device)
                    lib.call("lvsr_gather_rows", lib.stream_for(out), ptr(td), ldt, ptr(idd), n, nrows, width, ptr(b), ptr(out), ldo)
                    same_bits(take(out, width), rows if b is None else rows + bias, "gather n=%d width=%d" % (n, width))


def test_gather_rows_emulated():
    from emu import emu_lib
    run_gather("cpu", emu_lib())


@pytest.mark.gpu
def test_gather_rows_gpu(gpu_device):
    run_gather(gpu_device, native.get())


def test_row_count_limits_emulated():
    """Both launches carry a row count in gridDim.y (65535 at the most): one more is refused by name before anything is launched."""
    from emu import emu_lib
    lib, over = emu_lib(), GRID_Y_MAX + 1
    table, idx, out = torch.zeros(2, 1), torch.zeros(over, dtype=torch.int64), torch.zeros(over, 1)
    with pytest.raises(native.NativeError, match="lvsr_gather_rows.*65535"):
        lib.call("lvsr_gather_rows", lib.stream_for(out), ptr(table), 1, ptr(idx), over, 2, 1, None, ptr(out), 1)
    src, idx1, dst = torch.ones(1, 1), torch.zeros(1, dtype=torch.int64), torch.zeros(over, 1)
    with pytest.raises(native.NativeError, match="lvsr_scatter_add_rows.*65535"):
        lib.call("lvsr_scatter_add_rows", lib.stream_for(dst), ptr(src), 1, ptr(idx1), 1, over, 1, ptr(dst), 1, 0.0)
    assert float(dst.abs().max()) == 0 and float(out.abs().max()) == 0


# ---- 3. lvsr_act_fwd, lvsr_act_bwd ---------------------------------------------------------------------------------------------
# (1100, 1000) is more than the 4096 x 256 elements of one pass of the grid-stride loop; maxout halves the element count, so its
# second pass needs (1100, 1910)
ACT_CASES = ([(k, 1, 2) for k in range(4)] + [(k, 7, 33) for k in (0, 2, 3)] + [(k, 7, 34) for k in range(4)]
             + [(k, 1100, 1000) for k in range(4)] + [(1, 1100, 1910)])


def act_case(kind, n, P):
    rng = numpy.random.RandomState(10 * n + P + kind)
    x = rng.normal(0, 1.5, (n, P)).astype(F32)
    if kind == 1:                                   # pairs that tie exactly, also in the last pair of the last row
        x[0, 1] = x[0, 0]
        x[-1, P - 1] = x[-1, P - 2]
        if P > 20:
            x[n // 2, 17] = x[n // 2, 16]
    if kind == 2:                                   # +0.0 and -0.0 are not positive
        x[0, 0], x[-1, P - 1] = 0.0, -0.0
    return x, rng.normal(0, 1, (n, P // 2 if kind == 1 else P)).astype(F32)


def act_ref(kind, x, dy, tie_to_first=False):
    """-> y, dx: float32 for the exact kinds, float64 for tanh.  `tie_to_first`: the wrong maxout rule of the negative control."""
    if kind == 0:
        return x.copy(), dy.copy()
    if kind == 1:
        a, b = x[:, 0::2], x[:, 1::2]
        m = numpy.maximum(a, b)
        dx = numpy.zeros_like(x)
        dx[:, 0::2] = numpy.where(a == m, dy, F32(0))            # Theano's rule: every element equal to the maximum
        dx[:, 1::2] = numpy.where((b == m) & ~((a == m) & tie_to_first), dy, F32(0))
        return m, dx
    if kind == 2:
        return numpy.where(x > 0, x, F32(0)), numpy.where(x > 0, dy, F32(0))
    t = numpy.tanh(x.astype(F64))
    return t, dy.astype(F64) * (1.0 - t * t)


def run_act(device, lib):
    for kind, n, P in ACT_CASES:
        x, dy = act_case(kind, n, P)
        Pout = dy.shape[1]
        ldx, ldy, lddy, lddx = P + 3, Pout + 1, Pout + 2, P + 5
        xd, dyd = padded(x, ldx, device), padded(dy, lddy, device)
        y, dx = out_buf(n, ldy, device), out_buf(n, lddx, device)
        lib.call("lvsr_act_fwd", lib.stream_for(y), kind, ptr(xd), ldx, n, P, ptr(y), ldy)
        lib.call("lvsr_act_bwd", lib.stream_for(dx), kind, ptr(xd), ldx, ptr(dyd), lddy, n, P, ptr(dx), lddx)
        y, dx = take(y, Pout), take(dx, P)
        want_y, want_dx = act_ref(kind, x, dy)
        if kind == 3:
            close_grad(y, want_y, "act tanh forward")
            close_grad(dx, want_dx, "act tanh backward")
        else:
            same_bits(y, want_y, "act %d forward (%d, %d)" % (kind, n, P))
            same_bits(dx, want_dx, "act %d backward (%d, %d)" % (kind, n, P))
        if kind == 1:
            assert dx[0, 0] == dx[0, 1] == dy[0, 0] and dx[-1, P - 1] == dx[-1, P - 2] == dy[-1, -1]
        if kind == 2:
            assert dx[0, 0] == 0 and dx[-1, P - 1] == 0 and y[0, 0] == 0 and y[-1, P - 1] == 0
    report("act", device)


def test_act_emulated():
    from emu import emu_lib
    run_act("cpu", emu_lib())


@pytest.mark.gpu
def test_act_gpu(gpu_device):
    run_act(gpu_device, native.get())


def test_act_refusals_emulated():
    from emu import emu_lib
    lib = emu_lib()
    x, y = torch.zeros(2, 6), torch.zeros(2, 6)
    for kind, P in ((4, 4), (-1, 4), (1, 3)):
        with pytest.raises(native.NativeError, match="lvsr_act_fwd: bad activation"):
            lib.call("lvsr_act_fwd", lib.stream_for(y), kind, ptr(x), 6, 2, P, ptr(y), 6)
        with pytest.raises(native.NativeError, match="lvsr_act_bwd: bad activation"):
            lib.call("lvsr_act_bwd", lib.stream_for(y), kind, ptr(x), 6, ptr(x), 6, 2, P, ptr(y), 6)


def test_act_control():
    """A maxout gradient that goes to the first element of a tied pair only is rejected."""
    x, dy = act_case(1, 7, 34)
    y, dx = act_ref(1, x, dy)
    same_bits(dx.copy(), dx)
    with pytest.raises(AssertionError):
        same_bits(dx, act_ref(1, x, dy, tie_to_first=True)[1])


# ---- 4. lvsr_select_cost, lvsr_softmax_emit, lvsr_shallow_fusion ----------------------------------------------------------------
def run_select_cost(device, lib):
    V = 70
    ld = V + 3
    for n in (1, 257):                               # 257 rows: two work-groups
        rng = numpy.random.RandomState(n)
        x = rng.normal(0, 2, (n, V)).astype(F32)
        labels = rng.randint(0, V, n).astype(I64)
        mask = (rng.uniform(size=n) > 0.3).astype(F32)
        if n > 1:
            labels[1], labels[5], labels[-1], mask[2], mask[-1] = -1, V, V + 2, 0.0, 1.0
        xd = padded(x, ld, device)
        for lab in ([labels] if n > 1 else [labels, numpy.array([-1], I64), numpy.array([V], I64)]):
            ok = (lab >= 0) & (lab < V)
            picked = numpy.where(ok, x[numpy.arange(n), numpy.where(ok, lab, 0)], F32(0))
            for m in (None, mask):
                labd, md = dev(lab, device), dev(m, device)
                for scale in (-1.0, 0.5):            # powers of two: the products are exact in any order
                    cost = out_buf(1, n + 2, device)
                    lib.call("lvsr_select_cost", lib.stream_for(cost), ptr(xd), ld, ptr(labd), ptr(md), n, V, scale, ptr(cost))
                    want = F32(scale) * picked * (F32(1) if m is None else m)
                    got = take(cost, n)[0]
                    same_bits(got + F32(0), want + F32(0), "select_cost n=%d" % n)        # (+ 0: -0.0 and 0.0 are the same cost)
                    assert (got[~ok] == 0).all()


def test_select_cost_emulated():
    from emu import emu_lib
    run_select_cost("cpu", emu_lib())


@pytest.mark.gpu
def test_select_cost_gpu(gpu_device):
    run_select_cost(gpu_device, native.get())


def call_emit(lib, device, logits, ld, u, V, with_costs=True):
    """lvsr_softmax_emit on a device tensor of row stride ld -> classes, costs."""
    n = len(u)
    outputs = out_buf(1, n + 2, device, dtype=torch.int64, fill=-5)
    costs = out_buf(1, n + 2, device) if with_costs else None
    ud = dev(u, device)
    lib.call("lvsr_softmax_emit", lib.stream_for(logits), ptr(logits), ld, ptr(ud), n, V, ptr(outputs), ptr(costs))
    o = outputs.cpu().numpy()[0]
    assert (o[n:] == -5).all()
    return o[:n], None if costs is None else take(costs, n)[0]


def emit_case(n, V):
    x = numpy.random.RandomState(V + n).normal(0, 2, (n, V)).astype(F32)
    if V > 64:
        x[0, V - 1] = 100.0                          # row 0's maximum and all of its mass in the last class: the walk crosses every trip
    if n > 1:
        x[-1, 0] = 3.0                               # the row that is drawn at u = 0: class 0 has more than 1e-4 of the mass
    return x


def run_softmax_emit(device, lib):
    for V in (1, 65, 200):
        for n in (1, 6):
            x = emit_case(n, V)
            logp = log_softmax64(x)
            u, want = draw_uniforms(numpy.exp(logp), zero_last=n > 1)
            if V > 64:
                assert want[0] == V - 1 and (n == 1 or want[-1] == 0)
            xd = padded(x, V + 3, device)
            got, costs = call_emit(lib, device, xd, V + 3, u, V)
            equal_classes(got, want, "softmax_emit V=%d n=%d" % (V, n))
            close_logp(costs, -logp[numpy.arange(n), want], "emit cost")
            equal_classes(call_emit(lib, device, xd, V + 3, u, V, with_costs=False)[0], want)
    report("emit", device)


def test_softmax_emit_emulated():
    from emu import emu_lib
    run_softmax_emit("cpu", emu_lib())


@pytest.mark.gpu
def test_softmax_emit_gpu(gpu_device):
    run_softmax_emit(gpu_device, native.get())


def test_softmax_emit_control():
    """An emitted class that is off by one is rejected."""
    u, want = draw_uniforms(numpy.exp(log_softmax64(emit_case(6, 65))), zero_last=True)
    equal_classes(want.copy(), want)
    wrong = want.copy()
    wrong[3] += 1
    with pytest.raises(AssertionError):
        equal_classes(want, wrong)


FUSION_FLAGS = ((1, 0, 0), (0, 0, 0), (1, 1, 1), (0, 1, 0), (0, 0, 1))


def run_fusion_wide(device, lib):
    """run_fusion of tests/test_lm.py beyond one trip of the wave: V in {65, 200}, a padded row stride of the acoustic scores, and the
    row maximum of each of the three normalisations beyond column 63."""
    n = 7
    for V in (65, 200):
        rng = numpy.random.RandomState(V)
        am = rng.normal(0, 2, (n, V)).astype(F32)
        add = (100.0 + numpy.abs(rng.normal(0, 3, (n, V)))).astype(F32)
        ca, cl = 64 + rng.randint(0, V - 64, n), 64 + rng.randint(0, V - 64, n)
        am[numpy.arange(n), ca] += 100.0           # (by 100: a maximum that misses these columns overflows the exponentials)
        add[numpy.arange(n), cl] = 0.0
        add[2, 5] = 1e12
        ld = V + 3
        for flags in FUSION_FLAGS:
            a, l = padded(am, ld, device), dev(add, device)
            out = out_buf(n + 1, V, device)
            lib.call("lvsr_shallow_fusion", lib.stream_for(out), ptr(a), ld, ptr(l), n, V, 0.9, 0.5, flags[0], flags[1], flags[2], -1.0, ptr(out))
            ref = -LO.shallow_fusion(am, add, 0.5, 0.9, *[bool(f) for f in flags])
            got = out.cpu().numpy()
            assert (got[n] == SENT).all()
            close_logp(got[:n], ref, "fusion")
        # where the maxima of the three normalised quantities lie
        a64, l64 = 0.9 * am.astype(F64), -add.astype(F64)
        tot = log_softmax64(a64) + 0.5 * log_softmax64(l64)
        assert (a64.argmax(1) >= 64).all() and (l64.argmax(1) >= 64).all() and (tot.argmax(1) >= 64).all()
    report("fusion", device)


def test_shallow_fusion_wide_emulated():
    from emu import emu_lib
    run_fusion_wide("cpu", emu_lib())


@pytest.mark.gpu
def test_shallow_fusion_wide_gpu(gpu_device):
    run_fusion_wide(gpu_device, native.get())


# ---- 5. lvsr_readout_step, lvsr_readout_merge -------------------------------------------------------------------------------------
IDENT, MAXOUT, RELU, TANH = 0, 1, 2, 3
STEP_CASES = {
    # P = V with N % 4 != 0: the scalar columns of the matrix-vector product
    "no_post_merge": dict(n=3, D=5, E=3, P=70, V=70, act=IDENT, wout=False),
    "paper_width": dict(n=5, D=250, E=500, P=500, V=33, act=MAXOUT),
    "fusion": dict(n=4, D=7, E=9, P=66, V=65, act=MAXOUT, lm=True),
    "two_hidden_tanh": dict(n=3, D=64, E=128, P=256, V=129, act=TANH, hidden=(100, 37)),
    # scalar columns in several passes (N > 256), no state part
    "scalar_multipass": dict(n=2, D=9, E=11, P=1030, V=2047, act=RELU, hidden=(1027,), wms=False),
    # four-column vector loads in several passes (N > 1024), at the limits of the LDS layout
    "vector_multipass": dict(n=2, D=40, E=24, P=2048, V=2048, act=MAXOUT),
    # fewer contraction terms than slices of K
    "k_below_slices": dict(n=6, D=3, E=1, P=1, V=1, act=IDENT),
    # N % 4 == 0 behind a weight pointer that is not 16-byte aligned: scalar columns, chosen by the address alone
    "misaligned": dict(n=3, D=31, E=17, P=1028, V=1028, act=IDENT, misaligned=True),
    # the row maximum in the last column, beyond the first trip of the emitter's wave, by 100 (a maximum that misses it overflows)
    "late_maximum": dict(n=2, D=3, E=4, P=70, V=70, act=IDENT, wout=False, peak=True),
}
AM_BETA, LM_WEIGHT = 0.9, 0.5


def step_case(c, seed=0):
    """-> arrays (float32 inputs), ref (float64 r1, logits, logp of the step)."""
    rng = numpy.random.RandomState(seed + c["P"] + c["V"])
    n, D, E, P, V, act = c["n"], c["D"], c["E"], c["P"], c["V"], c["act"]
    wms, wout = c.get("wms", True), c.get("wout", True)
    f = lambda *shape, s=1.0: (s * rng.normal(0, 1, shape)).astype(F32)
    K1 = E + (D if wms else 0)
    a = dict(S=f(n, D), WA=f(n, E), Wmw=f(E, P, s=K1 ** -0.5), Wms=f(D, P, s=K1 ** -0.5) if wms else None, bias1=f(P, s=0.5),
             Wh=[], bh=[], Wout=None, bout=None, lm_add=numpy.abs(f(n, V, s=3.0)) if c.get("lm") else None)
    if c.get("peak"):
        a["bias1"][-1] += 100.0
    d = lambda x: x.astype(F64)
    r1 = d(a["bias1"]) + d(a["WA"]) @ d(a["Wmw"]) + (d(a["S"]) @ d(a["Wms"]) if wms else 0.0)
    logits = r1
    if wout:
        one = {IDENT: lambda x: x, RELU: lambda x: numpy.maximum(x, 0.0), TANH: numpy.tanh}
        cur = numpy.maximum(r1[:, 0::2], r1[:, 1::2]) if act == MAXOUT else one[act](r1)
        for w in c.get("hidden", ()):
            a["Wh"].append(f(cur.shape[1], w, s=2.0 * cur.shape[1] ** -0.5))
            a["bh"].append(f(w, s=0.5))
            cur = one[act](cur @ d(a["Wh"][-1]) + d(a["bh"][-1]))
        a["Wout"], a["bout"] = f(cur.shape[1], V, s=2.0 * cur.shape[1] ** -0.5), f(V, s=0.5)
        logits = cur @ d(a["Wout"]) + d(a["bout"])
    if c.get("lm"):
        logp = LO.shallow_fusion(logits, a["lm_add"], LM_WEIGHT, AM_BETA, True, True, True)
    else:
        logp = log_softmax64(logits)
    return a, dict(r1=r1, logits=logits, logp=logp)


def off_by_one_float(w, device):
    """The matrix as a view one float into a larger buffer: the address is 4 modulo 16."""
    buf = torch.zeros(w.size + 1, device=device)
    view = buf[1:].view(w.shape)
    view.copy_(torch.from_numpy(w))
    assert view.data_ptr() % 16 == 4
    return view


def step_tensors(c, a, device):
    mis = c.get("misaligned", False)
    t = dict(S=padded(a["S"], c["D"] + 3, device), WA=padded(a["WA"], c["E"] + 2, device))
    for k in ("Wmw", "Wms"):
        t[k] = None if a[k] is None else off_by_one_float(a[k], device) if mis else dev(a[k], device)
    for k in ("bias1", "Wout", "bout", "lm_add"):
        t[k] = dev(a[k], device)
    t["Wh"], t["bh"] = [dev(w, device) for w in a["Wh"]], [dev(b, device) for b in a["bh"]]
    return t


def call_step(lib, device, c, t, uniforms=None, logits=True, neglogp=True, R1=None, ldr1=0, **override):
    """-> dict(logits, neglogp (n,V) or None, outputs, costs (n) or None; `logits_dev`: the device tensor the kernel wrote)."""
    n, V = c["n"], c["V"]
    lg = out_buf(n + 1, V, device) if logits else None
    nl = out_buf(n + 1, V, device) if neglogp else None
    outs = out_buf(1, n + 2, device, dtype=torch.int64, fill=-5) if uniforms is not None else None
    costs = out_buf(1, n + 2, device) if uniforms is not None else None
    lm = t["lm_add"] is not None
    kw = dict(S=t["S"], WA=t["WA"], lds=c["D"] + 3, ldwa=c["E"] + 2, n=n, D=c["D"], E=c["E"], P=c["P"], V=V, act=c["act"], Wms=t["Wms"],
              Wmw=t["Wmw"], bias1=t["bias1"], Wout=t["Wout"], bout=t["bout"], lm_add=t["lm_add"], am_beta=AM_BETA if lm else 1.0,
              lm_weight=LM_WEIGHT if lm else 0.0, norm_am=1, norm_lm=int(lm), norm_tot=int(lm), neglogp=nl, logits=lg,
              uniforms=dev(uniforms, device), outputs=outs, costs=costs, n_hidden=len(t["Wh"]), dimh=[int(w.shape[1]) for w in t["Wh"]],
              Wh=t["Wh"], bh=t["bh"], R1=R1, ldr1=ldr1, emitter=0)
    kw.update(override)
    args = lib.make("lvsr_readout_step_args", **kw)
    lib.call("lvsr_readout_step", lib.stream_for(t["WA"]), ctypes.byref(args))
    res = dict(logits=None, neglogp=None, outputs=None, costs=None, logits_dev=lg)
    for k, buf in (("logits", lg), ("neglogp", nl)):
        if buf is not None:
            full = buf.cpu().numpy()
            assert (full[n] == SENT).all(), "a row past n was written"
            res[k] = full[:n]
    if outs is not None:
        o = outs.cpu().numpy()[0]
        assert (o[n:] == -5).all()
        res["outputs"], res["costs"] = o[:n], take(costs, n)[0]
    return res


BIT_EQUAL = {}            # (case, which kernel pair) -> were the costs of the two kernels the same bits?


def check_step(device, lib, name):
    c = STEP_CASES[name]
    n, V = c["n"], c["V"]
    a, ref = step_case(c)
    t = step_tensors(c, a, device)
    # (a row drawn at u = 0 where the reference gives class 0 of the last row 1e-4 of the mass; no wide vocabulary does)
    u, want = draw_uniforms(numpy.exp(ref["logp"]), zero_last=n > 1 and numpy.exp(ref["logp"][-1, 0]) >= 1e-4)
    full = call_step(lib, device, c, t, uniforms=u)
    close_logits(full["logits"], ref["logits"], "step logits")
    close_logp(full["neglogp"], -ref["logp"], "step neglogp")
    equal_classes(full["outputs"], want, "step classes (%s)" % name)
    close_logp(full["costs"], -ref["logp"][numpy.arange(n), want], "step cost")
    # without the emitter, and with neither logits nor neglogp: what is still written is the same bits
    plain = call_step(lib, device, c, t)
    same_bits(plain["logits"], full["logits"]), same_bits(plain["neglogp"], full["neglogp"])
    bare = call_step(lib, device, c, t, uniforms=u, logits=False, neglogp=False)
    equal_classes(bare["outputs"], full["outputs"]), same_bits(bare["costs"], full["costs"])
    same_bits(call_step(lib, device, c, t, logits=False)["neglogp"], full["neglogp"])
    same_bits(call_step(lib, device, c, t, neglogp=False)["logits"], full["logits"])
    # the same costs from the stand-alone kernels on the logits this one wrote ("the same arithmetic as ..." in the kernel source)
    lgd = full["logits_dev"]
    if c.get("lm"):
        out = out_buf(n + 1, V, device)
        lib.call("lvsr_shallow_fusion", lib.stream_for(out), ptr(lgd), V, ptr(t["lm_add"]), n, V, AM_BETA, LM_WEIGHT, 1, 1, 1, -1.0, ptr(out))
        other, pair = out.cpu().numpy()[:n], "shallow_fusion"
        emit_in = dev(-full["neglogp"], device)          # normalised log-probabilities: their softmax is the fused distribution
    else:
        nl = out_buf(n + 1, V, device)
        lib.call("lvsr_softmax_nll", lib.stream_for(nl), ptr(lgd), V, None, None, n, V, None, None, 0, 1.0, ptr(nl), V)
        other, pair = nl.cpu().numpy()[:n], "softmax_nll"
        emit_in = lgd
    close_logp(other, full["neglogp"].astype(F64), "step vs " + pair)
    BIT_EQUAL[(name, pair)] = bool(numpy.array_equal(other.view(numpy.uint32), full["neglogp"].view(numpy.uint32)))
    classes, costs = call_emit(lib, device, emit_in, V, u, V)
    equal_classes(classes, full["outputs"], "step vs softmax_emit (%s)" % name)
    close_logp(costs, full["costs"].astype(F64), "step vs softmax_emit cost")
    BIT_EQUAL[(name, "softmax_emit")] = bool(numpy.array_equal(costs.view(numpy.uint32), full["costs"].view(numpy.uint32)))
    print("%s on %s: costs bit-equal with %s: %s, with softmax_emit: %s" % (name, device, pair, BIT_EQUAL[(name, pair)], BIT_EQUAL[(name, "softmax_emit")]))
    report("step", device)


@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_readout_step_emulated(name):
    from emu import emu_lib
    check_step("cpu", emu_lib(), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_readout_step_gpu(gpu_device, name):
    check_step(gpu_device, native.get(), name)


MERGE_SHAPES = ((1, 5, 3, 17), (17, 250, 500, 250), (33, 64, 128, 256))


def run_merge(device, lib):
    for n, D, E, P in MERGE_SHAPES:
        for wms in (True, False):
            c = dict(n=n, D=D, E=E, P=P, V=P, act=IDENT, wout=False, wms=wms)
            a, ref = step_case(c, seed=5)
            t = step_tensors(c, a, device)
            packs = {}
            for k, K in (("Wmw", E), ("Wms", D)):
                if t[k] is not None:
                    packs[k] = torch.zeros(lib.pack_size(K, P), device=device)
                    lib.pack_b(t[k], packs[k])
            ldr1 = P + 3
            R1 = out_buf(n, ldr1, device)
            lib.call("lvsr_readout_merge", lib.stream_for(R1), ptr(t["S"]), D + 3, ptr(t["WA"]), E + 2, n, D, E, P, ptr(packs.get("Wms")),
                     ptr(packs["Wmw"]), ptr(t["bias1"]), ptr(R1), ldr1)
            close_logits(take(R1, P), ref["r1"], "merge r1")
            # the step kernel on these pre-activations and on its own products
            merged = call_step(lib, device, c, t, R1=R1, ldr1=ldr1)
            own = call_step(lib, device, c, t)
            same_bits(merged["logits"], take(R1, P), "step logits from R1")
            close_logits(own["logits"], ref["logits"], "merge: step logits")
            close_logits(merged["logits"], own["logits"].astype(F64), "merge: step with R1 vs without")
            close_logp(merged["neglogp"], -ref["logp"], "merge: step neglogp from R1")
    report("merge", device)


def test_readout_merge_emulated():
    from emu import emu_lib
    run_merge("cpu", emu_lib())


@pytest.mark.gpu
def test_readout_merge_gpu(gpu_device):
    run_merge(gpu_device, native.get())


def test_readout_step_control():
    """Logits that leave out the last term of the merge contraction are rejected."""
    c = STEP_CASES["no_post_merge"]
    a, ref = step_case(c)
    got = ref["logits"].astype(F32)
    close_logits(got, ref["logits"])
    last = numpy.outer(a["S"][:, -1].astype(F64), a["Wms"][-1].astype(F64))
    with pytest.raises(AssertionError):
        close_logits(got, ref["logits"] - last)
    c = dict(n=17, D=250, E=500, P=250, V=250, act=IDENT, wout=False)
    a, ref = step_case(c, seed=5)
    with pytest.raises(AssertionError):
        close_logits(ref["r1"].astype(F32), ref["r1"] - numpy.outer(a["S"][:, -1].astype(F64), a["Wms"][-1].astype(F64)))


def test_readout_step_refusals_emulated():
    from emu import emu_lib
    lib = emu_lib()
    c = dict(n=2, D=3, E=4, P=6, V=5, act=MAXOUT)
    a, _ = step_case(c)
    t = step_tensors(c, a, "cpu")
    u = numpy.array([0.5, 0.5], F32)
    call_step(lib, "cpu", c, t, uniforms=u)                                       # the block itself is accepted
    refused = [
        ("merge width must be V", dict(Wout=None, bout=None)),                    # P != V without an output layer
        ("bad activation", dict(P=5)),                                            # odd P with maxout
        ("further post-merge layers", dict(n_hidden=1, dimh=[3], Wh=[t["Wout"]], bh=[t["bout"]])),       # hidden layers with maxout
        ("emitter must be", dict(emitter=1, lm_add=torch.zeros(2, 5))),
        ("emit needs an output buffer", dict(uniforms=torch.zeros(2), outputs=None)),
    ]
    for message, override in refused:
        with pytest.raises(native.NativeError, match=message):
            call_step(lib, "cpu", c, t, **override)
    big = dict(n=1, D=1, E=1, P=2049, V=2049, act=IDENT, wout=False)
    a, _ = step_case(big)
    with pytest.raises(native.NativeError, match="LDS budget"):
        call_step(lib, "cpu", big, step_tensors(big, a, "cpu"))
    big = dict(n=1, D=1, E=1, P=4, V=2049, act=IDENT)
    a, _ = step_case(big)
    with pytest.raises(native.NativeError, match="LDS budget"):
        call_step(lib, "cpu", big, step_tensors(big, a, "cpu"))
