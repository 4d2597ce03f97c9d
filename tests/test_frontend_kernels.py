"""lvsr_frontend_batch and lvsr_feature_stats (csrc/fbank.hip) called directly.

lvsr_frontend_batch is compared BIT FOR BIT with lvsr_add_deltas_cmvn_batch on the same packed input, rearranged by NumPy into the
time-major padded batch (without deltas: with NumPy's float32 (v - m) * i): every output sits between guard bands, is filled with a
NaN pattern first and is compared whole, so a frame that was not written, a -0.0 in the padding, a mask that is not exactly 0 / 1 and a
store outside the buffer all show.  lvsr_feature_stats is compared with NumPy's float64 sums under the bound every float64 summation
order meets.  The bodies run on the CPU emulator (same sources) and, under the `gpu` marker, on the device."""
import numpy
import pytest
import torch

from lvsr_amd.native import NativeError, ptr

TILE = 56                      # DC_TILE of csrc/fbank.hip: the frames a work-group of lvsr_frontend_batch owns
GUARD = 256                    # floats of pattern in front of and behind every output
PATTERN = 0x7FC5A5A5           # a NaN no kernel computes

# shorter and longer than the +-4 frames the delta-delta reaches; one below, at and one above the tile and twice the tile
LENGTHS = [0, 1, 2, 4, 5, 8, 9, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1]
LAYOUTS = {
    "n1": [TILE + 1],
    "n3_boundaries_on_tile_edges": [TILE, 2 * TILE, 9],                      # utterances begin at frames 0, 56, 168 of the packed set
    "n65_boundaries_inside_tiles": LENGTHS + (LENGTHS[:7] * 8)[:52],         # every length, then short ones: 65 utterances
}
DIMS = [1, 5, 41, 64]


def _lib(device):
    if device == "cpu":
        from emu import emu_lib
        return emu_lib()
    from lvsr_amd import native
    return native.get()


def guarded(n, device):
    """-> (whole buffer, the n floats between its guard bands), all PATTERN"""
    whole = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.int32, device=device).view(torch.float32)
    return whole, whole[GUARD: GUARD + n]


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(numpy.uint32)


def expect_guarded(whole, inner):
    """what `whole` must hold: the pattern around `inner` (a float32 ndarray)"""
    want = numpy.full(whole.numel(), PATTERN, dtype=numpy.uint32)
    want[GUARD: GUARD + inner.size] = numpy.ascontiguousarray(inner, dtype=numpy.float32).ravel().view(numpy.uint32)
    return want


def reference(lib, device, feats, lens, deltas, mean, istd, T):
    """x (T, n, W) and mask (T, n) as the existing entry point and NumPy make them"""
    off = numpy.concatenate([[0], numpy.cumsum(lens)]).astype(numpy.int32)
    total, dim = feats.shape
    if deltas:
        out = torch.empty(total, 3 * dim, dtype=torch.float32, device=device)
        foff = torch.from_numpy(off).to(device)
        lib.call("lvsr_add_deltas_cmvn_batch", lib.stream_for(out), ptr(feats), ptr(foff), len(lens), total, dim, ptr(mean), ptr(istd), ptr(out))
        packed = out.cpu().numpy()
    else:
        packed = feats.cpu().numpy()
        if mean is not None:
            packed = (packed - mean.cpu().numpy()[None, :]) * istd.cpu().numpy()[None, :]          # float32, two rounded operations
            assert packed.dtype == numpy.float32
    x = numpy.zeros((T, len(lens), packed.shape[1]), numpy.float32)
    m = numpy.zeros((T, len(lens)), numpy.float32)
    for b, n in enumerate(lens):
        x[:n, b] = packed[off[b]: off[b] + n]
        m[:n, b] = 1.0
    return x, m


def launch(lib, feats, foff, lens, deltas, mean, istd, T, x, mask):
    lib.call("lvsr_frontend_batch", lib.stream_for(x), ptr(feats), ptr(foff), len(lens), int(feats.shape[0]), max(lens), int(feats.shape[1]),
             int(deltas), ptr(mean), ptr(istd), T, ptr(x), ptr(mask))


def make_inputs(device, lens, dim, seed):
    rng = numpy.random.RandomState(seed)
    total = int(sum(lens))
    feats = torch.from_numpy((rng.randn(total, dim) * 3.0 + 1.0).astype(numpy.float32)).to(device)
    foff = torch.from_numpy(numpy.concatenate([[0], numpy.cumsum(lens)]).astype(numpy.int32)).to(device)
    stats = {}
    for deltas in (0, 1):
        W = dim * (3 if deltas else 1)
        stats[deltas] = (torch.from_numpy(rng.randn(W).astype(numpy.float32)).to(device),
                         torch.from_numpy((0.5 + rng.rand(W)).astype(numpy.float32)).to(device))
    return feats, foff, stats


def run_frontend_batch(device, layout, dim):
    lib = _lib(device)
    lens = LAYOUTS[layout]
    feats, foff, stats = make_inputs(device, lens, dim, seed=dim + len(lens))
    longest = max(lens)
    # T: the longest utterance itself, rounded up to 64, and well above it (more than a whole tile of padding)
    Ts = (longest, (longest + 63) // 64 * 64, longest + TILE + 19)
    combos = [(deltas, with_stats, T) for deltas in (1, 0) for with_stats in (False, True) for T in Ts]
    if len(lens) > 8:          # the large set: every value of every axis, not their whole product (the emulator runs a thread at a time)
        combos = [(1, True, Ts[0]), (1, False, Ts[2]), (0, True, Ts[1]), (0, False, Ts[0])]
    for deltas, with_stats, T in combos:
        W = dim * (3 if deltas else 1)
        mean, istd = stats[deltas] if with_stats else (None, None)
        xw, x = guarded(T * len(lens) * W, device)
        mw, mask = guarded(T * len(lens), device)
        launch(lib, feats, foff, lens, deltas, mean, istd, T, x, mask)
        want_x, want_m = reference(lib, device, feats, lens, deltas, mean, istd, T)
        what = "%s dim %d deltas %d stats %s T %d" % (layout, dim, deltas, mean is not None, T)
        bad = numpy.nonzero(bits(xw) != expect_guarded(xw, want_x))[0]
        assert bad.size == 0, "%s: x differs at %d of its guarded buffer (%d places)" % (what, bad[0] - GUARD, bad.size)
        bad = numpy.nonzero(bits(mw) != expect_guarded(mw, want_m))[0]
        assert bad.size == 0, "%s: mask differs at %d of its guarded buffer" % (what, bad[0] - GUARD)


CASES = [(layout, dim) for layout in sorted(LAYOUTS) for dim in DIMS]


@pytest.mark.parametrize("layout,dim", CASES)
def test_frontend_batch_emulated(layout, dim):
    run_frontend_batch("cpu", layout, dim)


@pytest.mark.gpu
@pytest.mark.parametrize("layout,dim", CASES)
def test_frontend_batch_gpu(gpu_device, layout, dim):
    run_frontend_batch(gpu_device, layout, dim)


def run_captured(device):
    """The launch inside lvsr_region_begin / end: captured, then replayed, with the bits of the eager launch.  (The emulator has no
    stream capture: begin answers `not capturable` and the launches are eager.)"""
    lib = _lib(device)
    lens, dim, T = LAYOUTS["n65_boundaries_inside_tiles"], 41, 128
    feats, foff, stats = make_inputs(device, lens, dim, seed=7)
    mean, istd = stats[1]
    W = 3 * dim
    xw, x = guarded(T * len(lens) * W, device)
    mw, mask = guarded(T * len(lens), device)
    launch(lib, feats, foff, lens, 1, mean, istd, T, x, mask)
    eager_x, eager_m = bits(xw), bits(mw)
    want_x, want_m = reference(lib, device, feats, lens, 1, mean, istd, T)
    assert (eager_x == expect_guarded(xw, want_x)).all() and (eager_m == expect_guarded(mw, want_m)).all()
    on_gpu = torch.device(device).type == "cuda"
    stream = torch.cuda.Stream(device) if on_gpu else None            # capture cannot run on the legacy null stream
    key = repr(("test_frontend_kernels", x.data_ptr(), mask.data_ptr(), feats.data_ptr(), foff.data_ptr(), mean.data_ptr(),
                istd.data_ptr(), T, len(lens), dim)).encode()
    answers = []
    for _ in range(2):
        xw.view(torch.int32).fill_(PATTERN)
        mw.view(torch.int32).fill_(PATTERN)
        if on_gpu:
            torch.cuda.synchronize(device)
        with (torch.cuda.stream(stream) if on_gpu else _nothing()):
            rc = lib._lvsr_region_begin(lib.stream_for(x), key, len(key))
            assert rc in (0, 1, 2), lib.last_error()
            answers.append(rc)
            if rc != 1:
                launch(lib, feats, foff, lens, 1, mean, istd, T, x, mask)
            if rc == 0:
                assert lib._lvsr_region_end(lib.stream_for(x), 1) == 0, lib.last_error()
        if on_gpu:
            torch.cuda.synchronize(device)
        assert (bits(xw) == eager_x).all() and (bits(mw) == eager_m).all(), "region answer %d" % rc
    assert answers == ([0, 1] if on_gpu else [2, 2]), answers          # captured, then replayed


class _nothing(object):
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def test_frontend_batch_captured_emulated():
    run_captured("cpu")


@pytest.mark.gpu
def test_frontend_batch_captured_gpu(gpu_device):
    run_captured(gpu_device)


def run_refusals(device):
    lib = _lib(device)
    lens = [5, 9]
    feats, foff, stats = make_inputs(device, lens, 5, seed=1)
    mean, istd = stats[1]
    xw, x = guarded(16 * 2 * 15, device)
    mw, mask = guarded(16 * 2, device)
    with pytest.raises(NativeError, match="lvsr_frontend_batch: T = 8 is shorter than the longest utterance"):
        launch(lib, feats, foff, lens, 1, mean, istd, 8, x, mask)
    with pytest.raises(NativeError, match="lvsr_frontend_batch: mean and istd come together"):
        launch(lib, feats, foff, lens, 1, mean, None, 16, x, mask)
    with pytest.raises(NativeError, match="lvsr_frontend_batch: mean and istd come together"):
        launch(lib, feats, foff, lens, 1, None, istd, 16, x, mask)
    wide = torch.zeros(14, 65, dtype=torch.float32, device=device)
    with pytest.raises(NativeError, match="lvsr_frontend_batch: at most 64 coefficients"):
        launch(lib, wide, foff, lens, 0, None, None, 16, x, mask)
    # nothing was launched: both buffers still hold the pattern
    assert (bits(xw) == PATTERN).all() and (bits(mw) == PATTERN).all()


def test_frontend_batch_refusals_emulated():
    run_refusals("cpu")


@pytest.mark.gpu
def test_frontend_batch_refusals_gpu(gpu_device):
    run_refusals(gpu_device)


# ---- lvsr_feature_stats -----------------------------------------------------------------------------------------------------------
STATS_PARTS = 1024
STAT_SHAPES = [(rows, width) for rows in (1, 255, 8193) for width in (1, 15, 123, 192)]


def feature_stats(lib, x, rows, width, sums, accumulate, partials):
    lib.call("lvsr_feature_stats", lib.stream_for(sums), ptr(x), rows, width, ptr(partials), ptr(sums), accumulate)


def run_feature_stats(device, rows, width):
    """The bar: a float64 sum of `rows` terms, in ANY order, is off by at most (rows - 1) u sum |term| (1 + O(rows u)), u = 2^-53 (the
    terms themselves are exact: a float32 value and the float64 product of two float32 values); rows * 2^-53 * sum |term| covers it."""
    lib = _lib(device)
    rng = numpy.random.RandomState(rows + width)
    host = (10.0 + rng.randn(rows, width)).astype(numpy.float32)
    x = torch.from_numpy(host).to(device)
    x64 = host.astype(numpy.float64)
    ref = numpy.concatenate([x64.sum(axis=0), (x64 * x64).sum(axis=0)])
    bar = rows * 2.0 ** -53 * numpy.concatenate([numpy.abs(x64).sum(axis=0), (x64 * x64).sum(axis=0)])
    # the bar discriminates: squares taken in float32, and (over more than one row) a float32 accumulator, miss it everywhere
    sq32 = (host * host).astype(numpy.float64).sum(axis=0)
    assert (numpy.abs(sq32 - ref[width:]) > bar[width:]).all()
    if rows > 1:
        acc32 = numpy.zeros(width, numpy.float32)
        for r in range(rows):
            acc32 = acc32 + host[r]
        assert acc32.dtype == numpy.float32 and (numpy.abs(acc32.astype(numpy.float64) - ref[:width]) > bar[:width]).all()
    partials = torch.zeros(2 * width * STATS_PARTS, dtype=torch.float64, device=device)
    nan = float("nan")
    one = torch.full((2 * width,), nan, dtype=torch.float64, device=device)           # accumulate = 0 overwrites whatever is there
    feature_stats(lib, x, rows, width, one, 0, partials)
    got = one.cpu().numpy()
    err = numpy.abs(got - ref)
    print("rows %d width %d: largest error / bar = %.3g" % (rows, width, (err / bar).max()))
    assert (err <= bar).all(), (rows, width, (err / bar).max())
    # two runs: the same bits
    again = torch.full((2 * width,), nan, dtype=torch.float64, device=device)
    partials.fill_(nan)
    feature_stats(lib, x, rows, width, again, 0, partials)
    assert (again.cpu().numpy().view(numpy.uint64) == got.view(numpy.uint64)).all()
    # the rows in two calls, the second accumulating (the first half of one row is no row at all)
    half = rows // 2
    acc = torch.full((2 * width,), nan, dtype=torch.float64, device=device)
    feature_stats(lib, x[:half], half, width, acc, 0, partials)
    feature_stats(lib, x[half:], rows - half, width, acc, 1, partials)
    two = acc.cpu().numpy()
    assert (numpy.abs(two - ref) <= bar).all() and (numpy.abs(two - got) <= bar).all()


@pytest.mark.parametrize("rows,width", STAT_SHAPES)
def test_feature_stats_emulated(rows, width):
    run_feature_stats("cpu", rows, width)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,width", STAT_SHAPES)
def test_feature_stats_gpu(gpu_device, rows, width):
    run_feature_stats(gpu_device, rows, width)


def run_feature_stats_refusal(device):
    lib = _lib(device)
    x = torch.zeros(2, 257, dtype=torch.float32, device=device)
    sums = torch.zeros(2 * 257, dtype=torch.float64, device=device)
    with pytest.raises(NativeError, match="lvsr_feature_stats: at most 256 columns"):
        feature_stats(lib, x, 2, 257, sums, 0, sums)


def test_feature_stats_refusal_emulated():
    run_feature_stats_refusal("cpu")


@pytest.mark.gpu
def test_feature_stats_refusal_gpu(gpu_device):
    run_feature_stats_refusal(gpu_device)
