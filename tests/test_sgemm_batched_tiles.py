"""lvsr_sgemm_batched picks its tile like lvsr_sgemm does, counting the 128-tiles of all members: few of them run on 64 x 64 tiles.  Both
tile kernels contract over k in ascending order, so every member must equal the unbatched product of its slice BIT for bit whichever
tile either call selects.  The bodies run on the CPU emulator (same sources) and, under the `gpu` marker, on the device."""
import numpy
import pytest
import torch
from numpy.testing import assert_allclose

from emu import emu_lib


def _operand(rng, device, rows, cols, ld):
    """(rows, cols) view with row stride `ld` of a buffer whose other columns hold a marker."""
    back = torch.full((rows, ld), 77.0, device=device)
    back[:, :cols] = torch.tensor(rng.normal(size=(rows, cols)), dtype=torch.float32, device=device)
    return back[:, :cols]


def run_slices(device, lib, layout, M, N, K, batch, pad=0, knob=0):
    """Members stacked along the rows of each operand (stride = rows x leading dimension); `pad`: extra columns in every leading
    dimension (pad = 1: no multiple of 4, so no member but the first is 16-byte aligned either: the guarded loads).
    layout "NT": C = A (M,K) @ B (N,K)^T, the QR product of the decoder's backward pass; "TN": C = A (K,M)^T @ B (K,N), beta = 1, its
    dA product."""
    from lvsr_amd.native import ptr
    rng = numpy.random.RandomState(M + N + K + batch)
    transA, transB = layout == "TN", layout == "NT"
    ar, ac = (K, M) if transA else (M, K)
    br, bc = (N, K) if transB else (K, N)
    A = _operand(rng, device, batch * ar, ac, ac + pad)
    B = _operand(rng, device, batch * br, bc, bc + pad)
    C0 = torch.tensor(rng.normal(size=(batch * M, N)), dtype=torch.float32, device=device)
    beta = 1.0 if transA else 0.0
    C = torch.full((batch * M, N + pad), 77.0, device=device)[:, :N]
    C.copy_(C0)
    lib.set_knob("gemm_mid_tiles", knob)
    try:
        lib.call("lvsr_sgemm_batched", lib.stream_for(C), int(transA), int(transB), M, N, K, 0.5, ptr(A), A.stride(0), ar * A.stride(0),
                 ptr(B), B.stride(0), br * B.stride(0), beta, ptr(C), C.stride(0), M * C.stride(0), batch)
    finally:
        lib.set_knob("gemm_mid_tiles", 0)
    for b in (range(batch) if batch <= 8 else (0, batch // 2 + 1, batch - 1)):          # (many members: first, one inside, last)
        Ab, Bb = A[b * ar: (b + 1) * ar], B[b * br: (b + 1) * br]
        single = C0[b * M: (b + 1) * M].clone()
        lib.sgemm(Ab, Bb, single, transA=transA, transB=transB, alpha=0.5, beta=beta)
        got = C[b * M: (b + 1) * M]
        assert (got.cpu().numpy() == single.cpu().numpy()).all(), \
            "member %d differs from its unbatched product (max %g)" % (b, float((got - single).abs().max()))
        ref = 0.5 * ((Ab.T if transA else Ab).double() @ (Bb.T if transB else Bb).double()) + beta * C0[b * M: (b + 1) * M].double()
        # (the tolerances of tests/test_emu_gemm.py: its layout cases for short contractions, its tile-shape case for long ones)
        rtol, atol = (1e-5, 1e-5) if K <= 80 else (2e-5, 2e-4)
        assert_allclose(got.cpu().numpy(), ref.cpu().numpy(), rtol=rtol, atol=atol)
    if pad:
        back = torch.as_strided(C, (C.shape[0], C.stride(0)), (C.stride(0), 1))
        assert (back[:, N:] == 77.0).all(), "columns beyond N of a strided output were written"


# the step's two batched products at three utterances; a ragged shape on a leading dimension that is no multiple of 4
SMALL = [(100, 200, 512, 3, 0), (200, 512, 100, 3, 0), (65, 70, 33, 2, 1)]


@pytest.mark.parametrize("layout", ["NT", "TN"])
@pytest.mark.parametrize("M,N,K,batch,pad", SMALL)
def test_batched_members_equal_unbatched_emulated(layout, M, N, K, batch, pad):
    run_slices("cpu", emu_lib(), layout, M, N, K, batch, pad)


@pytest.mark.parametrize("layout", ["NT", "TN"])
def test_batched_on_128_tiles_equals_unbatched_on_64_tiles_emulated(layout):
    """128 members of two 128-tiles each: 256 tiles, which stay on 128 x 128 tiles under knob gemm_mid_tiles = 1 (never the 64-tiles
    beyond the first 255), while the unbatched product of a slice (two tiles) runs on 64 x 64 tiles.  (One ragged k-tile: 256
    emulated 128-tiles are seconds of CPU time each k-tile; the device twin runs deeper contractions.)"""
    run_slices("cpu", emu_lib(), layout, 130, 100, 24, 128, knob=1)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["NT", "TN"])
@pytest.mark.parametrize("M,N,K,batch,pad", SMALL)
def test_batched_members_equal_unbatched_gpu(gpu_device, layout, M, N, K, batch, pad):
    from lvsr_amd import native
    run_slices(gpu_device, native.get(), layout, M, N, K, batch, pad)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["NT", "TN"])
def test_batched_on_128_tiles_equals_unbatched_on_64_tiles_gpu(gpu_device, layout):
    """As the emulated case, and at the step's own shape with a contraction beyond 2048, which keeps 256 tiles on 128 x 128 tiles by
    default."""
    from lvsr_amd import native
    run_slices(gpu_device, native.get(), layout, 130, 100, 40, 128, knob=1)
    run_slices(gpu_device, native.get(), layout, 100, 200, 2080, 128)
