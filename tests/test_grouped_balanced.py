"""lvsr_sgemm_tn_grouped: one product launch for members of any alignment and depth, one fold launch over all outputs; the cut into
k-chunks through lvsr_sgemm_tn_grouped_plan.  Every body runs on the CPU emulator (same sources) and, under the `gpu` marker, on the device."""
import ctypes

import numpy
import pytest
import torch
from numpy.testing import assert_allclose

from emu import emu_lib

GROUP_MAX = 40          # csrc/gemm.hip


def _descs(lib, jobs, outs):
    arr = (lib.structs["lvsr_gemm_desc"] * len(jobs))()
    for d, (A, B, _, beta), C in zip(arr, jobs, outs):
        d.A, d.B, d.C, d.M, d.N, d.K = A.data_ptr(), B.data_ptr(), C.data_ptr(), A.shape[1], B.shape[1], A.shape[0]
        d.lda, d.ldb, d.ldc, d.beta = A.stride(0), B.stride(0), C.stride(0), beta
    return arr


def grouped(lib, jobs, outs, ws):
    """One lvsr_sgemm_tn_grouped call: jobs = [(A, B, C0, beta)], outputs into `outs`."""
    from lvsr_amd.native import ptr
    lib.call("lvsr_sgemm_tn_grouped", lib.stream_for(outs[0]), _descs(lib, jobs, outs), len(jobs), ptr(ws),
             ws.numel() * 4 if ws is not None else 0)


def plan(lib, jobs, outs, ws_bytes):
    """-> (ksplit, kchunk) per member, as the call above cuts them."""
    ks, kc = (ctypes.c_int * len(jobs))(), (ctypes.c_int * len(jobs))()
    lib.call("lvsr_sgemm_tn_grouped_plan", _descs(lib, jobs, outs), len(jobs), ws_bytes, ks, kc)
    return list(ks), list(kc)


PAD = 123.0             # what the columns of an output's backing buffer beyond N hold


def _outputs(jobs):
    """-> one output per job with C0's values AND C0's row stride (a clone of a column view would come back dense): a view of a backing
    buffer whose other columns hold PAD."""
    outs = []
    for _, _, C0, _ in jobs:
        back = torch.full((C0.shape[0], C0.stride(0)), PAD, device=C0.device)
        out = back[:, :C0.shape[1]]
        out.copy_(C0)
        assert out.stride(0) == C0.stride(0) and out.data_ptr() == back.data_ptr()
        outs.append(out)
    return outs


def _backing(out):
    return torch.as_strided(out, (out.shape[0], out.stride(0)), (out.stride(0), 1))


def _check(jobs, outs):
    for i, ((A, B, C0, beta), C) in enumerate(zip(jobs, outs)):
        ref = A.double().T @ B.double() + beta * C0.double()
        assert_allclose(C.cpu().numpy(), ref.cpu().numpy(), rtol=2e-4, atol=2e-4, err_msg="member %d" % i)
        assert (_backing(C)[:, C.shape[1]:] == PAD).all(), "member %d: columns beyond N of a strided output were written" % i


def _mixed_jobs(device):
    rng = numpy.random.RandomState(21)
    t = lambda *s: torch.tensor(rng.normal(size=s), dtype=torch.float32, device=device)
    K1, K2 = 2100, 1100                                                            # neither a multiple of 32
    return [(t(K1, 300)[:, 4:4 + 130], t(K1, 70), t(130, 100)[:, :70], 1.0),      # strided A, M = 130, ldc = 100 > N, beta = 1
            (t(K2, 40), t(K2, 260)[:, 8:8 + 132], t(40, 132), 1.0),                 # N = 132: two tile columns, beta = 1
            (t(K2, 64), t(K2, 33), torch.zeros(64, 33, device=device), 0.0),        # ldb = 33: guarded loads
            (t(K1, 34), t(K1, 256), torch.zeros(34, 256, device=device), 0.0),      # lda = 34: guarded loads
            (t(K2, 256), t(K2, 128), t(256, 160)[:, :128], 1.0),                    # whole tiles: the unguarded loads; ldc = 160, 16-B fold
            (t(50, 16), t(50, 16), torch.zeros(16, 16, device=device), 0.0)]        # K below any chunk


def run_mixed_alignment(device, lib):
    """Aligned and misaligned members in one call, ragged M / N / K, beta = 1 onto a strided output view — with a workspace (members
    are cut, the fold runs) and without one (one chunk per tile)."""
    jobs = _mixed_jobs(device)
    for ws in (torch.empty(1 << 20, device=device), None):
        outs = _outputs(jobs)
        assert outs[0].stride(0) == 100 and outs[4].stride(0) == 160, "beta = 1 onto strided output views, ldc > N"
        ksplit, kchunk = plan(lib, jobs, outs, ws.numel() * 4 if ws is not None else 0)
        assert all(c % 32 == 0 and s * c >= A.shape[0] > (s - 1) * c for s, c, (A, _, _, _) in zip(ksplit, kchunk, jobs))
        assert ksplit[-1] == 1 and (max(ksplit) > 1) == (ws is not None)
        if ws is not None:
            assert ksplit[2] > 1 and ksplit[3] > 1, "the members on the guarded loads are cut too"
            assert ksplit[0] > 1 and ksplit[4] > 1, "the fold writes both strided outputs: four scalars a thread, and a float4"
        grouped(lib, jobs, outs, ws)
        _check(jobs, outs)


def run_small_workspace(device, lib):
    """A workspace a few KB larger than ONE partial of the largest output: the common chunk depth grows beyond 1024 until the partials
    fit.  Here: room for two chunks each of the two K = 2100 members (35 608 floats), not for three and not for any cut of the K = 1100
    members — deeper chunks than with a large workspace, and members that are still cut, so partials are written and the fold runs."""
    jobs = _mixed_jobs(device)
    outs = _outputs(jobs)
    ws_floats = 36000
    assert max(c.shape[0] * c.shape[1] for c in outs) < ws_floats < max(c.shape[0] * c.shape[1] for c in outs) + 4096
    ksplit, kchunk = plan(lib, jobs, outs, ws_floats * 4)
    roomy, roomy_chunk = plan(lib, jobs, outs, 1 << 22)
    assert sum((s * c.shape[0] * c.shape[1] + 3) // 4 * 4 for s, c in zip(ksplit, outs) if s > 1) <= ws_floats
    assert ksplit == [2, 1, 1, 2, 1, 1] and roomy == [3, 2, 2, 3, 2, 1], (ksplit, roomy)
    assert kchunk[0] > roomy_chunk[0] > 0 and kchunk[0] > 1024
    ws = torch.full((ws_floats + 64,), PAD, device=device)
    grouped(lib, jobs, outs, ws[:ws_floats])
    _check(jobs, outs)
    assert (ws[ws_floats:] == PAD).all(), "partials were written behind the workspace"


def run_more_than_one_launch(device, lib):
    """45 members: the call spills into a second launch."""
    rng = numpy.random.RandomState(22)
    t = lambda *s: torch.tensor(rng.normal(size=s), dtype=torch.float32, device=device)
    jobs = []
    for i in range(GROUP_MAX + 5):
        K, M, N = 300 + 37 * i, 16 + 8 * (i % 5), 24 + (i % 3)
        jobs.append((t(K, M), t(K, N), t(M, N), float(i % 2)))
    outs = _outputs(jobs)
    grouped(lib, jobs, outs, torch.empty(1 << 20, device=device))
    _check(jobs, outs)


def run_unequal_depths(device, lib):
    """One member twenty times as deep as the others (the encoder's fork gradient beside the decoder's products): correct, the deep one
    cut into more chunks than the shallow ones, and the same bits when the call is made again."""
    rng = numpy.random.RandomState(23)
    t = lambda *s: torch.tensor(rng.normal(size=s), dtype=torch.float32, device=device)
    jobs = [(t(2400, 256), t(2400, 288), torch.zeros(256, 288, device=device), 0.0)]
    jobs += [(t(120, 64 + 32 * i), t(120, 96), torch.zeros(64 + 32 * i, 96, device=device), 0.0) for i in range(4)]
    ws = torch.empty(1 << 20, device=device)
    outs = _outputs(jobs)
    ksplit, _ = plan(lib, jobs, outs, ws.numel() * 4)
    assert ksplit[0] > 1 and ksplit[1:] == [1] * 4
    grouped(lib, jobs, outs, ws)
    _check(jobs, outs)
    again = _outputs(jobs)
    ws.fill_(7.0)
    grouped(lib, jobs, again, ws)
    for a, b in zip(outs, again):
        assert (a.cpu().numpy() == b.cpu().numpy()).all()


def run_fold_order(device, lib):
    """The fold == the sequential float32 sum of the chunk products in ascending chunk order, bit for bit: N = 33 (scalar path) and
    N = 64 with an aligned output (16-byte path), five chunks each (K = 4200: the cut is ~1024 deep, so five chunks need K > 4096).
    In front of the 16-byte member sits an aligned one with 5 * 7 * 9 = 315 floats of partials: an odd count, rounded up to a multiple of
    4 so that the next member's partials stay 16-byte aligned.  The chunk products come from the same kernel, one chunk per call
    without a workspace."""
    rng = numpy.random.RandomState(24)
    t = lambda *s: torch.tensor(rng.normal(size=s), dtype=torch.float32, device=device)
    K = 4200
    jobs = [(t(K, 48), t(K, 33), torch.zeros(48, 33, device=device), 0.0),
            (t(K, 8)[:, :7], t(K, 12)[:, :9], torch.zeros(7, 9, device=device), 0.0),
            (t(K, 130), t(K, 64), torch.zeros(130, 80, device=device)[:, :64], 0.0)]
    ws = torch.empty(1 << 20, device=device)
    outs = _outputs(jobs)
    ksplit, kchunk = plan(lib, jobs, outs, ws.numel() * 4)
    assert min(ksplit) >= 5 and (ksplit[1] * 7 * 9) % 4 != 0 and outs[2].stride(0) == 80, ksplit
    grouped(lib, jobs, outs, ws)
    for (A, B, C0, _), C, s, c in zip(jobs, outs, ksplit, kchunk):
        acc = numpy.zeros(tuple(C0.shape), numpy.float32)
        for z in range(s):
            part = torch.zeros(tuple(C0.shape), device=device)
            grouped(lib, [(A[z * c: (z + 1) * c], B[z * c: (z + 1) * c], C0, 0.0)], [part], None)
            acc = acc + part.cpu().numpy()
        assert acc.dtype == numpy.float32 and (C.cpu().numpy() == acc).all(), float(numpy.abs(C.cpu().numpy() - acc).max())


def test_mixed_alignment_emulated():
    run_mixed_alignment("cpu", emu_lib())


def test_small_workspace_emulated():
    run_small_workspace("cpu", emu_lib())


def test_more_than_one_launch_emulated():
    run_more_than_one_launch("cpu", emu_lib())


def test_unequal_depths_emulated():
    run_unequal_depths("cpu", emu_lib())


def test_fold_order_emulated():
    run_fold_order("cpu", emu_lib())


def test_cut_depends_on_sizes_only():
    """The cut fixes the order of every sum, so it may depend on M, N, K and the workspace size alone: the same sizes with other leading
    dimensions, on guarded instead of unguarded loads and at other addresses are cut alike."""
    lib = emu_lib()
    t = lambda *s: torch.zeros(*s)
    sizes = [(2100, 64, 32), (1100, 32, 96), (5000, 16, 16)]
    aligned = [(t(K, M), t(K, N), t(M, N), 0.0) for K, M, N in sizes]
    guarded = [(t(K, M + 2)[:, 1:1 + M], t(K, N + 1)[:, :N], t(M, N + 3)[:, :N], 1.0) for K, M, N in sizes]
    for ws_bytes in (1 << 22, 40000, 0):
        cuts = [plan(lib, jobs, _outputs(jobs), ws_bytes) for jobs in (aligned, guarded)]
        assert cuts[0] == cuts[1], (ws_bytes, cuts)
    assert plan(lib, aligned, _outputs(aligned), 1 << 22)[0] == [3, 2, 5] and plan(lib, aligned, _outputs(aligned), 0)[0] == [1, 1, 1]


def test_encoder_backward_with_and_without_group():
    """Encoder.backward with a GemmGroup (the recurrent weight gradients and the fork column sums leave at the flush, the fork
    products launch at once) and without one (everything launches at once): the same gradients, and the float64 oracle's."""
    from oracle import lvsr_oracle as O
    from lvsr_amd import spec, synthetic
    from lvsr_amd.params import ParameterStore, Workspace
    from lvsr_amd.bricks import Encoder
    lib = emu_lib()
    cfg = dict(input_dim=5, num_phonemes=6, dims_bidir=[32, 32], subsample=[1, 1], dim_dec=4, dim_matcher=7,
               attention_type="content", post_merge_dims=None, embed_outputs=True)
    T, B = 12, 3
    params = synthetic.make_params(cfg, seed=3)
    batch = synthetic.make_batch(cfg, B, T, 4, seed=5, ragged=True)
    x, m = torch.tensor(batch["recordings"]), torch.tensor(batch["recordings_mask"])
    orc = O.OracleRecognizer(cfg, params, dtype=torch.float64)
    enc_ref, _ = orc.encode(x.double(), m.double())
    dy = torch.tensor(numpy.random.RandomState(0).normal(size=tuple(enc_ref.shape)), dtype=torch.float64)
    (enc_ref * dy).sum().backward()
    got = {}
    for with_group in (False, True):
        store = ParameterStore(cfg, "cpu", params)
        ws = Workspace("cpu")
        enc = Encoder(spec.Dims(cfg), store, lib, ws, use_graph=False)
        enc.apply(x, m)
        if with_group:
            group = lib.group()
            enc.backward(dy.float(), group=group)
            assert len(group.first) == 2 * 4, "per layer: two recurrent products per direction"
            group.flush(ws.get("gemm_ws.grouped", (1 << 20,)))
            enc.finish_backward()
        else:
            enc.backward(dy.float())
        got[with_group] = {k: g.numpy().copy() for k, g in store.g.items() if "/encoder/" in k}
    for name, g in got[True].items():
        assert_allclose(g, got[False][name], rtol=2e-4, atol=2e-4, err_msg=name)
        for which in (False, True):
            assert_allclose(got[which][name], orc.p[name].grad.numpy(), rtol=2e-4, atol=2e-4, err_msg=name)


# ---- the same bodies on the device ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_mixed_alignment(gpu_device):
    from lvsr_amd import native
    run_mixed_alignment(gpu_device, native.get())


@pytest.mark.gpu
def test_small_workspace(gpu_device):
    from lvsr_amd import native
    run_small_workspace(gpu_device, native.get())


@pytest.mark.gpu
def test_more_than_one_launch(gpu_device):
    from lvsr_amd import native
    run_more_than_one_launch(gpu_device, native.get())


@pytest.mark.gpu
def test_unequal_depths(gpu_device):
    from lvsr_amd import native
    run_unequal_depths(gpu_device, native.get())


@pytest.mark.gpu
def test_fold_order(gpu_device):
    from lvsr_amd import native
    run_fold_order(gpu_device, native.get())


@pytest.mark.gpu
def test_eager_and_captured_region_agree(gpu_device):
    """The same call eager, captured into a Region and replayed: bit-identical outputs (the plan does not depend on how it is launched)."""
    from lvsr_amd import native
    lib = native.get()
    jobs = _mixed_jobs(gpu_device)
    jobs = [(A, B, C0, 0.0) for A, B, C0, _ in jobs]
    ws = torch.empty(1 << 20, device=gpu_device)
    eager = _outputs(jobs)
    grouped(lib, jobs, eager, ws)
    torch.cuda.synchronize()
    _check(jobs, eager)

    class Owner(object):
        pass
    owner, outs = Owner(), _outputs(jobs)
    side = torch.cuda.Stream(gpu_device)         # a capture needs a non-null stream
    states = []
    for rep in range(3):
        for o in outs:
            o.fill_(float("nan"))
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            region = lib.region(owner, ("grouped",), outs[0])
            region.run(lambda: grouped(lib, jobs, outs, ws))
        torch.cuda.synchronize()
        states.append(region.state)
        for a, b in zip(eager, outs):
            assert (a.cpu().numpy() == b.cpu().numpy()).all(), (rep, region.state)
    assert states == ["eager", "captured", "replayed"], states
