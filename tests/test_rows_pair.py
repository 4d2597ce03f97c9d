"""The launches a training step shares between neighbours: lvsr_gather_rows_pair / lvsr_scatter_add_rows_pair (two tables by one index
list) against two calls of the single forms, and lvsr_bigru_h0_many against the per-layer sums, BIT for bit.  The bodies run on the CPU
emulator (same sources) and, under the `gpu` marker, on the device."""
import numpy
import pytest
import torch

from emu import emu_lib


def _t(rng, device, *shape):
    return torch.tensor(rng.normal(size=shape), dtype=torch.float32, device=device)


def run_gather_pair(device, lib):
    """Widths below, at and beyond one block of 256 columns; strided outputs side by side in one buffer (as the decoder's xg holds them);
    an index outside the table (reads as zero); with and without a bias; one half left out."""
    from lvsr_amd.native import ptr
    rng = numpy.random.RandomState(31)
    nrows, n = 11, 37
    idx = torch.tensor(rng.randint(0, nrows, size=n), dtype=torch.int64, device=device)
    idx[3], idx[20] = -1, nrows
    for wa, wb, biased in ((70, 300, True), (256, 1, False), (33, 0, True), (0, 257, True)):
        ta, tb = _t(rng, device, nrows, wa + 3)[:, :wa], _t(rng, device, nrows, wb + 1)[:, :wb]
        ba, bb = (_t(rng, device, wa), _t(rng, device, wb)) if biased else (None, None)
        ld = wa + wb + 5
        got, want = torch.full((n, ld), 7.0, device=device), torch.full((n, ld), 7.0, device=device)
        st = lib.stream_for(got)
        lib.call("lvsr_gather_rows_pair", st, ptr(idx), n, nrows, ptr(ta), wa + 3, wa, ptr(ba), ptr(got), ld,
                 ptr(tb), wb + 1, wb, ptr(bb), ptr(got[:, wa:]), ld)
        lib.call("lvsr_gather_rows", st, ptr(ta), wa + 3, ptr(idx), n, nrows, wa, ptr(ba), ptr(want), ld)
        lib.call("lvsr_gather_rows", st, ptr(tb), wb + 1, ptr(idx), n, nrows, wb, ptr(bb), ptr(want[:, wa:]), ld)
        assert (got.cpu().numpy() == want.cpu().numpy()).all(), (wa, wb)
        assert (got[:, wa + wb:] == 7.0).all()
        if wa:
            ref = torch.where(((idx >= 0) & (idx < nrows))[:, None], ta[idx.clamp(0, nrows - 1)], torch.zeros((), device=device))
            assert (got[:, :wa] == (ref + ba if biased else ref)).all()


def run_scatter_pair(device, lib):
    """Repeated indices (every destination row adds several source rows, in ascending order), rows nobody hits, an index outside the
    table, more rows than one staged chunk of the index list (2048), beta = 0 and 1, the two sources side by side in one buffer."""
    from lvsr_amd.native import ptr
    rng = numpy.random.RandomState(32)
    nrows = 9
    for n, wa, wb, beta in ((50, 70, 300, 0.0), (2100, 256, 40, 1.0), (17, 0, 65, 0.0)):
        idx = torch.tensor(rng.randint(0, nrows - 1, size=n), dtype=torch.int64, device=device)      # row nrows - 1 is never hit
        idx[1] = nrows + 2
        src = _t(rng, device, n, wa + wb + 2)
        ga, gb = _t(rng, device, nrows, wa + 1)[:, :wa], _t(rng, device, nrows, wb + 4)[:, :wb]
        wa_ref, wb_ref = ga.clone(), gb.clone()
        ga_back, gb_back = ga.clone(), gb.clone()
        st = lib.stream_for(src)
        lib.call("lvsr_scatter_add_rows_pair", st, ptr(idx), n, nrows, ptr(src), wa + wb + 2, wa, ptr(ga), wa + 1, beta,
                 ptr(src[:, wa:]), wa + wb + 2, wb, ptr(gb), wb + 4, beta)
        lib.call("lvsr_scatter_add_rows", st, ptr(src), wa + wb + 2, ptr(idx), n, nrows, wa, ptr(wa_ref), wa, beta)
        lib.call("lvsr_scatter_add_rows", st, ptr(src[:, wa:]), wa + wb + 2, ptr(idx), n, nrows, wb, ptr(wb_ref), wb, beta)
        assert (ga.cpu().numpy() == wa_ref.cpu().numpy()).all() and (gb.cpu().numpy() == wb_ref.cpu().numpy()).all(), (n, wa, wb)
        # against float64: the sum of the rows that hit, onto beta times what was there
        for got, before, cols in ((ga, ga_back, slice(0, wa)), (gb, gb_back, slice(wa, wa + wb))):
            ref = beta * before.double()
            ok = (idx >= 0) & (idx < nrows)
            ref.index_add_(0, idx[ok], src[ok][:, cols].double())
            numpy.testing.assert_allclose(got.cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=1e-4)


def run_h0_many(device, lib):
    """Layers of different widths (one beyond a block of 256 units) and a batch that is no multiple of 16: per unit the sum over the
    utterances in ascending order, rows of the padding never read."""
    rng = numpy.random.RandomState(33)
    B, Bp = 5, 16
    layers = []
    for H in (40, 300, 256):
        dh = _t(rng, device, 12 * Bp * H)
        dh.view(-1)[:2 * Bp * H].view(2, Bp, H)[:, B:] = float("nan")
        layers.append((H, dh, torch.zeros(H, device=device), torch.zeros(H, device=device)))
    arr = (lib.structs["lvsr_h0_desc"] * len(layers))()
    for e, (H, dh, of, ob) in zip(arr, layers):
        e.dh, e.out_f, e.out_b, e.Bp, e.B, e.H = dh.data_ptr(), of.data_ptr(), ob.data_ptr(), Bp, B, H
    lib.call("lvsr_bigru_h0_many", lib.stream_for(layers[0][1]), arr, len(layers))
    for H, dh, of, ob in layers:
        rows = dh[:2 * Bp * H].view(2, Bp, H).cpu().numpy()
        for d, out in ((0, of), (1, ob)):
            want = numpy.zeros(H, numpy.float32)
            for b in range(B):
                want = want + rows[d, b]
            assert (out.cpu().numpy() == want).all(), H


def test_gather_pair_emulated():
    run_gather_pair("cpu", emu_lib())


def test_scatter_pair_emulated():
    run_scatter_pair("cpu", emu_lib())


def test_h0_many_emulated():
    run_h0_many("cpu", emu_lib())


@pytest.mark.gpu
def test_gather_pair_gpu(gpu_device):
    from lvsr_amd import native
    run_gather_pair(gpu_device, native.get())


@pytest.mark.gpu
def test_scatter_pair_gpu(gpu_device):
    from lvsr_amd import native
    run_scatter_pair(gpu_device, native.get())


@pytest.mark.gpu
def test_h0_many_gpu(gpu_device):
    from lvsr_amd import native
    run_h0_many(gpu_device, native.get())
