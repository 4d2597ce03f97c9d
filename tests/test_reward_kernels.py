"""The kernels of the task-loss-estimation criteria (csrc/reward.hip, the argmax emitter of lvsr_readout_step), called directly:
lvsr_reward_gain against what the reference's own reward_matrix / gain_matrix wrote (tests/golden/reward_op.npz) and against a
NumPy restatement, lvsr_reward_mse against a float64 restatement of RewardRegressionEmitter.cost and its gradient, the emitter
against numpy.argmax.  Every body runs on the CPU emulator build and on the product library."""
import json
import os

import numpy
import pytest
import torch

from conftest import GOLDEN
from lvsr_amd import native
from lvsr_amd.native import ptr


# ---- NumPy restatements ---------------------------------------------------------------------------------------------------
def reward_gain_numpy(gt, pred, eos, V):
    """RewardOp.perform (lvsr/ops.py:244-285) in the column formulation: col_j[i] = edit distance between y[:i] and yhat[:j].
    A groundtruth column without EOS is used whole (the reference raises there).  -> rewards, gains (Lp,B,V) int64, mask (Lp,B)."""
    Lp, B = pred.shape
    rewards = numpy.full((Lp, B, V), -1, numpy.int64)
    gains = numpy.full((Lp, B, V), -1000, numpy.int64)
    mask = numpy.zeros((Lp, B), numpy.float32)
    for b in range(B):
        y = list(gt[:, b])
        if eos in y:
            y = y[: y.index(eos) + 1]
        y = numpy.array(y)
        yh = list(pred[:, b])
        n = yh.index(eos) + 1 if eos in yh else Lp
        ar = numpy.arange(len(y) + 1)
        col = ar.copy()
        for j in range(n):
            if j > 0:
                t = numpy.empty_like(col)
                t[0] = j
                t[1:] = numpy.minimum(prev[1:] + 1, prev[:-1] + (y != yh[j - 1]))
                col = numpy.minimum.accumulate(t - ar) + ar
            r = numpy.full(V, -(col.min() + 1), numpy.int64)
            for i in range(len(y)):
                r[y[i]] = max(r[y[i]], -col[i])
            r[eos] = -col[len(y) - 1]
            rewards[j, b] = r
            gains[j, b] = r if j == 0 else r - rewards[j - 1, b, yh[j - 1]]
            prev = col
        mask[:n, b] = 1
    return rewards, gains, mask


def reward_mse_numpy(mode, r, gains, rewards, labels, mask, min_reward):
    """RewardRegressionEmitter.cost (lvsr/bricks/__init__.py:134-183) times the mask, and d sum(cost) / d readouts, in float64."""
    r, gains, rewards = r.astype(numpy.float64), gains.astype(numpy.float64), rewards.astype(numpy.float64)
    L, B, V = r.shape
    m = numpy.ones((L, B)) if mask is None else mask.astype(numpy.float64)
    if mode == "mse_gain":
        d = r - numpy.maximum(gains, min_reward)
        return m * (d ** 2).sum(-1), 2 * m[:, :, None] * d
    li, bi = numpy.meshgrid(numpy.arange(L), numpy.arange(B), indexing="ij")
    picked = r[li, bi, labels]
    picked[0] = 0
    d = r + picked.cumsum(0)[:, :, None] - rewards
    e = 2 * m[:, :, None] * d
    dl = e.copy()
    suffix = e.sum(-1)[::-1].cumsum(0)[::-1]
    dl[li[1:], bi[1:], labels[1:]] += suffix[1:]
    return m * (d ** 2).sum(-1), dl


def _torch_cost(mode, r, gains, rewards, labels, mask, min_reward):
    """The reference's expressions, operation by operation, on torch float64 (autograd checks the hand-derived gradient above)."""
    L, B, V = r.shape
    m = torch.ones(L, B, dtype=torch.float64) if mask is None else torch.from_numpy(mask).double()
    if mode == "mse_gain":
        g = torch.clamp(torch.from_numpy(gains).double(), min=min_reward)
        return (((r - g) ** 2).sum(-1) * m)
    picked = r.reshape(L * B, V)[torch.arange(L * B), torch.from_numpy(labels).reshape(-1)].reshape(L, B)
    picked = torch.cat([torch.zeros(1, B, dtype=torch.float64), picked[1:]])
    pr = r + picked.cumsum(0)[:, :, None]
    return ((pr - torch.from_numpy(rewards).double()) ** 2).sum(-1) * m


# ---- lvsr_reward_gain ---------------------------------------------------------------------------------------------------------
def run_reward_gain(lib, device, gt, pred, eos, V, with_mask=True):
    Lp, B = pred.shape
    g, p = torch.from_numpy(gt.astype(numpy.int64)).to(device), torch.from_numpy(pred.astype(numpy.int64)).to(device)
    rw = torch.full((Lp, B, V), 7.0, device=device)
    gn = torch.full((Lp, B, V), 7.0, device=device)
    pm = torch.full((Lp, B), 7.0, device=device) if with_mask else None
    lib.call("lvsr_reward_gain", lib.stream_for(rw), ptr(g), int(gt.shape[0]), ptr(p), Lp, B, int(eos), int(V), ptr(rw), ptr(gn), ptr(pm))
    return rw.cpu().numpy(), gn.cpu().numpy(), None if pm is None else pm.cpu().numpy()


def load_reward_fixture():
    z = numpy.load(os.path.join(GOLDEN, "reward_op.npz"), allow_pickle=False)
    return z, json.loads(str(z["meta"]))


def random_case(rng, k):
    V = int(rng.randint(2, 9))
    eos = int(rng.choice([0, V - 1, rng.randint(V)]))
    B, Lg, Lp = int(rng.randint(1, 4)), int(rng.randint(1, 9)), int(rng.randint(1, 12))
    gt = rng.randint(V, size=(Lg, B))
    gt[rng.randint(Lg, size=B), numpy.arange(B)] = eos          # at least one EOS per groundtruth column, anywhere
    pred = rng.randint(V, size=(Lp, B))
    if k % 3 == 0:                                                # predictions close to the groundtruth
        n = min(Lg, Lp)
        pred[:n] = gt[:n]
        pred[rng.randint(Lp), rng.randint(B)] = rng.randint(V)
    return gt, pred, eos, V


def check_reward_gain(lib, device):
    z, meta = load_reward_fixture()
    for k, case in enumerate(meta["cases"]):
        gt, pred, eos, V = z["gt%d" % k], z["pred%d" % k], case["eos"], case["V"]
        want_r, want_g = z["rewards%d" % k].astype(numpy.int64), z["gains%d" % k].astype(numpy.int64)
        # the restatement equals the reference's own functions, the kernel equals both
        nr, ng, nm = reward_gain_numpy(gt, pred, eos, V)
        assert numpy.array_equal(nr, want_r) and numpy.array_equal(ng, want_g), case
        rw, gn, pm = run_reward_gain(lib, device, gt, pred, eos, V)
        assert numpy.array_equal(rw, want_r.astype(numpy.float32)), case
        assert numpy.array_equal(gn, want_g.astype(numpy.float32)), case
        assert numpy.array_equal(pm, nm), case
    rng = numpy.random.RandomState(11)
    for k in range(50):
        gt, pred, eos, V = random_case(rng, k)
        nr, ng, nm = reward_gain_numpy(gt, pred, eos, V)
        rw, gn, pm = run_reward_gain(lib, device, gt, pred, eos, V, with_mask=k % 2 == 0)
        assert numpy.array_equal(rw, nr.astype(numpy.float32)) and numpy.array_equal(gn, ng.astype(numpy.float32)), (k, gt, pred, eos)
        assert pm is None or numpy.array_equal(pm, nm)
    # a groundtruth without EOS (the reference raises): the whole column is used, nothing faults
    gt, pred = numpy.array([[1, 2], [2, 2], [3, 1]]), numpy.array([[1, 2], [3, 2], [0, 1], [2, 0]])
    nr, ng, nm = reward_gain_numpy(gt, pred, 0, 5)
    rw, gn, pm = run_reward_gain(lib, device, gt, pred, 0, 5)
    assert numpy.array_equal(rw, nr) and numpy.array_equal(gn, ng) and numpy.array_equal(pm, nm)
    # the limits of the LDS layout are refused by name
    big = numpy.zeros((1025, 1), numpy.int64)
    with pytest.raises(native.NativeError, match="RG_MAX_Y"):
        run_reward_gain(lib, device, big, pred[:, :1], 0, 5)
    with pytest.raises(native.NativeError, match="RG_MAX_V"):
        run_reward_gain(lib, device, gt[:, :1], pred[:, :1], 0, 2049)
    # ... and hold what they promise: 1023 groundtruth characters + EOS
    gt = numpy.concatenate([1 + numpy.arange(1023) % 3, [0]])[:, None]
    pred = numpy.concatenate([gt[5:200, 0], [0]])[:, None]
    nr, ng, nm = reward_gain_numpy(gt, pred, 0, 4)
    rw, gn, pm = run_reward_gain(lib, device, gt, pred, 0, 4)
    assert numpy.array_equal(rw, nr) and numpy.array_equal(gn, ng) and numpy.array_equal(pm, nm)


def test_reward_gain_emulated():
    from emu import emu_lib
    check_reward_gain(emu_lib(), torch.device("cpu"))


@pytest.mark.gpu
def test_reward_gain_gpu(gpu_device):
    check_reward_gain(native.get(), gpu_device)


# ---- lvsr_reward_mse ------------------------------------------------------------------------------------------------------------
MSE_CASES = [(mode, V, masked, mr) for mode in ("mse_gain", "mse_reward") for V in (5, 65) for masked in (False, True) for mr in (-1.0, -5.0)]


def check_reward_mse(lib, device, mode, V, masked, min_reward):
    L, B, eos = 12, 3, 0
    rng = numpy.random.RandomState(V + 7 * masked)
    gt = rng.randint(1, V, size=(8, B))
    gt[[7, 4, 5], numpy.arange(B)] = eos
    pred = rng.randint(1, V, size=(L, B))
    pred[:6] = gt[:6]
    pred[2, 0], pred[4, 1], pred[9, 1] = 3, 2, eos                   # EOS absent / later than / at the groundtruth's position
    rewards, gains, pmask = reward_gain_numpy(gt, pred, eos, V)
    rewards, gains = rewards.astype(numpy.float32), gains.astype(numpy.float32)
    r = (2.0 * rng.randn(L, B, V)).astype(numpy.float32)
    mask = pmask if masked else None
    want_c, want_d = reward_mse_numpy(mode, r, gains, rewards, pred, mask, min_reward)
    # the hand-derived gradient of the restatement is the autograd gradient of the reference's expressions
    rt = torch.from_numpy(r).double().requires_grad_()
    ct = _torch_cost(mode, rt, gains, rewards, pred, mask, min_reward)
    ct.sum().backward()
    numpy.testing.assert_allclose(want_c, ct.detach().numpy(), rtol=1e-12, atol=1e-12)
    numpy.testing.assert_allclose(want_d, rt.grad.numpy(), rtol=1e-12, atol=1e-9)
    t = lambda x, dt=torch.float32: None if x is None else torch.from_numpy(numpy.ascontiguousarray(x)).to(dt).to(device)
    rd, gd, wd, ld_, md = t(r), t(gains), t(rewards), t(pred, torch.int64), t(mask)
    cost = torch.full((L, B), 7.0, device=device)
    dl = torch.full((L * B, V), 7.0, device=device)
    lib.call("lvsr_reward_mse", lib.stream_for(cost), 0 if mode == "mse_gain" else 1, ptr(rd), V, ptr(gd), ptr(wd), ptr(ld_), ptr(md),
             L, B, V, float(min_reward), ptr(cost), ptr(dl), V)
    got_c, got_d = cost.cpu().numpy(), dl.cpu().numpy().reshape(L, B, V)
    # float32 additions feeding one element: at most L (prefix / suffix over labels) + V (over classes), 8x for the products' roundings
    tol = 8 * (L + V) * 2.0 ** -24
    err_c, err_d = numpy.abs(got_c - want_c).max(), numpy.abs(got_d - want_d).max()
    print("%s V=%d masked=%s min_reward=%g: cost error %.3g (bound %.3g), gradient error %.3g (bound %.3g)"
          % (mode, V, masked, min_reward, err_c, tol * numpy.abs(want_c).max(), err_d, tol * numpy.abs(want_d).max()))
    assert err_c <= tol * numpy.abs(want_c).max()
    assert err_d <= tol * numpy.abs(want_d).max()
    if masked:
        off = mask == 0
        assert off.any() and (got_c[off] == 0).all() and (got_d[off] == 0).all()


def check_reward_mse_limit(lib, device):
    """mse_reward keeps a prefix and a suffix sum per label position in LDS: more than RM_MAX_L = 4096 positions are refused by name;
    mse_gain has no such limit."""
    L, B, V = 4097, 1, 2
    z = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device=device)
    r, g, w, lab, cost, dl = z(L * B, V), z(L, B, V), z(L, B, V), z(L, B, dt=torch.int64), z(L, B), z(L * B, V)
    g.fill_(-3.0)
    args = lambda mode: (lib.stream_for(cost), mode, ptr(r), V, ptr(g), ptr(w), ptr(lab), None, L, B, V, -1.0, ptr(cost), ptr(dl), V)
    with pytest.raises(native.NativeError, match="RM_MAX_L"):
        lib.call("lvsr_reward_mse", *args(1))
    lib.call("lvsr_reward_mse", *args(0))
    assert float(cost.min()) == 2.0 and float(cost.max()) == 2.0 and float(dl.max()) == 2.0          # (0 - max(-3, -1))^2 per class


def test_reward_mse_limit_emulated():
    from emu import emu_lib
    check_reward_mse_limit(emu_lib(), torch.device("cpu"))


@pytest.mark.gpu
def test_reward_mse_limit_gpu(gpu_device):
    check_reward_mse_limit(native.get(), gpu_device)


@pytest.mark.parametrize("mode,V,masked,min_reward", MSE_CASES)
def test_reward_mse_emulated(mode, V, masked, min_reward):
    from emu import emu_lib
    check_reward_mse(emu_lib(), torch.device("cpu"), mode, V, masked, min_reward)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,V,masked,min_reward", MSE_CASES)
def test_reward_mse_gpu(gpu_device, mode, V, masked, min_reward):
    check_reward_mse(native.get(), gpu_device, mode, V, masked, min_reward)


# ---- lvsr_readout_step with the reward-regression emitter -------------------------------------------------------------------------
def check_argmax_emitter(lib, device):
    import ctypes
    n, E, V = 6, 3, 70
    rng = numpy.random.RandomState(5)
    W = rng.uniform(-1, 1, size=(E, V)).astype(numpy.float32)
    W[0, 7] = W[0, 66] = 5.0            # row 0: classes 7 and 66 tie (different lanes); the first wins
    W[1, 3] = W[1, 67] = 5.0            # row 1: classes 3 and 67 tie (the same lane)
    wa = rng.uniform(-1, 1, size=(n, E)).astype(numpy.float32)
    wa[0], wa[1] = [1, 0, 0], [0, 1, 0]
    t = lambda x: torch.from_numpy(x).to(device)
    Wd, wad, bias = t(W), t(wa), torch.zeros(V, device=device)
    logits, neglogp = torch.full((n, V), 7.0, device=device), torch.full((n, V), 7.0, device=device)
    outputs, costs = torch.full((n,), -1, dtype=torch.int64, device=device), torch.full((n,), 7.0, device=device)
    args = lib.make("lvsr_readout_step_args", S=None, WA=wad, lds=0, ldwa=E, n=n, D=0, E=E, P=V, V=V, act=0, Wms=None, Wmw=Wd, bias1=bias,
                    Wout=None, bout=None, lm_add=None, am_beta=1.0, lm_weight=0.0, norm_am=1, norm_lm=0, norm_tot=0, neglogp=neglogp,
                    logits=logits, uniforms=None, outputs=outputs, costs=costs, n_hidden=0, R1=None, ldr1=0, emitter=1)
    lib.call("lvsr_readout_step", lib.stream_for(logits), ctypes.byref(args))
    lg, nl, out, c = logits.cpu().numpy(), neglogp.cpu().numpy(), outputs.cpu().numpy(), costs.cpu().numpy()
    numpy.testing.assert_allclose(lg, wa @ W, rtol=1e-5, atol=1e-6)
    assert lg[0, 7] == lg[0, 66] == lg[0].max() and lg[1, 3] == lg[1, 67] == lg[1].max()
    assert numpy.array_equal(nl.view(numpy.uint32), (-lg).view(numpy.uint32))            # bit for bit
    assert numpy.array_equal(out, lg.argmax(axis=1)) and out[0] == 7 and out[1] == 3
    assert numpy.array_equal(c, lg[numpy.arange(n), out])


def test_argmax_emitter_emulated():
    from emu import emu_lib
    check_argmax_emitter(emu_lib(), torch.device("cpu"))


@pytest.mark.gpu
def test_argmax_emitter_gpu(gpu_device):
    check_argmax_emitter(native.get(), gpu_device)
