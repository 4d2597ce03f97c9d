"""The training / validation observables (csrc/observables.hip, lvsr_amd/observables.py): the three kernels against what the
reference's own expressions wrote (tests/golden/misc_reference.npz) and against float64 NumPy restatements of
lvsr/expressions.py:14-25 and lvsr/main.py:534-541, then inside the training step (eager, captured, replayed), and through the
stage driver.  Every body runs on the CPU emulator build and on the GPU."""
import math
import os
import sys

import numpy
import pytest
import torch
import torch.multiprocessing as mp
from numpy.testing import assert_allclose

from conftest import golden_path
from lvsr_amd import observables as OBS
from lvsr_amd import synthetic
from lvsr_amd.bricks.recognizer import SpeechRecognizer
from lvsr_amd.params import Workspace
from lvsr_amd.training import Trainer
from test_adaptive_noise import _dataset, _free_port, _lib
from test_mse_criterion import CFG, GREEDY_L, GREEDY_T, mse_cfg

U = 2.0 ** -24                     # unit roundoff of float32


# ---- float64 restatements ---------------------------------------------------------------------------------------------------
def penalty_numpy(w, mask=None):
    """monotonicity_penalty (lvsr/expressions.py:14-19): the two cumulative sums taken separately, then subtracted."""
    c = numpy.cumsum(w.astype(numpy.float64), axis=2)
    p = numpy.maximum(c[1:] - c[:-1], 0).sum(axis=2)
    if mask is not None:
        p = p * mask[1:].astype(numpy.float64)
    return p.sum()


def entropy_numpy(w, mask=None):
    """entropy (lvsr/expressions.py:22-25): the reference's sign (not negated)."""
    w = w.astype(numpy.float64)
    e = (w * numpy.log(w + 1e-7)).sum(axis=2)
    if mask is not None:
        e = e * mask.astype(numpy.float64)
    return e.sum()


def segment_norms_numpy(seg, p, g, s, grad_scale):
    """lvsr/main.py:534-541 per row of the segment table, in float64 -> (nseg,3) [norm, gradient norm, step norm] / sqrt(size)."""
    out = numpy.zeros((len(seg), 3))
    for i, (off, rows, cols, _) in enumerate(seg):
        n = rows * cols
        gs = (g[off:off + n] * numpy.float32(grad_scale)).astype(numpy.float64)       # the float32 product the optimiser forms too
        out[i] = [math.sqrt((x ** 2).sum()) / math.sqrt(n) for x in (p[off:off + n].astype(numpy.float64), gs, s[off:off + n].astype(numpy.float64))]
    return out


def align_bounds(L, B, Tp, penalty, entropy):
    """Worst-case float32 deviation of the kernel's own summation order (u = 2^-24).
    A scanned prefix of values that sum to at most 1: six rounded additions of the 64-lane scan, one to add the carry, and the
    carry itself went through ceil(T'/64) chunks: c = 7 + ceil(T'/64) roundings of values <= 1, so <= c u.  A penalty term
    max(C1 - C0, 0): both prefixes (2 c u) and the subtraction (u).  A row folds T' such terms, each <= 1, with ceil(T'/64)
    lane-strided additions and the six of the xor tree: (ceil(T'/64) + 6) u T' more.  So a row is off by at most T' (3 c + 1) u; the
    rows are added in float64 and the total is rounded once (|total| u).
    An entropy term w logf(w + 1e-7f): the rounded argument moves the logarithm by u (w u in the term), logf is good to 2 ulp and
    the product is rounded (3 u |term|): <= 4 u max(|term|, w); over a row sum w <= 1 and sum |term| <= ln T' + 1, and the fold adds
    (ceil(T'/64) + 6) u (ln T' + 1): a row is off by at most (ceil(T'/64) + 10) (ln T' + 1) u."""
    chunks = -(-Tp // 64)
    c = 7 + chunks
    pen = max(L - 1, 0) * B * Tp * (3 * c + 1) * U + abs(penalty) * U
    ent = L * B * (chunks + 10) * (math.log(Tp) + 1) * U + abs(entropy) * U
    return pen, ent


# ---- calling the kernels ------------------------------------------------------------------------------------------------------
def call_alignment(lib, device, w, mask, accumulate=False, out=None):
    """weights as the [1:] slice of an (L+1,B,T') tensor, as the decoder's buffer is"""
    L, B, Tp = w.shape
    full = torch.full((L + 1, B, Tp), 7.0, device=device)
    full[1:] = torch.from_numpy(w)
    m = None if mask is None else torch.from_numpy(mask.astype(numpy.float32)).to(device)
    out = torch.full((3,), 7.0, dtype=torch.float64, device=device) if out is None else out
    OBS.alignment_stats(lib, full[1:], m, out, Workspace(torch.device(device)), accumulate=accumulate)
    return out.cpu().numpy()


def dirichlet_case(rng, L, B, Tp, null_mask=False):
    lengths = rng.randint(max(1, Tp // 2), Tp + 1, size=B)
    lengths[0] = Tp
    w = numpy.zeros((L, B, Tp), numpy.float32)
    for b in range(B):
        w[:, b, :lengths[b]] = rng.dirichlet(numpy.full(lengths[b], 0.3), size=L)
    if null_mask:
        return w, None
    mask = numpy.zeros((L, B), numpy.float32)
    for b in range(B):
        mask[: rng.randint(1, L + 1), b] = 1
    mask[:, 0] = 1
    mask[1:, B - 1] = 0              # one utterance masked from label 1 on (B = 1: the only one)
    return w, mask


# ---- test 1: the reference's own values -----------------------------------------------------------------------------------------------
def run_golden(lib, device):
    z = numpy.load(golden_path("misc_reference"), allow_pickle=False)
    w, m = z["expr_weights"].astype(numpy.float32), z["expr_mask"].astype(numpy.float32)
    assert w.shape == (6, 3, 9)
    plain = call_alignment(lib, device, w, None)
    masked = call_alignment(lib, device, w, m)
    assert_allclose(plain[0], z["monotonicity_penalty"], rtol=1e-5)
    assert_allclose(masked[0], z["monotonicity_penalty_masked"], rtol=1e-5)
    assert_allclose(masked[1], z["entropy"], rtol=1e-5)
    assert plain[2] == 18 and masked[2] == m.sum()


def test_alignment_reference_golden_emulated():
    run_golden(_lib("cpu"), "cpu")


@pytest.mark.gpu
def test_alignment_reference_golden_gpu(gpu_device):
    run_golden(_lib(gpu_device), gpu_device)


# ---- test 2: the alignment kernel against the restatement -----------------------------------------------------------------------
ALIGN_SHAPES = [(1, 1, 1), (2, 1, 1), (2, 3, 63), (3, 2, 64), (3, 2, 65), (7, 3, 130), (5, 4, 200)]


def run_alignment(lib, device, shape):
    L, B, Tp = shape
    rng = numpy.random.RandomState(L * 1000 + Tp)
    w, mask = dirichlet_case(rng, L, B, Tp, null_mask=shape == (3, 2, 64))
    got = call_alignment(lib, device, w, mask)
    want = numpy.array([penalty_numpy(w, mask), entropy_numpy(w, mask), L * B if mask is None else mask.sum()])
    pen_bound, ent_bound = align_bounds(L, B, Tp, want[0], want[1])
    print("%s penalty %.9g (deviation %.3g, bound %.3g), entropy %.9g (deviation %.3g, bound %.3g)"
          % (shape, got[0], abs(got[0] - want[0]), pen_bound, got[1], abs(got[1] - want[1]), ent_bound))
    assert abs(got[0] - want[0]) <= pen_bound and abs(got[1] - want[1]) <= ent_bound
    assert got[2] == want[2]
    if L == 1:
        assert got[0] == 0
    assert numpy.isfinite(got).all()                                       # exact zeros behind the lengths: 0, not NaN
    again = call_alignment(lib, device, w, mask)
    assert got.tobytes() == again.tobytes()
    # accumulate: twice into one record = the sum of the two
    out = torch.zeros(3, dtype=torch.float64, device=device)
    call_alignment(lib, device, w, mask, accumulate=True, out=out)
    twice = call_alignment(lib, device, w, mask, accumulate=True, out=out)
    assert numpy.array_equal(twice, got + got)


@pytest.mark.parametrize("shape", ALIGN_SHAPES)
def test_alignment_stats_emulated(shape):
    run_alignment(_lib("cpu"), "cpu", shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ALIGN_SHAPES)
def test_alignment_stats_gpu(gpu_device, shape):
    run_alignment(_lib(gpu_device), gpu_device, shape)


# ---- test 3: tensor statistics ------------------------------------------------------------------------------------------------
def call_tensor_stats(lib, device, x, floor=None):
    out = torch.full((3,), 7.0, dtype=torch.float64, device=device)
    OBS.tensor_stats(lib, torch.from_numpy(x).to(device), out, Workspace(torch.device(device)), floor=floor)
    return out.cpu().numpy()


def run_tensor_stats(lib, device, n):
    rng = numpy.random.RandomState(n % 1000)
    x = rng.normal(0, 3, size=n).astype(numpy.float32)
    x[rng.randint(n)] = -0.0                                                  # (n = 1: the whole buffer is one negative zero)
    assert n == 1 or (x.min() < 0 < x.max())
    got = call_tensor_stats(lib, device, x)
    mn, mx = numpy.float32(got[0]), numpy.float32(got[1])
    assert mn.tobytes() == x.min().tobytes() and mx.tobytes() == x.max().tobytes()
    want = numpy.abs(x.astype(numpy.float64)).sum()
    print("n = %d: sum |x| %.17g, float64 NumPy %.17g, deviation %.3g" % (n, got[2], want, abs(got[2] - want)))
    assert abs(got[2] - want) <= U * want                                   # float32 rounding of the final value
    assert got.tobytes() == call_tensor_stats(lib, device, x).tobytes()
    floored = call_tensor_stats(lib, device, x, floor=-1.0)
    fx = numpy.maximum(x, numpy.float32(-1.0))
    assert numpy.float32(floored[0]).tobytes() == fx.min().tobytes() and numpy.float32(floored[1]).tobytes() == fx.max().tobytes()
    assert abs(floored[2] - numpy.abs(fx.astype(numpy.float64)).sum()) <= U * floored[2]


TENSOR_SIZES = [1, 63, 64, 65, 4097, 2 ** 20 + 3]


@pytest.mark.parametrize("n", TENSOR_SIZES)
def test_tensor_stats_emulated(n):
    run_tensor_stats(_lib("cpu"), "cpu", n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", TENSOR_SIZES)
def test_tensor_stats_gpu(gpu_device, n):
    run_tensor_stats(_lib(gpu_device), gpu_device, n)


# ---- test 4: segment norms ----------------------------------------------------------------------------------------------------------
def synthetic_table():
    """segments of 1, 5, 4096, 4097 and 70000 elements at odd offsets, then one with a zero gradient and one with a zero gradient
    and a zero step"""
    shapes = [(1, 1), (1, 5), (64, 64), (241, 17), (700, 100), (3, 11), (2, 7)]
    seg, off = [], 3
    for rows, cols in shapes:
        seg.append([off, rows, cols, 0])
        off += rows * cols + 5 + (rows * cols + 1) % 2                       # keeps every offset odd
    assert all(s[0] % 2 == 1 for s in seg)
    return seg, off


def check_norms(got, seg, p, g, s, scale):
    want = segment_norms_numpy(seg, p, g, s, scale)
    assert_allclose(got[:, :3], want, rtol=2.0 ** -22, atol=0)
    with numpy.errstate(divide="ignore", invalid="ignore"):
        ratio = got[:, 2] / got[:, 1]                                       # float32 / float32, as the reference's step_norm / grad_norm
    assert got.dtype == numpy.float32 and ratio.tobytes() == got[:, 3].tobytes()
    return want


def run_segment_norms(lib, device):
    seg, total = synthetic_table()
    rng = numpy.random.RandomState(5)
    p, g, s = (rng.normal(0, sc, size=total).astype(numpy.float32) for sc in (1.0, 3.0, 0.01))
    for k in (5, 6):
        g[seg[k][0]: seg[k][0] + seg[k][1] * seg[k][2]] = 0
    s[seg[6][0]: seg[6][0] + seg[6][1] * seg[6][2]] = 0
    scale = 1.0 / 3.0
    segments = torch.tensor(seg, dtype=torch.int64, device=device)
    norms = OBS.SegmentNorms(lib, segments)
    items = norms.items.cpu().numpy()
    assert items[:, 2].max() <= OBS.ITEM_MAX and [int(items[items[:, 0] == k, 2].sum()) for k in range(len(seg))] == [r * c for _, r, c, _ in seg]
    dp, dg, ds = (torch.from_numpy(a.copy()).to(device) for a in (p, g, s))          # (copies: on the emulator .to() shares memory)
    tot = torch.zeros(1, dtype=torch.float64, device=device)
    norms.enqueue(3, tot, param=dp, grad=dg, step=ds, grad_scale=scale)
    got = norms.out.cpu().numpy().copy()
    want = check_norms(got, seg, p, g, s, scale)
    assert numpy.isinf(got[5, 3]) and numpy.isnan(got[6, 3])                 # a zero gradient: the reference's division, not a trap
    sizes = numpy.array([r * c for _, r, c, _ in seg], numpy.float64)
    assert_allclose(float(tot[0]), math.sqrt((want[:, 2] ** 2 * sizes).sum()), rtol=2.0 ** -22)
    norms.enqueue(3, tot, param=dp, grad=dg, step=ds, grad_scale=scale)
    assert got.tobytes() == norms.out.cpu().numpy().tobytes()
    # the two phases around an update: the parameter norms are those in front of it
    norms.enqueue(1, tot, param=dp, grad=dg, grad_scale=scale)
    dp -= ds
    norms.enqueue(2, tot, step=ds)
    assert got.tobytes() == norms.out.cpu().numpy().tobytes()
    # what the optimiser did to the step on the fly: RemoveNotFinite on segment 3, then a guarded (skipped) step
    flags = torch.zeros(len(seg), dtype=torch.int32, device=device)
    flags[3] = 1
    scratch = torch.zeros(4, dtype=torch.float32, device=device)
    dp.copy_(torch.from_numpy(p))
    norms.enqueue(3, tot, param=dp, grad=dg, step=ds, grad_scale=scale, segflag=flags, scratch=scratch, remove_not_finite=1,
                  nonfinite_scaler=0.25)
    bad = norms.out.cpu().numpy()
    assert_allclose(bad[3, 2], 0.75 * want[3, 0], rtol=2.0 ** -22)
    assert numpy.delete(bad, 3, 0).tobytes() == numpy.delete(got, 3, 0).tobytes()
    scratch[3] = 1
    norms.enqueue(3, tot, param=dp, grad=dg, step=ds, grad_scale=scale, segflag=flags, scratch=scratch, remove_not_finite=1)
    assert not norms.out[:, 2].cpu().numpy().any() and float(tot[0]) == 0.0
    # BurnIn: with clipping state and scratch[2] raised the optimiser applies a zero step; without the state the word means nothing
    scratch[3], scratch[2] = 0, 1
    norms.enqueue(3, tot, param=dp, grad=dg, step=ds, grad_scale=scale, scratch=scratch)
    assert got.tobytes() == norms.out.cpu().numpy().tobytes()
    clip_state = torch.zeros(8, dtype=torch.float64, device=device)
    norms.enqueue(3, tot, param=dp, grad=dg, step=ds, grad_scale=scale, scratch=scratch, clip_state=clip_state)
    burnt = norms.out.cpu().numpy()
    assert not burnt[:, 2].any() and float(tot[0]) == 0.0 and burnt[:, :2].tobytes() == got[:, :2].tobytes()
    scratch[2] = 0
    norms.enqueue(3, tot, param=dp, grad=dg, step=ds, grad_scale=scale, scratch=scratch, clip_state=clip_state)
    assert got.tobytes() == norms.out.cpu().numpy().tobytes()
    # the real table of the tiny network's store
    rec = SpeechRecognizer(device=device, params=synthetic.make_params(CFG, seed=3), lib=lib, net_config=CFG)
    trainer = Trainer(rec, distributed=False)
    seg = trainer.segments.cpu().numpy().tolist()
    n = rec.store.flat.numel()
    p, g, s = (rng.normal(0, sc, size=n).astype(numpy.float32) for sc in (1.0, 3.0, 0.01))
    norms = OBS.SegmentNorms(lib, trainer.segments)
    norms.enqueue(3, tot, param=torch.from_numpy(p).to(device), grad=torch.from_numpy(g).to(device), step=torch.from_numpy(s).to(device),
                  grad_scale=scale)
    check_norms(norms.out.cpu().numpy(), seg, p, g, s, scale)
    trainer.close()


def test_segment_norms_emulated():
    run_segment_norms(_lib("cpu"), "cpu")


@pytest.mark.gpu
def test_segment_norms_gpu(gpu_device):
    run_segment_norms(_lib(gpu_device), gpu_device)


# ---- test 5: in the step --------------------------------------------------------------------------------------------------------
STEP_B, STEP_T, STEP_L = 3, 30, 12
RULES = dict(gradient_threshold=100.0, rules=("momentum", "adadelta"), scale=0.1, distributed=False)


def check_step(trainer, rec, obs, mask, flat_before, B, global_batch_size=None):
    """trainer.observables() against the restatements applied to the device tensors themselves (B: utterances of this rank's shard)"""
    last = rec.generator.last
    w = last["weights"].cpu().numpy()
    L, _, Tp = w.shape
    pen, ent = penalty_numpy(w, mask), entropy_numpy(w, mask)
    pen_bound, ent_bound = align_bounds(L, B, Tp, pen, ent)
    print("step: penalty %.9g (deviation %.3g, bound %.3g), entropy %.9g (deviation %.3g, bound %.3g)"
          % (obs["weights_penalty"], abs(obs["weights_penalty"] - pen), pen_bound, obs["weights_entropy"], abs(obs["weights_entropy"] - ent), ent_bound))
    assert abs(obs["weights_penalty"] - pen) <= pen_bound and abs(obs["weights_entropy"] - ent) <= ent_bound
    msum = L * B if mask is None else float(mask.sum())
    assert obs["mask_sum"] == msum and obs["mask_density"] == float(numpy.float32(msum / (L * B)))
    r = last["readouts"].cpu().numpy()
    assert numpy.float32(obs["min_energy"]).tobytes() == r.min().tobytes() and numpy.float32(obs["max_energy"]).tobytes() == r.max().tobytes()
    for name, t in (("mean_attended", rec.encoded), ("mean_bottom_output", rec.bottom_output)):
        x = t.cpu().numpy().astype(numpy.float64)
        assert_allclose(obs[name], numpy.abs(x).mean(), rtol=2 * U)           # float32 rounding of the sum, then of the mean
    assert (obs["batch_size"], obs["max_num_phonemes"], obs["max_recording_length"]) == (B, L, int(rec.bottom_output.shape[0]))
    assert obs["max_attended_length"] == obs["max_attended_mask_length"] == Tp
    seg = trainer.segments.cpu().numpy().tolist()
    g, s = rec.store.grad.cpu().numpy(), trainer.step_buf.cpu().numpy()
    want = segment_norms_numpy(seg, flat_before, g, s, 1.0 / (global_batch_size or B))
    got = numpy.stack([obs[name + "_stats"] for name in rec.store.offsets])
    assert got.shape == (len(seg), 4)
    assert_allclose(got[:, :3], want, rtol=2.0 ** -22, atol=0)
    with numpy.errstate(divide="ignore", invalid="ignore"):
        assert (got[:, 2] / got[:, 1]).tobytes() == got[:, 3].tobytes()
    sizes = numpy.array([r_ * c for _, r_, c, _ in seg], numpy.float64)
    assert_allclose(obs["total_step_norm"], math.sqrt((want[:, 2] ** 2 * sizes).sum()), rtol=2.0 ** -22)
    assert_allclose(rec.store.flat.cpu().numpy(), flat_before - s, rtol=0, atol=0)      # (the step is the one that was applied)


def assert_replayed(rec):
    if rec.device.type == "cuda":
        states = list(rec._regions.values())
        assert any(s["seen"] >= 3 for s in states) and not any(s.get("bad") for s in states), "the step was not captured and replayed"


def run_in_step(lib, device):
    params = synthetic.make_params(CFG, seed=3)
    batch = synthetic.make_batch(CFG, STEP_B, STEP_T, STEP_L, seed=13, ragged=True)
    assert not batch["labels_mask"].all()
    rec = SpeechRecognizer(device=device, params=params, lib=lib, net_config=CFG)
    plain = SpeechRecognizer(device=device, params=params, lib=lib, net_config=CFG)
    with Trainer(rec, observables=True, **RULES) as trainer, Trainer(plain, **RULES) as off:
        for k in range(3):                                                   # on the GPU: the eager pass, the captured one, a replay
            before = rec.store.flat.cpu().numpy().copy()
            trainer.train_step(batch)
            off.train_step(batch)
            obs = trainer.observables()
            assert "min_gain" not in obs
            check_step(trainer, rec, obs, batch["labels_mask"], before, STEP_B)
        assert_replayed(rec)
        assert_replayed(plain)
        assert rec.store.flat.cpu().numpy().tobytes() == plain.store.flat.cpu().numpy().tobytes()      # observables change nothing
        with pytest.raises(ValueError):
            off.observables()


def test_observables_in_step_emulated():
    run_in_step(_lib("cpu"), "cpu")


@pytest.mark.gpu
def test_observables_in_step_gpu(gpu_device):
    run_in_step(_lib(gpu_device), gpu_device)


def run_greedy_step(lib, device):
    """mse_gain with greedy exploration: the statistics are those of the prediction-driven pass under the device-written mask"""
    min_reward = -5.0
    params = synthetic.make_params(CFG, seed=3, scale=2.0)
    batch = synthetic.make_batch(CFG, 3, GREEDY_T, GREEDY_L, seed=13, ragged=True)
    rec = SpeechRecognizer(device=device, params=params, lib=lib, net_config=mse_cfg("mse_gain", min_reward))
    with Trainer(rec, observables=True, exploration="greedy", **RULES) as trainer:
        for k in range(3):
            before = rec.store.flat.cpu().numpy().copy()
            trainer.train_step(batch)
            obs = trainer.observables()
            mask = rec.prediction_mask.cpu().numpy()
            assert mask.shape == (GREEDY_L + 10, 3) and not mask.all()
            check_step(trainer, rec, obs, mask, before, 3)
            gains = numpy.maximum(rec.generator.last["gain_matrix"].cpu().numpy(), numpy.float32(min_reward))
            assert obs["min_gain"] == float(gains.min()) and obs["max_gain"] == float(gains.max()) and obs["min_gain"] >= min_reward
        assert_replayed(rec)


def test_observables_greedy_step_emulated():
    run_greedy_step(_lib("cpu"), "cpu")


@pytest.mark.gpu
def test_observables_greedy_step_gpu(gpu_device):
    run_greedy_step(_lib(gpu_device), gpu_device)


def run_against_oracle(lib, device):
    """an all-ones-mask batch: the two alignment channels against the float64 oracle's weights pushed through the restatement"""
    from oracle import lvsr_oracle as O
    params = synthetic.make_params(CFG, seed=3)
    batch = synthetic.make_batch(CFG, STEP_B, STEP_T, STEP_L, seed=13, ragged=False)
    assert batch["labels_mask"].all() and batch["recordings_mask"].all()
    rec = SpeechRecognizer(device=device, params=params, lib=lib, net_config=CFG)
    with Trainer(rec, observables=dict(parameter_stats=False), **RULES) as trainer:
        trainer.train_step(batch)
        obs = trainer.observables()
    assert not any(k.endswith("_stats") for k in obs)
    out = O.OracleRecognizer(CFG, params, dtype=torch.float64).cost(batch["recordings"], batch["recordings_mask"], batch["labels"],
                                                                    batch["labels_mask"])
    w = out["weights"].detach().numpy()
    print("penalty %.9g vs oracle %.9g, entropy %.9g vs oracle %.9g" % (obs["weights_penalty"], penalty_numpy(w), obs["weights_entropy"], entropy_numpy(w)))
    assert_allclose(obs["weights_penalty"], penalty_numpy(w, batch["labels_mask"]), rtol=1e-4)
    assert_allclose(obs["weights_entropy"], entropy_numpy(w, batch["labels_mask"]), rtol=1e-4)


def test_observables_against_oracle_emulated():
    run_against_oracle(_lib("cpu"), "cpu")


@pytest.mark.gpu
def test_observables_against_oracle_gpu(gpu_device):
    run_against_oracle(_lib(gpu_device), gpu_device)


# ---- data parallelism: the optimiser runs eagerly behind the all-reduce, the forward pass in a region that replays -----------------
DP_BATCHES = [(3, 30, 12, 13), (2, 23, 7, 14)]          # two minibatch shapes (B, T, L, seed), met alternately
DP_VALID = (3, 17, 5, 15)


def _validation_pass(rec):
    """what main.validate_observables does per batch: it leaves another batch's views on the recognizer and the generator"""
    b = synthetic.make_batch(CFG, *DP_VALID[:3], seed=DP_VALID[3], ragged=True)
    record = OBS.ValidationRecord(rec)
    record.add(rec.cost(recordings=b["recordings"], inputs_mask=b["recordings_mask"], labels=b["labels"], labels_mask=b["labels_mask"],
                        save_for_backward=False))
    assert numpy.isfinite(record.read()).all()


def _same_observables(a, b):
    assert set(a) == set(b)
    for k in a:
        assert numpy.asarray(a[k]).tobytes() == numpy.asarray(b[k]).tobytes(), k


def run_one_rank_dp(lib, device, overlap):
    """Data parallelism of ONE rank, in this process and without a process group: `distributed` is raised by hand and the
    all-reduce — of one rank the identity — is left out.  What remains is what the test is about: the forward and backward passes
    are a graph region WITHOUT the optimiser (two regions with `overlap`), the guard, the norms and the optimiser follow eagerly.
    Over two alternating minibatch shapes, each met eagerly, captured and replayed, with a validation pass in between, every step's
    observables must be, bit for bit, those of the single-process trainer (whole step in one region) on the same batches, whose
    alignment and tensor channels test_observables_in_step checks against the restatements; and the parameters end bit-identical."""
    params = synthetic.make_params(CFG, seed=3)
    batches = [synthetic.make_batch(CFG, B, T, L, seed=seed, ragged=True) for B, T, L, seed in DP_BATCHES]
    rec = SpeechRecognizer(device=device, params=params, lib=lib, net_config=CFG)
    single = SpeechRecognizer(device=device, params=params, lib=lib, net_config=CFG)
    with Trainer(rec, observables=True, overlap_allreduce=overlap, **RULES) as trainer, Trainer(single, observables=True, **RULES) as ref:
        trainer.distributed, trainer._all_reduce = True, lambda g, wait=True: None
        for k in range(6):
            batch = batches[k % 2]
            B = int(batch["labels"].shape[1])
            before = rec.store.flat.cpu().numpy().copy()
            trainer.train_step(batch, global_batch_size=B)
            ref.train_step(batch)
            obs, want = trainer.observables(), ref.observables()
            print("step %d (B = %d): penalty %.9g / %.9g, entropy %.9g / %.9g, step norm %.9g / %.9g"
                  % (k, B, obs["weights_penalty"], want["weights_penalty"], obs["weights_entropy"], want["weights_entropy"],
                     obs["total_step_norm"], want["total_step_norm"]))
            _same_observables(obs, want)
            assert (obs["batch_size"], obs["max_num_phonemes"]) == tuple(batch["labels"].shape[::-1])
            if k < 2:          # the eager pass of each shape: the views on the recognizer are this batch's
                check_step(trainer, rec, obs, batch["labels_mask"], before, B)
            _validation_pass(rec)
        assert_replayed(rec)
        assert rec.store.flat.cpu().numpy().tobytes() == single.store.flat.cpu().numpy().tobytes()


@pytest.mark.parametrize("overlap", [False, True])
def test_observables_one_rank_dp_emulated(overlap):
    run_one_rank_dp(_lib("cpu"), "cpu", overlap)


@pytest.mark.gpu
@pytest.mark.parametrize("overlap", [False, True])
def test_observables_one_rank_dp_gpu(gpu_device, overlap):
    run_one_rank_dp(_lib(gpu_device), gpu_device, overlap)


def _dp_worker(rank, world, port, out_dir, overlap):
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.dirname(here), os.path.join(os.path.dirname(here), "attention-lvcsr_amd")]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    from emu import emu_lib
    rec = SpeechRecognizer(device="cpu", params=synthetic.make_params(CFG, seed=3), lib=emu_lib(), net_config=CFG)
    rules = dict(RULES, distributed=None)
    kept = {}
    with Trainer(rec, observables=True, overlap_allreduce=overlap, **rules) as trainer:
        assert trainer.distributed and trainer.world == world
        for k in range(4):
            B, T, L, seed = DP_BATCHES[k % 2]
            shard = synthetic.shard_batch(synthetic.make_batch(CFG, 2 * B, T, L, seed=seed + 10 * k, ragged=True), rank, world)
            before = rec.store.flat.numpy().copy()
            trainer.train_step(shard, global_batch_size=2 * B)
            obs = trainer.observables()
            check_step(trainer, rec, obs, shard["labels_mask"], before, B, global_batch_size=2 * B)
            kept["entropy%d" % k] = obs["weights_entropy"]
            kept["step_norm%d" % k] = obs["total_step_norm"]
            kept["stats%d" % k] = numpy.stack([obs[name + "_stats"] for name in rec.store.offsets])
            if k == 1:
                _validation_pass(rec)
    numpy.savez(os.path.join(out_dir, "rank%d.npz" % rank), flat=rec.store.flat.numpy(), **kept)
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("overlap", [False, True])
def test_observables_two_ranks_emulated(tmp_path, overlap):
    """World 2 over gloo: every step of every rank against the restatements (in the worker); the alignment channels are the rank's
    own shard's, the per-parameter statistics come from the all-reduced gradient and agree across the ranks bit for bit."""
    mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path), overlap), nprocs=2, join=True)
    r0, r1 = numpy.load(str(tmp_path / "rank0.npz")), numpy.load(str(tmp_path / "rank1.npz"))
    assert numpy.array_equal(r0["flat"], r1["flat"])
    for k in range(4):
        assert r0["stats%d" % k].tobytes() == r1["stats%d" % k].tobytes() and r0["step_norm%d" % k] == r1["step_norm%d" % k]
        assert r0["entropy%d" % k] != r1["entropy%d" % k]


# ---- test 6: the driver ---------------------------------------------------------------------------------------------------------------
PRIMARY = {"weights_penalty", "weights_entropy", "min_energy", "max_energy", "mean_attended", "mean_bottom_output", "mask_density",
           "batch_size", "max_num_phonemes", "max_recording_length", "max_attended_length", "max_attended_mask_length",
           "total_step_norm"}
NET = dict(dims_bidir=[4], dim_dec=5, dim_matcher=6, attention_type="content", embed_outputs=True)


def run_driver(device, tmp_path):
    from lvsr_amd import main
    from lvsr_amd.checkpoint import save_parameters
    from lvsr_amd.data import Data
    conf = lambda **mon: dict(net=NET, training=dict(gradient_threshold=10.0, scale=0.05, rules=["momentum", "adadelta"], num_batches=4),
                              **mon)
    start = str(tmp_path / "start.npz")
    save_parameters(start, synthetic.make_params(dict(NET, input_dim=5, num_phonemes=6, post_merge_dims=None, data_prepend_eos=False),
                                                 seed=8, scale=0.5))
    ds = _dataset()
    data = Data({"train": ds, "valid": ds}, batch_size=3)
    lib = _lib(device)
    rec, log = main.train(conf(monitoring=dict(observables=dict(every=2))), data, str(tmp_path / "on.zip"), params=start, device=device,
                          lib=lib, distributed=False)
    batch_rows = [r for r in log if "total_gradient_norm" in r]
    assert len(batch_rows) == 4
    for r in batch_rows:
        assert PRIMARY <= set(r) and "mask_sum" not in r and not any(k.endswith("_stats") for k in r)
        assert all(numpy.isfinite(r[k]) for k in PRIMARY)
        assert r["batch_size"] == 3 and 0 < r["mask_density"] <= 1 and r["total_step_norm"] > 0
    names = list(rec.store.offsets)
    for k in (2, 4):
        i = log.index(batch_rows[k - 1])
        avg, window = log[i + 1], batch_rows[k - 2: k]
        assert avg["iterations_done"] == k and avg["average_over"] == 2
        # the aggregation schemes of lvsr/main.py:555-569, from the batch rows (mask sum = density x labels x utterances)
        mask_sums = [round(w["mask_density"] * w["max_num_phonemes"] * w["batch_size"]) for w in window]
        assert_allclose(avg["average_weights_penalty_per_recording"], sum(w["weights_penalty"] for w in window) / 6.0, rtol=1e-12)
        assert_allclose(avg["average_weights_entropy_per_label"], sum(w["weights_entropy"] for w in window) / sum(mask_sums), rtol=1e-12)
        assert_allclose(avg["average_train_cost"], numpy.mean([w["train_cost"] for w in window]), rtol=1e-12)
        stats = [key for key in avg if key.endswith("_stats")]
        assert sorted(stats) == sorted(n + "_stats" for n in names)
        assert all(numpy.shape(avg[key]) == (4,) and numpy.isfinite(avg[key][:3]).all() for key in stats)
    assert sum("average_over" in r for r in log) == 2
    epoch_rows = [r for r in log if "valid_cost" in r]
    assert epoch_rows and all(numpy.isfinite(r["valid_weights_entropy_per_label"]) and numpy.isfinite(r["valid_weights_penalty_per_recording"])
                              for r in epoch_rows)
    # the new validation pass returns what `validate` returns, and the alignment channels of the whole part
    valid = main.validate_observables(rec, data, "valid")
    assert valid["cost"] == main.validate(rec, data, "valid") == epoch_rows[-1]["valid_cost"] and valid["num_utterances"] == 6
    assert valid["weights_entropy_per_label"] == epoch_rows[-1]["valid_weights_entropy_per_label"] < 0
    # off: exactly today's rows
    _, plain = main.train(conf(), data, str(tmp_path / "off.zip"), params=start, device=device, lib=lib, distributed=False)
    assert [set(r) for r in plain if "total_gradient_norm" in r] == [{"iterations_done", "epochs_done", "train_cost", "total_gradient_norm",
                                                                      "gradient_norm_threshold"}] * 4
    assert [set(r) for r in plain if "valid_cost" in r] == [set(r) - {"valid_weights_entropy_per_label", "valid_weights_penalty_per_recording"}
                                                            for r in epoch_rows]
    assert len(plain) == len(log) - 2
    for a, b in zip([r for r in plain if "total_gradient_norm" in r], batch_rows):
        assert a["train_cost"] == b["train_cost"] and a["total_gradient_norm"] == b["total_gradient_norm"]
    noisy = dict(conf(monitoring=dict(observables=True)), regularization=dict(adaptive_noise=dict(model_cost_coefficient=0.1, init_sigma=1e-3)))
    with pytest.raises(NotImplementedError, match="parameter_stats"):
        main.train(noisy, data, str(tmp_path / "noisy.zip"), params=start, device=device, lib=lib, distributed=False)
    # the other observables work with adaptive noise; the keyword does what the monitoring key does
    del noisy["monitoring"]
    _, nlog = main.train(noisy, data, str(tmp_path / "noisy.zip"), params=start, device=device, lib=lib, distributed=False,
                         observables=dict(every=2, parameter_stats=False))
    assert all(PRIMARY <= set(r) and numpy.isfinite(r["total_step_norm"]) and "model_cost" in r for r in nlog if "total_gradient_norm" in r)
    assert sum("average_over" in r for r in nlog) == 2 and not any(k.endswith("_stats") for r in nlog for k in r)


def test_driver_emulated(tmp_path):
    run_driver("cpu", tmp_path)


@pytest.mark.gpu
def test_driver_gpu(gpu_device, tmp_path):
    run_driver(gpu_device, tmp_path)


def test_settings():
    assert OBS.settings(None) is None and OBS.settings(False) is None
    assert OBS.settings(True) == dict(every=10, parameter_stats=True)
    assert OBS.settings(dict(every=3)) == dict(every=3, parameter_stats=True)
    with pytest.raises(ValueError):
        OBS.settings(dict(evry=3))
    with pytest.raises(ValueError):
        OBS.settings(dict(every=0))
    items, first = OBS.work_items([[0, 1, 1, 0], [4, 3, 4096, 0], [12292, 2, 3, 1]], item_max=8192)
    assert items.tolist() == [[0, 0, 1], [1, 0, 8192], [1, 8192, 4096], [2, 0, 6]] and first.tolist() == [0, 1, 3, 4]
