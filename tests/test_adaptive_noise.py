"""Adaptive weight noise (lvsr/graph.py:71-249, lvsr/main.py:425-456): the Philox / Box-Muller stream, the two kernels against a
float64 restatement of graph.py:159-247, one training step against the float64 oracle, graph replay, the clean-weights invariant,
checkpoints under the reference's names, data parallelism and the TIMIT recipe's three stages.  Each check runs on the emulator
(`_emulated`) and on the MI355X (`_gpu`)."""
import ctypes
import os
import socket
import sys
from collections import OrderedDict

import numpy
import pytest
import torch
import torch.multiprocessing as mp
from numpy.testing import assert_allclose

from lvsr_amd import synthetic
from lvsr_amd import weight_noise as WN
from lvsr_amd.bricks.recognizer import SpeechRecognizer
from lvsr_amd.native import ptr
from lvsr_amd.training import Trainer

S = 2048.0                                         # log_sigma_scale, graph.py:159
M64 = (1 << 64) - 1


def _lib(device):
    if device == "cpu":
        from emu import emu_lib
        return emu_lib()
    from lvsr_amd import native
    return native.get()


def _s64(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


# ---- the stream, restated from its definition (include/lvsr_hip.h) ---------------------------------------------------
def philox(q, c, seed):
    """Philox4x32-10 (Salmon et al., SC'11) of counters (q lo, q hi, c lo, c hi) under key (seed lo, seed hi): q an uint64 array."""
    q = numpy.asarray(q, numpy.uint64)
    m32 = numpy.uint64(0xFFFFFFFF)
    x = [q & m32, q >> numpy.uint64(32), numpy.full(q.shape, c & 0xFFFFFFFF, numpy.uint64),
         numpy.full(q.shape, (c >> 32) & 0xFFFFFFFF, numpy.uint64)]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for r in range(10):
        p0 = numpy.uint64(0xD2511F53) * x[0]
        p1 = numpy.uint64(0xCD9E8D57) * x[2]
        x = [(p1 >> numpy.uint64(32)) ^ x[1] ^ numpy.uint64(k0), p1 & m32, (p0 >> numpy.uint64(32)) ^ x[3] ^ numpy.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return numpy.stack(x, axis=-1).astype(numpy.uint32)


def normals(q, c, seed):
    """(len(q), 4) float64 normals of Philox blocks q: Box-Muller on u = (2 (x >> 9) + 1) 2^-24."""
    x = philox(q, c, seed).astype(numpy.float64)
    u = (2.0 * numpy.floor(x / 512.0) + 1.0) * 2.0 ** -24
    r0, r1 = numpy.sqrt(-2.0 * numpy.log(u[:, 0])), numpy.sqrt(-2.0 * numpy.log(u[:, 2]))
    t0, t1 = 2 * numpy.pi * u[:, 1], 2 * numpy.pi * u[:, 3]
    return numpy.stack([r0 * numpy.cos(t0), r0 * numpy.sin(t0), r1 * numpy.cos(t1), r1 * numpy.sin(t1)], axis=-1)


def device_normals(lib, device, seed, counter, first, nblocks, raw=False):
    z = torch.zeros(4 * nblocks, dtype=torch.float32, device=device)
    w = torch.zeros(4 * nblocks, dtype=torch.int32, device=device) if raw else None
    lib.call("lvsr_philox_normal", lib.stream_for(z), _s64(seed), _s64(counter), _s64(first), nblocks, ptr(z), ptr(w))
    out = z.cpu().numpy().reshape(-1, 4)
    return (out, w.cpu().numpy().view(numpy.uint32).reshape(-1, 4)) if raw else out


KAT = [((0, 0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((M64, M64, M64), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x85a308d3243f6a88, 0x0370734413198a2e, 0x299f31d0a4093822), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def run_stream(device):
    lib = _lib(device)
    for (q, c, key), want in KAT:
        assert " ".join("%08x" % w for w in philox([q], c, key)[0]) == want            # the restatement
        _, raw = device_normals(lib, device, key, c, q, 1, raw=True)
        assert " ".join("%08x" % w for w in raw[0]) == want                              # the device
    n = 1 << 20                                                                          # 4 M normals
    first, counter, seed = (1 << 31) - 1000, (1 << 32) + 7, 0x1234567890
    z = device_normals(lib, device, seed, counter, first, n)
    want = normals(numpy.arange(first, first + n, dtype=numpy.uint64), counter, seed)
    assert numpy.abs(z - want).max() < 1e-5
    flat = z.reshape(-1).astype(numpy.float64)
    assert abs(flat.mean()) < 3e-3 and abs(flat.var() - 1.0) < 3e-3
    from scipy import stats
    assert stats.kstest(flat, "norm").statistic <= 1.95 / numpy.sqrt(flat.size)
    nxt = device_normals(lib, device, seed, counter + 1, first, n).reshape(-1)
    assert abs(numpy.corrcoef(flat, nxt)[0, 1]) < 3e-3                                   # consecutive steps
    assert abs(numpy.corrcoef(flat[:-1], flat[1:])[0, 1]) < 3e-3                         # neighbouring indices


def test_stream_emulated():
    run_stream("cpu")


@pytest.mark.gpu
def test_stream_gpu(gpu_device):
    run_stream(gpu_device)


# ---- the kernels against the float64 restatement of graph.py:159-247 --------------------------------------------------
def oracle_prior(mu, ls2, c, N):
    """graph.py:185-212 in float64 (prior_u, prior_s2 rounded to float32 as the reference casts them)."""
    mu, ls2 = [numpy.concatenate([numpy.asarray(v, numpy.float64).ravel() for v in d]) for d in (mu, ls2)]
    s2 = numpy.exp(ls2.astype(numpy.float32) * numpy.float32(S)).astype(numpy.float64)      # float32, as the graph computes it
    count = mu.size
    pu = float(numpy.float32(mu.sum() / count))
    ps2 = float(numpy.float32((s2.sum() + ((mu - pu) ** 2).sum()) / count))
    lc = (0.5 * (numpy.log(ps2) - ls2 * S).sum() + (((mu - pu) ** 2) + s2 - ps2).sum() / (2 * ps2)) / N * c
    return pu, ps2, lc


def oracle_rewrite(mu, ls2, g, pu, ps2, c, N):
    """graph.py:235-247 in float64: (d/dmu, d/dls2)."""
    mu, ls2, g = (numpy.asarray(v, numpy.float64) for v in (mu, ls2, g))
    s2 = numpy.exp(ls2.astype(numpy.float32) * numpy.float32(S)).astype(numpy.float64)
    return c * (mu - pu) / (N * ps2) + g, (c * 0.5 / N * S) * (s2 / ps2 - 1.0) + (0.5 * S) * s2 * g * g


def run_kernel_known_answers(device):
    lib = _lib(device)
    rng = numpy.random.RandomState(5)
    sizes = [(3, 7), (1, 5), (40, 33), (1, 1), (16, 64), (9,)]
    seg, off = [], 0
    for shp in sizes:
        rows, cols = (shp[0], shp[1]) if len(shp) == 2 else (1, shp[0])
        seg.append([off, rows, cols, 0])
        off += (rows * cols + 3) // 4 * 4
    n = off
    segments = torch.tensor(seg, dtype=torch.int64, device=device)
    for scale in ("prior", "hessian"):
        mu = numpy.zeros(n, numpy.float32)
        ls2 = numpy.zeros(n, numpy.float32)
        g = numpy.zeros(n, numpy.float32)
        for o, r, cc, _ in seg:
            k = r * cc
            mu[o:o + k] = rng.normal(0.1, 0.3, k)
            if scale == "prior":
                ls2[o:o + k] = WN.initial_ls2(1e-12)
            else:
                ls2[o:o + k] = numpy.log(rng.uniform(1e-3, 0.5, k)) / S
            g[o:o + k] = rng.normal(0, 2.0, k)
        c, N, seed, B = 0.3, 123.0, 77, 4.0
        t = lambda a: torch.from_numpy(a).to(device)
        mu_d, ls2_d, g_d = t(mu), t(ls2), t(g)
        noisy = torch.full((n,), 7.0, device=device)
        gtheta = torch.full((2 * n,), 9.0, device=device)
        counter = torch.tensor([5], dtype=torch.int64, device=device)
        stats = torch.zeros(WN.STATS, dtype=torch.float64, device=device)
        a = lib.make("lvsr_wnoise_args", mu=mu_d, ls2=ls2_d, noisy=noisy, segments=segments, nseg=len(seg), n=n, seed=seed,
                     counter=counter, stats=stats, grad=g_d, grad_scale=1.0 / B, coef=c, num_examples=N, gtheta=gtheta)
        lib.call("lvsr_wnoise_sample", lib.stream_for(noisy), ctypes.byref(a))
        lib.call("lvsr_wnoise_grad", lib.stream_for(noisy), ctypes.byref(a))
        assert int(counter[0]) == 6
        lib.call("lvsr_wnoise_grad", lib.stream_for(noisy), ctypes.byref(a))
        assert int(counter[0]) == 7                                                      # one per rewrite
        z = normals(numpy.arange(n // 4, dtype=numpy.uint64), 5, seed).reshape(-1)
        got, gt, st = noisy.cpu().numpy(), gtheta.cpu().numpy(), stats.cpu().numpy()
        parts = lambda a_: [a_[o:o + r * cc] for o, r, cc, _ in seg]
        pu, ps2, lc = oracle_prior(parts(mu), parts(ls2), c, N)
        assert_allclose([st[4], st[5], st[6]], [pu, ps2, lc], rtol=1e-6)
        valid = numpy.zeros(n, bool)
        for o, r, cc, _ in seg:
            valid[o:o + r * cc] = True
        s2 = numpy.exp(ls2.astype(numpy.float32) * numpy.float32(S)).astype(numpy.float64)
        assert_allclose(got[valid], (mu + z * numpy.sqrt(s2))[valid], rtol=1e-5, atol=1e-6)
        assert (got[~valid] == 7.0).all()                                                # padding never written
        dm, dl = oracle_rewrite(mu, ls2, g / B, pu, ps2, c, N)
        assert_allclose(gt[:n][valid], dm[valid], rtol=1e-5, atol=1e-7)
        # d/dls2 is the sum of a model-cost term and the Hessian estimate, which cancel where they balance: relative to their
        # magnitudes (s2 = expf(.) itself may differ from numpy's float32 exp by an ulp)
        mag = c * 0.5 / N * S * (s2 / ps2 + 1.0) + 0.5 * S * s2 * (g / B) ** 2
        assert (numpy.abs(gt[n:] - dl) <= 1e-5 * numpy.maximum(numpy.abs(dl), mag) + 1e-7)[valid].all()
        assert (gt[:n][~valid] == 0).all() and (gt[n:][~valid] == 0).all()
        if scale == "hessian":
            assert numpy.abs((0.5 * S) * s2 * (g / B) ** 2)[valid].max() > 10 * abs(c * 0.5 / N * S)


def test_kernel_known_answers_emulated():
    run_kernel_known_answers("cpu")


@pytest.mark.gpu
def test_kernel_known_answers_gpu(gpu_device):
    run_kernel_known_answers(gpu_device)


# ---- one training step against the float64 oracle -----------------------------------------------------------------------
CFG = dict(input_dim=5, num_phonemes=6, dims_bidir=[3, 3], subsample=[1, 2], dim_dec=4, dim_matcher=7,
           attention_type="content_and_conv", conv_n=2, conv_num_filters=3, post_merge_dims=[8],
           post_merge_activation="maxout2", embed_outputs=True, data_prepend_eos=False)
RULES = dict(gradient_threshold=5.0, rules=("momentum", "adadelta"), scale=0.5, momentum=0.3, decay_rate=0.9, epsilon=1e-6)


def run_step_vs_oracle(device):
    from oracle import lvsr_oracle as O
    from oracle import optimizer_oracle as OO
    lib = _lib(device)
    params = synthetic.make_params(CFG, seed=21)
    batch = synthetic.make_batch(CFG, 3, 12, 4, seed=5, ragged=True)
    B = 3
    rec = SpeechRecognizer(device=device, params=params, lib=lib, net_config=CFG)
    c, N, sigma = 0.1, 100.0, 1e-2
    tr = Trainer(rec, distributed=False, adaptive_noise=dict(model_cost_coefficient=c, init_sigma=sigma), num_examples=N, **RULES)
    st = rec.store
    n = st.flat.numel()
    z = normals(numpy.arange(n // 4, dtype=numpy.uint64), 0, 1).reshape(-1)
    ls2 = WN.initial_ls2(sigma)
    s2 = float(numpy.exp(numpy.float32(ls2) * numpy.float32(S)))
    noisy = OrderedDict()
    for k, (o, cnt) in st.offsets.items():
        noisy[k] = (params[k].astype(numpy.float64).ravel() + z[o:o + cnt] * numpy.sqrt(s2)).astype(numpy.float32).reshape(params[k].shape)
    tr.train_step(batch)
    gt = tr.noise.gtheta.cpu().numpy()
    _, grads = O.OracleRecognizer(CFG, noisy, dtype=torch.float64).cost_and_grads(batch)
    pu, ps2, _ = oracle_prior([params[k] for k in st.offsets], [numpy.full(params[k].size, ls2) for k in st.offsets], c, N)
    for k, (o, cnt) in st.offsets.items():
        g = numpy.asarray(grads[k], numpy.float64).ravel() / B
        dm, dl = oracle_rewrite(params[k].ravel(), numpy.full(cnt, ls2), g, pu, ps2, c, N)
        for want, got in ((dm, gt[o:o + cnt]), (dl, gt[n + o:n + o + cnt])):
            cos = numpy.dot(want, got) / max(1e-30, numpy.linalg.norm(want) * numpy.linalg.norm(got))
            assert cos >= 0.99999 or numpy.abs(want - got).max() < 1e-9, k
            assert numpy.abs(want - got).max() <= 1e-3 * max(1e-12, numpy.abs(want).max()), k
    # the step rules over means and log-variances together (max_norm off; ls2 keys that is_weight cannot match)
    cur = OrderedDict((k, params[k].astype(numpy.float32)) for k in st.offsets)
    cur.update(("ls2:" + k + ":", numpy.full(params[k].shape, ls2, numpy.float32)) for k in st.offsets)
    g = OrderedDict((k, gt[o:o + cnt].reshape(params[k].shape)) for k, (o, cnt) in st.offsets.items())
    g.update(("ls2:" + k + ":", gt[n + o:n + o + cnt].reshape(params[k].shape)) for k, (o, cnt) in st.offsets.items())
    new = OO.TrainingRules(**RULES).step(cur, g)
    theta = tr.noise.theta.cpu().numpy()
    for k, (o, cnt) in st.offsets.items():
        assert_allclose(theta[o:o + cnt], new[k].ravel(), rtol=2e-5, atol=2e-6, err_msg=k)
        assert_allclose(theta[n + o:n + o + cnt], new["ls2:" + k + ":"].ravel(), rtol=2e-5, atol=2e-6, err_msg=k)
    assert torch.equal(st.flat, tr.noise.mu)


def test_step_against_float64_oracle_emulated():
    run_step_vs_oracle("cpu")


@pytest.mark.gpu
def test_step_against_float64_oracle_gpu(gpu_device):
    run_step_vs_oracle(gpu_device)


# ---- graph replay, clean-weights invariant ---------------------------------------------------------------------------
def _noisy_trainer(device, use_graph=True, **kw):
    params = synthetic.make_params(CFG, seed=21)
    rec = SpeechRecognizer(device=device, params=params, lib=_lib(device), net_config=CFG, use_graph=use_graph)
    conf = dict(RULES, max_norm=1.0)
    conf.update(kw)
    return rec, Trainer(rec, distributed=False, adaptive_noise=dict(model_cost_coefficient=0.1, init_sigma=1e-2),
                        num_examples=50, **conf)


def run_replay(device):
    batch = synthetic.make_batch(CFG, 3, 12, 4, seed=5, ragged=True)
    out = {}
    for use_graph in (True, False):
        rec, tr = _noisy_trainer(device, use_graph)
        noise = []
        for _ in range(3):                                       # eager, capture, replay
            before = tr.noise.mu.clone()
            tr.train_step(batch)
            noise.append(tr.noise.stats[6].item())
            assert not torch.equal(before, tr.noise.mu)
        out[use_graph] = (tr.noise.theta.cpu(), tr.velocity.cpu(), tr.ms_step.cpu(), tr.ms_dx.cpu(), int(tr.noise.counter[0]),
                          rec.store.flat.cpu())
        assert out[use_graph][4] == 3
        tr.close()
    for a, b in zip(out[True], out[False]):
        assert (torch.equal(a, b) if torch.is_tensor(a) else a == b)
    # the noise differs from step to step: step 2 and 3 ran on different weights
    lib = _lib(device)
    z1, z2 = device_normals(lib, device, 1, 1, 0, 64), device_normals(lib, device, 1, 2, 0, 64)
    assert not numpy.array_equal(z1, z2)


def test_graph_replay_emulated():
    run_replay("cpu")


@pytest.mark.gpu
def test_graph_replay_gpu(gpu_device):
    run_replay(gpu_device)


def run_clean_weights(device, tmp_path):
    from lvsr_amd import main
    rec, tr = _noisy_trainer(device)
    for s in range(2):
        tr.train_step(synthetic.make_batch(CFG, 3, 12, 4, seed=7 + s, ragged=True))
        assert torch.equal(rec.store.flat, tr.noise.mu)
    path = str(tmp_path / "clean.zip")
    rec.save_params(path)

    class _Data(object):
        def __init__(self, batches):
            self.batches = batches

        def get_stream(self, part, shuffle=False):
            return iter(self.batches)
    data = _Data([synthetic.make_batch(CFG, 2, 10, 3, seed=40 + i, ragged=True) for i in range(2)])
    got = main.validate(rec, data)
    fresh = SpeechRecognizer(device=device, params=synthetic.make_params(CFG, seed=1), lib=_lib(device), net_config=CFG)
    fresh.load_params(path)
    assert sorted(fresh.noise_values) == sorted(rec.store.shapes)
    assert got == main.validate(fresh, data)
    tr.close()


def test_clean_weights_invariant_emulated(tmp_path):
    run_clean_weights("cpu", tmp_path)


@pytest.mark.gpu
def test_clean_weights_invariant_gpu(gpu_device, tmp_path):
    run_clean_weights(gpu_device, tmp_path)


# ---- checkpoints ---------------------------------------------------------------------------------------------------
def run_checkpoints(device, tmp_path):
    from lvsr_amd.checkpoint import load_parameters
    rec, tr = _noisy_trainer(device)
    tr.train_step(synthetic.make_batch(CFG, 3, 12, 4, seed=5, ragged=True))
    path = str(tmp_path / "noisy.zip")
    rec.save_params(path)
    vals = load_parameters(path)
    names = set(rec.store.shapes)
    assert set(vals) == names | {"/adaptive_noise." + k[1:] for k in names}
    import tarfile
    import numpy as np
    with tarfile.open(path) as tar:
        npz = np.load(tar.extractfile("_parameters"))
        assert "|adaptive_noise.recognizer|generator|readout|post_merge|bias.b" in npz.files
    ls2 = tr.noise.ls2_values()
    # a plain recognizer loads it (the log-variances are set aside) and decodes
    plain = SpeechRecognizer(device=device, params=synthetic.make_params(CFG, seed=2), lib=_lib(device), net_config=CFG)
    plain.load_params(path)
    for k, v in rec.store.get_values().items():
        assert numpy.array_equal(plain.store.get_values()[k], v)
    plain.init_beam_search(3)
    x = synthetic.make_batch(CFG, 1, 12, 4, seed=9)["recordings"][:, 0]
    outs, costs = plain.beam_search({"recordings": x}, round_to_inf=1e9)
    assert len(outs) >= 1
    # a noisy trainer on it starts from its log-variances; without them from float32(log(init_sigma) * 2 / 2048)
    tr2 = Trainer(plain, distributed=False, adaptive_noise=dict(init_sigma=1e-3), num_examples=10, **RULES)
    n = plain.store.flat.numel()
    for k, (o, cnt) in plain.store.offsets.items():
        assert numpy.array_equal(tr2.noise.ls2[o:o + cnt].cpu().numpy(), ls2[WN.noise_name(k)].ravel())
    fresh = SpeechRecognizer(device=device, params=synthetic.make_params(CFG, seed=2), lib=_lib(device), net_config=CFG)
    tr3 = Trainer(fresh, distributed=False, adaptive_noise=dict(init_sigma=1e-3), num_examples=10, **RULES)
    want = numpy.float32(numpy.log(1e-3) * 2 / 2048)
    for k, (o, cnt) in fresh.store.offsets.items():
        assert (tr3.noise.ls2[o:o + cnt].cpu().numpy() == want).all()
    assert tr3.noise.theta.numel() == 2 * n
    # training state: saved with noise, refused without it, and the reverse
    state = tr2.state_dict()
    tr2.close()
    tr3.close()
    off = Trainer(fresh, distributed=False, **RULES)
    with pytest.raises(ValueError):
        off.load_state_dict(state)
    tr4 = Trainer(fresh, distributed=False, adaptive_noise=True, num_examples=10, **RULES)
    with pytest.raises(ValueError):
        tr4.load_state_dict(off.state_dict())
    with pytest.raises(ValueError):
        Trainer(fresh, distributed=False, adaptive_noise=True, **RULES)                   # num_examples is required
    tr.close()


def test_checkpoints_emulated(tmp_path):
    run_checkpoints("cpu", tmp_path)


@pytest.mark.gpu
def test_checkpoints_gpu(gpu_device, tmp_path):
    run_checkpoints(gpu_device, tmp_path)


# ---- the recipe: nips_baseline.yaml's three stages at tiny dimensions ----------------------------------------------------
RECIPE = """
net:
  dims_bidir: [4]
  dim_dec: 5
  dim_matcher: 6
  attention_type: content
  embed_outputs: true
  enc_transition: !!python/name:blocks.bricks.recurrent.GatedRecurrent
  dec_transition: !!python/name:blocks.bricks.recurrent.GatedRecurrent
initialization:
  /recognizer:
    weights_init: !!python/object/apply:blocks.initialization.IsotropicGaussian [0.3]
    biases_init: !!python/object/apply:blocks.initialization.Constant [0.0]
    rec_weights_init: !!python/object/apply:blocks.initialization.Orthogonal []
    initial_states_init: !!python/object/apply:blocks.initialization.IsotropicGaussian [0.001]
training:
  gradient_threshold: 100.0
  scale: 0.1
  decay_rate: 0.95
  epsilon: 1.0e-8
  rules: [momentum, adadelta]
regularization:
  max_norm: 1.0
stages:
  pretraining:
    number: 0
    regularization:
      max_norm: 1.0
    training:
      num_epochs: 2
  main:
    number: 100
    regularization:
      adaptive_noise:
        model_cost_coefficient: 0.1
        init_sigma: 1.0e-12
    training:
      restart_from: _best_ll
      num_epochs: 2
  annealing:
    number: 200
    regularization:
      adaptive_noise:
        model_cost_coefficient: 0.1
        init_sigma: 1.0e-12
    training:
      epsilon: 1.0e-10
      restart_from: _best_ll
      num_epochs: 1
"""


def _dataset(n=6, F=5, V=6, seed=0):
    from lvsr_amd.data import ArrayDataset
    rng = numpy.random.RandomState(seed)
    recs = [rng.normal(size=(rng.randint(6, 14), F)) for _ in range(n)]
    labs = [rng.randint(0, V - 1, size=rng.randint(2, 5)) for _ in range(n)]
    return ArrayDataset(recs, labs, num_characters=V, bos_label=V - 2)


def run_recipe(device, tmp_path):
    from lvsr_amd import config, main
    from lvsr_amd.checkpoint import load_parameters
    from lvsr_amd.data import Data
    y = tmp_path / "nips_like.yaml"
    y.write_text(RECIPE)
    cfg = config.Configuration(str(y))
    ds = _dataset()
    data = Data({"train": ds, "valid": ds}, batch_size=3)
    save = str(tmp_path / "run")
    rec, log = main.train_multistage(cfg, data, save, device=device, lib=_lib(device), distributed=False)
    files = sorted(os.listdir(save))
    assert files == ["annealing.zip", "annealing_best_ll.zip", "main.zip", "main_best_ll.zip", "pretraining.zip",
                     "pretraining_best_ll.zip"]
    for f in files:
        keys = load_parameters(os.path.join(save, f))
        noisy = [k for k in keys if k.startswith("/adaptive_noise.")]
        assert bool(noisy) == (not f.startswith("pretraining")), f
        if noisy:
            assert len(noisy) == len(keys) // 2
    stage = None
    rows = {}
    for r in log:
        stage = r.get("stage", stage)
        rows.setdefault(stage, []).append(r)
    for name in ("main", "annealing"):
        batch_rows = [r for r in rows[name] if "total_gradient_norm" in r]
        assert batch_rows and all({"model_cost", "model_prior_mean", "model_prior_variance"} <= set(r) for r in batch_rows)
        assert all(numpy.isfinite(r["model_cost"]) for r in batch_rows)
        assert all(numpy.isfinite(r["valid_cost"]) for r in rows[name] if "valid_cost" in r)
    assert not any("model_cost" in r for r in rows["pretraining"])
    # annealing started from main_best_ll's log-variances: its first step's prior variance is theirs
    best = load_parameters(os.path.join(save, "main_best_ll.zip"))
    mus = numpy.concatenate([v.ravel() for k, v in best.items() if not k.startswith("/adaptive_noise.")]).astype(numpy.float64)
    s2 = numpy.concatenate([numpy.exp(v.ravel().astype(numpy.float32) * numpy.float32(S)) for k, v in best.items()
                            if k.startswith("/adaptive_noise.")]).astype(numpy.float64)
    pu = float(numpy.float32(mus.mean()))
    first = [r for r in rows["annealing"] if "model_prior_variance" in r][0]
    assert_allclose(first["model_prior_variance"], (s2.sum() + ((mus - pu) ** 2).sum()) / mus.size, rtol=1e-5)
    init = numpy.float32(numpy.log(1e-12) * 2 / 2048)
    assert any((v != init).any() for k, v in best.items() if k.startswith("/adaptive_noise."))      # the ls2 did move
    return cfg, data, save


def test_recipe_three_stages_emulated(tmp_path):
    run_recipe("cpu", tmp_path)


@pytest.mark.gpu
def test_recipe_three_stages_gpu(gpu_device, tmp_path):
    run_recipe(gpu_device, tmp_path)


def run_resume(device, tmp_path):
    """resume=True after one epoch of a noisy stage ends where the uninterrupted run ends."""
    from lvsr_amd import main
    from lvsr_amd.checkpoint import load_parameters, save_parameters
    from lvsr_amd.data import Data
    net = dict(dims_bidir=[4], dim_dec=5, dim_matcher=6, attention_type="content", embed_outputs=True)
    conf = lambda epochs: dict(net=net, training=dict(gradient_threshold=10.0, scale=0.05, rules=["momentum", "adadelta"],
                                                      num_epochs=epochs),
                               regularization=dict(max_norm=1.0, adaptive_noise=dict(model_cost_coefficient=0.1, init_sigma=1e-3)))
    start = str(tmp_path / "start.npz")
    save_parameters(start, synthetic.make_params(dict(net, input_dim=5, num_phonemes=6, post_merge_dims=None,
                                                      data_prepend_eos=False), seed=8, scale=0.5))
    ds = _dataset()
    data = Data({"train": ds, "valid": ds}, batch_size=3)
    lib = _lib(device)
    main.train(conf(2), data, str(tmp_path / "full.zip"), params=start, device=device, lib=lib, distributed=False)
    main.train(conf(1), data, str(tmp_path / "part.zip"), params=start, device=device, lib=lib, distributed=False)
    main.train(conf(2), data, str(tmp_path / "part.zip"), params=str(tmp_path / "part.zip"), device=device, lib=lib,
               distributed=False, resume=True)
    a, b = load_parameters(str(tmp_path / "full.zip")), load_parameters(str(tmp_path / "part.zip"))
    assert set(a) == set(b) and any(k.startswith("/adaptive_noise.") for k in a)
    for k in a:
        assert numpy.array_equal(a[k], b[k]), k


def test_resume_noisy_stage_emulated(tmp_path):
    run_resume("cpu", tmp_path)


@pytest.mark.gpu
def test_resume_noisy_stage_gpu(gpu_device, tmp_path):
    run_resume(gpu_device, tmp_path)


def test_refusals_stay():
    from emu import emu_lib
    from lvsr_amd import main
    from lvsr_amd.data import Data
    ds = _dataset()
    data = Data({"train": ds, "valid": ds}, batch_size=3)
    net = dict(dims_bidir=[4], dim_dec=5, dim_matcher=6, attention_type="content", embed_outputs=True)
    an = dict(model_cost_coefficient=0.1, init_sigma=1e-12)
    for reg in ({"dropout": 0.5}, {"noise": 0.075}, {"penalty_coof": 0.1}, {"decay": 1e-4}):
        for extra in ({}, {"adaptive_noise": an}):
            with pytest.raises(NotImplementedError):
                main.train(dict(net=net, training=dict(scale=0.1), regularization=dict(reg, **extra)), data, "/nonexistent/x.zip",
                           params="/nonexistent/p.npz", device="cpu", lib=emu_lib(), distributed=False)


# ---- data parallelism: world 2 over gloo on the emulator ----------------------------------------------------------------
DP_CFG = dict(CFG, embed_outputs=False)
DP_RULES = dict(gradient_threshold=5.0, rules=("momentum", "adadelta"), scale=0.5, momentum=0.0, decay_rate=0.9, epsilon=1e-6,
                max_norm=1.0)
DP_NOISE = dict(model_cost_coefficient=0.1, init_sigma=1e-12)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, out_dir, overlap):
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.dirname(here), os.path.join(os.path.dirname(here), "attention-lvcsr_amd")]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    from emu import emu_lib
    rec = SpeechRecognizer(device="cpu", params=synthetic.make_params(DP_CFG, seed=31), lib=emu_lib(), net_config=DP_CFG)
    tr = Trainer(rec, overlap_allreduce=overlap, adaptive_noise=DP_NOISE, num_examples=20, **DP_RULES)
    for step in range(2):
        gb = synthetic.make_batch(DP_CFG, 4, 13, 5, seed=100 + step, ragged=True)
        tr.train_step(synthetic.shard_batch(gb, rank, world), global_batch_size=4)
    numpy.savez(os.path.join(out_dir, "rank%d.npz" % rank), theta=tr.noise.theta.numpy(), flat=rec.store.flat.numpy())
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("overlap", [False, True])
def test_two_ranks_noisy_step_emulated(tmp_path, overlap):
    from emu import emu_lib
    mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path), overlap), nprocs=2, join=True)
    r0, r1 = numpy.load(str(tmp_path / "rank0.npz")), numpy.load(str(tmp_path / "rank1.npz"))
    assert numpy.array_equal(r0["theta"], r1["theta"]) and numpy.array_equal(r0["flat"], r1["flat"])
    rec = SpeechRecognizer(device="cpu", params=synthetic.make_params(DP_CFG, seed=31), lib=emu_lib(), net_config=DP_CFG)
    tr = Trainer(rec, distributed=False, adaptive_noise=DP_NOISE, num_examples=20, **DP_RULES)
    for step in range(2):
        tr.train_step(synthetic.make_batch(DP_CFG, 4, 13, 5, seed=100 + step, ragged=True), global_batch_size=4)
    assert_allclose(r0["theta"], tr.noise.theta.numpy(), rtol=1e-4, atol=1e-5)
