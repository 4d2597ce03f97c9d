"""The task-loss-estimation criteria (net.criterion mse_gain / mse_reward) through the whole recognizer: teacher-forced cost and
gradients against the float64 oracle's readouts under the reference's loss expressions, a prediction that differs from the
groundtruth, greedy exploration inside the training step, the Trainer, beam search and the configuration surface.  Every body runs on
the CPU emulator build and on the GPU."""
import numpy
import pytest
import torch
from numpy.testing import assert_allclose

from oracle import lvsr_oracle as O
from lvsr_amd import config, native, spec, synthetic
from lvsr_amd.bricks.recognizer import SpeechRecognizer
from lvsr_amd.training import Trainer
from test_reward_kernels import _torch_cost, reward_gain_numpy

CFG = dict(input_dim=5, num_phonemes=6, dims_bidir=[3, 3], subsample=[1, 2], dim_dec=4, dim_matcher=7,
           attention_type="content_and_conv", conv_n=2, conv_num_filters=3, prior=dict(type="window_around_median", before=1, after=2),
           post_merge_dims=[8], post_merge_activation="maxout2", embed_outputs=False, data_prepend_eos=False)
EOS, V = 5, 6
B, T, L = 3, 13, 5


def mse_cfg(criterion, min_reward=-1.0):
    return dict(CFG, criterion=criterion, min_reward=min_reward)


def emu():
    from emu import emu_lib
    return emu_lib(), "cpu"


def prediction_mask_numpy(P, eos=EOS):
    """lvsr/main.py:254-259: ones up to and including the first EOS of every column."""
    m = (numpy.cumsum(P == eos, axis=0) < 1).astype(numpy.float32)
    m = numpy.roll(m, 1, 0)
    m[0] = 1
    return m


def oracle_mse(criterion, min_reward, params, batch, prediction=None, prediction_mask=None, dtype=torch.float64):
    """Reference values: the oracle's readouts (with their autograd graph) under RewardRegressionEmitter.cost's expressions
    (test_reward_kernels._torch_cost) on the fixture-checked reward / gain matrices.  -> cost matrix, gradients by name."""
    orc = O.OracleRecognizer(CFG, params, dtype=dtype)
    for v in orc.p.values():
        v.grad = None
    pred = batch["labels"] if prediction is None else prediction
    pm = batch["labels_mask"] if prediction is None else prediction_mask
    out = orc.cost(batch["recordings"], batch["recordings_mask"], pred, pm)
    rewards, gains, _ = reward_gain_numpy(batch["labels"], pred, EOS, V)
    cm = _torch_cost(criterion, out["readouts"].double(), gains, rewards, numpy.asarray(pred), pm, min_reward)
    cm.sum().backward()
    grads = {k: (v.grad.detach().double().numpy().copy() if v.grad is not None else numpy.zeros(tuple(v.shape))) for k, v in orc.p.items()}
    return cm.detach().numpy(), grads


def check_cost_and_grads(rec, cm, want_cm, want_grads):
    # the bars of test_recognizer_vs_reference_golden for the small cases
    assert_allclose(cm.cpu().numpy(), want_cm, rtol=2e-4, atol=2e-5)
    got = rec.store.get_grads()
    errs = {name: numpy.abs(got[name] - ref).max() / max(1e-3, numpy.abs(ref).max()) for name, ref in want_grads.items()}
    worst = max(errs, key=errs.get)
    print("largest gradient error / max: %.3g (%s)" % (errs[worst], worst))
    for name, err in errs.items():
        assert err <= 2e-4, name


GREEDY_T, GREEDY_L = 6, 2          # greedy exploration generates L + 10 labels whatever L is: the smallest ragged batch that has an EOS and a label before it


def setup(criterion, min_reward, lib, device, scale=1.0, T=T, L=L, **net):
    params = synthetic.make_params(dict(CFG, **net), seed=3, scale=scale)
    batch = synthetic.make_batch(CFG, B, T, L, seed=13, ragged=True)
    rec = SpeechRecognizer(device=device, params=params, lib=lib, net_config=dict(mse_cfg(criterion, min_reward), **net))
    return params, batch, rec


# ---- imitative: the labels drive the decoder ---------------------------------------------------------------------------------
def run_imitative(criterion, min_reward, lib, device):
    params, batch, rec = setup(criterion, min_reward, lib, device)
    cm = rec.cost_and_gradients(batch)
    want_cm, want_grads = oracle_mse(criterion, min_reward, params, batch)
    check_cost_and_grads(rec, cm, want_cm, want_grads)
    last = rec.generator.last
    rewards, gains, _ = reward_gain_numpy(batch["labels"], batch["labels"], EOS, V)
    assert numpy.array_equal(last["reward_matrix"].cpu().numpy(), rewards) and numpy.array_equal(last["gain_matrix"].cpu().numpy(), gains)
    assert tuple(last["readouts"].shape) == (L, B, V)


def perturbed_prediction(labels):
    """A fixed prediction (L + 2, B) next to the groundtruth: EOS one position earlier (column 0), two later (column 1), absent (column 2)."""
    P = numpy.full((L + 2, B), 1, numpy.int64)
    P[:L] = labels
    P[P == EOS] = 2
    P[1, 2] = 3
    n = [int(list(labels[:, b]).index(EOS)) for b in range(B)]
    P[max(n[0] - 1, 0), 0] = EOS
    P[n[1] + 2, 1] = EOS
    return P


def run_prediction(criterion, min_reward, lib, device):
    params, batch, rec = setup(criterion, min_reward, lib, device)
    P = perturbed_prediction(batch["labels"])
    M = prediction_mask_numpy(P)
    assert M[:, 2].all() and not M[:, 0].all() and M[:, 1].sum() == list(batch["labels"][:, 1]).index(EOS) + 3
    cm = rec.cost(recordings=batch["recordings"], inputs_mask=batch["recordings_mask"], labels=batch["labels"],
                  labels_mask=batch["labels_mask"], prediction=P, prediction_mask=M)
    rec.backward()
    assert tuple(cm.shape) == (L + 2, B)
    want_cm, want_grads = oracle_mse(criterion, min_reward, params, batch, P, M)
    check_cost_and_grads(rec, cm, want_cm, want_grads)


CRITERIA = [("mse_gain", -5.0), ("mse_gain", -1.0), ("mse_reward", -1.0)]


@pytest.mark.parametrize("criterion,min_reward", CRITERIA)
def test_mse_imitative_emulated(criterion, min_reward):
    run_imitative(criterion, min_reward, *emu())


@pytest.mark.parametrize("criterion,min_reward", CRITERIA)
def test_mse_prediction_emulated(criterion, min_reward):
    run_prediction(criterion, min_reward, *emu())


@pytest.mark.gpu
@pytest.mark.parametrize("criterion,min_reward", CRITERIA)
def test_mse_imitative_gpu(gpu_device, criterion, min_reward):
    run_imitative(criterion, min_reward, None, gpu_device)


@pytest.mark.gpu
@pytest.mark.parametrize("criterion,min_reward", CRITERIA)
def test_mse_prediction_gpu(gpu_device, criterion, min_reward):
    run_prediction(criterion, min_reward, None, gpu_device)


# ---- greedy exploration ------------------------------------------------------------------------------------------------------
def run_greedy(criterion, lib, device, **net):
    L = GREEDY_L
    params, batch, rec = setup(criterion, -5.0, lib, device, scale=2.0, T=GREEDY_T, L=L, **net)
    N = L + 10
    steps = []
    for k in range(3 if torch.device(device).type == "cuda" else 1):          # on the GPU: the eager pass, the captured one, a replay
        cm = rec.cost_and_gradients(batch, exploration="greedy")
        steps.append((cm.cpu().numpy().copy(), rec.store.grad.cpu().numpy().copy(), rec.prediction.cpu().numpy().copy(),
                      rec.generator.last["readouts"].cpu().numpy().copy()))
    cm1, g1, P1, r1 = steps[0]
    assert cm1.shape == (N, B) and P1.shape == (N, B)
    for cm_k, g_k, P_k, _ in steps[1:]:
        assert numpy.array_equal(cm_k, cm1) and numpy.array_equal(g_k, g1) and numpy.array_equal(P_k, P1)
    if rec.device.type == "cuda":
        states = list(rec._regions.values())
        assert any(s["seen"] >= 3 for s in states) and not any(s.get("bad") for s in states), "the greedy step was not captured and replayed"
    # the two-call path: generate, mask on the host, teacher-forced cost on the prediction, backward
    P = rec.generate(n_steps=N, recordings=batch["recordings"], inputs_mask=batch["recordings_mask"])["outputs"].cpu().numpy()
    assert numpy.array_equal(P, P1)
    M = prediction_mask_numpy(P)
    assert numpy.array_equal(rec.prediction_mask.cpu().numpy(), M)
    cm2 = rec.cost(recordings=batch["recordings"], inputs_mask=batch["recordings_mask"], labels=batch["labels"],
                   labels_mask=batch["labels_mask"], prediction=P, prediction_mask=M)
    rec.backward()
    assert numpy.array_equal(cm2.cpu().numpy(), cm1) and numpy.array_equal(rec.store.grad.cpu().numpy(), g1)
    assert numpy.isfinite(g1).all() and numpy.abs(g1).max() > 0
    # the prediction is the argmax of the teacher-forced readouts (up to float32 ties) wherever it is not masked
    picked = numpy.take_along_axis(r1, P[:, :, None], axis=2)[:, :, 0]
    assert ((picked >= r1.max(axis=2) - 1e-5 * numpy.abs(r1).max()) | (M == 0)).all()
    # greedy exploration is for the mse criteria
    plain = SpeechRecognizer(device=device, params=params, lib=lib, net_config=dict(CFG, **net))
    with pytest.raises(NotImplementedError):
        plain.cost_and_gradients(batch, exploration="greedy")


@pytest.mark.parametrize("criterion", ["mse_gain", "mse_reward"])
def test_greedy_exploration_emulated(criterion):
    run_greedy(criterion, *emu())


@pytest.mark.gpu
@pytest.mark.parametrize("criterion", ["mse_gain", "mse_reward"])
def test_greedy_exploration_gpu(gpu_device, criterion):
    run_greedy(criterion, None, gpu_device)


@pytest.mark.gpu
def test_greedy_exploration_stacked_decoder_gpu(gpu_device):
    """A two-layer RecurrentStack decoder: its own `generate` runs inside the captured step too (nothing may allocate there, or the
    region drops the capture and stays eager).  GPU only: the emulator captures nothing."""
    run_greedy("mse_gain", None, gpu_device, dec_stack=2)


# ---- Trainer: three steps of the iclr_reward recipe ---------------------------------------------------------------------------
def run_trainer(lib, device):
    T, L = GREEDY_T, GREEDY_L
    params, batch, rec = setup("mse_gain", -5.0, lib, device, T=T, L=L)
    before = rec.get_parameter_values()
    trainer = Trainer.from_config(rec, dict(exploration="greedy", gradient_threshold=100.0, rules=["momentum", "adadelta"], scale=0.1),
                                  adaptive_clipping=False, distributed=False)
    assert trainer.exploration == "greedy"
    for k in range(3):
        cm = trainer.train_step(synthetic.make_batch(CFG, B, T, L, seed=13 + k, ragged=True))
        assert tuple(cm.shape) == (L + 10, B) and bool(torch.isfinite(cm).all())
        assert not trainer.step_was_skipped()
    after = rec.get_parameter_values()
    assert all(numpy.isfinite(v).all() for v in after.values())
    assert any(numpy.abs(after[k] - before[k]).max() > 0 for k in after)
    trainer.close()


def test_trainer_greedy_steps_emulated():
    run_trainer(*emu())


@pytest.mark.gpu
def test_trainer_greedy_steps_gpu(gpu_device):
    run_trainer(None, gpu_device)


# ---- beam search: costs = -readouts -----------------------------------------------------------------------------------------------
def run_beam(lib, device):
    params, batch, rec = setup("mse_gain", -5.0, lib, device, scale=2.0)
    tl = int(batch["recordings_mask"][:, 0].sum())
    x = batch["recordings"][:tl, 0]
    rec.init_beam_search(4)
    outs, costs = rec.beam_search({"recordings": x}, char_discount=0.0, round_to_inf=1e9, stop_on="optimistic_future_cost")
    assert outs and all(o[-1] == EOS for o in outs)
    for hyp, cost in zip(outs, costs):
        rec.analyze({"recordings": x}, batch["labels"][:, 0], prediction=numpy.array(hyp))
        r = rec.generator.last["readouts"][:, 0, :].cpu().numpy()
        total = -float(sum(r[t, c] for t, c in enumerate(hyp)))
        # a path has <= 20 float32 additions; measured on this case: relative deviation <= 8.5e-8 on the emulator build, <= 1.6e-7 on the GPU
        print("beam cost %.8g, -sum of readouts %.8g, relative deviation %.3g" % (cost, total, abs(cost - total) / abs(total)))
        assert_allclose(cost, total, rtol=1e-5, atol=0)
    batch_results = rec.beam_search_batch([x, x], char_discount=0.0, round_to_inf=1e9, stop_on="optimistic_future_cost")
    assert batch_results[0][0][0] == outs[0]


def test_beam_search_mse_emulated():
    run_beam(*emu())


@pytest.mark.gpu
def test_beam_search_mse_gpu(gpu_device):
    run_beam(None, gpu_device)


# ---- configuration surface -----------------------------------------------------------------------------------------------------------
# exp/timit/configs/iclr_reward.yaml with its parent chain merged (net and training sections; the stages that change either), in the
# reference's config dialect
ICLR_REWARD = """
net:
    dim_dec: 256
    dims_bidir: [256, 256, 256]
    subsample: [1, 1, 1]
    dim_matcher: 512
    bottom:
        bottom_class: !!python/name:lvsr.bricks.recognizer.SpeechBottom
        dims: []
        activation: !!python/object/apply:blocks.bricks.Rectifier []
    enc_transition: !!python/name:blocks.bricks.recurrent.GatedRecurrent
    dec_transition: !!python/name:blocks.bricks.recurrent.GatedRecurrent
    attention_type: content_and_conv
    conv_n: 100
    conv_num_filters: 10
    energy_normalizer: logistic
    prior:
        type: expanding
        initial_begin: 0
        initial_end: 10000
        min_speed: 0.0
        max_speed: 10.0
    post_merge_dims: [256]
    post_merge_activation: !!python/object/apply:blocks.bricks.Maxout [2]
    use_states_for_readout: True
    max_decoded_length_scale: 3.
    criterion:
        name: mse_gain
        min_reward: -5
    lm: {}
training:
    rules: [momentum, adadelta]
    scale: 1.0
    momentum: 0.0
    decay_rate: 0.95
    epsilon: 1.0e-8
    burn_in_steps: 0
    exploration: greedy
    gradient_threshold: 100.0
stages:
    pretraining:
        number: 0
        training:
            num_epochs: 30
        net:
            criterion:
                min_reward: -1
    pretraining2:
        number: 50
        training:
            num_epochs: 30
            restart_from: _best_ll
"""


def test_configuration_surface(tmp_path):
    path = tmp_path / "iclr_reward.yaml"
    path.write_text(ICLR_REWARD)
    cfg = config.Configuration(str(path))
    sizes = dict(input_dim=123, num_phonemes=63)
    net = spec.from_reference_kwargs(**cfg.net_kwargs(**sizes))
    assert net["criterion"] == "mse_gain" and net["min_reward"] == -5.0 and net["energy_normalizer"] == "logistic"
    # the stage's override carries only min_reward: the criterion's name comes through the recursive merge
    assert list(cfg.ordered_stages) == ["pretraining", "pretraining2"]
    assert cfg.ordered_stages["pretraining"]["net"]["criterion"] == {"name": "mse_gain", "min_reward": -1}
    pre = spec.from_reference_kwargs(**cfg.net_kwargs(stage="pretraining", **sizes))
    assert pre["criterion"] == "mse_gain" and pre["min_reward"] == -1.0
    pre2 = spec.from_reference_kwargs(**cfg.net_kwargs(stage="pretraining2", **sizes))
    assert pre2["criterion"] == "mse_gain" and pre2["min_reward"] == -5.0
    assert all(cfg.ordered_stages[st]["training"]["exploration"] == "greedy" for st in cfg.ordered_stages)
    assert spec.from_reference_kwargs(**dict(cfg.net_kwargs(**sizes), criterion={"name": "mse_reward"}))["min_reward"] == -1.0
    # the emitter has no parameters: names and shapes are those of the log-likelihood network
    plain = spec.from_reference_kwargs(**dict(cfg.net_kwargs(**sizes), criterion={"name": "log_likelihood"}))
    assert spec.parameter_shapes(net) == spec.parameter_shapes(plain)
    with pytest.raises(ValueError, match="Unknown criterion"):
        spec.from_reference_kwargs(**dict(cfg.net_kwargs(**sizes), criterion={"name": "ctc"}))
    with pytest.raises(NotImplementedError, match="language model"):
        spec.from_reference_kwargs(**dict(cfg.net_kwargs(**sizes), lm={"path": "lm.fst"}))
    # the recipe's training section builds the trainer (on the tiny network: the full one is not needed for that)
    lib, device = emu()
    training = cfg.ordered_stages["pretraining"]["training"]
    rec = SpeechRecognizer(device=device, lib=lib, params=synthetic.make_params(CFG, seed=1), net_config=mse_cfg("mse_gain", pre["min_reward"]))
    trainer = Trainer.from_config(rec, training, distributed=False)
    assert trainer.exploration == "greedy" and trainer.conf["clip_threshold"] == 100.0
    assert Trainer.from_config(rec, {}, distributed=False).exploration == "imitative"
    with pytest.raises(NotImplementedError, match="mixed"):
        Trainer.from_config(rec, dict(training, exploration="mixed"), distributed=False)
    with pytest.raises(ValueError):
        Trainer.from_config(rec, dict(training, exploration="imitation"), distributed=False)      # wsj_reward10.yaml's spelling
    ll = SpeechRecognizer(device=device, lib=lib, params=synthetic.make_params(CFG, seed=1), net_config=CFG)
    with pytest.raises(NotImplementedError, match="mse criterion"):
        Trainer.from_config(ll, training, distributed=False)

    class FakeLM(object):
        out_dim = 6
    with pytest.raises(NotImplementedError, match="language model"):
        rec.set_language_model(FakeLM())
