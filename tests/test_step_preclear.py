"""A training step that clears the granule planes of all its persistent encoder launches in ONE launch at the head of the forward pass
(Encoder.preclear, the default) against the same steps with a clear in front of every launch: cost matrix, every gradient slice —
the initial states' (summed for all layers in one launch) and the feedback tables' (one scatter for two) among them — and the parameters
after each step, BIT for bit.

The minibatches differ from step to step, and that is what the comparison rests on: epochs restart at 1 in every persistent launch, so
a plane that was not cleared makes a consumer take the previous launch's granule for this launch's — with equal data it would hold the
right values.  A forward pass that saves nothing for a backward pass (analyze) runs between two steps: it clears for itself."""
import numpy
import pytest
import torch

from lvsr_amd import spec, synthetic
from lvsr_amd.bricks.recognizer import SpeechRecognizer
from lvsr_amd.training import Trainer

RULES = dict(gradient_threshold=100.0, rules=("momentum", "adadelta"), scale=0.1, momentum=0.0, decay_rate=0.95, epsilon=1e-8, max_norm=1.0)


def _steps(make, cfg, B, T, L, ragged):
    """Three training steps on three different minibatches of one shape (on the device: enqueued eagerly, captured, replayed), an analyze
    call between the second and the third -> [(cost matrix, gradients, parameters) after each step], the analyze result, the recognizer."""
    rec = make()
    tr = Trainer(rec, distributed=False, **RULES)
    out = []
    for k in range(3):
        batch = synthetic.make_batch(cfg, B, T, L, seed=100 + k, ragged=ragged)
        if rec.device.type == "cuda":
            batch = {name: torch.from_numpy(v).to(rec.device) for name, v in batch.items()}
        cm = tr.train_step(batch)
        if rec.device.type == "cuda":
            torch.cuda.synchronize()
        assert not tr.step_was_skipped()
        out.append((cm.cpu().numpy().copy(), rec.store.get_grads(), rec.store.get_values()))
        if k == 1:
            one = synthetic.make_batch(cfg, 1, T, L, seed=7)
            seen = rec.analyze({"recordings": one["recordings"][:, 0]}, one["labels"][:, 0])
    tr.close()
    return out, seen, rec


def compare(make, cfg, B, T, L, ragged):
    def variant(preclear):
        def build():
            rec = make()
            rec.encoder.preclear = preclear
            return rec
        return build
    head, seen_head, rec = _steps(variant(True), cfg, B, T, L, ragged)
    each, seen_each, _ = _steps(variant(False), cfg, B, T, L, ragged)
    names = [k[0] for k in rec.ws._bufs]
    n_layers = len(cfg["dims_bidir"])
    assert all("enc%d.sync" % i in names and "enc%d.sync_bwd" % i in names for i in range(n_layers)), \
        "not every encoder layer ran on the persistent kernels with planes cleared at the head"
    for k, ((cm_a, g_a, p_a), (cm_b, g_b, p_b)) in enumerate(zip(head, each)):
        assert (cm_a.view(numpy.uint32) == cm_b.view(numpy.uint32)).all(), "cost matrix of step %d" % k
        for name in g_a:
            assert (g_a[name].view(numpy.uint32) == g_b[name].view(numpy.uint32)).all(), "gradient %s of step %d" % (name, k)
            assert (p_a[name].view(numpy.uint32) == p_b[name].view(numpy.uint32)).all(), "parameter %s after step %d" % (name, k)
    assert not (head[0][0] == head[1][0]).all(), "the minibatches were meant to differ"
    for a, b in zip(seen_head, seen_each):
        assert (numpy.asarray(a) == numpy.asarray(b)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("ragged", [False, True])
def test_head_clear_equals_clears_per_launch_gpu(gpu_device, ragged):
    """The WSJ-base network (H = 256: clusters of four work-groups; persistent decoder) at the smallest shape at which every persistent
    launch of the step has planes: B = 2, T = 16 (subsampled to 4), L = 4."""
    cfg = spec.wsj_base()
    params = synthetic.make_params(cfg, seed=10)
    compare(lambda: SpeechRecognizer(device=gpu_device, params=params, net_config=cfg), cfg, 2, 16, 4, ragged)


@pytest.mark.slow
def test_head_clear_equals_clears_per_launch_emulated():
    """On the emulator with concurrent work-groups: two layers of H = 140 / 132 (clusters of four work-groups, one utterance each), the
    second subsampling; the decoder on its step kernels.  Clusters are OS threads there and a step takes tens of seconds (four minutes
    in all): run with --runslow; the device twin above is the quick one."""
    from emu import emu_lib
    lib = emu_lib()
    lib._dll.hipemu_set_concurrent(1)
    lib.set_knob("persist_rows", 1)
    try:
        if not lib.emulates_concurrency():
            pytest.skip("the emulator build does not run work-groups concurrently")
        cfg = dict(input_dim=6, num_phonemes=6, dims_bidir=[140, 132], subsample=[1, 2], dim_dec=4, dim_matcher=7,
                   attention_type="content", post_merge_dims=None, embed_outputs=False)
        params = synthetic.make_params(cfg, seed=3)
        compare(lambda: SpeechRecognizer(device="cpu", params=params, lib=lib, net_config=cfg, use_persistent=True,
                                         use_persistent_decoder=False), cfg, 2, 6, 3, True)
    finally:
        lib._dll.hipemu_set_concurrent(0)
        lib.set_knob("persist_rows", 0)
