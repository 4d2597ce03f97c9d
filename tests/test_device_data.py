"""The training set in device memory (lvsr_amd/device_data.py) and the kernel that assembles its minibatches (csrc/batch.hip,
lvsr_assemble_batch): the kernel alone against Data.pad_batch, the epoch plan against a walk over Data.get_stream, the stream, a
few training steps and the stage driver against the host path.  The feature copies values and writes the constants 0 and 1, so
every comparison is exact (numpy.array_equal; float tensors are compared as their bit patterns).  Every device body runs on the
CPU emulator build and on the product library."""
import ctypes

import numpy
import pytest
import torch

from lvsr_amd import native
from lvsr_amd.data import ArrayDataset, Data, DeviceData


def _same_bits(a, b):
    a, b = numpy.ascontiguousarray(a), numpy.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == numpy.float32:
        a, b = a.view(numpy.uint32), b.view(numpy.uint32)
    return numpy.array_equal(a, b)


def _host(t):
    return t.cpu().numpy() if torch.is_tensor(t) else numpy.asarray(t)


# ---- 4.1 the kernel alone against Data.pad_batch ---------------------------------------------------------------------------
FRAME_LEN = [1, 2, 5, 8, 8, 3, 1]
LABEL_LEN = [1, 4, 2, 6, 1, 3, 6]
WIDTHS = [1, 3, 123, 128, 260]       # odd, rows not 16-byte aligned (123: 492 B), an aligned width, more than 256 floats per row
# (name, index table, first column in the table, B, T, L)
KERNEL_CASES = [
    ("one column, T and L its own lengths", [3], 0, 1, 8, 6),
    ("one column with padded tails", [2], 0, 1, 9, 6),
    ("B = 5, non-monotone, a repeat, first and last utterance; T = the longest: that column has no padding", [6, 0, 3, 3, 1], 0, 5, 8, 6),
    ("T and L 4 past the longest: every column has a padded tail", [6, 0, 3, 3, 1], 0, 5, 12, 10),
    ("index as a pointer into a longer table", [5, 2, 6, 0, 3, 3, 1, 4], 2, 5, 8, 6),
]


def _kernel_store(F, seed=0):
    rng = numpy.random.RandomState(seed + F)
    recs = [rng.normal(size=(t, F)).astype(numpy.float32) for t in FRAME_LEN]
    labs = [rng.randint(1, 50, size=l).astype(numpy.int64) for l in LABEL_LEN]
    return recs, labs


def run_kernel(device, lib, F):
    recs, labs = _kernel_store(F)
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(device)
    frames, labels = dev(numpy.concatenate(recs)), dev(numpy.concatenate(labs))
    frame_off = dev(numpy.concatenate([[0], numpy.cumsum(FRAME_LEN)]).astype(numpy.int64))
    label_off = dev(numpy.concatenate([[0], numpy.cumsum(LABEL_LEN)]).astype(numpy.int64))
    for name, table, first, B, T, L in KERNEL_CASES:
        want = Data.pad_batch([(recs[u], labs[u]) for u in table[first: first + B]], min_frames=T, min_labels=L)
        assert want["recordings"].shape == (T, B, F) and want["labels"].shape == (L, B), name
        # the outputs sit inside larger allocations: one guard row in front and one behind, everything pre-filled with garbage
        rec = torch.full((T + 2, B, F), float("nan"), dtype=torch.float32, device=device)
        rmask = torch.full((T + 2, B), float("nan"), dtype=torch.float32, device=device)
        lab = torch.full((L + 2, B), -1, dtype=torch.int64, device=device)
        lmask = torch.full((L + 2, B), float("nan"), dtype=torch.float32, device=device)
        index = dev(numpy.asarray(table, numpy.int64))
        args = lib.make("lvsr_batch_args", frames=frames, frame_off=frame_off, labels=labels, label_off=label_off,
                        index=index.data_ptr() + 8 * first, n=len(FRAME_LEN), B=B, T=T, L=L, F=F, recordings=rec[1:],
                        recordings_mask=rmask[1:], out_labels=lab[1:], labels_mask=lmask[1:])
        lib.call("lvsr_assemble_batch", lib.stream_for(rec), ctypes.byref(args))
        if device.type == "cuda":
            torch.cuda.synchronize()
        got = dict(recordings=_host(rec), recordings_mask=_host(rmask), labels=_host(lab), labels_mask=_host(lmask))
        for k, full in got.items():
            assert _same_bits(full[1:-1], want[k]), (name, F, k)
            guards = full[[0, -1]]
            assert (guards == -1).all() if k == "labels" else numpy.isnan(guards).all(), (name, F, k, "guard rows written")
    # bad arguments fail on the host, with a message
    args.B = 0
    with pytest.raises(native.NativeError, match="bad sizes"):
        lib.call("lvsr_assemble_batch", lib.stream_for(rec), ctypes.byref(args))


@pytest.mark.parametrize("F", WIDTHS)
def test_assemble_kernel_emulated(F):
    from emu import emu_lib
    run_kernel(torch.device("cpu"), emu_lib(), F)


@pytest.mark.gpu
@pytest.mark.parametrize("F", WIDTHS)
def test_assemble_kernel_gpu(gpu_device, F):
    run_kernel(gpu_device, native.get(), F)


# ---- the option grid of the plan and stream tests ------------------------------------------------------------------------------
def _dataset(n, F=5, V=9, seed=0, tagged=False):
    """Ragged utterances of 6..13 frames and 2..4 labels; tagged: every value of utterance i is i (recognisable in a host batch)."""
    rng = numpy.random.RandomState(seed)
    recs = [rng.normal(size=(rng.randint(6, 14), F)).astype(numpy.float32) for _ in range(n)]
    labs = [rng.randint(1, V - 2, size=rng.randint(2, 5)) for _ in range(n)]
    if tagged:
        recs = [numpy.full_like(r, i) for i, r in enumerate(recs)]
    return ArrayDataset(recs, labs, num_characters=V, bos_label=V - 2)


# (name, dataset sizes {part: n}, Data keywords, get_stream keywords incl. the part)
GRID = [
    ("in order, trailing partial batch", dict(train=11), dict(batch_size=4), dict(part="train", shuffle=False)),
    ("shuffled, seed 1", dict(train=11), dict(batch_size=4), dict(part="train", shuffle=True, seed=1)),
    ("shuffled, seed 2", dict(train=11), dict(batch_size=4), dict(part="train", shuffle=True, seed=2)),
    ("sort_k_batches", dict(train=11), dict(batch_size=3, sort_k_batches=2), dict(part="train", shuffle=True, seed=1)),
    ("max_length drops utterances", dict(train=11), dict(batch_size=4, sort_k_batches=2, max_length=10),
     dict(part="train", shuffle=True, seed=2)),
    ("num_examples", dict(train=11), dict(batch_size=4), dict(part="train", shuffle=True, seed=1, num_examples=7)),
    ("validation batch size", dict(train=11, valid=8), dict(batch_size=4, validation_batch_size=3, sort_k_batches=2),
     dict(part="valid", shuffle=False)),
    ("world 2, rank 0: trailing global batch of 1 dropped", dict(train=9), dict(batch_size=4),
     dict(part="train", shuffle=True, seed=1, rank=0, world=2)),
    ("world 2, rank 1: trailing global batch of 1 dropped", dict(train=9), dict(batch_size=4),
     dict(part="train", shuffle=True, seed=1, rank=1, world=2)),
    ("world 2 with sort_k and padding multiples", dict(train=11), dict(batch_size=4, sort_k_batches=2, pad_frames_to=4, pad_labels_to=2),
     dict(part="train", shuffle=True, seed=2, rank=1, world=2)),
]
STREAM_GRID = GRID + [
    ("add_bos", dict(train=11), dict(batch_size=4, add_bos=1), dict(part="train", shuffle=True, seed=1)),
    ("no EOS", dict(train=11), dict(batch_size=4, add_eos=False), dict(part="train", shuffle=False)),
    ("float64 normalization", dict(train=11), dict(batch_size=4, normalization="float64"), dict(part="train", shuffle=True, seed=1)),
    ("float32 normalization", dict(train=11), dict(batch_size=4, normalization="float32"), dict(part="train", shuffle=True, seed=1)),
    ("padding multiples", dict(train=11), dict(batch_size=4, pad_frames_to=4, pad_labels_to=2), dict(part="train", shuffle=True, seed=1)),
]


def _make_data(sizes, kw, tagged=False):
    datasets = {part: _dataset(n, seed=3 + j, tagged=tagged) for j, (part, n) in enumerate(sorted(sizes.items()))}
    kw = dict(kw)
    if kw.get("normalization"):
        dtype = numpy.dtype(kw["normalization"])
        allf = numpy.concatenate(datasets["train"].recordings).astype(numpy.float64)
        kw["normalization"] = (allf.mean(0).astype(dtype), allf.std(0).astype(dtype))
    return Data(datasets, **kw)


# ---- 4.2 the plan, host only ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GRID, ids=[c[0] for c in GRID])
def test_plan_is_the_order_of_the_host_stream(case):
    _, sizes, kw, stream_kw = case
    data = _make_data(sizes, kw, tagged=True)
    stream_kw = dict(stream_kw)
    part = stream_kw.pop("part")
    dd = DeviceData(data, device="cpu", parts=())            # nothing uploaded: planning needs neither a library nor a device
    plan = dd.plan(part, **stream_kw)
    walked = [b for b in data.get_stream(part, **stream_kw) if b is not None]
    assert len(plan) == len(walked) and len(plan) >= 2
    seen = 0
    for (index, T, L, gbs), batch in zip(plan, walked):
        tags = batch["recordings"][0, :, 0].astype(numpy.int64)           # every utterance has at least one frame
        assert numpy.array_equal(dd.dataset_index(part)[index], tags)
        assert (T, L) == (batch["recordings"].shape[0], batch["labels"].shape[0])
        assert gbs == batch.get("global_batch_size")
        seen += len(index)
    if stream_kw.get("world", 1) == 2 and sizes["train"] == 9:
        assert len(plan) == 2 and [p[3] for p in plan] == [4, 4]          # 4 + 4 + 1: the last global batch is dropped
    if kw.get("max_length"):
        assert seen < sizes[part]


# ---- 4.3 the stream ---------------------------------------------------------------------------------------------------------------
def run_stream(device, lib, case):
    _, sizes, kw, stream_kw = case
    data = _make_data(sizes, kw)
    stream_kw = dict(stream_kw)
    part = stream_kw.pop("part")
    dd = DeviceData(data, device=device, lib=lib, chunk_bytes=1000)       # a chunk smaller than the part: several uploads
    assert dd.nbytes(part) > 1000
    want = [b for b in data.get_stream(part, **stream_kw) if b is not None]
    got = list(dd.get_stream(part, **stream_kw))                          # the whole epoch is drawn before anything is compared
    if device.type == "cuda":
        torch.cuda.synchronize()
    assert len(got) == len(want) and len(got) >= 2
    for g, w in zip(got, want):
        assert list(g) == list(w)
        for k in w:
            if k == "global_batch_size":
                assert g[k] == w[k]
            else:
                assert g[k].device.type == device.type
                assert _same_bits(_host(g[k]), w[k]), (case[0], k)
    # examples (batches=False) come from the host pipeline
    ex = list(dd.get_stream(part, batches=False, shuffle=False))
    assert len(ex) == len(dd.dataset_index(part)) and isinstance(ex[0][0], numpy.ndarray)


@pytest.mark.parametrize("case", STREAM_GRID, ids=[c[0] for c in STREAM_GRID])
def test_stream_equals_the_host_stream_emulated(case):
    from emu import emu_lib
    run_stream(torch.device("cpu"), emu_lib(), case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", STREAM_GRID, ids=[c[0] for c in STREAM_GRID])
def test_stream_equals_the_host_stream_gpu(gpu_device, case):
    run_stream(gpu_device, native.get(), case)


def test_surface_of_data():
    data = _make_data(dict(train=6, valid=5), dict(batch_size=4, validation_batch_size=2))
    dd = DeviceData(data, device="cpu", parts=())
    assert dd.datasets is data.datasets and dd.info_dataset is data.info_dataset
    assert (dd.batch_size, dd.validation_batch_size, dd.num_labels, dd.eos_label, dd.bos_label, dd.num_features()) == \
        (4, 2, data.num_labels, data.eos_label, data.bos_label, data.num_features())
    # a part that is not on the device streams from the host
    assert isinstance(next(iter(dd.get_stream("valid", shuffle=False)))["recordings"], numpy.ndarray)


# ---- 4.6 refusals ---------------------------------------------------------------------------------------------------------------
def run_refusals(device, lib):
    data = _make_data(dict(train=6), dict(batch_size=4))
    dd = DeviceData(data, device=device, lib=lib)
    n = len(dd.dataset_index("train"))
    st = dd._stores["train"]
    T, L = int(st.frame_len.max()), int(st.label_len.max())
    longest, wordiest = int(st.frame_len.argmax()), int(st.label_len.argmax())
    assert dd.assemble("train", [0, n - 1], T, L)["recordings"].shape == (T, 2, 5)
    calls = []
    launch = dd._launch
    dd._launch = lambda *a: calls.append(a) or launch(*a)
    for index, t, l in (([0, n], T, L), ([-1], T, L), ([longest], T - 1, L), ([wordiest], T, L - 1), ([], T, L)):
        with pytest.raises(ValueError):
            dd.assemble("train", index, t, l)
    assert not calls                                                        # refused before any launch


def test_refusals_emulated():
    from emu import emu_lib
    run_refusals(torch.device("cpu"), emu_lib())


@pytest.mark.gpu
def test_refusals_gpu(gpu_device):
    run_refusals(gpu_device, native.get())


# ---- 4.4 training steps ---------------------------------------------------------------------------------------------------------
EMU_NET = dict(input_dim=5, num_phonemes=6, dims_bidir=[4], dim_dec=5, dim_matcher=6, attention_type="content", post_merge_dims=None,
               embed_outputs=True, data_prepend_eos=False)          # the emulator runs a step of this net in seconds, of timit_tiny in tens


def _train_data(cfg):
    """Nine utterances in three minibatches of one shape (the padding multiples), so that the step's graph region is run eagerly,
    captured and replayed."""
    rng = numpy.random.RandomState(11)
    F, V = cfg["input_dim"], cfg["num_phonemes"]
    recs = [rng.normal(size=(rng.randint(5, 9), F)).astype(numpy.float32) for _ in range(9)]
    labs = [rng.randint(0, V - 1, size=rng.randint(2, 4)) for _ in range(9)]
    ds = ArrayDataset(recs, labs, num_characters=V)
    allf = numpy.concatenate(recs).astype(numpy.float64)
    return Data({"train": ds}, batch_size=3, sort_k_batches=3, pad_frames_to=8, pad_labels_to=4,
                normalization=(allf.mean(0), allf.std(0)))


def _three_steps(device, lib, cfg, data):
    from lvsr_amd import synthetic
    from lvsr_amd.bricks.recognizer import SpeechRecognizer
    from lvsr_amd.training import Trainer
    rec = SpeechRecognizer(device=device, params=synthetic.make_params(cfg, seed=3, scale=0.5), lib=lib, net_config=cfg)
    tr = Trainer(rec, gradient_threshold=100.0, rules=("momentum", "adadelta"), scale=0.1, distributed=False)
    steps = []
    for batch in data.get_stream("train", shuffle=True, seed=5):
        cm = tr.train_step(batch)
        if device.type == "cuda":
            torch.cuda.synchronize()
        staged = {k: _host(rec.ws.get("in." + k, tuple(batch[k].shape), batch[k].dtype if torch.is_tensor(batch[k])
                                      else torch.from_numpy(batch[k]).dtype)).copy() for k in batch}
        steps.append((staged, _host(cm).copy()))
    tr.close()
    return steps, rec.store.get_values()


def run_training(device, lib, cfg):
    data = _train_data(cfg)
    host_a, params_a = _three_steps(device, lib, cfg, data)
    host_b, params_b = _three_steps(device, lib, cfg, data)
    dev, params_d = _three_steps(device, lib, cfg, DeviceData(data, device=device, lib=lib))
    assert len(host_a) == len(dev) == 3
    shapes = {tuple(s["recordings"].shape) + tuple(s["labels"].shape) for s, _ in host_a}
    assert len(shapes) == 1, "the three steps must share one shape"
    for (hs, hcm), (ds, dcm) in zip(host_a, dev):
        for k in hs:
            assert _same_bits(ds[k], hs[k]), ("staged in." + k)
        assert _same_bits(dcm, hcm)
    # the parameters: the device path must equal the host path wherever the host path equals itself from run to run
    deterministic = all(_same_bits(params_a[k], params_b[k]) for k in params_a) and \
        all(_same_bits(a[1], b[1]) for a, b in zip(host_a, host_b))
    if deterministic:
        for k in params_a:
            assert _same_bits(params_d[k], params_a[k]), k
    return deterministic


def test_training_steps_equal_the_host_path_emulated():
    from emu import emu_lib
    assert run_training(torch.device("cpu"), emu_lib(), EMU_NET), "the emulator runs a step in a fixed order: two host runs must agree"


@pytest.mark.gpu
def test_training_steps_equal_the_host_path_gpu(gpu_device):
    from lvsr_amd import spec
    deterministic = run_training(gpu_device, native.get(), spec.timit_tiny())
    print("two runs of the host path gave the same parameters: %s" % deterministic)


# ---- 4.5 the stage driver ---------------------------------------------------------------------------------------------------------
def test_stage_driver_with_device_data_logs_the_same_costs(tmp_path):
    from emu import emu_lib
    from lvsr_amd import main, synthetic
    from lvsr_amd.checkpoint import save_parameters
    conf = dict(net=dict(dims_bidir=[4], dim_dec=5, dim_matcher=6, attention_type="content", embed_outputs=True),
                training=dict(gradient_threshold=10.0, scale=0.05, momentum=0.0, rules=["momentum"], num_epochs=2),
                regularization=dict(max_norm=3.0))
    rng = numpy.random.RandomState(4)
    recs = [rng.normal(size=(6 + (i % 5), 5)).astype(numpy.float32) for i in range(7)]
    labs = [rng.randint(0, 5, size=2 + (i % 3)) for i in range(7)]
    data = Data({"train": ArrayDataset(recs, labs, 6), "valid": ArrayDataset(recs[:3], labs[:3], 6)}, batch_size=4,
                validation_batch_size=3, sort_k_batches=2)
    start = str(tmp_path / "start.npz")
    save_parameters(start, synthetic.make_params(dict(conf["net"], input_dim=5, num_phonemes=6, post_merge_dims=None,
                                                      data_prepend_eos=False), seed=8, scale=0.5))
    kw = dict(params=start, device="cpu", lib=emu_lib(), distributed=False)
    _, host = main.train(conf, data, str(tmp_path / "host.zip"), **kw)
    _, flag = main.train(conf, data, str(tmp_path / "flag.zip"), device_data=True, **kw)
    assert len(host) == 2 * 2 + 2 and sum("valid_cost" in r for r in host) == 2        # minibatches of 4 and 3, twice, + 2 epoch rows
    assert len(flag) == len(host)
    for a, b in zip(flag, host):
        assert set(a) == set(b)
        for k in ("train_cost", "valid_cost", "iterations_done"):
            assert a.get(k) == b.get(k), (k, a, b)
    # one step of the same run through train_multistage(device_data=True), which wraps the data once and hands train() a DeviceData
    one = dict(conf, training=dict(conf["training"], num_epochs=None, num_batches=1))
    seen = []
    upload = DeviceData._upload
    try:
        DeviceData._upload = lambda self, part: seen.append(part) or upload(self, part)
        _, direct = main.train_multistage(one, data, str(tmp_path / "direct.zip"), device_data=True, **kw)
    finally:
        DeviceData._upload = upload
    assert sorted(seen) == ["train", "valid"]
    assert direct[0]["iterations_done"] == 1 and direct[0]["train_cost"] == host[0]["train_cost"]
