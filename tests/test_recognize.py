"""From waveforms to hypotheses (lvsr_amd/frontend.py, audio.py, decode.recognize, the staged entry points of the recognizer and
the beam search) against the path that existed before: Fbank.batch -> add_deltas_cmvn_batch -> copy to the host -> slices ->
SpeechRecognizer._pad_recordings / beam_search_batch.  Same device on both sides, so features are compared bit for bit and searches
token for token with equal costs.  The bodies run on the CPU emulator and, under the `gpu` marker, on the device."""
import wave

import numpy
import pytest
import torch

from lvsr_amd import audio, decode, synthetic
from lvsr_amd.bricks.recognizer import SpeechRecognizer
from lvsr_amd.frontend import FrontEnd
from lvsr_amd.search import CandidateNotFoundError

CFG = dict(input_dim=15, num_phonemes=8, dims_bidir=[4, 4], subsample=[1, 2], dim_dec=6, dim_matcher=8,
           attention_type="content_and_conv", conv_n=2, conv_num_filters=2, post_merge_dims=[6],
           post_merge_activation="maxout2", embed_outputs=False, data_prepend_eos=False, max_decoded_length_scale=4)
FBANK = dict(num_mel=4, use_energy=True)          # 5 static coefficients, 15 with deltas
FRAMES = [4, 10, 21, 38, 38]                      # five utterances: chunks of two leave a chunk of one
BEAM, BATCH = 3, 2
SEARCH = dict(char_discount=0.2, round_to_inf=1e9, stop_on="patience")


def _lib(device):
    if device == "cpu":
        from emu import emu_lib
        return emu_lib()
    from lvsr_amd import native
    return native.get()


def waveforms():
    rng = numpy.random.RandomState(11)
    out = []
    for i, f in enumerate(FRAMES):
        n = 400 + 160 * (f - 1) + (37 * i) % 160          # f frames, with samples to spare behind the last one
        t = numpy.arange(n)
        amp = 300.0 * (1 + i) * (1.0 + 0.8 * numpy.sin(t / (150.0 + 40 * i)))
        out.append(numpy.clip(rng.randn(n) * amp, -32000, 32000).astype(numpy.int16))
    return out


_made = {}


def setup(device):
    """-> dict(wavs, fe: the fitted front end, rec, ...), made once per device"""
    key = str(device)
    if key in _made:
        return _made[key]
    lib = _lib(device)
    wavs = waveforms()
    fe = FrontEnd(device=device, lib=lib, fbank=FBANK)
    assert fe.num_features == 15 and [fe.num_frames(len(w)) for w in wavs] == FRAMES
    fe.fit([wavs[:2], wavs[2:]])
    rec = SpeechRecognizer(device=device, params=synthetic.make_params(CFG, seed=7, scale=2.0), lib=lib, net_config=CFG)
    rec.init_beam_search(BEAM)
    _made[key] = dict(wavs=wavs, fe=fe, rec=rec, lib=lib, old={})
    return _made[key]


def glue_features(fe, wavs):
    """the hand-written path: the list of (T_i, 15) host arrays.  (Always over the very list of waveforms the new path gets:
    lvsr_fbank_batch transforms the frames of a set in pairs, so a frame's last bits depend on its neighbour in the set.)"""
    fb = fe.fbank
    feats, foff = fb.batch(wavs)
    out = fb.add_deltas_cmvn_batch(feats, foff, mean=fe.mean, std=fe.std).cpu().numpy()
    off = foff.cpu().numpy()
    return [out[off[i]: off[i + 1]] for i in range(len(wavs))]


def same_bits(a, b):
    a, b = numpy.ascontiguousarray(a, numpy.float32), numpy.ascontiguousarray(b, numpy.float32)
    return a.shape == b.shape and (a.view(numpy.uint32) == b.view(numpy.uint32)).all()


# ---- FrontEnd.fit, save / load ------------------------------------------------------------------------------------------------------
def run_fit(device, tmp_path):
    s = setup(device)
    fe, wavs = s["fe"], s["wavs"]
    fb = fe.fbank
    feats, foff = fb.batch(wavs)
    X = fb.add_deltas_cmvn_batch(feats, foff).cpu().numpy().astype(numpy.float64)          # the device's own un-normalised features
    N = X.shape[0]
    assert N == sum(FRAMES)
    mean = X.sum(axis=0) / N                                                               # lvsr/preprocessing.py:13-35
    std = numpy.sqrt((X ** 2).sum(axis=0) / N - mean ** 2)
    # float64 sums in another order differ by N 2^-53 relative, times the cancellation of s2 / N - mean^2 (below 1e4 here: asserted):
    # far below half a float32 ulp, so the float32 values are equal or, where the float64 value sits on a rounding boundary, neighbours
    assert ((X ** 2).sum(axis=0) / N / (std ** 2)).max() < 1e4
    for got, ref in ((fe.mean, mean), (fe.std, std)):
        ref32 = ref.astype(numpy.float32)
        assert got.dtype == numpy.float32 and (numpy.abs(got - ref32) <= numpy.spacing(numpy.abs(ref32))).all()
    path = str(tmp_path / "front_end.npz")
    fe.save(path)
    with numpy.load(path, allow_pickle=False) as z:
        assert "mean" in z.files and int(z["fbank_num_mel"]) == 4
    again = FrontEnd.load(path, device=device, lib=s["lib"])
    assert again.fbank_settings == fe.fbank_settings and again.deltas == fe.deltas
    x0, m0, l0 = fe.batch(wavs)
    x0, m0 = x0.cpu().numpy().copy(), m0.cpu().numpy().copy()
    x1, m1, l1 = again.batch(wavs)
    assert l0 == l1 and same_bits(x0, x1.cpu().numpy()) and same_bits(m0, m1.cpu().numpy())
    with pytest.raises(ValueError, match="no frames"):
        FrontEnd(device=device, lib=s["lib"], fbank=FBANK).fit([[wavs[0][:100]]])
    with pytest.raises(ValueError, match="variance of column 0"):
        FrontEnd(device=device, lib=s["lib"], fbank=FBANK).fit([[numpy.zeros(400 + 160 * 3, numpy.int16)]])


def test_fit_emulated(tmp_path):
    run_fit("cpu", tmp_path)


@pytest.mark.gpu
def test_fit_gpu(gpu_device, tmp_path):
    run_fit(gpu_device, tmp_path)


# ---- FrontEnd.batch = the glue ------------------------------------------------------------------------------------------------------
def run_batch(device):
    s = setup(device)
    fe, rec = s["fe"], s["rec"]
    for index in ([0, 1, 2, 3, 4], [3, 0], [2]):
        want_x, want_m = rec._pad_recordings(glue_features(fe, [s["wavs"][i] for i in index]), 64)
        x, mask, lengths = fe.batch([s["wavs"][i] for i in index])
        assert lengths == [FRAMES[i] for i in index]
        assert x.device.type == torch.device(device).type and same_bits(want_x, x.cpu().numpy()) and same_bits(want_m, mask.cpu().numpy())
    # a caller's T; a T that is too short
    x, mask, _ = fe.batch(s["wavs"][:2], T=11)
    assert tuple(x.shape) == (11, 2, 15) and same_bits(x.cpu().numpy()[:10, 1], glue_features(fe, s["wavs"][:2])[1]) and float(mask.sum()) == 14.0
    with pytest.raises(ValueError, match="shorter than the longest"):
        fe.batch(s["wavs"][:2], T=9)
    # without deltas: the static columns, normalised by their own statistics
    plain = FrontEnd(device=device, lib=s["lib"], fbank=FBANK, deltas=False, mean=fe.mean[:5], std=fe.std[:5])
    x5, _, _ = plain.batch(s["wavs"][:3])
    assert tuple(x5.shape) == (64, 3, 5) and same_bits(x5.cpu().numpy()[:21, 2], glue_features(fe, s["wavs"][:3])[2][:, :5])


def test_batch_is_the_glue_emulated():
    run_batch("cpu")


@pytest.mark.gpu
def test_batch_is_the_glue_gpu(gpu_device):
    run_batch(gpu_device)


# ---- decode.recognize against beam_search_batch on the glue's arrays ----------------------------------------------------------------
def old_path(s, chunk):
    key = tuple(chunk)
    if key not in s["old"]:
        s["old"][key] = s["rec"].beam_search_batch(glue_features(s["fe"], [s["wavs"][i] for i in chunk]), **SEARCH)
    return s["old"][key]


def same_result(a, b):
    if isinstance(a, Exception) or isinstance(b, Exception):
        return type(a) is type(b)
    return a[0] == b[0] and a[1] == b[1]          # tokens; costs as Python floats: equal means the same bits (none is a nan)


def run_recognize(device, sort):
    s = setup(device)
    fe, rec, wavs = s["fe"], s["rec"], s["wavs"]
    plan = decode.recognize_plan([len(w) for w in wavs], BATCH, sort)
    # (utterances 3 and 4 have 38 frames each; 4 has more samples behind its last frame)
    assert plan == ([[4, 3], [2, 1], [0]] if sort else [[0, 1], [2, 3], [4]])
    named = [("utt%d" % i, w) for i, w in enumerate(wavs)]
    staged = []                                      # every hypothesis of every chunk, as recognize got them
    rec.beam_search_staged = lambda *a, **kw: staged.append(SpeechRecognizer.beam_search_staged(rec, *a, **kw)) or staged[-1]
    try:
        rows = decode.recognize(rec, fe, named, beam_size=BEAM, batch=BATCH, to_text=lambda labels: "".join(chr(97 + t) for t in labels),
                                sort=sort, **SEARCH)
    finally:
        del rec.beam_search_staged
    assert len(staged) == len(plan)
    assert [r["id"] for r in rows] == [n for n, _ in named] and [r["num_frames"] for r in rows] == FRAMES
    found = 0
    for chunk, new in zip(plan, staged):
        old = old_path(s, chunk)
        assert len(new) == len(old) and all(same_result(a, b) for a, b in zip(new, old)), (chunk, new, old)
        for i, res in zip(chunk, old):
            row = rows[i]
            if isinstance(res, CandidateNotFoundError):
                assert row["recognized"] == [] and row["search_cost"] != row["search_cost"] and row["error"] == "CandidateNotFoundError"
            else:
                assert not isinstance(res, Exception), res
                assert row["recognized"] == res[0][0] and row["search_cost"] == res[1][0] and "error" not in row
                found += 1
            assert row["text"] == "".join(chr(97 + t) for t in row["recognized"])
    assert found >= 3                                # the comparison is about searches that end
    if not sort:                                     # bare arrays: the ids are the positions
        assert [r["id"] for r in decode.recognize(rec, fe, wavs[:1], beam_size=BEAM, batch=BATCH, **SEARCH)] == [0]


def test_recognize_sorted_emulated():
    run_recognize("cpu", True)


def test_recognize_input_order_emulated():
    run_recognize("cpu", False)


@pytest.mark.gpu
def test_recognize_sorted_gpu(gpu_device):
    run_recognize(gpu_device, True)


@pytest.mark.gpu
def test_recognize_input_order_gpu(gpu_device):
    run_recognize(gpu_device, False)


def test_recognize_plan():
    assert decode.recognize_plan([5, 9, 9, 2, 7], 2, True) == [[1, 2], [4, 0], [3]]
    assert decode.recognize_plan([5, 9, 9, 2, 7], 2, False) == [[0, 1], [2, 3], [4]]
    assert decode.recognize_plan([], 4, True) == [] and decode.recognize_plan([3, 1], 64, True) == [[0, 1]]


# ---- refusals in front of any launch -------------------------------------------------------------------------------------------------
def run_refusals(device):
    s = setup(device)
    fe, rec, wavs, lib = s["fe"], s["rec"], s["wavs"], s["lib"]
    x, mask, lengths = fe.batch(wavs[:2])          # (a good batch for the staged entry points below)
    graphs, generations = lib._lvsr_graph_count(), (rec.ws.generation, fe.ws.generation)
    calls = []
    lib.call = lambda name, *a: calls.append(name) or type(lib).call(lib, name, *a)
    try:
        with pytest.raises(ValueError, match="'short'.*fewer than one frame"):
            decode.recognize(rec, fe, [("ok", wavs[1]), ("short", wavs[0][:399])], beam_size=BEAM, **SEARCH)
        narrow = FrontEnd(device=device, lib=lib, fbank=FBANK, deltas=False)
        del calls[:]                                 # (building a front end uploads tables; it launches nothing)
        with pytest.raises(ValueError, match="5 features per frame, the recognizer takes 15"):
            decode.recognize(rec, narrow, wavs[:2], beam_size=BEAM, **SEARCH)
        with pytest.raises(ValueError, match="use beam_search_batch"):
            rec.beam_search_staged(x, mask, lengths, validate_solution_function=lambda *a: True, **SEARCH)
        with pytest.raises(ValueError, match="5 features per frame"):
            rec.compute_contexts_staged(x[:, :, :5].contiguous(), mask)
        with pytest.raises(ValueError, match="float32"):
            rec.compute_contexts_staged(x.double(), mask)
        assert calls == []
    finally:
        del lib.call
    assert lib._lvsr_graph_count() == graphs and (rec.ws.generation, fe.ws.generation) == generations


def test_refusals_emulated():
    run_refusals("cpu")


@pytest.mark.gpu
def test_refusals_gpu(gpu_device):
    run_refusals(gpu_device)


# ---- audio ------------------------------------------------------------------------------------------------------------------------
def write_wav(path, samples, rate=16000, width=2, channels=1):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(samples.tobytes())


def test_read_wav_and_scp(tmp_path):
    samples = waveforms()[1]
    write_wav(tmp_path / "a.wav", samples)
    got = audio.read_wav(tmp_path / "a.wav", sample_rate=16000.0)
    assert got.dtype == numpy.int16 and got.shape == samples.shape and (got == samples).all()
    write_wav(tmp_path / "eight.wav", (samples >> 8).astype(numpy.int8).view(numpy.uint8), width=1)
    with pytest.raises(ValueError, match="sample width of 1 bytes"):
        audio.read_wav(tmp_path / "eight.wav")
    write_wav(tmp_path / "stereo.wav", numpy.stack([samples, samples], axis=1), channels=2)
    with pytest.raises(ValueError, match="2 channels"):
        audio.read_wav(tmp_path / "stereo.wav")
    write_wav(tmp_path / "slow.wav", samples, rate=8000)
    with pytest.raises(ValueError, match="sample rate 8000 Hz"):
        audio.read_wav(tmp_path / "slow.wav", sample_rate=16000.0)
    scp = tmp_path / "wav.scp"
    scp.write_text("utt1 %s\n\nutt2  %s \n" % (tmp_path / "a.wav", tmp_path / "slow.wav"))
    assert audio.read_wav_scp(scp) == [("utt1", str(tmp_path / "a.wav")), ("utt2", str(tmp_path / "slow.wav"))]
    scp.write_text("utt1 %s\nutt2 sph2pipe -f wav x.sph |\n" % (tmp_path / "a.wav"))
    with pytest.raises(ValueError, match="utt2 is a piped command"):
        audio.read_wav_scp(scp)
