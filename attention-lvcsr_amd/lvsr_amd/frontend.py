"""From waveforms to the recognizer's input batch on the device: `Fbank` (log mel-filterbank + energy), deltas, global CMVN,
time-major layout and padding in two launches (lvsr_fbank_batch, lvsr_frontend_batch), and the global CMVN statistics the
reference's `Normalization` computes (lvsr/preprocessing.py:13-35) by lvsr_feature_stats.  What crosses to the device per batch is
the PCM itself and two offset tables — about 2.5 bytes per sample in place of 4 x 123 bytes per frame of padded features."""
import numpy
import torch

from .features import Fbank
from .native import ptr
from .params import Workspace

STATS_PARTS = 1024             # work-groups of lvsr_feature_stats' first stage at the most (its `partials`: 2 * width * 1024 doubles)
MAX_DIM = 64                   # static coefficients per frame lvsr_frontend_batch takes (DC_MAXDIM of csrc/fbank.hip)
# the keyword arguments of features.Fbank a saved front end carries, with Fbank's defaults
FBANK_DEFAULTS = dict(num_mel=40, use_energy=True, sample_rate=16000.0, frame_length_ms=25.0, frame_shift_ms=10.0, preemph=0.97,
                      remove_dc=True, low_freq=20.0, high_freq=0.0)


def _host_wavs(wavs):
    return [numpy.asarray(w.cpu() if torch.is_tensor(w) else w, dtype=numpy.int16).ravel() for w in wavs]


class FrontEnd(object):
    def __init__(self, device="cuda:0", lib=None, fbank=None, deltas=True, mean=None, std=None):
        """`fbank`: keyword arguments of `features.Fbank`; `mean` / `std`: the global statistics over `num_features` columns (both or
        neither; `fit` computes them)."""
        from . import native
        self.lib = lib if lib is not None else native.get()
        self.device = torch.device(device)
        unknown = sorted(set(fbank or {}) - set(FBANK_DEFAULTS))
        if unknown:
            raise ValueError("FrontEnd: unknown fbank setting(s) %s" % unknown)
        self.fbank_settings = dict(FBANK_DEFAULTS, **(fbank or {}))
        self.fbank = Fbank(device=self.device, lib=self.lib, **self.fbank_settings)
        if not self.fbank.batchable:
            raise ValueError("FrontEnd: the batched filterbank holds the filters as at most 64 (filter, 16-bin chunk) items")
        self.deltas = bool(deltas)
        self.dim = self.fbank.num_mel + int(self.fbank.use_energy)
        if self.dim > MAX_DIM:
            raise ValueError("FrontEnd: lvsr_frontend_batch takes at most %d static coefficients per frame, not %d" % (MAX_DIM, self.dim))
        self.num_features = self.dim * (3 if self.deltas else 1)
        self.sample_rate = float(self.fbank_settings["sample_rate"])
        self.ws = Workspace(self.device)
        self.set_statistics(mean, std)

    def set_statistics(self, mean, std):
        if (mean is None) != (std is None):
            raise ValueError("FrontEnd: mean and std come together or not at all")
        if mean is None:
            self.mean = self.std = self._mean = self._istd = None
            return
        self.mean = numpy.ascontiguousarray(mean, dtype=numpy.float32).ravel()
        self.std = numpy.ascontiguousarray(std, dtype=numpy.float32).ravel()
        if self.mean.shape != (self.num_features,) or self.std.shape != (self.num_features,):
            raise ValueError("FrontEnd: statistics of %d / %d columns for %d features" % (self.mean.size, self.std.size, self.num_features))
        self._mean = torch.from_numpy(self.mean).to(self.device)
        # (the reciprocal as Fbank.add_deltas_cmvn_batch takes it: float32, on the device)
        self._istd = (1.0 / torch.as_tensor(self.std, dtype=torch.float32, device=self.device)).contiguous()

    def num_frames(self, num_samples):
        return self.fbank.num_frames(num_samples)

    # ---- launches ------------------------------------------------------------------------------------------------
    def _static(self, wavs):
        """lvsr_fbank_batch over a list of waveforms -> (feats, frame_off on the device, frames per utterance on the host); the
        only copies to the device are the PCM and the two offset tables."""
        host = _host_wavs(wavs)
        if not host:
            raise ValueError("FrontEnd: no waveforms")
        lens = numpy.array([len(w) for w in host], dtype=numpy.int64)
        nfr = [self.fbank.num_frames(int(n)) for n in lens]
        wav_off = numpy.concatenate([[0], numpy.cumsum(lens)]).astype(numpy.int64)
        frame_off = numpy.concatenate([[0], numpy.cumsum(nfr)]).astype(numpy.int64)
        if frame_off[-1] >= 1 << 31:
            raise ValueError("FrontEnd: %d frames in one batch (the offsets are 32-bit)" % frame_off[-1])
        wav = torch.from_numpy(numpy.concatenate(host)).to(self.device, non_blocking=True)
        feats, foff = self.fbank.batch_resident(wav, torch.from_numpy(wav_off).to(self.device, non_blocking=True),
                                                torch.from_numpy(frame_off.astype(numpy.int32)).to(self.device, non_blocking=True),
                                                len(host), int(frame_off[-1]))
        return feats, foff, nfr

    def batch(self, wavs, pad_to=64, T=None):
        """wavs: list of 1-D int16 arrays / tensors -> (x (T, B, num_features), mask (T, B) on the device, lengths: the frames of
        every utterance, a host list).  T: the longest utterance rounded up to a multiple of `pad_to` (as
        SpeechRecognizer.compute_contexts_batch pads), or the caller's.  Two launches and no synchronisation; x and mask are this
        object's buffers and hold their values until the next call."""
        feats, foff, lengths = self._static(wavs)
        longest = max(lengths)
        if T is None:
            T = max(1, (longest + pad_to - 1) // pad_to) * pad_to
        if int(T) < max(1, longest):
            raise ValueError("FrontEnd.batch: T = %d is shorter than the longest utterance (%d frames)" % (T, longest))
        T, B = int(T), len(lengths)
        x = self.ws.get("frontend.x", (T, B, self.num_features))
        mask = self.ws.get("frontend.mask", (T, B))
        self.lib.call("lvsr_frontend_batch", self.lib.stream_for(x), ptr(feats), ptr(foff), B, int(feats.shape[0]), int(longest), self.dim,
                      int(self.deltas), ptr(self._mean), ptr(self._istd), T, ptr(x), ptr(mask))
        return x, mask, lengths

    # ---- global statistics ---------------------------------------------------------------------------------------
    def fit(self, wav_batches):
        """Global mean / standard deviation over every frame of `wav_batches` (an iterable of lists of waveforms), as the reference's
        Normalization takes them: float64 sums (on the device, lvsr_feature_stats), mean = s / N, std = sqrt(s2 / N - mean^2) in
        float64 on the host, stored as float32.  One read-back, at the end.  -> self"""
        W = self.num_features
        sums = torch.zeros(2 * W, dtype=torch.float64, device=self.device)
        partials = self.ws.get("frontend.stats_partials", (2 * W * STATS_PARTS,), torch.float64)
        frames = 0
        for wavs in wav_batches:
            feats, foff, nfr = self._static(wavs)
            if not sum(nfr):
                continue
            if self.deltas:
                feats = self.fbank.add_deltas_cmvn_batch(feats, foff)
            self.lib.call("lvsr_feature_stats", self.lib.stream_for(sums), ptr(feats), int(feats.shape[0]), W, ptr(partials), ptr(sums), 1)
            frames += sum(nfr)
        if frames == 0:
            raise ValueError("FrontEnd.fit: no frames (every waveform is shorter than one frame)")
        s = sums.cpu().numpy()
        mean = s[:W] / frames
        var = s[W:] / frames - mean ** 2
        bad = numpy.nonzero(~(var > 0))[0]
        if len(bad):
            raise ValueError("FrontEnd.fit: the variance of column %d is %g over %d frames: no standard deviation to divide by"
                             % (bad[0], var[bad[0]], frames))
        self.set_statistics(mean.astype(numpy.float32), numpy.sqrt(var).astype(numpy.float32))
        return self

    # ---- persistence ---------------------------------------------------------------------------------------------
    def save(self, path):
        """One .npz (no pickled objects): the fbank settings, `deltas`, and the statistics when there are any."""
        arrays = {"fbank_" + k: numpy.asarray(v) for k, v in self.fbank_settings.items()}
        arrays["deltas"] = numpy.asarray(self.deltas)
        if self.mean is not None:
            arrays.update(mean=self.mean, std=self.std)
        with open(path, "wb") as f:
            numpy.savez(f, **arrays)

    @classmethod
    def load(cls, path, device="cuda:0", lib=None):
        with numpy.load(path, allow_pickle=False) as z:
            fbank = {k: type(v)(z["fbank_" + k][()]) for k, v in FBANK_DEFAULTS.items()}
            return cls(device=device, lib=lib, fbank=fbank, deltas=bool(z["deltas"][()]),
                       mean=z["mean"] if "mean" in z.files else None, std=z["std"] if "std" in z.files else None)
