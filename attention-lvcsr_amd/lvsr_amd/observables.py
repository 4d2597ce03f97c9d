"""The reference's training and validation observables (lvsr/main.py:317-396, 526-569; lvsr/expressions.py:14-25), computed on
the device inside the training step (csrc/observables.hip) and read as one small record.

Per step (the `primary` channels): weights_penalty, weights_entropy, min_energy / max_energy (of the READOUTS: the reference's
`energies` here are readout.readout's output, main.py:354-356), mean_attended, mean_bottom_output, mask_density, total_step_norm,
min_gain / max_gain under an mse criterion (of the gain matrix behind maximum(., min_reward)), and the shapes batch_size,
max_num_phonemes, max_recording_length, max_attended_length, max_attended_mask_length; `<parameter>_stats` = [norm, gradient norm,
step norm, step norm / gradient norm], each norm over sqrt(elements) (main.py:534-541).

The inputs where they live: the alignment is `generator.last["weights"]` (the slice [1:] of the decoder's (L+1,B,T') buffer), its
mask the staged labels mask — under greedy exploration the device-written prediction mask —, the readouts `gen.logits`, the encoder
output `recognizer.encoded`, the bottom output the last bottom activation (the staged recordings without a bottom MLP), the flat
parameter / gradient / step buffers the optimiser's own.
"""
import ctypes

import numpy
import torch

from .native import ptr

ITEM_MAX = 8192                      # csrc/observables.hip OBS_ITEM_MAX
TS_PARTS = 3 * 1024                  # doubles of lvsr_tensor_stats' partials
DEFAULTS = dict(every=10, parameter_stats=True)
# the device record (float64): three words per group
ALIGN, ENERGY, ATTENDED, BOTTOM, GAIN, STEP_NORM, RECORD = 0, 3, 6, 9, 12, 15, 16


def settings(observables):
    """`Trainer(observables=)` / `monitoring.observables` (True, or a mapping with `every`, `parameter_stats`) -> the full
    settings, or None when it is off."""
    if not observables:
        return None
    conf = dict(DEFAULTS)
    if isinstance(observables, dict):
        unknown = set(observables) - set(DEFAULTS)
        if unknown:
            raise ValueError("unknown observables settings %s (known: %s)" % (sorted(unknown), sorted(DEFAULTS)))
        conf.update(observables)
    conf["every"] = int(conf["every"])
    if conf["every"] < 1:
        raise ValueError("observables.every must be a positive number of batches")
    conf["parameter_stats"] = bool(conf["parameter_stats"])
    return conf


def work_items(segments, item_max=ITEM_MAX):
    """The balanced work list of lvsr_segment_norms over a (nseg,4) segment table [offset, rows, cols, flags]:
    -> items (nitems,3) int64 [segment, start, count <= item_max], seg_first (nseg+1) int32."""
    items, first = [], [0]
    for s, (_, rows, cols, _) in enumerate(numpy.asarray(segments).tolist()):
        size = int(rows) * int(cols)
        for start in range(0, size, item_max):
            items.append((s, start, min(item_max, size - start)))
        first.append(len(items))
    return numpy.array(items, numpy.int64).reshape(-1, 3), numpy.array(first, numpy.int32)


def alignment_stats(lib, weights, mask, out, ws, accumulate=False):
    """Enqueue lvsr_alignment_stats on weights (L,B,T') — rows may be strided views of a larger buffer —, mask (L,B) or None,
    into the three doubles of `out`; `ws`: the Workspace the partials come from."""
    L, B, Tp = (int(s) for s in weights.shape)
    assert weights.stride(2) == 1 and weights.stride(0) == B * weights.stride(1), "the (l,b) rows must be equally spaced"
    assert mask is None or (mask.is_contiguous() and tuple(mask.shape) == (L, B))
    partials = ws.get("obs.align_partials", (2 * L * B,), torch.float64)
    lib.call("lvsr_alignment_stats", lib.stream_for(out), ptr(weights), int(weights.stride(1)), L, B, Tp, ptr(mask), ptr(partials),
             ptr(out), int(bool(accumulate)))


def utterance_stats(lib, weights, mask, costs, out, ws, lengths=None):
    """Enqueue lvsr_utterance_stats on weights (L,B,T') — rows may be strided views of a larger buffer —, mask / costs (L,B) or
    None, lengths (B) int32 or None (each utterance's own attended length), into `out` (B,4) float64: per utterance the summed
    cost, weights_std times its label count, monotonicity_penalty and the label count."""
    L, B, Tp = (int(s) for s in weights.shape)
    assert weights.stride(2) == 1 and weights.stride(0) == B * weights.stride(1), "the (l,b) rows must be equally spaced"
    for t in (mask, costs):
        assert t is None or (t.is_contiguous() and tuple(t.shape) == (L, B) and t.dtype == torch.float32)
    assert lengths is None or (lengths.is_contiguous() and tuple(lengths.shape) == (B,) and lengths.dtype == torch.int32)
    assert out.is_contiguous() and tuple(out.shape) == (B, 4) and out.dtype == torch.float64
    partials = ws.get("obs.utterance_partials", (3 * L * B,), torch.float64)
    lib.call("lvsr_utterance_stats", lib.stream_for(out), ptr(weights), int(weights.stride(1)), L, B, Tp, ptr(mask), ptr(costs),
             ptr(lengths), ptr(partials), ptr(out))


TIMES = 8                            # doubles per (l,b) row of lvsr_alignment_times
PEAK, PEAK_WEIGHT, MEAN, SPREAD, START, END, MASS, COST = range(TIMES)


def alignment_times(lib, weights, mask, costs, out, lengths=None, lo=0.1, hi=0.9):
    """Enqueue lvsr_alignment_times on weights (L,B,T') — rows may be strided views of a larger buffer —, mask / costs (L,B) or
    None, lengths (B) int32 or None (each utterance's own attended length), into `out` (L,B,8) float64: per label the peak position,
    the weight there, the mean position, the spread, the positions at which the running sum reaches `lo` and `hi` of its total, the
    total, and the label's cost (the slots PEAK .. COST above)."""
    L, B, Tp = (int(s) for s in weights.shape)
    assert weights.stride(2) == 1 and weights.stride(0) == B * weights.stride(1), "the (l,b) rows must be equally spaced"
    for t in (mask, costs):
        assert t is None or (t.is_contiguous() and tuple(t.shape) == (L, B) and t.dtype == torch.float32)
    assert lengths is None or (lengths.is_contiguous() and tuple(lengths.shape) == (B,) and lengths.dtype == torch.int32)
    assert out.is_contiguous() and tuple(out.shape) == (L, B, TIMES) and out.dtype == torch.float64
    lib.call("lvsr_alignment_times", lib.stream_for(out), ptr(weights), int(weights.stride(1)), L, B, Tp, ptr(mask), ptr(costs),
             ptr(lengths), float(lo), float(hi), ptr(out))


def tensor_stats(lib, x, out, ws, floor=None):
    """Enqueue lvsr_tensor_stats on the contiguous tensor x into the three doubles of `out` (min, max, sum |x|)."""
    assert x.is_contiguous() and x.dtype == torch.float32
    partials = ws.get("obs.tensor_partials", (TS_PARTS,), torch.float64)
    lib.call("lvsr_tensor_stats", lib.stream_for(out), ptr(x), int(x.numel()), int(floor is not None), float(floor or 0.0),
             ptr(partials), ptr(out))


class SegmentNorms(object):
    """lvsr_segment_norms over one segment table: the work list (built once), the partials and the outputs."""

    def __init__(self, lib, segments):
        dev = segments.device
        self.lib, self.segments, self.nseg = lib, segments, int(segments.shape[0])
        items, first = work_items(segments.cpu().numpy())
        self.items, self.seg_first = torch.from_numpy(items).to(dev), torch.from_numpy(first).to(dev)
        self.nitems = int(items.shape[0])
        self.partials = torch.zeros(max(1, self.nitems) * 3, dtype=torch.float64, device=dev)
        self.segsums = torch.zeros(self.nseg * 3, dtype=torch.float64, device=dev)
        self.out = torch.zeros(self.nseg, 4, dtype=torch.float32, device=dev)

    def enqueue(self, phase, total, param=None, grad=None, step=None, grad_scale=1.0, segflag=None, scratch=None, clip_state=None,
                remove_not_finite=0, nonfinite_scaler=0.0):
        """phase 1: in front of the optimiser (param, grad); 2: behind it (step -> out, total); 3: both."""
        lib = self.lib
        a = lib.make("lvsr_segnorm_args", param=param, grad=grad, step=step, segments=self.segments, items=self.items,
                     seg_first=self.seg_first, nseg=self.nseg, nitems=self.nitems, grad_scale=float(grad_scale),
                     nonfinite_scaler=float(nonfinite_scaler), remove_not_finite=int(remove_not_finite), segflag=segflag,
                     scratch=scratch, clip_state=clip_state, partials=self.partials, segsums=self.segsums, out=self.out, total=total)
        lib.call("lvsr_segment_norms", lib.stream_for(self.out), ctypes.byref(a), int(phase))


class Observables(object):
    """The observables of one Trainer: a device record, its pinned host mirror, and the launches around the optimiser step.
    Everything is allocated here or taken from the recognizer's workspace: nothing allocates inside the step's graph region."""

    def __init__(self, trainer, every=10, parameter_stats=True):
        rec = trainer.rec
        self.trainer, self.rec, self.lib = trainer, rec, rec.lib
        self.every, self.parameter_stats = int(every), bool(parameter_stats)
        dev = rec.store.device
        self.record = torch.zeros(RECORD, dtype=torch.float64, device=dev)
        self.norms = SegmentNorms(rec.lib, trainer.segments)
        pin = (lambda t: t.pin_memory()) if dev.type == "cuda" else (lambda t: t)
        self.host_record = pin(torch.zeros(RECORD, dtype=torch.float64))
        self.host_stats = pin(torch.zeros(self.norms.nseg, 4, dtype=torch.float32))
        self.names = list(rec.store.offsets)
        self.shapes = {}               # minibatch shape -> what the host knows of a step of that shape (a replayed graph enqueues nothing)
        self._shape = None

    def key(self):
        return ("observables", self.every, self.parameter_stats)

    def begin_step(self, batch):
        """Host side of a step, outside the graph region: which shape's record the next `read` decodes."""
        self._shape = (tuple(batch["recordings"].shape), tuple(batch["labels"].shape))

    def _opt_words(self):
        t = self.trainer
        return dict(segflag=t.segflag, scratch=t.scratch, clip_state=t.clip_state, remove_not_finite=t.conf["remove_not_finite"],
                    nonfinite_scaler=t.conf["nonfinite_scaler"])

    def enqueue_inputs(self):
        """Right behind the forward pass, inside the graph region that holds it (`cost_and_gradients(after_forward=)`): the alignment
        and tensor channels.  What the forward pass left on the recognizer (`generator.last`, `cost_mask`, `encoded`, `bottom_output`)
        is read here and only here: these attributes are those of the minibatch being enqueued exactly while its region's body
        runs — a replay does not refresh them, and a validation pass in between overwrites them."""
        rec, gen, lib, ws, r = self.rec, self.rec.generator, self.lib, self.rec.ws, self.record
        weights, mask = gen.last["weights"], rec.cost_mask
        readouts, attended, bottom = gen.last["readouts"], rec.encoded, rec.bottom_output
        alignment_stats(lib, weights, mask, r[ALIGN:ALIGN + 3], ws)
        tensor_stats(lib, readouts, r[ENERGY:ENERGY + 3], ws)
        tensor_stats(lib, attended, r[ATTENDED:ATTENDED + 3], ws)
        tensor_stats(lib, bottom, r[BOTTOM:BOTTOM + 3], ws)
        if gen.mse:
            tensor_stats(lib, gen.last["gain_matrix"], r[GAIN:GAIN + 3], ws, floor=gen.min_reward)
        L, B, Tp = (int(s) for s in weights.shape)
        self.shapes[self._shape] = dict(batch_size=B, max_num_phonemes=L, max_recording_length=int(bottom.shape[0]),
                                        max_attended_length=int(attended.shape[0]), max_attended_mask_length=int(rec.encoded_mask.shape[0]),
                                        n_attended=attended.numel(), n_bottom=bottom.numel(), mse=bool(gen.mse))

    def enqueue_before(self, param, grad, grad_scale):
        """In front of lvsr_opt_step (behind the all-reduce): phase 1 of the norms — the parameter as the gradient saw it.
        Without the per-parameter table the sums of p^2 still feed total_step_norm: RemoveNotFinite replaces the step of a
        non-finite tensor by p (1 - nonfinite_scaler), which phase 2 accounts for from them.  Only with both off is the pass
        over `param` and `grad` left out (the gradient sums then go nowhere)."""
        if self.parameter_stats or self.trainer.conf["remove_not_finite"]:
            self.norms.enqueue(1, self.record[STEP_NORM:], param=param, grad=grad, grad_scale=grad_scale)

    def enqueue_after(self, step):
        """Behind lvsr_opt_step: phase 2 of the norms, then the record to its host mirror."""
        self.norms.enqueue(2, self.record[STEP_NORM:], step=step, **self._opt_words())
        self.host_record.copy_(self.record, non_blocking=True)
        if self.parameter_stats:
            self.host_stats.copy_(self.norms.out, non_blocking=True)

    def read(self):
        """dict of the last step, named as in the reference (synchronises)."""
        dev = self.record.device
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        info = self.shapes.get(self._shape)
        if info is None:
            raise ValueError("no training step of this trainer has run yet")
        r = self.host_record.numpy()
        f32 = lambda v: float(numpy.float32(v))
        L, B = info["max_num_phonemes"], info["batch_size"]
        out = dict(weights_penalty=f32(r[ALIGN]), weights_entropy=f32(r[ALIGN + 1]), mask_sum=float(r[ALIGN + 2]),
                   mask_density=f32(r[ALIGN + 2] / (L * B)), min_energy=f32(r[ENERGY]), max_energy=f32(r[ENERGY + 1]),
                   mean_attended=f32(r[ATTENDED + 2] / info["n_attended"]), mean_bottom_output=f32(r[BOTTOM + 2] / info["n_bottom"]),
                   total_step_norm=f32(r[STEP_NORM]))
        if info["mse"]:
            out.update(min_gain=f32(r[GAIN]), max_gain=f32(r[GAIN + 1]))
        out.update((k, info[k]) for k in ("batch_size", "max_num_phonemes", "max_recording_length", "max_attended_length",
                                          "max_attended_mask_length"))
        if self.parameter_stats:
            stats = self.host_stats.numpy()
            out.update((name + "_stats", stats[i].copy()) for i, name in enumerate(self.names))
        return out


class ValidationRecord(object):
    """Device accumulator of a validation pass: the summed cost and the alignment channels over all batches, read once."""

    def __init__(self, recognizer):
        self.rec = recognizer
        self.acc = torch.zeros(4, dtype=torch.float64, device=recognizer.store.device)      # penalty, entropy, mask sum | cost

    def add(self, cost_matrix):
        """Behind `recognizer.cost(...)` of a batch: its alignment under the mask the cost was taken with, and its summed cost."""
        rec = self.rec
        with rec._on_stream():
            alignment_stats(rec.lib, rec.generator.last["weights"], rec.cost_mask, self.acc[:3], rec.ws, accumulate=True)
            self.acc[3:] += cost_matrix.sum().double()

    def read(self):
        """-> (cost sum, penalty sum, entropy sum, mask sum) (synchronises)."""
        a = self.acc.cpu().numpy()
        return float(a[3]), float(a[0]), float(a[1]), float(a[2])
