"""The training set resident in device memory, minibatches assembled there (include/lvsr_hip.h lvsr_assemble_batch,
csrc/batch.hip).

`Data.get_stream` is host Python for every utterance of every epoch: EOS / BOS by numpy.hstack, normalisation, zero-filled padding
utterance by utterance, then a copy from pageable memory.  The dataset is static, so `DeviceData` does the per-utterance part ONCE
— through the wrapped `Data`'s own stream, so the uploaded bits are those the host path produces — keeps the result in HBM as a
ragged store (frames and labels back to back, 64-bit offset tables), and builds every minibatch with one launch: per step the host
only plans (which utterances, which padded lengths) and enqueues.

Equivalence with the host path: the store holds what `data.get_stream(part, batches=False, shuffle=False)` yields;
the epoch plan is made by `Data._sort_k` and `Data._batches` themselves, run over zero-width stand-ins that carry an utterance's
store slot and its lengths, with `Data.pad_batch` deriving the padded lengths; the kernel copies values and writes 0 / 1.  Batches
are therefore equal to the host path's bit for bit (tests/test_device_data.py).
"""
import copy
import ctypes

import numpy
import torch

from . import native
from .data import Data


class _Ref(numpy.ndarray):
    """Stand-in for an utterance's recording in the planning pass: a (T_i, 0) array (the length is all `_sort_k` and `pad_batch`
    look at) that remembers its slot in the store."""
    slot = -1


class _Store(object):
    """One part of the dataset on the device."""
    def __init__(self):
        self.frames = self.labels = self.frame_off = self.label_off = None      # device tensors
        self.frame_len = self.label_len = None                                  # host int64 (n)
        self.index_of = None         # (n) store slot -> index in the host dataset (`max_length` drops utterances)
        self.slot_of = None          # (dataset size) dataset index -> store slot, or -1
        self.refs = self.label_stubs = None
        self.n = self.F = 0


def _upload_rows(arrays, total_rows, width, dtype, device, chunk_bytes):
    """Concatenate `arrays` (an iterable of (rows_i, width) host arrays, consumed once) into one device tensor (total_rows, width)
    through a staging buffer of at most `chunk_bytes`: no second full copy on the host."""
    out = torch.empty((total_rows, width), dtype=dtype, device=device)
    np_dtype = numpy.dtype({torch.float32: numpy.float32, torch.int64: numpy.int64}[dtype])
    cap = max(1, int(chunk_bytes) // max(1, width * np_dtype.itemsize))
    stage = numpy.empty((min(cap, max(1, total_rows)), width), np_dtype)
    cap, fill, pos = stage.shape[0], 0, 0

    def flush():
        nonlocal fill, pos
        if fill:
            out[pos: pos + fill].copy_(torch.from_numpy(stage[:fill]))        # pageable source: returns when the buffer is free again
            pos, fill = pos + fill, 0
    for a in arrays:
        a = a.reshape(len(a), width)
        done = 0
        while done < len(a):
            k = min(cap - fill, len(a) - done)
            stage[fill: fill + k] = a[done: done + k]
            fill, done = fill + k, done + k
            if fill == cap:
                flush()
    flush()
    assert pos == total_rows, (pos, total_rows)
    return out


class DeviceData(object):
    """DeviceData(data, device="cuda:0", lib=None, parts=None, chunk_bytes=256 << 20): `data` (a `Data`) with the parts named in
    `parts` (default: all of them) resident on `device`, uploaded in chunks of at most `chunk_bytes`.  Same surface as `Data`;
    `get_stream(part, batches=True)` yields the same dictionaries in the same order with DEVICE tensors as values.  A part that was
    not uploaded streams from the host `Data`."""
    def __init__(self, data, device="cuda:0", lib=None, parts=None, chunk_bytes=256 << 20):
        self.data = data
        self.device = torch.device(device)
        self._lib = lib
        self.chunk_bytes = int(chunk_bytes)
        self._stores = {}
        for part in (list(data.datasets) if parts is None else parts):
            self._upload(part)

    @property
    def lib(self):
        """The native library (the product build unless one was given): needed to upload and to assemble, not to plan."""
        if self._lib is None:
            self._lib = native.get()
        return self._lib

    # ---- the surface of Data -------------------------------------------------------------------------
    datasets = property(lambda self: self.data.datasets)
    batch_size = property(lambda self: self.data.batch_size)
    validation_batch_size = property(lambda self: self.data.validation_batch_size)
    info_dataset = property(lambda self: self.data.info_dataset)
    num_labels = property(lambda self: self.data.num_labels)
    eos_label = property(lambda self: self.data.eos_label)
    bos_label = property(lambda self: self.data.bos_label)

    def num_features(self):
        return self.data.num_features()

    def nbytes(self, part):
        """Device memory the part occupies (frames, labels, the two offset tables)."""
        st = self._stores[part]
        assert self.uploaded(part), "part %r is not on the device" % part
        return sum(int(t.numel()) * t.element_size() for t in (st.frames, st.labels, st.frame_off, st.label_off))

    def dataset_index(self, part):
        """(n,) int64: store slot -> index of the utterance in `datasets[part]` (`max_length` drops utterances from the store)."""
        return self._store(part).index_of

    def uploaded(self, part):
        return part in self._stores and self._stores[part].frames is not None

    # ---- construction --------------------------------------------------------------------------------
    def _store(self, part):
        """Host side of a part's store (slot map, lengths, the planner's stand-ins); made on first use, needs no device."""
        st = self._stores.get(part)
        if st is not None:
            return st
        data, ds, st = self.data, self.data.datasets[part], _Store()
        kept, frame_len, label_len = [], [], []
        for i in range(ds.num_examples):
            for rec, lab in data._examples(ds, [i]):           # EOS / BOS and the length filter exactly as the host stream applies them
                kept.append(i)
                frame_len.append(len(rec))
                label_len.append(len(lab))
        if not kept:
            raise ValueError("part %r: no utterance passes max_length = %r" % (part, data.max_length))
        st.n, st.F = len(kept), ds.dim()
        st.index_of = numpy.asarray(kept, numpy.int64)
        st.slot_of = numpy.full(ds.num_examples, -1, numpy.int64)
        st.slot_of[st.index_of] = numpy.arange(st.n)
        st.frame_len, st.label_len = numpy.asarray(frame_len, numpy.int64), numpy.asarray(label_len, numpy.int64)
        st.refs = []
        for slot, t in enumerate(frame_len):
            ref = numpy.empty((t, 0), numpy.float32).view(_Ref)
            ref.slot = slot
            st.refs.append(ref)
        stubs = {l: numpy.zeros(l, numpy.int64) for l in set(label_len)}
        st.label_stubs = [stubs[l] for l in label_len]
        self._stores[part] = st
        return st

    def _upload(self, part):
        if self.device.type != "cuda" and not self.lib.is_emulator:
            raise native.NativeError("DeviceData keeps the dataset on an MI355X (cuda:N) device; no CPU fallback")
        data, st = self.data, self._store(part)
        labels = []

        def frames():
            # the VALUES come from the host stream itself: EOS / BOS, the filter, `(r - mean) / std` in the statistics' dtype and the
            # cast to float32 are its expressions, so the uploaded bits are those the host path pads into its minibatches
            count = 0
            for rec, lab in data.get_stream(part, batches=False, shuffle=False):
                assert rec.dtype == numpy.float32 and len(rec) == st.frame_len[count] and len(lab) == st.label_len[count]
                labels.append(numpy.asarray(lab, numpy.int64))
                count += 1
                yield rec
            assert count == st.n, "host stream and slot map disagree"
        st.frames = _upload_rows(frames(), int(st.frame_len.sum()), st.F, torch.float32, self.device, self.chunk_bytes)
        st.labels = _upload_rows(labels, int(st.label_len.sum()), 1, torch.int64, self.device, self.chunk_bytes).reshape(-1)
        for name, lens in (("frame_off", st.frame_len), ("label_off", st.label_len)):
            off = numpy.zeros(st.n + 1, numpy.int64)
            numpy.cumsum(lens, out=off[1:])
            setattr(st, name, _upload_rows([off], st.n + 1, 1, torch.int64, self.device, self.chunk_bytes).reshape(-1))

    # ---- the epoch plan (host only) ------------------------------------------------------------------------
    @staticmethod
    def _plan_batch(examples, *args, **kwargs):
        """Takes Data.pad_batch's place in Data._batches: the padded lengths are those the real pad_batch gives the stand-ins."""
        shaped = Data.pad_batch(examples, *args, **kwargs)
        return dict(index=numpy.asarray([r.slot for r, _ in examples], numpy.int64), T=int(shaped["recordings"].shape[0]),
                    L=int(shaped["labels"].shape[0]))

    def plan(self, part, shuffle=True, seed=None, rng=None, num_examples=None, rank=0, world=1):
        """The epoch `Data.get_stream(part, ...)` would produce, as a list of (store indices (B,) int64, T, L, global_batch_size or
        None): same permutation, same filter-then-sort-k chunks (Python's stable sort on the length), same batch sizes and trailing
        rules, padded lengths including pad_frames_to / pad_labels_to; under data parallelism the lengths of the GLOBAL minibatch
        with the columns rank::world.  (A global minibatch smaller than the world, for which the host stream yields None, has no
        entry.)"""
        data, st = self.data, self._store(part)
        n = data.datasets[part].num_examples if num_examples is None else num_examples
        order = numpy.arange(n)
        if shuffle:
            rng = rng if rng is not None else numpy.random.RandomState(seed)
            order = rng.permutation(n)
        stream = ((st.refs[s], st.label_stubs[s]) for s in st.slot_of[order] if s >= 0)
        if data.sort_k_batches:
            stream = data._sort_k(stream, data.batch_size * data.sort_k_batches)
        bs = data.batch_size if part == "train" else data.validation_batch_size
        # Data's own batching generator with pad_batch swapped for the planner's: same grouping, same trailing-batch rules
        planner = copy.copy(data)
        planner.pad_batch = self._plan_batch
        return [(b["index"], b["T"], b["L"], b.get("global_batch_size"))
                for b in planner._batches(stream, bs, rank, world) if b is not None]

    # ---- assembly ------------------------------------------------------------------------------------------
    def _check(self, st, index, T, L):
        index = numpy.asarray(index, numpy.int64).reshape(-1)
        if index.size == 0:
            raise ValueError("empty minibatch")
        if index.min() < 0 or index.max() >= st.n:
            raise ValueError("utterance index outside the store [0, %d): %s" % (st.n, index[(index < 0) | (index >= st.n)].tolist()))
        if st.frame_len[index].max() > T or st.label_len[index].max() > L:
            raise ValueError("padded lengths (T %d, L %d) are smaller than a selected utterance (%d frames, %d labels)"
                             % (T, L, st.frame_len[index].max(), st.label_len[index].max()))
        return index

    def _launch(self, st, table, first, B, T, L):
        """One lvsr_assemble_batch launch on the device's current stream; columns = table[first: first + B] (device int64)."""
        dev = self.device
        out = dict(recordings=torch.empty((T, B, st.F), dtype=torch.float32, device=dev),
                   recordings_mask=torch.empty((T, B), dtype=torch.float32, device=dev),
                   labels=torch.empty((L, B), dtype=torch.int64, device=dev),
                   labels_mask=torch.empty((L, B), dtype=torch.float32, device=dev))
        args = self.lib.make("lvsr_batch_args", frames=st.frames, frame_off=st.frame_off, labels=st.labels, label_off=st.label_off,
                             index=table.data_ptr() + 8 * first, n=st.n, B=B, T=T, L=L, F=st.F, recordings=out["recordings"],
                             recordings_mask=out["recordings_mask"], out_labels=out["labels"], labels_mask=out["labels_mask"])
        self.lib.call("lvsr_assemble_batch", self.lib.stream_for(out["recordings"]), ctypes.byref(args))
        return out

    def assemble(self, part, index, T, L):
        """One minibatch of the utterances `index` (store slots, host integers) padded to (T, L).  ValueError, before anything is
        launched, for an index outside the store or a T / L smaller than a selected utterance."""
        if not self.uploaded(part):
            raise KeyError("part %r is not on the device" % (part,))
        st = self._stores[part]
        index = self._check(st, index, int(T), int(L))
        table = torch.from_numpy(index).to(self.device)
        return self._launch(st, table, 0, len(index), int(T), int(L))

    def get_stream(self, part, batches=True, shuffle=True, num_examples=None, rng=None, seed=None, rank=0, world=1):
        """`Data.get_stream` with the minibatches built on the device: the epoch is planned on the host, its index table is uploaded
        once, and every dictionary (keys, key order and shapes of the host path) is filled by one launch — no host-to-device copy per
        step.  Every batch owns its tensors: it stays valid after the next one is requested."""
        if not batches or not self.uploaded(part):
            return self.data.get_stream(part, batches=batches, shuffle=shuffle, num_examples=num_examples, rng=rng, seed=seed,
                                        rank=rank, world=world)
        st = self._stores[part]
        entries = self.plan(part, shuffle=shuffle, seed=seed, rng=rng, num_examples=num_examples, rank=rank, world=world)
        return self._assembled(st, entries, world)

    def _assembled(self, st, entries, world):
        if not entries:
            return
        for index, T, L, _ in entries:
            self._check(st, index, T, L)
        table = torch.from_numpy(numpy.concatenate([e[0] for e in entries])).to(self.device)
        first = 0
        for index, T, L, gbs in entries:
            batch = self._launch(st, table, first, len(index), T, L)
            first += len(index)
            if world > 1:
                batch["global_batch_size"] = gbs
            yield batch
