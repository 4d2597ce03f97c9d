"""Host-side mirror of `lvsr.bricks.recognizer.SpeechRecognizer` (lvsr/bricks/recognizer.py:159-562): same
constructor keywords (the `net:` section of the reference's YAML), same method names
(`cost`, `analyze`, `init_beam_search`, `beam_search`, `load_params`), parameters under the reference's
Blocks names — with every tensor operation executed by the HIP library on an MI355X.

What Theano derived symbolically is explicit here: `cost(...)` is the forward pass (cost matrix (L,B)),
`backward()` the gradient of `cost.sum()` wrt all parameters (lvsr/main.py:340-345 divides by the batch
size afterwards; `cost_and_gradients` does the same).
"""
import contextlib
import logging
import os

import numpy
import torch

from .. import spec
from ..params import ParameterStore, Workspace
from . import Encoder, SpeechBottom
from .generator import SequenceGenerator

logger = logging.getLogger(__name__)


class SpeechRecognizer(object):
    def __init__(self, device="cuda:0", params=None, lib=None, use_graph=True, use_persistent=None, net_config=None,
                 use_persistent_decoder=None, **net_kwargs):
        """`net_kwargs` = the reference's constructor keywords (recognizer.py:176-204), or pass an
        already-normalised `net_config` (lvsr_amd.spec).  `params` = dict name -> ndarray (Blocks names).
        `use_persistent` / `use_persistent_decoder`: force (True) or forbid (False) the persistent cluster kernels of the
        encoder / of the decoder's teacher-forced label loop; None = use them where they are available and faster."""
        from .. import native
        lm_config = dict(net_kwargs.get("lm") or {})
        cfg = net_config if net_config is not None else spec.from_reference_kwargs(**net_kwargs)
        self.d = spec.Dims(cfg)
        self.cfg = self.d.cfg
        self.device = torch.device(device)
        self.lib = lib if lib is not None else native.get()
        if self.device.type != "cuda" and not self.lib.is_emulator:
            raise native.NativeError("SpeechRecognizer runs on an MI355X (cuda:N) device only; no CPU fallback")
        self.eos_label = self.cfg["eos_label"]
        self.data_prepend_eos = self.cfg["data_prepend_eos"]
        self.max_decoded_length_scale = self.cfg["max_decoded_length_scale"]
        self.store = ParameterStore(cfg, self.device, params)
        self.ws = Workspace(self.device)
        self.use_graph = bool(use_graph) and self.device.type == "cuda"
        self.bottom = SpeechBottom(self.d, self.store, self.lib, self.ws)
        self.encoder = Encoder(self.d, self.store, self.lib, self.ws, use_graph=self.use_graph, use_persistent=use_persistent)
        if self.d.n_dec > 1:         # RecurrentStack decoder (recognizer.py:250-262)
            from .generator_stack import StackedSequenceGenerator as generator_class
        else:
            generator_class = SequenceGenerator
        self.generator = generator_class(self.d, self.store, self.lib, self.ws, use_graph=self.use_graph,
                                         use_persistent=use_persistent_decoder)
        # hipGraph capture cannot run on the legacy null stream: the hot path owns a side stream
        self.stream = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None
        self.beam_size = None
        # adaptive weight noise: log-variances found in a loaded checkpoint (parameter name -> array), set aside for a noisy trainer,
        # and the noise state of the trainer attached now (its log-variances go into save_params), lvsr_amd/weight_noise.py
        self.noise_values = {}
        self.weight_noise = None
        if lm_config.get("path"):                                  # recognizer.py:322-337
            from ..lm import language_model_from_config
            self.set_language_model(language_model_from_config(lm_config, net_kwargs.get("character_map"), self.device,
                                                               self.lib))

    # ---- plumbing ----------------------------------------------------------------------------------
    @contextlib.contextmanager
    def _on_stream(self):
        if self.stream is None:
            yield
            return
        cur = torch.cuda.current_stream(self.device)
        if cur == self.stream:                                      # re-entrant
            yield
            return
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            yield
        cur.wait_stream(self.stream)

    def _t(self, x, dtype, name):
        if x is None:
            return None
        if not torch.is_tensor(x):
            x = torch.from_numpy(numpy.ascontiguousarray(x))
        x = x.to(dtype)
        buf = self.ws.get("in." + name, tuple(x.shape), dtype)
        buf.copy_(x, non_blocking=True)
        return buf

    def get_parameter_values(self):
        return self.store.get_values()

    def set_parameter_values(self, values):
        self.store.set_values(values)

    def load_params(self, path):
        """recognizer.py:408-412: load a Blocks checkpoint (tar with `_parameters`) or an .npz by parameter name.  The log-variances
        of adaptive noise (`/adaptive_noise.*`, lvsr/main.py:462-470) are set aside in `noise_values` for a noisy trainer; without
        one they are ignored, as Blocks' Model.set_parameter_values logs and skips unknown names (libs/blocks/blocks/model.py:137-141)."""
        from ..checkpoint import load_parameters
        from ..weight_noise import is_noise_name, param_name
        values, noise = {}, {}
        for k, v in load_parameters(path).items():
            if not is_noise_name(k):
                values[k] = v
                continue
            p = param_name(k)
            if p not in self.store.shapes or tuple(numpy.shape(v)) != tuple(self.store.shapes[p]):
                raise ValueError("%s does not match a parameter of this recognizer (shape %s)" % (k, numpy.shape(v)))
            noise[p] = numpy.asarray(v, numpy.float32)
        self.store.set_values(values)
        self.noise_values = noise
        if noise:
            logger.info("%s: %d adaptive-noise log-variances set aside (used by a trainer with adaptive noise)", path, len(noise))

    def save_params(self, path, extra=None):
        """Blocks-style checkpoint of the parameters; while a trainer with adaptive noise is attached, the current log-variances
        too, under the reference's names (lvsr_amd/weight_noise.py)."""
        from ..checkpoint import save_parameters
        values = self.store.get_values()
        if self.weight_noise is not None:
            values.update(self.weight_noise.ls2_values())
        save_parameters(path, values, extra=extra)

    def initialize(self, initialization, seed=1):
        """Apply the reference's `initialization:` config section (lvsr/main.py:225-232): brick paths mapped to
        {weights_init, biases_init, rec_weights_init, initial_states_init}, applied shallow-to-deep; recurrent weights
        follow GatedRecurrent._initialize (libs/blocks/blocks/bricks/recurrent.py:567-580: state_to_gates =
        hstack[init, init]).  The RNG stream is numpy.random.RandomState(seed) per parameter name — it does NOT
        reproduce Blocks' per-brick seeding (parity tests always load explicit parameter values)."""
        import zlib
        chosen = {}
        for path in sorted(initialization, key=lambda s: s.count("/")):
            for name in self.store.shapes:
                if name.startswith(path.rstrip("/") + "/") or name == path:
                    chosen.setdefault(name, {}).update(initialization[path])
        values = {}
        for name, shape in self.store.shapes.items():
            conf = chosen.get(name, {})
            rng = numpy.random.RandomState((zlib.crc32(name.encode()) + seed) % (2 ** 31))
            leaf = name.rsplit("/", 1)[-1]
            rec = conf.get("rec_weights_init", conf.get("weights_init"))
            if leaf.endswith("state_to_state") and rec is not None:
                v = rec.generate(rng, shape)
            elif leaf.endswith("state_to_gates") and rec is not None:
                H = shape[0]
                v = numpy.hstack([rec.generate(rng, (H, H)), rec.generate(rng, (H, H))])
            elif leaf.endswith("initial_state"):
                init = conf.get("initial_states_init")
                v = init.generate(rng, shape) if init is not None else numpy.zeros(shape, numpy.float32)
            elif leaf.endswith(".b"):
                init = conf.get("biases_init")
                v = init.generate(rng, shape) if init is not None else numpy.zeros(shape, numpy.float32)
            else:
                init = conf.get("weights_init")
                if init is None:
                    raise ValueError("no weights_init configured for %s" % name)
                v = init.generate(rng, shape)
            values[name] = numpy.asarray(v, numpy.float32)
        self.store.set_values(values)

    # ---- training cost (recognizer.py:375-390) -------------------------------------------------------
    def cost(self, recordings=None, inputs_mask=None, labels=None, labels_mask=None, save_for_backward=True, prediction=None,
             prediction_mask=None, **kw):
        """-> cost matrix (L,B) on the device.  `recordings` (T,B,F), `inputs_mask` (T,B) or None,
        `labels` (L,B) int64, `labels_mask` (L,B) or None.
        `prediction` (Lp,B) int64 / `prediction_mask` (get_cost_graph, recognizer.py:423-450): the prediction drives the decoder and
        is what the cost is taken on -> (Lp,B); the labels are the groundtruth its rewards are measured against (mse criteria)."""
        if "recordings_mask" in kw:
            inputs_mask = kw.pop("recordings_mask")
        if kw:
            raise TypeError("unknown inputs: %s" % sorted(kw))
        with self._on_stream():
            x, xm, y, ym = self._stage(recordings, inputs_mask, labels, labels_mask)
            if prediction is None:
                return self._forward(x, xm, y, ym, save_for_backward)
            pr, pm = self._t(prediction, torch.int64, "prediction"), self._t(prediction_mask, torch.float32, "prediction_mask")
            return self._forward(x, xm, pr, pm, save_for_backward, groundtruth=y)

    def _stage(self, recordings, inputs_mask, labels, labels_mask):
        return (self._t(recordings, torch.float32, "recordings"), self._t(inputs_mask, torch.float32, "recordings_mask"),
                self._t(labels, torch.int64, "labels"), self._t(labels_mask, torch.float32, "labels_mask"))

    def _forward(self, x, xm, y, ym, save_for_backward=True, groundtruth=None):
        self.bottom_output = self.bottom.apply(x, save_for_backward)
        encoded, encoded_mask = self.encoder.apply(self.bottom_output, xm, save_for_backward=save_for_backward)
        self.encoded, self.encoded_mask = encoded, encoded_mask
        self.cost_mask = ym          # the mask the cost matrix is taken under (lvsr_amd/observables.py)
        return self.generator.cost_matrix(y, ym, attended=encoded, attended_mask=encoded_mask,
                                          save_for_backward=save_for_backward, groundtruth=groundtruth)

    LENGTH_EXPAND = 10          # greedy exploration generates this many labels more than the groundtruth has (lvsr/main.py:251)

    def _forward_greedy(self, x, xm, y):
        """The forward pass of a training step with greedy exploration (add_exploration, lvsr/main.py:245-283): encode once, let the
        argmax emitter generate L + 10 labels, measure them against the groundtruth `y` (reward / gain matrices and the mask of the
        prediction up to its first EOS, on the device), then the teacher-forced pass on the prediction.  No host synchronisation.
        -> cost matrix (L + 10, B)."""
        gen = self.generator
        self.bottom_output = self.bottom.apply(x, True)
        encoded, encoded_mask = self.encoder.apply(self.bottom_output, xm, save_for_backward=True)
        self.encoded, self.encoded_mask = encoded, encoded_mask
        prediction = gen.generate(n_steps=int(y.shape[0]) + self.LENGTH_EXPAND, attended=encoded, attended_mask=encoded_mask)["outputs"]
        rw = gen.reward_matrices(y, prediction, want_mask=True)
        self.prediction, self.prediction_mask = prediction, rw["mask"]
        self.cost_mask = rw["mask"]
        return gen.cost_matrix(prediction, rw["mask"], attended=encoded, attended_mask=encoded_mask, rewards=rw)

    # ---- free-running generation (recognizer.py:393-406, 535-547) ------------------------------------------------------
    def generate(self, n_steps=None, inputs_mask=None, recordings=None, uniforms=None, seed=None, **kw):
        """SpeechRecognizer.generate: encoder, then SequenceGenerator.generate for `n_steps` steps on the whole batch.
        -> dict(states, outputs, weighted_averages, weights, energies, costs) of device tensors, time-major."""
        if "recordings_mask" in kw:
            inputs_mask = kw.pop("recordings_mask")
        if kw:
            raise TypeError("unknown inputs: %s" % sorted(kw))
        with self._on_stream():
            x = self._t(recordings, torch.float32, "recordings")
            xm = self._t(inputs_mask, torch.float32, "recordings_mask")
            encoded, encoded_mask = self.encoder.apply(self.bottom.apply(x, False), xm, save_for_backward=False)
            return self.generator.generate(n_steps=n_steps, batch_size=int(encoded.shape[1]), attended=encoded,
                                           attended_mask=encoded_mask, uniforms=uniforms, seed=seed)

    def sample(self, inputs, n_steps=None, uniforms=None, seed=None):
        """SpeechRecognizer.sample (recognizer.py:540-547): one utterance, no input mask, n_steps defaults to
        frames / max_decoded_length_scale; -> the sampled label sequence (n_steps, 1) as a numpy array."""
        x = numpy.asarray(dict(inputs)["recordings"], dtype=numpy.float32)
        if n_steps is None:
            n_steps = int(x.shape[0] / self.max_decoded_length_scale)
        out = self.generate(n_steps=n_steps, inputs_mask=None, recordings=x[:, None, :],
                            uniforms=None if uniforms is None else numpy.asarray(uniforms, numpy.float32).reshape(n_steps, 1), seed=seed)
        return out["outputs"].cpu().numpy()

    def backward(self):
        """Gradient of cost.sum() wrt all parameters -> self.store.grad (flat) / self.store.g (named views)."""
        with self._on_stream():
            # the small weight-gradient products of decoder and encoder (recurrent matrices, readout, ...) are collected in one
            # group and run as ONE grouped launch at the end: alone none of them fills the chip
            group = self.lib.group()
            d_encoded = self.generator.backward(group)
            self._backward_encoder(d_encoded, group)

    def _backward_decoder(self):
        """The decoder's half of backward() with a grouped launch of its own: afterwards every gradient under
        /recognizer/generator is final (the tail of the flat gradient buffer, `decoder_bucket()`).  -> d_encoded."""
        with self._on_stream():
            group = self.lib.group()
            d_encoded = self.generator.backward(group)
            group.flush(self.ws.get("gemm_ws.grouped", (1 << 26,)))
            return d_encoded

    def _backward_encoder(self, d_encoded, group=None):
        """Encoder (and bottom) half of backward(): adds the encoder's products to `group` (the decoder's, from backward(); a fresh
        one otherwise) and flushes it."""
        with self._on_stream():
            if group is None:
                group = self.lib.group()
            d_bottom = self.encoder.backward(d_encoded, need_input_grad=bool(self.d.bottom_dims), group=group)
            group.flush(self.ws.get("gemm_ws.grouped", (1 << 26,)))
            self.encoder.finish_backward()
            if self.d.bottom_dims:
                self.bottom.backward(d_bottom)

    def decoder_bucket(self):
        """(offset, count) of the decoder's gradients in the flat buffers: the parameters under /recognizer/generator are laid out
        behind everything else (spec.parameter_shapes), so they form one contiguous tail."""
        offs = self.store.offsets
        first = min(o for k, (o, n) in offs.items() if k.startswith("/recognizer/generator"))
        assert all(k.startswith("/recognizer/generator") == (o >= first) for k, (o, n) in offs.items()), "decoder parameters are not a tail"
        return first, self.store.flat.numel() - first

    def cost_and_gradients(self, batch, tail=None, tail_key=None, region=True, between=None, head=None, exploration=None,
                           after_forward=None):
        """One training forward+backward on a batch dict in the reference's layout.
        Returns the cost matrix (L,B) on the device; gradients of its sum are in self.store.grad.
        `tail` (optional callable, described by the hashable `tail_key`) enqueues more work behind the backward pass — the
        optimiser step — inside the same graph region: the whole step is then ONE hipGraph launch per minibatch shape.
        `between` (optional callable, data parallelism with overlapped exchange): called — eagerly, outside any graph region — when
        the decoder's gradients are final and before the encoder's backward pass is enqueued; the step is then TWO graph regions
        (forward + decoder backward | encoder backward [+ tail]).
        `head` (optional callable, described by `tail_key` as well) enqueues work in front of the forward pass inside the (first)
        graph region: the noisy weights of adaptive noise.
        `after_forward` (optional callable, described by `tail_key` as well) enqueues work right behind the forward pass, inside the
        graph region that holds the forward pass: it may use what the forward pass left on this object (`encoded`, `cost_mask`,
        `generator.last`, ...), which a later replay of the region does not refresh — the training observables.
        `exploration`: None / "imitative" = the decoder is driven by the labels; "greedy" (mse criteria, `training.exploration` of the
        reference, lvsr/main.py:245-283) = by its own argmax prediction of L + 10 labels, generated inside the same graph region
        (`_forward_greedy`); the cost matrix is then (L + 10, B)."""
        if exploration not in (None, "imitative", "greedy"):
            raise ValueError("unknown exploration %r" % (exploration,))
        greedy = exploration == "greedy"
        if greedy and not self.generator.mse:
            raise NotImplementedError("greedy exploration needs an mse criterion (the softmax emitter samples; not built for training)")
        if greedy and between is not None:
            raise NotImplementedError("greedy exploration with an overlapped gradient exchange is not built")
        with self._on_stream():
            x, xm, y, ym = self._stage(batch["recordings"], batch.get("recordings_mask"), batch["labels"],
                                       batch.get("labels_mask"))
            shape_key = (tuple(x.shape), tuple(y.shape), xm is None, ym is None)
            volatile = (x.data_ptr(), y.data_ptr(), 0 if xm is None else xm.data_ptr(), 0 if ym is None else ym.data_ptr(),
                        self.ws.generation, self.store.flat.data_ptr(), self.store.grad.data_ptr())
            plain = region and self.use_graph and not self.encoder.overlap
            if between is not None:
                def first_half():
                    if head is not None:
                        head()
                    cm = self._forward(x, xm, y, ym)
                    if after_forward is not None:
                        after_forward()
                    return cm, self._backward_decoder()

                key1 = ("train_step_fwd_dec",) + shape_key + ((tail_key,) if head is not None or after_forward is not None else ())
                cm, d_encoded = self.lib.region(self, key1, x, enabled=plain, volatile=volatile).run(first_half)
                between()

                def second_half():
                    self._backward_encoder(d_encoded)
                    if tail is not None:
                        tail()
                    return True
                vol2 = volatile + (d_encoded.data_ptr(), self.ws.generation)
                self.lib.region(self, ("train_step_enc",) + shape_key + (tail_key,), x, enabled=plain, volatile=vol2).run(second_half)
                return cm

            def enqueue():
                if head is not None:
                    head()
                cm = self._forward_greedy(x, xm, y) if greedy else self._forward(x, xm, y, ym)
                if after_forward is not None:
                    after_forward()
                self.backward()
                if tail is not None:
                    tail()
                return cm
            key = ("train_step",) + shape_key + (tail_key, "greedy" if greedy else "imitative")
            return self.lib.region(self, key, x, enabled=plain, volatile=volatile).run(enqueue)

    # ---- analyze (recognizer.py:452-494) -----------------------------------------------------------
    def analyze(self, inputs, groundtruth, prediction=None):
        """Single utterance: -> [cost (L,), weights (L,T'), energies (L,T')] as numpy arrays."""
        x = numpy.asarray(dict(inputs)["recordings"], dtype=numpy.float32)
        y = numpy.asarray(groundtruth if groundtruth is not None else prediction, dtype=numpy.int64)
        pr = None if prediction is None else numpy.asarray(prediction, dtype=numpy.int64)[:, None]
        cm = self.cost(recordings=x[:, None, :], inputs_mask=None, labels=y[:, None], labels_mask=None,
                       save_for_backward=False, prediction=pr)
        last = self.generator.last
        torch.cuda.synchronize() if self.device.type == "cuda" else None
        return [cm[:, 0].cpu().numpy(), last["weights"][:, 0, :].cpu().numpy(), last["energies"][:, 0, :].cpu().numpy()]

    def _pad_recordings(self, recordings, pad_to):
        """list of (T_i, F) arrays -> x (T,B,F), mask (T,B) float32, T the longest length rounded up to a multiple of `pad_to`"""
        recs = [numpy.asarray(r, dtype=numpy.float32).reshape(len(r), -1) for r in recordings]
        T = max(len(r) for r in recs)
        T = (T + pad_to - 1) // pad_to * pad_to
        x = numpy.zeros((T, len(recs), recs[0].shape[1]), numpy.float32)
        m = numpy.zeros((T, len(recs)), numpy.float32)
        for i, r in enumerate(recs):
            x[: len(r), i] = r
            m[: len(r), i] = 1.0
        return x, m

    @staticmethod
    def _pad_labels(seqs):
        """list of label sequences -> labels (L,B) int64 (padded with 0), mask (L,B) float32"""
        L = max(len(s) for s in seqs)
        y = numpy.zeros((L, len(seqs)), numpy.int64)
        m = numpy.zeros((L, len(seqs)), numpy.float32)
        for i, s in enumerate(seqs):
            y[: len(s), i] = s
            m[: len(s), i] = 1.0
        return y, m

    def analyze_batch(self, recordings, groundtruths, predictions=None, want_alignments=False, pad_to=64):
        """`analyze` for a chunk of utterances in one ragged pass, with the report's reductions on the device (lvsr/main.py:732-736,
        778-790, 816-823).  `recordings`: list of (T_i, F) arrays; `groundtruths`: list of label sequences; `predictions`: None, or a
        list of label sequences / None entries (an empty prediction counts as None: Theano's scan has no 0-length sequences,
        main.py:816-817).  Under an mse criterion every ground truth ends in EOS, as in training.
        -> one dict per utterance: groundtruth = dict(cost, weights_std, monotonicity_penalty, length), prediction = the same for the
        prediction — its cost taken against the ground truth, as analyze(inputs, groundtruth, prediction) does — or None.
        ONE encoder pass (padded as `compute_contexts_batch` pads) and one teacher-forced decoder pass per label set on the same
        contexts, the second over the utterances that have a prediction only; behind each, lvsr_utterance_stats reduces cost matrix and
        alignment to four numbers per utterance, which are all that is copied to the host — one synchronisation per call.
        `want_alignments`: each entry also carries `weights` and `energies` (L_i, T'_i), cut to the utterance's own labels and
        attended length (more copies)."""
        from ..observables import utterance_stats
        B = len(recordings)
        if B == 0:
            return []
        if len(groundtruths) != B or (predictions is not None and len(predictions) != B):
            raise ValueError("analyze_batch: %d recordings, %d groundtruths%s" % (
                B, len(groundtruths), "" if predictions is None else ", %d predictions" % len(predictions)))
        gts = [[int(t) for t in g] for g in groundtruths]
        if any(len(g) == 0 for g in gts):
            raise ValueError("analyze_batch: an empty groundtruth")
        preds = [None] * B if predictions is None else [None if p is None or len(p) == 0 else [int(t) for t in p] for p in predictions]
        cols = [i for i, p in enumerate(preds) if p is not None]
        dev, gen, ws = self.device, self.generator, self.ws
        x, xm = self._pad_recordings(recordings, pad_to)
        y, ym = self._pad_labels(gts)
        aligned = {}

        def keep(which, index, Ls):
            """the alignments of a pass, cut on the host"""
            W, E = gen.last["weights"].cpu().numpy(), gen.last["energies"].cpu().numpy()
            for j, i in enumerate(index):
                aligned[which, i] = (W[: Ls[j], j, : tp_host[i]].copy(), E[: Ls[j], j, : tp_host[i]].copy())

        with self._on_stream():
            xb, xmb = self._t(x, torch.float32, "recordings"), self._t(xm, torch.float32, "recordings_mask")
            yb, ymb = self._t(y, torch.int64, "labels"), self._t(ym, torch.float32, "labels_mask")
            encoded, encoded_mask = self.encoder.apply(self.bottom.apply(xb, False), xmb, save_for_backward=False)
            lengths = encoded_mask.sum(dim=0).to(torch.int32)
            tp_host = lengths.cpu().numpy().tolist() if want_alignments else None
            record = ws.get("analyze.record", (2, B, 4), torch.float64)
            cm = gen.cost_matrix(yb, ymb, attended=encoded, attended_mask=encoded_mask, save_for_backward=False)
            utterance_stats(self.lib, gen.last["weights"], ymb, cm, record[0], ws, lengths=lengths)
            if want_alignments:
                keep("groundtruth", range(B), [len(g) for g in gts])
            if cols:
                p, pm = self._pad_labels([preds[i] for i in cols])
                pb, pmb = self._t(p, torch.int64, "prediction"), self._t(pm, torch.float32, "prediction_mask")
                if len(cols) == B:
                    enc, encm, gtb, lens = encoded, encoded_mask, yb, lengths
                else:
                    # the columns that have a prediction, gathered: no all-masked column reaches the decoder kernels
                    idx = torch.tensor(cols, dtype=torch.int64).to(dev, non_blocking=True)
                    enc, encm = encoded.index_select(1, idx), encoded_mask.index_select(1, idx)
                    gtb, lens = yb.index_select(1, idx), lengths.index_select(0, idx)
                cm = gen.cost_matrix(pb, pmb, attended=enc, attended_mask=encm, save_for_backward=False, groundtruth=gtb)
                utterance_stats(self.lib, gen.last["weights"], pmb, cm, record[1, :len(cols)], ws, lengths=lens)
                if want_alignments:
                    keep("prediction", cols, [len(preds[i]) for i in cols])
            host = record.cpu().numpy()                       # the one synchronisation

        def entry(r):
            n = int(r[3])
            return dict(cost=float(r[0]), weights_std=float(r[1]) / n, monotonicity_penalty=float(r[2]), length=n)
        out = [dict(groundtruth=entry(host[0, i]), prediction=None) for i in range(B)]
        for j, i in enumerate(cols):
            out[i]["prediction"] = entry(host[1, j])
        for (which, i), (W, E) in aligned.items():
            out[i][which].update(weights=W, energies=E)
        return out

    # ---- alignment times (an addition: the reference shows alignments as pictures, lvsr/notebook.py:81) ----------------------------
    @staticmethod
    def _quantiles(quantiles):
        lo, hi = (float(q) for q in quantiles)
        if not 0.0 <= lo <= hi <= 1.0:
            raise ValueError("quantiles must satisfy 0 <= lo <= hi <= 1, got (%r, %r)" % (lo, hi))
        return lo, hi

    def _align_contexts(self, encoded, encoded_mask, label_seqs, quantiles):
        """The teacher-forced pass of `align_batch` / `align_staged` over contexts that are already computed: ONE
        `cost_matrix(save_for_backward=False)` over the columns that have labels (gathered, as `analyze_batch` gathers the columns that
        have a prediction: no all-masked column reaches the decoder kernels), ONE lvsr_alignment_times launch, ONE copy of L B 8
        doubles — the only synchronisation.  Runs on the caller's stream.  -> list of (L_i, 8) float64 arrays."""
        from ..observables import TIMES, alignment_times
        lo, hi = quantiles
        seqs = [[int(t) for t in s] for s in label_seqs]
        if len(seqs) != int(encoded.shape[1]):
            raise ValueError("%d label sequences for %d utterances" % (len(seqs), int(encoded.shape[1])))
        out = [numpy.zeros((0, TIMES)) for _ in seqs]
        cols = [i for i, s in enumerate(seqs) if s]
        if not cols:
            return out
        gen, ws = self.generator, self.ws
        y, ym = self._pad_labels([seqs[i] for i in cols])
        yb, ymb = self._t(y, torch.int64, "labels"), self._t(ym, torch.float32, "labels_mask")
        if len(cols) != len(seqs):
            idx = torch.tensor(cols, dtype=torch.int64).to(self.device, non_blocking=True)
            encoded, encoded_mask = encoded.index_select(1, idx), encoded_mask.index_select(1, idx)
        lengths = encoded_mask.sum(dim=0).to(torch.int32)
        cm = gen.cost_matrix(yb, ymb, attended=encoded, attended_mask=encoded_mask, save_for_backward=False)
        record = ws.get("align.times", tuple(cm.shape) + (TIMES,), torch.float64)
        alignment_times(self.lib, gen.last["weights"], ymb, cm, record, lengths=lengths, lo=lo, hi=hi)
        host = record.cpu().numpy()                           # the one synchronisation
        for j, i in enumerate(cols):
            out[i] = host[: len(seqs[i]), j].copy()
        return out

    def align_batch(self, recordings, label_seqs, pad_to=64, quantiles=(0.1, 0.9)):
        """Where on the attended axis every label of every utterance sits: `recordings` a list of (T_i, F) arrays, `label_seqs` a list
        of label sequences (ground truths for forced alignment, hypotheses for time stamps) -> a list of (L_i, 8) float64 arrays, the
        rows of lvsr_alignment_times (include/lvsr_hip.h; `observables.PEAK` .. `COST`): peak position, weight there, mean position,
        spread, the positions at which the running sum of the alignment reaches quantiles[0] and quantiles[1] of its total, the
        total, the label's cost.  Positions count attended (subsampled) frames: `decode.token_times` turns them into seconds.
        Padded as `analyze_batch` pads; ONE encoder pass, ONE teacher-forced `cost_matrix(save_for_backward=False)` pass, one
        lvsr_alignment_times launch, one copy of L B 8 doubles — the only synchronisation; nothing of the (L,B,T') alignment leaves the
        device.  An empty label sequence gives a (0,8) array (its column is gathered out in front of the decoder pass).  Under an mse
        criterion the labels are their own ground truth; with a language model attached the cost is the fused one, as in `analyze`."""
        quantiles = self._quantiles(quantiles)
        if len(recordings) == 0:
            return []
        if len(label_seqs) != len(recordings):
            raise ValueError("align_batch: %d recordings, %d label sequences" % (len(recordings), len(label_seqs)))
        x, xm = self._pad_recordings(recordings, pad_to)
        with self._on_stream():
            xb, xmb = self._t(x, torch.float32, "recordings"), self._t(xm, torch.float32, "recordings_mask")
            encoded, encoded_mask = self.encoder.apply(self.bottom.apply(xb, False), xmb, save_for_backward=False)
            return self._align_contexts(encoded, encoded_mask, label_seqs, quantiles)

    def align_staged(self, x, mask, lengths, label_seqs, quantiles=(0.1, 0.9), reuse_contexts=False):
        """`align_batch` over a batch that is already on the device (`frontend.FrontEnd.batch`): x (T,B,F), mask (T,B), `lengths` the
        frames of every utterance (host integers).  The argument checks of `compute_contexts_staged`; the features are not copied.  As
        `BeamSearch.begin_staged` does, a batch of one runs over its own frames without a mask — so what is aligned here is what a
        staged search of the same batch saw.
        `reuse_contexts`: no encoder pass; the teacher-forced pass reads the contexts that this recognizer's last
        `compute_contexts_staged` made from this very x and mask (the staged search of the chunk: `decode.recognize(timestamps=True)`)
        — refused when that call saw other tensors; that they still hold the same values is the caller's word."""
        quantiles = self._quantiles(quantiles)
        self._check_staged(x, mask, "align_staged")
        B = int(x.shape[1])
        if len(lengths) != B or len(label_seqs) != B:
            raise ValueError("align_staged: %d utterances, %d lengths, %d label sequences" % (B, len(lengths), len(label_seqs)))
        if B == 1 and 0 < int(lengths[0]) <= int(x.shape[0]):
            x, mask = x[: int(lengths[0])], None
        with self._on_stream():
            if reuse_contexts:
                if getattr(self, "_staged", None) is None or self._staged[0] != self._staged_key(x, mask):
                    raise ValueError("align_staged: reuse_contexts, but the last compute_contexts_staged call saw other tensors")
                encoded, encoded_mask = self._staged[1:]
            else:
                encoded, encoded_mask = self._encode_staged(x, mask, "align_staged")
            return self._align_contexts(encoded, encoded_mask, label_seqs, quantiles)

    # ---- decoding (recognizer.py:496-533) ------------------------------------------------------------
    def compute_contexts(self, recordings):
        """Encoder at batch 1 with NO input mask (init_beam_search builds the graph with use_mask=False,
        recognizer.py:506; Encoder.apply then returns an all-ones mask, lvsr/bricks/__init__.py:78)."""
        x = numpy.asarray(recordings, dtype=numpy.float32)
        if x.ndim == 2:
            x = x[:, None, :]
        xb = self._t(x, torch.float32, "recordings")
        encoded, encoded_mask = self.encoder.apply(self.bottom.apply(xb, False), None, save_for_backward=False)
        self.generator.init_generation(encoded, encoded_mask)

    def compute_contexts_batch(self, recordings, pad_to=64):
        """Encoder pass of several utterances at once (`recordings`: list of (T_i, F) arrays) for `BeamSearch.search_batch`: padded
        to a common length (a multiple of `pad_to` frames, so that few distinct shapes — and captured graphs — occur) under an input
        mask.  A masked recurrent step keeps its state (recurrent.py:297-300), so every utterance's contexts are those of its own
        unmasked batch-1 pass (`compute_contexts`) up to its own attended length."""
        x, m = self._pad_recordings(recordings, pad_to)
        xb, mb = self._t(x, torch.float32, "recordings"), self._t(m, torch.float32, "recordings_mask")
        encoded, encoded_mask = self.encoder.apply(self.bottom.apply(xb, False), mb, save_for_backward=False)
        self.generator.init_generation(encoded, encoded_mask)

    def beam_search_batch(self, recordings, **kwargs):
        """`beam_search` for a list of utterances in one set of launches -> list of (outputs, costs) or of the exception the
        single search would have raised (CandidateNotFoundError, ...)."""
        self.init_beam_search(self.beam_size)
        recs = [numpy.asarray(r, dtype=numpy.float32) for r in recordings]
        limits = [int(r.shape[0] / self.max_decoded_length_scale) for r in recs]
        results = self._beam_search.search_batch(recs, self.eos_label, limits, ignore_first_eol=self.data_prepend_eos, **kwargs)
        return [r if isinstance(r, Exception) else ([[int(t) for t in o] for o in r[0]], [float(c) for c in r[1]]) for r in results]

    def compute_contexts_staged(self, x, mask):
        """The encoder pass of `compute_contexts_batch` over a batch that is already on the device (`frontend.FrontEnd.batch`):
        x (T,B,F) float32, mask (T,B) float32 — or None: no input mask, as `compute_contexts` runs a single utterance.  No copy: the
        tensors are read where they are, so they must keep their values until the searches that use the contexts have begun."""
        encoded, encoded_mask = self._encode_staged(x, mask, "compute_contexts_staged")
        # what `align_staged(reuse_contexts=True)` teacher-forces over: the contexts, and which tensors they were made from
        self._staged = (self._staged_key(x, mask), encoded, encoded_mask)
        self.generator.init_generation(encoded, encoded_mask)

    @staticmethod
    def _staged_key(x, mask):
        return (x.data_ptr(), tuple(x.shape), None if mask is None else (mask.data_ptr(), tuple(mask.shape)))

    def _encode_staged(self, x, mask, where):
        """The argument checks and the encoder pass of the staged entry points -> (encoded, encoded_mask)."""
        self._check_staged(x, mask, where)
        return self.encoder.apply(self.bottom.apply(x, False), mask, save_for_backward=False)

    def _check_staged(self, x, mask, where):
        tensors = [("x", x, 3)] + ([("mask", mask, 2)] if mask is not None else [])
        for name, t, nd in tensors:
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != nd or not t.is_contiguous():
                raise ValueError("%s: %s must be a contiguous float32 tensor of %d dimensions" % (where, name, nd))
            if t.device.type != self.device.type or (self.device.index is not None and t.device.index != self.device.index):
                raise ValueError("%s: %s lives on %s, the recognizer on %s" % (where, name, t.device, self.device))
        if int(x.shape[2]) != self.d.F:
            raise ValueError("%s: %d features per frame, the recognizer takes %d" % (where, x.shape[2], self.d.F))
        if mask is not None and tuple(mask.shape) != tuple(x.shape[:2]):
            raise ValueError("%s: mask %s for recordings %s" % (where, tuple(mask.shape), tuple(x.shape)))

    def beam_search_staged(self, x, mask, lengths, **kwargs):
        """`beam_search_batch` for a batch staged on the device: x (T,B,F), mask (T,B), `lengths` the frames of every utterance (a
        host sequence: the length limits are int(lengths[i] / max_decoded_length_scale), as for host recordings).  -> the same list of
        (outputs, costs) or exceptions.  A host-side language model or a validator is refused (BeamSearch.search_staged)."""
        self.init_beam_search(self.beam_size)
        lengths = [int(n) for n in lengths]
        limits = [int(n / self.max_decoded_length_scale) for n in lengths]
        results = self._beam_search.search_staged(x, mask, limits, self.eos_label, lengths=lengths, ignore_first_eol=self.data_prepend_eos,
                                                  **kwargs)
        return [r if isinstance(r, Exception) else ([[int(t) for t in o] for o in r[0]], [float(c) for c in r[1]]) for r in results]

    def init_beam_search(self, beam_size):
        from ..search import BeamSearch
        if getattr(self, "_beam_search", None) is not None and self.beam_size == beam_size:
            return
        self.beam_size = beam_size
        self._beam_search = BeamSearch(beam_size, self)

    def beam_search(self, inputs, **kwargs):
        """-> (outputs: list of label lists, costs: list of floats), best first."""
        self.init_beam_search(self.beam_size)
        inputs = dict(inputs)
        rec = numpy.asarray(inputs.pop("recordings"), dtype=numpy.float32)
        if inputs:
            raise Exception("Unknown inputs passed to beam search: {}".format(inputs.keys()))     # recognizer.py:525-528
        max_length = int(rec.shape[0] / self.max_decoded_length_scale)                             # :519-520
        outputs, search_costs = self._beam_search.search(
            {"recordings": rec[:, None, :]}, self.eos_label, max_length, ignore_first_eol=self.data_prepend_eos, **kwargs)
        return [[int(t) for t in o] for o in outputs], [float(c) for c in search_costs]

    def set_language_model(self, language_model):
        """Attach (or detach with None) an `lvsr_amd.lm.FSTLanguageModel` for shallow-fusion decoding — the `lm:`
        sub-section of the reference's net config (recognizer.py:322-343)."""
        if language_model is not None and self.generator.mse:
            raise NotImplementedError("criterion %s with a language model is not built" % self.generator.criterion)
        if language_model is not None and language_model.out_dim != self.d.V:
            raise ValueError("language model covers %d characters, the recognizer %d" % (language_model.out_dim, self.d.V))
        self.generator.language_model = language_model

    def lm_initial_states(self, n):
        return self.generator.language_model.initial_states(n)
