"""Host-side mirror of the attention sequence generator: Blocks `SequenceGenerator`
(libs/blocks/blocks/bricks/sequence_generators.py:910-949) with `AttentionRecurrent` transition
(libs/blocks/blocks/bricks/attention.py:479-772), the lvsr attention bricks (lvsr/bricks/attention.py:42-237),
`Readout` + post-merge (sequence_generators.py:531-707, lvsr/bricks/recognizer.py:298-320) and
`SoftmaxEmitter` (:751-800), as wired by `SpeechRecognizer.__init__` (lvsr/bricks/recognizer.py:250-343).

`cost_matrix(outputs, mask, attended=, attended_mask=)` keeps the reference signature
(sequence_generators.py:317-326); `backward()` is the counterpart of theano.grad through it.  With the mse_gain / mse_reward
criteria the emitter is `RewardRegressionEmitter` (lvsr/bricks/__init__.py:119-202): `outputs` is then the prediction that drives
the decoder and `groundtruth=` what its rewards are measured against.  All arithmetic
is in the C-ABI library; torch only owns buffers/views.
"""
import ctypes

import numpy
import torch

from ..native import ptr
from .beam_state import BeamState

ACT_KIND = {"identity": 0, "maxout2": 1, "rectifier": 2, "tanh": 3}
NORMALIZER_KIND = {"softmax": 0, "logistic": 1, "relu": 2}
PRIOR_KIND = {"expanding": 0, "window_around_mean": 1, "window_around_median": 2}
ATT_MS = 32     # match-dim slice per work-group in the energy kernels (csrc/decoder.h)


def _f32(x):
    return float(numpy.float32(x))


class SequenceGenerator(object):
    language_model = None
    current_search = None        # the BeamState of the search set begun last (`beam_begin`)

    def __init__(self, dims, store, lib, workspace, use_graph=True, use_persistent=None):
        self.d = dims
        self.store = store
        self.lib = lib
        self.ws = workspace
        self.use_graph = use_graph
        self.use_persistent = use_persistent      # None: auto (persistent label loop and reverse walk when available), True / False: forced on / off
        self.use_persistent_bwd = None            # None: follows use_persistent; False: step kernels for the reverse walk only (probes)
        self._packs = None
        self._pack_cache = {}
        self._saved = None
        # the emitter (recognizer.py:285-297): SoftmaxEmitter, or RewardRegressionEmitter for the mse_gain / mse_reward criteria
        self.criterion = dims.cfg["criterion"]
        self.mse = self.criterion != "log_likelihood"
        self.min_reward = float(dims.cfg["min_reward"])
        g = "/recognizer/generator"
        att = g + "/att_trans/" + ("conv_att" if dims.conv else "cont_att")
        self.n = dict(
            Wpre=att + "/preprocess.W", bpre=att + "/preprocess.b", Ws=att + "/state_trans/transform_states.W",
            we=att + "/energy_comp/linear.W", eb=att + "/energy_comp/linear.b", filters=att + "/conv1d.filters", handler=att + "/handler.W",
            Wdi=g + "/att_trans/distribute/fork_inputs.W", Wdg=g + "/att_trans/distribute/fork_gate_inputs.W",
            Whh=g + "/att_trans/transition.state_to_state", Whg=g + "/att_trans/transition.state_to_gates",
            h0=g + "/att_trans/transition.initial_state",
            Wfi=g + "/fork/fork_inputs.W", bfi=g + "/fork/fork_inputs.b",
            Wfg=g + "/fork/fork_gate_inputs.W", bfg=g + "/fork/fork_gate_inputs.b",
            Wms=g + "/readout/merge/transform_states.W", Wmw=g + "/readout/merge/transform_weighted_averages.W",
            bpm=g + "/readout/post_merge/bias.b", Wout=g + "/readout/post_merge/mlp/linear_%d.W" % len(dims.pm_hidden),
            bout=g + "/readout/post_merge/mlp/linear_%d.b" % len(dims.pm_hidden), bro=g + "/readout/bias.b",
            table=g + "/readout/lookupfeedback/lookuptable.W")
        # further post-merge layers (recognizer.py:309-317): linear_0 .. linear_{n-2} with the activation behind each
        self.pm_hidden = [(g + "/readout/post_merge/mlp/linear_%d.W" % j, g + "/readout/post_merge/mlp/linear_%d.b" % j, w)
                          for j, w in enumerate(dims.pm_hidden)]

    # ---- what a stacked decoder (bricks/generator_stack.py) replaces ----------------------------------------------
    def _state_width(self):
        """Width of the `states` the attention and the readout see."""
        return self.d.D

    def _merge_states_weight(self):
        """readout/merge/transform_states.W as one (state width, P) matrix."""
        return self.store.p[self.n["Wms"]]

    def _initial_state(self):
        return self.store.p[self.n["h0"]]

    def _AW(self, Tp, B):
        """Buffer of AW = attended @ [fork_inputs.W | fork_gate_inputs.W]: (T'*B, 3D) with the rows a multiple of 4 floats apart (the
        persistent backward reads them 16 bytes at a time; D = 250 of the wsj_paper configs gives 750 columns).  -> (view, row stride);
        the padding columns are never written and never contribute (the vector they meet is zero there)."""
        ld = (3 * self.d.D + 3) // 4 * 4
        return self.ws.get("gen.AW", (Tp * B, ld))[:, : 3 * self.d.D], ld

    def _merge_states_backward(self, S2, dR1, gws, group=None):
        """Gradient of the readout's state source: weight gradient into the store, -> dS_r (rows, state width)."""
        d, p, g, n, lib, ws = self.d, self.store.p, self.store.g, self.n, self.lib, self.ws
        wgrad, _ = lib.weight_grad_calls(group, gws)
        wgrad(S2, dR1, g[n["Wms"]])
        dS_r = ws.get("gen.dS_r", (S2.shape[0], d.D))
        lib.sgemm(dR1, p[n["Wms"]], dS_r, transB=True)
        return dS_r

    # ---- packed operand copies ------------------------------------------------------------------
    def _packed(self, packs=True):
        """The operand copies of the current parameters.  packs=False: only allocate the packed copies (and make the plain
        concatenations) — the persistent kernels of the teacher-forced pass read the plain weights, so a training step that stays on
        them never pays the nine pack launches; `_ensure_packs` makes them when a step kernel is about to run."""
        if self._packs is not None and self._packs["version"] == self.store.version and not self.lib.capturing:
            if packs:
                self._ensure_packs(self._packs)
            return self._packs
        p, lib, ws, n, d = self.store.p, self.lib, self.ws, self.n, self.d
        ent = dict(version=self.store.version)
        jobs = []

        def pack(key, W, trans=False):
            K, N = (W.shape[1], W.shape[0]) if trans else (W.shape[0], W.shape[1])
            buf = ws.get("gen.%s_p" % key, (lib.pack_size(K, N),))
            jobs.append((W, buf, trans))
            ent[key] = buf
        pack("Ws", p[n["Ws"]]); pack("WsT", p[n["Ws"]], True)
        pack("Whg", p[n["Whg"]]); pack("WhgT", p[n["Whg"]], True)
        pack("Whh", p[n["Whh"]]); pack("WhhT", p[n["Whh"]], True)
        pack("Wdi", p[n["Wdi"]]); pack("Wdg", p[n["Wdg"]])
        wd = ws.get("gen.Wd_cat", (d.E, 3 * d.D))
        lib.copy_many([(p[n["Wdi"]], wd[:, : d.D]), (p[n["Wdg"]], wd[:, d.D:])])
        pack("WdT", wd, True)
        ent["_jobs"], ent["packed"] = jobs, False
        if packs:
            self._ensure_packs(ent)
        self._packs = ent
        return ent

    MERGE_ROWS = 64          # rows of a beam step from which the readout's merge products run as 16-row tiles (lvsr_readout_merge)

    def _readout_packs(self):
        """Packed copies of the merge weights for lvsr_readout_merge (many-row readout of the batched beam search), per parameter version."""
        hit = getattr(self, "_ro_packs", None)
        if hit is not None and hit["version"] == self.store.version:
            return hit
        d, p, n, lib, ws = self.d, self.store.p, self.n, self.lib, self.ws
        ent = dict(version=self.store.version, Wms=None)
        Wmw = p[n["Wmw"]]
        ent["Wmw"] = ws.get("gen.Wmw_p", (lib.pack_size(int(Wmw.shape[0]), int(Wmw.shape[1])),))
        jobs = [(Wmw, ent["Wmw"], False)]
        if d.use_states_for_readout:
            Wms = self._merge_states_weight()
            ent["Wms"] = ws.get("gen.Wms_p", (lib.pack_size(int(Wms.shape[0]), int(Wms.shape[1])),))
            jobs.append((Wms.contiguous(), ent["Wms"], False))
        lib.pack_many(jobs)
        self._ro_packs = ent
        return ent

    def _ensure_packs(self, ent):
        if not ent.get("packed", True):
            self.lib.pack_many(ent["_jobs"], use_graph=self.use_graph, cache=self._pack_cache)
            ent["packed"] = True

    def _prior(self):
        pr = self.d.cfg["prior"]
        if not self.d.conv:
            return 0, (0.0, 0.0, 0.0, 0.0)
        kind = PRIOR_KIND.get(pr.get("type", "expanding"))
        if kind is None:
            raise Exception("Unknown prior type: %s" % pr.get("type"))       # lvsr/bricks/attention.py:158-159
        if kind == 0:
            return 0, (float(pr["initial_begin"]), float(pr["initial_end"]), _f32(pr["min_speed"]), _f32(pr["max_speed"]))
        return kind, (float(pr["before"]), float(pr["after"]), 0.0, 0.0)

    def _pos_needed(self):
        """Do the rows carry window centres (slot `pos`)?  The windowed priors of a location-aware attention only."""
        return bool(self.d.conv and self._prior()[0] != 0)

    # ---- slots and argument block shared by training and generation -----------------------------------
    def _attdec_bufs(self, prefix, suffix, steps, rows, Tp=None, att=True, gru=True, ZB=False, **given):
        """The slots of `lvsr_attdec_args` for `steps` label steps of `rows` rows: workspace buffers `prefix + slot + suffix`.
        att: the attention part (S, W, pos, WA, EN, sW, CV, ep; ZB = with the normaliser sums the backward pass reads);
        gru: the GRU part (U, R, C, RH, sg, xin).  `given`: slots the caller holds already — xg and ymask, state slots it
        has initialised, a stack layer's column block of S and its distribution input WA; they are not requested."""
        d, ws = self.d, self.ws
        D, Kc = d.D, max(d.K, 1)

        def get(slot, *shape):
            return given[slot] if slot in given else ws.get(prefix + slot + suffix, shape)
        b = dict(given)
        if att:
            b.update(S=get("S", steps + 1, rows, self._state_width()), W=get("W", steps + 1, rows, Tp),
                     pos=get("pos", steps + 1, rows) if self._pos_needed() else None,
                     WA=get("WA", steps, rows, d.E), EN=get("EN", steps, rows, Tp), ZB=get("ZB", steps, rows) if ZB else None,
                     sW=get("sW", steps, rows, d.M), CV=get("CV", steps, rows, Kc, Tp) if d.conv else None)
        if gru:
            b.update(U=get("U", steps, rows, D), R=get("R", steps, rows, D), C=get("C", steps, rows, D), RH=get("RH", steps, rows, D),
                     sg=get("sg", rows, 2 * D), xin=get("xin", rows, D))
        if att:
            b["ep"] = get("ep", rows, (d.M + ATT_MS - 1) // ATT_MS, Tp)
        return b

    def _strides(self, B, broadcast, groups=0, group_Tp=None):
        """How row b of a block finds its utterance in A / PA / Am."""
        d = self.d
        if groups:         # batched beam search: rows [g B/groups, (g+1) B/groups) read utterance g (lvsr_attdec_args.group_rows)
            return dict(A_ts=groups * d.E, A_bs=d.E, PA_ts=groups * d.M, PA_bs=d.M, Am_ts=groups, Am_bs=1,
                        group_rows=B // groups, step_stride=16, group_Tp=group_Tp)
        if broadcast:      # one utterance shared by every hypothesis (beam search)
            return dict(A_ts=d.E, A_bs=0, PA_ts=d.M, PA_bs=0, Am_ts=1, Am_bs=0)
        return dict(A_ts=B * d.E, A_bs=d.E, PA_ts=B * d.M, PA_bs=d.M, Am_ts=B, Am_bs=1)

    def _att_fields(self, A, PA, Am, L, B, D, bufs, phases, step0, broadcast, groups=0, group_Tp=None):
        """The attention half of the argument block over states of width D: sizes, prior, normaliser, the energy parameters, the
        contexts with their strides, and the slots.  The weights of the state transformer are the caller's (packed or plain)."""
        d, p, n = self.d, self.store.p, self.n
        kind, pp = self._prior()
        f = dict(Tp=int(A.shape[0]), B=B, L=L, E=d.E, D=D, M=d.M, K=d.K, c=d.c, prior_type=kind, step0=step0, phases=phases,
                 p0=pp[0], p1=pp[1], p2=pp[2], p3=pp[3], A=A, PA=PA, Am=Am, w_e=p[n["we"]],
                 normalizer=NORMALIZER_KIND[d.normalizer], e_bias=p[n["eb"]] if d.energy_bias else None,
                 filters=p[n["filters"]] if d.conv else None, handler=p[n["handler"]] if d.conv else None)
        f.update(self._strides(B, broadcast, groups, group_Tp))
        f.update(bufs)
        return f

    def _gru_fields(self, pk, l=""):
        """The packed weights of a GRU block (layer l of a stack)."""
        return dict(Whg_p=pk["Whg%s" % l], Whh_p=pk["Whh%s" % l], Wdi_p=pk["Wdi%s" % l], Wdg_p=pk["Wdg%s" % l])

    def _attdec_fields(self, pk, A, PA, Am, L, B, bufs, phases, step0, broadcast, groups=0, group_Tp=None):
        f = self._att_fields(A, PA, Am, L, B, self.d.D, bufs, phases, step0, broadcast, groups, group_Tp)
        f.update(self._gru_fields(pk), Ws_p=pk["Ws"])
        return f

    def _feedback_forks(self, labels_flat, nrows, layers, fb_buf=None, pair=False):
        """xg (nrows,3D) = fork(feedback(labels)) for every (parameter names, xg) of `layers`: LookupFeedback / OneOfNFeedback
        then Fork of two Linear bricks (sequence_generators.py:263-264, 839-842; lvsr/bricks/__init__.py:97-104); one pair
        here, one per layer of a stack (fork_inputs#l)."""
        d, p, lib = self.d, self.store.p, self.lib
        st = lib.stream_for(layers[0][1])
        if d.embed:
            lib.call("lvsr_gather_rows", st, ptr(p[self.n["table"]]), d.FB, ptr(labels_flat), nrows, d.V + 1, d.FB,
                     None, ptr(fb_buf), d.FB)
        for n, xg in layers:
            if d.embed:
                lib.sgemm(fb_buf, p[n["Wfi"]], xg[:, : d.D], bias=p[n["bfi"]])
                lib.sgemm(fb_buf, p[n["Wfg"]], xg[:, d.D:], bias=p[n["bfg"]])
            elif pair:        # (the training step) both fork matrices by the one label list: one launch
                lib.call("lvsr_gather_rows_pair", st, ptr(labels_flat), nrows, d.FB,
                         ptr(p[n["Wfi"]]), d.D, d.D, ptr(p[n["bfi"]]), ptr(xg), 3 * d.D,
                         ptr(p[n["Wfg"]]), 2 * d.D, 2 * d.D, ptr(p[n["bfg"]]), ptr(xg[:, d.D:]), 3 * d.D)
            else:
                lib.call("lvsr_gather_rows", st, ptr(p[n["Wfi"]]), d.D, ptr(labels_flat), nrows, d.FB, d.D,
                         ptr(p[n["bfi"]]), ptr(xg), 3 * d.D)
                lib.call("lvsr_gather_rows", st, ptr(p[n["Wfg"]]), 2 * d.D, ptr(labels_flat), nrows, d.FB, 2 * d.D,
                         ptr(p[n["bfg"]]), ptr(xg[:, d.D:]), 3 * d.D)

    def _feedback_forks_backward(self, l, n, sv, DXG, dfb, wgrad, pair=False):
        """Layer l's share of the backward pass of `_feedback_forks` (n = its parameter names, DXG (rows,3D) the gradient of its
        xg): the fork's weight gradients; with lookup feedback the gradient of the embedded labels `dfb` adds up over the layers
        and goes to the table after the last."""
        d, p, g, lib = self.d, self.store.p, self.store.g, self.lib
        dpc, dg = DXG[:, : d.D], DXG[:, d.D:]
        nrows, st, labels_flat = int(DXG.shape[0]), lib.stream_for(DXG), sv["labels"].view(-1)
        if d.embed:
            wgrad(sv["fb"], dpc, g[n["Wfi"]])
            wgrad(sv["fb"], dg, g[n["Wfg"]])
            lib.sgemm(dpc, p[n["Wfi"]], dfb, transB=True, beta=0.0 if l == 0 else 1.0)
            lib.sgemm(dg, p[n["Wfg"]], dfb, transB=True, beta=1.0)
            if l == d.n_dec - 1:
                lib.call("lvsr_scatter_add_rows", st, ptr(dfb), d.FB, ptr(labels_flat), nrows, d.V + 1, d.FB,
                         ptr(g[self.n["table"]]), d.FB, 0.0)
        elif pair:
            lib.call("lvsr_scatter_add_rows_pair", st, ptr(labels_flat), nrows, d.FB,
                     ptr(dpc), 3 * d.D, d.D, ptr(g[n["Wfi"]]), d.D, 0.0,
                     ptr(dg), 3 * d.D, 2 * d.D, ptr(g[n["Wfg"]]), 2 * d.D, 0.0)
        else:
            lib.call("lvsr_scatter_add_rows", st, ptr(dpc), 3 * d.D, ptr(labels_flat), nrows, d.FB, d.D,
                     ptr(g[n["Wfi"]]), d.D, 0.0)
            lib.call("lvsr_scatter_add_rows", st, ptr(dg), 3 * d.D, ptr(labels_flat), nrows, d.FB, 2 * d.D,
                     ptr(g[n["Wfg"]]), 2 * d.D, 0.0)

    def preprocess(self, attended):
        """attention.preprocess (lvsr/bricks/attention.py:228-230): PA = attended @ W + b."""
        d, p, n = self.d, self.store.p, self.n
        Tp, B = int(attended.shape[0]), int(attended.shape[1])
        PA = self.ws.get("gen.PA", (Tp, B, d.M))
        self.lib.sgemm(attended.view(Tp * B, d.E), p[n["Wpre"]], PA.view(Tp * B, d.M), bias=p[n["bpre"]])
        return PA

    def _readout(self, S2, WA2, nrows, tag):
        """Readout.readout (sequence_generators.py:614-619) + post-merge (recognizer.py:298-320) -> logits."""
        d, p, n, lib, ws = self.d, self.store.p, self.n, self.lib, self.ws
        R1 = ws.get("gen.R1" + tag, (nrows, d.P))
        self._pm_acts = []                       # (input, pre-activation) of every further post-merge layer, for the backward pass
        bias = p[n["bpm"]] if d.post_merge else p[n["bro"]]
        lib.sgemm(WA2, p[n["Wmw"]], R1, bias=bias)
        if d.use_states_for_readout:
            lib.sgemm(S2, self._merge_states_weight(), R1, beta=1.0)
        if not d.post_merge:
            return R1, None, R1
        R2 = ws.get("gen.R2" + tag, (nrows, d.Pout))
        lib.call("lvsr_act_fwd", lib.stream_for(R2), ACT_KIND[d.act], ptr(R1), d.P, nrows, d.P, ptr(R2), d.Pout)
        for j, (wn, bn, width) in enumerate(self.pm_hidden):
            pre = ws.get("gen.pm_pre%d" % j + tag, (nrows, width))
            lib.sgemm(R2, p[wn], pre, bias=p[bn])
            post = ws.get("gen.pm_post%d" % j + tag, (nrows, width))
            lib.call("lvsr_act_fwd", lib.stream_for(post), ACT_KIND[d.act], ptr(pre), width, nrows, width, ptr(post), width)
            self._pm_acts.append((R2, pre))
            R2 = post
        logits = ws.get("gen.logits" + tag, (nrows, d.V))
        lib.sgemm(R2, p[n["Wout"]], logits, bias=p[n["bout"]])
        return R1, R2, logits

    # ---- persistent label loop -------------------------------------------------------------------
    def _persist_sync(self, query, args, name, emulated=True):
        """The int32 workspace `name` of a persistent kernel, of the size the library's `query` gives for the argument block, or
        None when the kernel does not apply: the configuration is outside its limits (0 bytes) or — `emulated`, on the CPU
        emulator — work-groups are not run concurrently."""
        nbytes = int(getattr(self.lib, "_" + query)(ctypes.byref(args)))
        if emulated and self.lib.is_emulator and not self.lib.emulates_concurrency():
            nbytes = 0
        return self.ws.get(name, ((nbytes + 3) // 4,), torch.int32) if nbytes else None

    def _persistent_ws(self, fields):
        """Workspace of the persistent decoder kernel for this argument block, or None when the step kernels run
        (`use_persistent=False`, or `_persist_sync` finds the kernel not applicable)."""
        if self.use_persistent is not None and not self.use_persistent:
            return None
        sync = self._persist_sync("lvsr_attdec_persist_ws_bytes", self.lib.make("lvsr_attdec_args", **fields), "gen.sync")
        if sync is None and self.use_persistent:
            raise ValueError("persistent decoder kernel requested but not available for this configuration")
        return sync

    def _persistent_bwd_ws(self, fwd_args):
        """Workspace of the persistent backward kernel, or None (`use_persistent` / `use_persistent_bwd` False, or not applicable)."""
        # Default since round 3: 33.4 us per label against 41.5 for the four step kernels (profiles/r03_decoder_bwd_persist_probe.txt),
        # WSJ-base step 18.3 -> 17.4 ms.
        if self.use_persistent is False or self.use_persistent_bwd is False:
            return None
        return self._persist_sync("lvsr_attdec_bwd_persist_ws_bytes", fwd_args, "gen.sync_bwd")

    def _plain(self, n, AW, AW_ld):
        """lvsr_attdec_plain: the unpacked weights (parameter names n) a persistent kernel reads, and AW = attended @ [Wdi | Wdg]."""
        p = self.store.p
        return self.lib.make("lvsr_attdec_plain", Ws=p[n["Ws"]], Whg=p[n["Whg"]], Whh=p[n["Whh"]], AW=AW, AW_ld=AW_ld)

    def _cluster_partials(self, query, fwd_args, B):
        """(accH, accWe, accEb) of a persistent reverse walk: one row per work-group (`query`: work-groups per utterance of the
        launch) — written, not accumulated, so nothing to clear."""
        d, ws = self.d, self.ws
        P = int(getattr(self.lib, "_" + query)(ctypes.byref(fwd_args)))
        return (ws.get("gen.accH_p", (B * P, max(d.K, 1) * d.M)), ws.get("gen.accWe_p", (B * P, d.M)),
                ws.get("gen.accEb_p", (B * P, 1)))

    def _QR(self, sv, dWA_r):
        """QR[:, b] = dWA_r_b (L,E) @ attended_b^T (E,T') for every utterance b, one batched launch: the readout's share of the
        alignment gradient in the reassociated glimpse contraction of the persistent reverse walks."""
        d, lib = self.d, self.lib
        L, B, Tp = sv["L"], sv["B"], sv["Tp"]
        QR = self.ws.get("gen.QR", (L, B, Tp))
        lib.call("lvsr_sgemm_batched", lib.stream_for(QR), 0, 1, L, Tp, d.E, 1.0, ptr(dWA_r), B * d.E, d.E,
                 ptr(sv["A"]), B * d.E, d.E, 0.0, ptr(QR), B * Tp, Tp, B)
        return QR

    def check_persistent(self):
        """After a synchronisation point: raise if the persistent decoder kernel gave up waiting for its cluster."""
        for k, buf in self.ws._bufs.items():
            if k[0] in ("gen.sync", "gen.sync_bwd") and int(buf[0]) != 0:
                buf[:16].zero_()          # sticky abort word (no launch clears it): cleared once reported
                raise RuntimeError("persistent decoder kernel aborted (a work-group of a cluster was not scheduled); results since "
                                   "the last check are invalid")

    # ---- teacher-forced cost ---------------------------------------------------------------------
    def _check_emitter(self):
        if self.mse and self.language_model is not None:
            raise NotImplementedError("criterion %s with a language model is not built" % self.criterion)

    def reward_matrices(self, groundtruth, prediction, want_mask=False):
        """RewardOp (lvsr/ops.py:236-294) on the device: groundtruth (Lg,B), prediction (Lp,B) int64 -> dict(rewards, gains (Lp,B,V),
        mask (Lp,B): the prediction up to and including its first EOS, lvsr/main.py:254-259; only with `want_mask`).  Groundtruth
        columns must end in EOS (a column without one is used whole; the reference raises there)."""
        d, lib, ws = self.d, self.lib, self.ws
        Lp, B = int(prediction.shape[0]), int(prediction.shape[1])
        gt, pred = groundtruth.contiguous(), prediction.contiguous()
        out = dict(rewards=ws.get("gen.reward_matrix", (Lp, B, d.V)), gains=ws.get("gen.gain_matrix", (Lp, B, d.V)),
                   mask=ws.get("gen.prediction_mask", (Lp, B)) if want_mask else None)
        lib.call("lvsr_reward_gain", lib.stream_for(out["rewards"]), ptr(gt), int(gt.shape[0]), ptr(pred), Lp, B, int(d.cfg["eos_label"]),
                 d.V, ptr(out["rewards"]), ptr(out["gains"]), ptr(out["mask"]))
        return out

    def cost_matrix(self, outputs, mask=None, attended=None, attended_mask=None, save_for_backward=True, groundtruth=None,
                    rewards=None):
        """outputs (L,B) int64 labels, mask (L,B) or None, attended (T',B,E), attended_mask (T',B) -> costs (L,B).
        Also keeps `self.last` = dict(weights, energies, states, weighted_averages, readouts) (the auxiliary variables
        `SpeechRecognizer.analyze` extracts, recognizer.py:452-494).
        mse criteria: `outputs` / `mask` are the prediction, `groundtruth` (Lg,B; default: `outputs`, the placeholder the reference's
        get_cost_graph swaps, recognizer.py:437-449) is what the rewards are measured against; `rewards`: the result of
        `reward_matrices` when the caller has run it already.  `last` also holds gain_matrix and reward_matrix."""
        self._check_emitter()
        d, p, n, lib, ws = self.d, self.store.p, self.n, self.lib, self.ws
        L, B = int(outputs.shape[0]), int(outputs.shape[1])
        Tp = int(attended.shape[0])
        pk = self._packed(packs=False)
        # a pass that saves for a backward pass (the training step) shares launches between neighbours (`_forward_recurrent`); any
        # other caller (analyze) issues the launches it always did
        self._merge_launches = bool(save_for_backward)
        A = attended.contiguous()
        Am = attended_mask.contiguous()
        labels = outputs.contiguous()
        ym = None if mask is None else mask.contiguous()
        PA = self.preprocess(A)
        rc = self._forward_recurrent(pk, A, PA, Am, labels, ym, L, B, Tp)
        bufs, S, W, WA = rc["bufs"], rc["bufs"]["S"], rc["bufs"]["W"], rc["bufs"]["WA"]
        SW = self._state_width()
        S2, WA2 = S[:L].view(L * B, SW), WA.view(L * B, d.E)
        R1, R2, logits = self._readout(S2, WA2, L * B, "")
        cost = ws.get("gen.cost", (L, B))
        dlogits = ws.get("gen.dlogits", (L * B, d.V))
        if self.mse:
            # RewardRegressionEmitter.cost (lvsr/bricks/__init__.py:134-183) in place of the softmax cross-entropy
            rw = rewards if rewards is not None else self.reward_matrices(labels if groundtruth is None else groundtruth, labels)
            lib.call("lvsr_reward_mse", lib.stream_for(cost), int(self.criterion == "mse_reward"), ptr(logits), d.V, ptr(rw["gains"]),
                     ptr(rw["rewards"]), ptr(labels), ptr(ym), L, B, d.V, self.min_reward, ptr(cost), ptr(dlogits), d.V)
        else:
            lib.call("lvsr_softmax_nll", lib.stream_for(cost), ptr(logits), d.V, ptr(labels), ptr(ym), L * B, d.V,
                     ptr(cost), ptr(dlogits), d.V, 1.0, None, 0)
        lm = self.language_model
        self._cost_has_lm = lm is not None
        if lm is not None:
            # SequenceGenerator.evaluate with a language model (sequence_generators.py:286-296): the readout of label i is fused
            # (ShallowFusionReadout) with the look-ahead costs of the FST state set reached by labels[:i], the emitter is LMEmitter:
            # cost = -fused[label].  This is what `analyze` reports in the decode driver when `net.lm` is configured.
            lm_add = self._lm_lookahead(lm, labels, ym, L, B)
            fused = ws.get("gen.fused", (L * B, d.V))
            lib.call("lvsr_shallow_fusion", lib.stream_for(cost), ptr(logits), d.V, ptr(lm_add), L * B, d.V, float(lm.am_beta),
                     float(lm.lm_weight), int(lm.norm[0]), int(lm.norm[1]), int(lm.norm[2]), 1.0, ptr(fused))
            lib.call("lvsr_select_cost", lib.stream_for(cost), ptr(fused), d.V, ptr(labels), ptr(ym), L * B, d.V, -1.0,
                     ptr(cost))
        self.last = dict(weights=W[1:], energies=bufs["EN"], states=S[:L], weighted_averages=WA, readouts=logits.view(L, B, d.V))
        if self.mse:
            self.last.update(gain_matrix=rw["gains"], reward_matrix=rw["rewards"])
        if save_for_backward:
            self._saved = dict(L=L, B=B, Tp=Tp, A=A, Am=Am, PA=PA, labels=labels, ym=ym, bufs=bufs,
                               R1=R1, R2=R2, dlogits=dlogits, pk=pk, pm_acts=list(self._pm_acts))
            self._saved.update(rc["saved"])
        return cost

    def _forward_recurrent(self, pk, A, PA, Am, labels, ym, L, B, Tp):
        """The label loop of the teacher-forced pass: fork(feedback(labels)) and the AttentionRecurrent scan
        (sequence_generators.py:263-277).  -> dict(bufs = the state slots / per-label tensors (S, W, WA, EN, ...), saved =
        what `_backward_recurrent` needs beyond them)."""
        d, p, n, lib, ws = self.d, self.store.p, self.n, self.lib, self.ws
        xg = ws.get("gen.xg", (L * B, 3 * d.D))
        fb = ws.get("gen.fb", (L * B, d.FB)) if d.embed else None
        merge = getattr(self, "_merge_launches", False)
        self._feedback_forks(labels.view(-1), L * B, [(n, xg)], fb, pair=merge)
        bufs = self._attdec_bufs("gen.", "", L, B, Tp, ZB=True, xg=xg, ymask=ym)
        S, W = bufs["S"], bufs["W"]
        self._initial_slots(S, W, B, Tp, merge)
        fields = self._attdec_fields(pk, A, PA, Am, L, B, bufs, phases=3, step0=0, broadcast=False)
        sync = self._persistent_ws(fields)
        if sync is not None:
            # one persistent launch for the whole label loop (csrc/decoder_persist.hip): a memset and a kernel, no graph needed
            fwd_args = lib.make("lvsr_attdec_args", **fields)
            # gate inputs of the glimpse, reassociated: AW = attended @ [fork_inputs.W | fork_gate_inputs.W] once per batch
            wd = ws.get("gen.Wd_cat", (d.E, 3 * d.D))
            AW, AW_ld = self._AW(Tp, B)
            lib.sgemm(A.view(Tp * B, d.E), wd, AW)
            lib.call("lvsr_attdec_fwd_persistent", lib.stream_for(S), ctypes.byref(fwd_args), ctypes.byref(self._plain(n, AW, AW_ld)),
                     ptr(sync), 0)
            lib.call("lvsr_attdec_glimpses", lib.stream_for(S), ctypes.byref(fwd_args))
        else:
            self._ensure_packs(pk)
            fwd_args = lib.run("lvsr_attdec_fwd", "lvsr_attdec_args", S, self.use_graph, **fields)
        return dict(bufs=bufs, saved=dict(xg=xg, fb=fb, fields=fields, AW_valid=sync is not None))

    def _initial_slots(self, S, W, B, Tp, merge):
        """Slot 0 of the teacher-forced pass: S[0] = initial_state tiled (recurrent.py:622-624), W[0] = initial_glimpses (one-hot on
        frame 0 with a location-aware attention, else zeros; lvsr/bricks/attention.py:215-222) — two row broadcasts in ONE launch (a
        copy, a fill and a strided fill before).  The row W[0] repeats lives in a workspace of its own, written when it comes into
        being; without `merge`, and inside a graph capture that finds the row new (a captured write would never run if the capture
        is dropped), the three plain operations are enqueued."""
        d, p, n, lib, ws = self.d, self.store.p, self.n, self.lib, self.ws
        row = ws.get("gen.W0_row", (Tp,)) if merge else None
        if row is None or getattr(self, "_w0_row_ptr", None) != row.data_ptr():
            if row is None or lib.capturing:
                S[0].copy_(p[n["h0"]].unsqueeze(0).expand(B, d.D))
                W[0].zero_()
                if d.conv:
                    W[0, :, 0] = 1.0
                return
            base = ws._bufs[("gen.W0_row", torch.float32)]
            base.zero_()
            if d.conv:
                base[0] = 1.0
            self._w0_row_ptr = row.data_ptr()
        lib.copy_many([(p[n["h0"]].unsqueeze(0).expand(B, d.D), S[0]), (row.unsqueeze(0).expand(B, Tp), W[0])])

    def _lm_lookahead(self, lm, labels, ym, L, B):
        """(L*B, V) look-ahead costs `lm_add` of the teacher-forced label sequences: row (i, b) = FSTCostsOp of the state set after
        labels[:i, b] (LanguageModel.evaluate -> FSTTransition.apply, lvsr/bricks/language_models.py:34-50; masked steps keep the
        previous state set).  One FST step per label for the whole batch — on the device with a DeviceFSTLanguageModel."""
        dev = labels.device
        out = self.ws.get("gen.lm_add", (L, B, self.d.V))
        st = lm.initial_states(B)
        on_dev = lm.on_device
        lab = labels if on_dev else labels.cpu().numpy()
        msk = None if ym is None else (ym if on_dev else ym.cpu().numpy())
        for i in range(L):
            out[i].copy_(lm.stage(st, dev))
            if i + 1 == L:
                break
            new = lm.transition(st, lab[i])
            if msk is not None:
                if on_dev:
                    keep = msk[i] > 0
                    st = {k: torch.where(keep.view(-1, *([1] * (v.dim() - 1))), new[k], st[k]) for k, v in new.items()}
                else:
                    keep = msk[i] > 0
                    st = {k: numpy.where(keep.reshape((-1,) + (1,) * (v.ndim - 1)), new[k], st[k]) for k, v in new.items()}
            else:
                st = new
        return out.view(L * B, self.d.V)

    def backward(self, group=None):
        """Gradient of sum(cost_matrix) wrt every generator parameter (written to store.g) and wrt `attended`
        (returned, (T',B,E)).  With a `group` (native.GemmGroup) the weight-gradient products and bias column sums join it and
        are final only after the caller's flush; without one they launch here."""
        d, p, g, n, lib, ws = self.d, self.store.p, self.store.g, self.n, self.lib, self.ws
        sv = self._saved
        assert sv is not None, "cost_matrix() must run first"
        if getattr(self, "_cost_has_lm", False):
            lm = self.language_model
            # with the acoustic readout normalised alone and am_beta = 1 the language-model term is a constant of the parameters
            # and the gradient is the plain one (dlogits of the softmax); the other fusion settings are decode-time options
            if lm is None or tuple(lm.norm) != (True, False, False) or float(lm.am_beta) != 1.0:
                raise NotImplementedError("gradient through ShallowFusionReadout is built for normalize_am_weights only (am_beta = 1)")
        L, B, Tp = sv["L"], sv["B"], sv["Tp"]
        bufs, pk = sv["bufs"], sv["pk"]
        nrows = L * B
        gws = ws.get("gemm_ws", (1 << 22,))
        wgrad, colsum = lib.weight_grad_calls(group, gws)
        S2, WA2 = bufs["S"][:L].view(nrows, self._state_width()), bufs["WA"].view(nrows, d.E)
        dlogits, R1, R2 = sv["dlogits"], sv["R1"], sv["R2"]
        # ---- readout backward
        if d.post_merge:
            wgrad(R2, dlogits, g[n["Wout"]])
            colsum(dlogits, g[n["bout"]])
            dR2 = ws.get("gen.dR2", (nrows, R2.shape[1]))
            lib.sgemm(dlogits, p[n["Wout"]], dR2, transB=True)
            for j in range(len(self.pm_hidden) - 1, -1, -1):          # the further post-merge layers, last first
                wn, bn, width = self.pm_hidden[j]
                xin, pre = sv["pm_acts"][j]
                dpre = ws.get("gen.pm_dpre%d" % j, (nrows, width))
                lib.call("lvsr_act_bwd", lib.stream_for(dpre), ACT_KIND[d.act], ptr(pre), width, ptr(dR2), width, nrows, width,
                         ptr(dpre), width)
                wgrad(xin, dpre, g[wn])
                colsum(dpre, g[bn])
                dR2 = ws.get("gen.pm_dx%d" % j, (nrows, xin.shape[1]))
                lib.sgemm(dpre, p[wn], dR2, transB=True)
            dR1 = ws.get("gen.dR1", (nrows, d.P))
            lib.call("lvsr_act_bwd", lib.stream_for(dR1), ACT_KIND[d.act], ptr(R1), d.P, ptr(dR2), d.Pout, nrows, d.P,
                     ptr(dR1), d.P)
            colsum(dR1, g[n["bpm"]])
        else:
            dR1 = dlogits
            colsum(dR1, g[n["bro"]])
        wgrad(WA2, dR1, g[n["Wmw"]])
        dWA_r = ws.get("gen.dWA_r", (nrows, d.E))
        lib.sgemm(dR1, p[n["Wmw"]], dWA_r, transB=True)
        dS_r = None
        if d.use_states_for_readout:
            dS_r = self._merge_states_backward(S2, dR1, gws, group)
        rb = self._backward_recurrent(sv, dWA_r, dS_r, gws, group)
        accH, accWe, accEb, DCV, dPA, DWA = rb["accH"], rb["accWe"], rb["accEb"], rb["DCV"], rb["dPA"], rb["DWA"]
        st = lib.stream_for(dPA)
        colsum(accWe, g[n["we"]].view(-1))
        if d.energy_bias:
            colsum(accEb, g[n["eb"]])
        if d.conv:
            colsum(accH, g[n["handler"]].view(-1))
            # partial sums per chunk of (label, utterance) rows: at most one chunk per row (large per-GPU batches outgrow gemm_ws)
            fws = ws.get("gen.filter_ws", (max(1 << 20, L * B * d.K * (2 * d.c + 1)),))
            lib.call("lvsr_attdec_filter_grad", st, ctypes.byref(rb["fwd_args"]), ptr(DCV), ptr(g[n["filters"]]), ptr(fws),
                     fws.numel() * 4)
        # ---- attended: preprocess backward + glimpse backward
        A2, dPA2 = sv["A"].view(Tp * B, d.E), dPA.view(Tp * B, d.M)
        wgrad(A2, dPA2, g[n["Wpre"]])
        colsum(dPA2, g[n["bpre"]])
        dA = ws.get("gen.dA", (Tp, B, d.E))
        lib.sgemm(dPA2, p[n["Wpre"]], dA.view(Tp * B, d.E), transB=True)
        W = bufs["W"]
        # dA[:, b, :] += alpha_b^T (T',L) @ dwa_b (L,E) for every utterance b: one batched launch
        lib.call("lvsr_sgemm_batched", lib.stream_for(dA), 1, 0, Tp, d.E, L, 1.0, ptr(W[1:]), B * Tp, Tp,
                 ptr(DWA), B * d.E, d.E, 1.0, ptr(dA), B * d.E, d.E, B)
        return dA

    def _backward_recurrent(self, sv, dWA_r, dS_r, gws, group=None):
        """Reverse walk over the labels and the weight gradients of the transition, the glimpse distribution, the state
        transformer and the feedback fork.  -> dict(accH, accWe, accEb: partial sums of the handler / energy vector / energy
        bias gradients (folded by the caller), DCV, dPA, DWA, fwd_args: the forward argument block of the attention)."""
        d, p, g, n, lib, ws = self.d, self.store.p, self.store.g, self.n, self.lib, self.ws
        L, B, Tp = sv["L"], sv["B"], sv["Tp"]
        bufs, pk = sv["bufs"], sv["pk"]
        nrows = L * B
        S2, WA2 = bufs["S"][:L].view(nrows, d.D), bufs["WA"].view(nrows, d.E)
        nslice = (d.M + ATT_MS - 1) // ATT_MS
        ntile = (Tp + 63) // 64
        Kc = max(d.K, 1)
        wgrad, colsum = lib.weight_grad_calls(group, gws)
        DXG = ws.get("gen.DXG", (nrows, 3 * d.D))
        # The glimpse contraction is reassociated (as in the persistent forward): q = DXG . AW + QR — the kernels need no dwa and do
        # not write DWA; the total gradient wrt the weighted averages is formed after the walk, accumulated onto the readout's share
        # where it lies: DWA = dWA_r + DXG @ [Wdi | Wdg]^T
        DWA = dWA_r.view(L, B, d.E)
        DSW = ws.get("gen.DSW", (nrows, d.M))
        DCV = ws.get("gen.DCV", (L, B, Kc, Tp)) if d.conv else None
        dPA = ws.get("gen.dPA", (Tp, B, d.M))
        ds = ws.get("gen.ds", (B, d.D))
        lib.clear_many([(dPA.data_ptr(), dPA.numel() * 4), (ds.data_ptr(), ds.numel() * 4)], ds)       # both accumulate: one launch
        wd = ws.get("gen.Wd_cat", (d.E, 3 * d.D))
        AW, AW_ld = self._AW(Tp, B)
        if not sv.get("AW_valid"):
            lib.sgemm(sv["A"].view(Tp * B, d.E), wd, AW)
        QR = self._QR(sv, dWA_r)
        fwd_args = lib.make("lvsr_attdec_args", **sv["fields"])
        psync = self._persistent_bwd_ws(fwd_args)
        if psync is not None:
            # the whole reverse walk as one persistent launch (csrc/decoder_persist_bwd.hip); its handler / energy-vector / bias
            # gradient partials come one row per work-group — written, not accumulated: nothing but dPA and ds to clear
            accH, accWe, accEb = self._cluster_partials("lvsr_attdec_bwd_persist_clusters", fwd_args, B)
            bw = lib.make("lvsr_attdec_bwd_args", dS_r=dS_r, DXG=DXG, DSW=DSW, DCV=DCV, dPA=dPA, accH=accH, accWe=accWe, accEb=accEb,
                          ds=ds, AW=AW, QR=QR, AW_ld=AW_ld)
            bw.f = fwd_args
            lib.call("lvsr_attdec_bwd_persistent", lib.stream_for(ds), ctypes.byref(bw), ctypes.byref(self._plain(n, AW, AW_ld)), ptr(psync))
        else:
            self._ensure_packs(pk)
            accH = ws.get("gen.accH", (B * ntile, Kc * d.M), zero=True)
            accWe = ws.get("gen.accWe", (B * ntile, d.M), zero=True)
            accEb = ws.get("gen.accEb", (B * ntile, 1), zero=True)
            bw = lib.make("lvsr_attdec_bwd_args", WhhT_p=pk["WhhT"], WhgT_p=pk["WhgT"], WdT_p=pk["WdT"], WsT_p=pk["WsT"],
                          dWA_r=dWA_r, dS_r=dS_r, DXG=DXG, DWA=DWA, DSW=DSW, DCV=DCV, dPA=dPA, accH=accH, accWe=accWe, accEb=accEb,
                          ds=ds, dalp=ws.get("gen.dalp", (B, Kc, Tp), zero=True), dspart=ws.get("gen.dspart", (B, d.D)),
                          dsacc=ws.get("gen.dsacc", (B, d.D)), Q=ws.get("gen.Q", (B, Tp)),
                          dcvp=ws.get("gen.dcvp", (B, nslice, Kc, Tp)) if d.conv else None,
                          dswp=ws.get("gen.dswp", (B, ntile, d.M)), AW=AW, QR=QR, AW_ld=AW_ld)
            bw.f = fwd_args
            lib.call("lvsr_attdec_bwd", lib.stream_for(ds), ctypes.byref(bw), int(self.use_graph))
        lib.sgemm(DXG, wd, dWA_r, transB=True, beta=1.0)
        # ---- weight gradients as batched GEMMs over all steps
        dpc, dg = DXG[:, : d.D], DXG[:, d.D:]
        RH2 = bufs["RH"].view(nrows, d.D)
        wgrad(RH2, dpc, g[n["Whh"]])
        wgrad(S2, dg, g[n["Whg"]])
        wgrad(WA2, dpc, g[n["Wdi"]])
        wgrad(WA2, dg, g[n["Wdg"]])
        wgrad(S2, DSW, g[n["Ws"]])
        colsum(ds, g[n["h0"]])
        colsum(dpc, g[n["bfi"]])
        colsum(dg, g[n["bfg"]])
        self._feedback_forks_backward(0, n, sv, DXG, ws.get("gen.dfb", (nrows, d.FB)) if d.embed else None, wgrad, pair=True)
        return dict(accH=accH, accWe=accWe, accEb=accEb, DCV=DCV, dPA=dPA, DWA=DWA, fwd_args=fwd_args)

    # ---- generation mode (what BeamSearch drives: libs/blocks/blocks/search.py:97-142) -----------------------
    def init_generation(self, attended, attended_mask):
        """context_computer (search.py:97-104): keep the single utterance's contexts; every hypothesis of the
        beam reads them with a zero batch stride (no tiling as in search.py:336-338)."""
        d = self.d
        Tp, N = int(attended.shape[0]), int(attended.shape[1])
        A = attended.contiguous()
        PA = self.preprocess(A)
        if N == 1:
            self._gen = dict(Tp=Tp, A=A.view(Tp, d.E), Am=attended_mask.contiguous().view(Tp), PA=PA.view(Tp, d.M))
        else:
            # several utterances at once (BeamSearch.search_batch): the beams of all of them advance in the same launches, every
            # row reading the contexts of its own utterance (`beam_begin` with groups); `lengths` = attended length of each
            Am = attended_mask.contiguous()
            self._gen = dict(Tp=Tp, A=A, Am=Am, PA=PA, N=N, lengths=self.ws.get("gen.glen", (N,), torch.int32))
            self._gen["lengths"].copy_(Am.sum(dim=0).to(torch.int32))

    # ---- free-running generation: SequenceGenerator.generate / initial_states, SoftmaxEmitter.emit ---------------------------
    def initial_states(self, batch_size, attended=None, attended_mask=None):
        """BaseSequenceGenerator.initial_states (sequence_generators.py:404-422): initial values of the `generate` states:
        states = tiled initial_state (recurrent.py:622-624), outputs = SoftmaxEmitter.initial_outputs (num_phonemes,
        recognizer.py:286), glimpses = initial_glimpses (lvsr/bricks/attention.py:215-222)."""
        d = self.d
        h0 = self._initial_state()
        dev = h0.device
        B = int(batch_size)
        Tp = int(attended.shape[0]) if attended is not None else 0
        out = dict(states=h0.unsqueeze(0).expand(B, self._state_width()).clone(),
                   outputs=torch.full((B,), 0 if self.mse else d.V, dtype=torch.int64, device=dev),      # RewardRegressionEmitter: zeros
                   weighted_averages=torch.zeros(B, d.E, device=dev), weights=torch.zeros(B, Tp, device=dev))
        if d.conv:
            if Tp:
                out["weights"][:, 0] = 1.0
            out["energies"] = out["weights"].clone()
            out["step"] = torch.zeros(B, dtype=torch.int64, device=dev)
        return out

    def emit(self, readouts, uniforms=None, seed=None):
        """SoftmaxEmitter.emit (sequence_generators.py:770-776) on readouts (n,V): one class per row by inverse CDF of the
        softmax at a uniform number per row.  `uniforms` (n) in [0,1) or None = drawn from torch's Philox generator
        (`seed`; the reference draws from Theano's MRG31k3p: another stream of the same distribution).  -> (outputs, costs)."""
        d, lib = self.d, self.lib
        x = readouts.contiguous()
        n = int(x.shape[0])
        u = self._uniforms((n,), uniforms, seed, x.device)
        out = torch.empty(n, dtype=torch.int64, device=x.device)
        cost = torch.empty(n, dtype=torch.float32, device=x.device)
        lib.call("lvsr_softmax_emit", lib.stream_for(x), ptr(x), int(x.stride(0)), ptr(u), n, int(x.shape[1]), ptr(out),
                 ptr(cost))
        return out, cost

    def _uniforms(self, shape, uniforms, seed, dev):
        if uniforms is not None:
            u = torch.as_tensor(numpy.ascontiguousarray(uniforms, dtype=numpy.float32)) if not torch.is_tensor(uniforms) else uniforms
            u = u.to(dev).to(torch.float32).contiguous()
            assert tuple(u.shape) == tuple(shape), "uniforms must have shape %s" % (tuple(shape),)
            return u
        if dev.type == "cuda":
            gen = torch.Generator(device=dev)
            gen.manual_seed(int(seed if seed is not None else 1))
            return torch.rand(shape, generator=gen, device=dev, dtype=torch.float32)
        gen = torch.Generator()
        gen.manual_seed(int(seed if seed is not None else 1))
        return torch.rand(shape, generator=gen, dtype=torch.float32)

    def generate(self, n_steps=None, batch_size=None, attended=None, attended_mask=None, uniforms=None, seed=None):
        """BaseSequenceGenerator.generate under its `recurrent` wrapper (sequence_generators.py:328-377): per step
        take_glimpses(previous states and glimpses) -> readout -> emit -> cost -> feedback/fork -> compute_states, all on the
        device with no host synchronisation.  attended (T',B,E), attended_mask (T',B); `uniforms` (n_steps,B) fixes the
        draws (see `emit`).  -> dict(states (n,B,D), outputs (n,B) int64, weighted_averages (n,B,E), weights (n,B,T'),
        energies (n,B,T'), costs (n,B))."""
        d, p, n, lib, ws = self.d, self.store.p, self.n, self.lib, self.ws
        self._check_emitter()
        if self.language_model is not None:
            # With a language model the reference's emitter is LMEmitter, whose `emit` returns zeros "that should never be used"
            # (lvsr/bricks/language_models.py:160-163): free-running generation is not a path of the reference there — beam search
            # (which picks the outputs itself) and the teacher-forced cost (cost_matrix / analyze, built) are.
            raise NotImplementedError("generate() with a language model: the reference's LMEmitter.emit returns zeros (not a "
                                      "sampling path); use beam_search, or cost / analyze for teacher-forced costs")
        N = int(n_steps)
        Tp, B = int(attended.shape[0]), int(attended.shape[1])
        assert batch_size is None or int(batch_size) == B
        pk = self._packed()
        A, Am = attended.contiguous(), attended_mask.contiguous()
        PA = self.preprocess(A)
        dev = A.device
        # RewardRegressionEmitter.emit is the argmax (lvsr/bricks/__init__.py:186-188): no random numbers
        u = None if self.mse else self._uniforms((N, B), uniforms, seed, dev)
        pos_needed = self._pos_needed()
        S = ws.get("sg.S", (N + 1, B, d.D))
        W = ws.get("sg.W", (N + 1, B, Tp))
        # `initial_states` written in place (nothing is allocated: greedy exploration runs this inside a captured training step)
        S[0].copy_(self._initial_state().unsqueeze(0).expand(B, d.D))
        W[0].zero_()
        if d.conv:
            W[0, :, 0] = 1.0
        full = self._attdec_bufs("sg.", "", N, B, Tp, S=S, W=W, xg=ws.get("sg.xg", (N, B, 3 * d.D)), ymask=None)
        outputs = ws.get("sg.outputs", (N, B), torch.int64)
        costs = ws.get("sg.costs", (N, B))
        fb = ws.get("sg.fb", (B, d.FB)) if d.embed else None
        if pos_needed:
            full["pos"][0].zero_()
        st = lib.stream_for(S)
        for t in range(N):
            # step t works on the slots from t on; the scratch of a step (sg, xin, ep) is shared by all of them
            bufs = {k: v if v is None or k in ("sg", "xin", "ep") else v[t:] for k, v in full.items()}
            skip = 4 if pos_needed else 0
            fa = self._attdec_fields(pk, A, PA, Am, 1, B, bufs, phases=1 | skip, step0=t, broadcast=False)
            lib.call("lvsr_attdec_fwd", st, ctypes.byref(lib.make("lvsr_attdec_args", **fa)), 0)
            ra = self._readout_step_args(S[t], full["WA"][t], B, uniforms=None if u is None else u[t], outputs=outputs[t], costs=costs[t])
            lib.call("lvsr_readout_step", st, ctypes.byref(ra))
            self._feedback_forks(outputs[t], B, [(n, full["xg"][t])], fb)
            fg = self._attdec_fields(pk, A, PA, Am, 1, B, bufs, phases=2, step0=t, broadcast=False)
            lib.call("lvsr_attdec_fwd", st, ctypes.byref(lib.make("lvsr_attdec_args", **fg)), 0)
        return dict(states=S[1:], outputs=outputs, weighted_averages=full["WA"], weights=W[1:], energies=full["EN"], costs=costs)

    def beam_begin(self, K, eol, max_length, ignore_first_eol=False, char_discount=0.0, round_to_inf=1e9, stop_on="patience",
                   force_merge=False):
        """Begin the device-resident beam search(es) over the contexts set by `init_generation` -> its `BeamState`
        (bricks/beam_state.py), from now on the one search set this generator serves: the launches of an earlier state raise."""
        self._check_emitter()
        self.current_search = BeamState(self, K, eol, max_length, ignore_first_eol, char_discount, round_to_inf, stop_on, force_merge)
        return self.current_search

    def _readout_step_args(self, S2, WA2, n, neglogp=None, lm_add=None, uniforms=None, outputs=None, costs=None, logits=None, R1=None):
        """Argument block of the fused generation-time readout + emitter (lvsr_readout_step)."""
        d, p, n_ = self.d, self.store.p, self.n
        lm = self.language_model
        return self.lib.make(
            "lvsr_readout_step_args", S=S2, WA=WA2, lds=int(S2.stride(0)), ldwa=int(WA2.stride(0)), n=n, D=self._state_width(), E=d.E,
            P=d.P, V=d.V, act=ACT_KIND[d.act] if d.post_merge else 0,
            Wms=self._merge_states_weight() if d.use_states_for_readout else None, Wmw=p[n_["Wmw"]],
            bias1=p[n_["bpm"]] if d.post_merge else p[n_["bro"]], Wout=p[n_["Wout"]] if d.post_merge else None,
            bout=p[n_["bout"]] if d.post_merge else None, lm_add=lm_add,
            am_beta=lm.am_beta if lm_add is not None else 1.0, lm_weight=lm.lm_weight if lm_add is not None else 0.0,
            norm_am=int(lm.norm[0]) if lm_add is not None else 1, norm_lm=int(lm.norm[1]) if lm_add is not None else 0,
            norm_tot=int(lm.norm[2]) if lm_add is not None else 0, neglogp=neglogp, logits=logits, uniforms=uniforms,
            R1=R1, ldr1=0 if R1 is None else int(R1.stride(0)), emitter=int(self.mse),
            outputs=outputs, costs=costs, n_hidden=len(self.pm_hidden), Wh=[p[w] for w, _, _ in self.pm_hidden],
            bh=[p[b] for _, b, _ in self.pm_hidden], dimh=[w for _, _, w in self.pm_hidden])
