"""Host-side mirror of lvsr.bricks: Encoder (lvsr/bricks/__init__.py:54-83) driving the HIP kernels.

`Encoder.apply(input_, mask)` keeps the reference signature and returns `(encoded, encoded_mask)`;
`Encoder.backward(d_encoded)` is the BPTT counterpart the reference gets from theano.grad.
All arithmetic happens in the C-ABI library (lvsr_sgemm / lvsr_bigru_fwd / lvsr_bigru_bwd / lvsr_colsum);
torch is used for buffers and views only.
"""
import contextlib

import torch


class SpeechBottom(object):
    """lvsr.bricks.recognizer.SpeechBottom (recognizer.py:105-157): Identity, or an MLP applied to every frame."""
    ACT = {"identity": 0, "rectifier": 2, "tanh": 3}

    def __init__(self, dims, store, lib, workspace):
        self.d, self.store, self.lib, self.ws = dims, store, lib, workspace
        self._saved = None

    def apply(self, recordings, save_for_backward=True):
        d, p, lib, ws = self.d, self.store.p, self.lib, self.ws
        if not d.bottom_dims:
            return recordings
        T, B = int(recordings.shape[0]), int(recordings.shape[1])
        x = recordings.contiguous().view(T * B, d.F)
        saved = []
        for j, o in enumerate(d.bottom_dims):
            z = ws.get("bottom%d.z" % j, (T * B, o))
            lib.sgemm(x, p["/recognizer/bottom/bottom/linear_%d.W" % j], z, bias=p["/recognizer/bottom/bottom/linear_%d.b" % j])
            a = ws.get("bottom%d.a" % j, (T * B, o))
            lib.call("lvsr_act_fwd", lib.stream_for(a), self.ACT[d.bottom_act], native_ptr(z), o, T * B, o, native_ptr(a), o)
            saved.append((x, z))
            x = a
        if save_for_backward:
            self._saved = saved
        return x.view(T, B, d.bottom_dims[-1])

    def backward(self, d_out):
        d, p, g, lib, ws = self.d, self.store.p, self.store.g, self.lib, self.ws
        if not d.bottom_dims:
            return
        gws = ws.get("gemm_ws", (1 << 22,))
        da = d_out.contiguous().view(-1, d.bottom_dims[-1])
        n = int(da.shape[0])
        for j in reversed(range(len(d.bottom_dims))):
            x, z = self._saved[j]
            o = d.bottom_dims[j]
            dz = ws.get("bottom%d.dz" % j, (n, o))
            lib.call("lvsr_act_bwd", lib.stream_for(dz), self.ACT[d.bottom_act], native_ptr(z), o, native_ptr(da), o, n, o,
                     native_ptr(dz), o)
            W = "/recognizer/bottom/bottom/linear_%d.W" % j
            lib.sgemm(x, dz, g[W], transA=True, ws=gws)
            lib.colsum(dz, g["/recognizer/bottom/bottom/linear_%d.b" % j], ws=gws)
            if j > 0:
                dx = ws.get("bottom%d.dx" % j, (n, int(x.shape[1])))
                lib.sgemm(dz, p[W], dx, transB=True)
                da = dx


def native_ptr(t):
    from ..native import ptr
    return ptr(t)


class Encoder(object):
    # the persistent cluster kernels win while a cluster serves at most this many utterances (measured on MI355X, H = 256,
    # T = 800: 2.0 / 2.7 / 7.5 us per forward step at 1 / 2 / 4 utterances per cluster against 6.3 for the step kernels)
    PERSIST_MAX_ROWS = 2

    # per-GPU batches above this run the encoder in PASSES of at most this many utterances on the cluster kernels (utterances are
    # independent in the encoder); measured on MI355X: B = 128 as 2 x 64 instead of one pass on the step kernels
    PASS_ROWS = 64

    def __init__(self, dims, store, lib, workspace, use_graph=True, use_persistent=None, pfx="enc"):
        """use_persistent: True / False force the persistent cluster kernels (csrc/encoder_persist.hip) on or off (where
        the shape allows them); None (default) = on the GPU whenever a cluster serves at most PERSIST_MAX_ROWS utterances,
        otherwise two step kernels per time step."""
        # needs co-resident work-groups: the GPU, or the emulator with concurrent work-groups switched on (tests)
        can = not lib.is_emulator or lib.emulates_concurrency()
        self.persist_auto = use_persistent is None
        self.use_persistent = can and (not lib.is_emulator if use_persistent is None else bool(use_persistent))
        self.d = dims
        self.store = store
        self.lib = lib
        self.ws = workspace
        self.use_graph = use_graph
        self.pfx = pfx               # workspace-name prefix of the per-layer buffers ("enc"; the passes of a large batch: "enc.p<k>_")
        self._passes = []            # child encoders, one per pass (_apply_in_passes)
        self.force_passes = False    # tests: passes whatever kernels the children run on
        self._pass_cols = None
        self._saved = None
        self._packs = {}
        self._cats = {}
        self._pack_cache = {}
        # weight-gradient GEMMs on a second stream: measured SLOWER on MI355X (70.0 vs 66.4 ms per WSJ-base step: the
        # concurrent GEMM work-groups delay the latency-bound step kernels more than the overlap saves), so off by default
        # (round 3, persistent cluster kernels, groups flushed per layer on the second stream inside the step graph: 16.36 vs
        # 15.64 ms — the GEMM work-groups sharing the CUs slow the polling clusters by more than the 1.4 ms they hide)
        # (round 6, tools/probes/cu_partition_probe.py: the side stream created with hipExtStreamCreateWithCUMask on its own CUs and the
        # clusters on the others — eager launches only, a hipGraph kernel node has no CU-mask attribute: profiles/r06_cu_partition.md)
        self.overlap = False        # measured and rejected (comment above); the attribute keeps the second-stream code reachable for probes
        # A forward pass that saves for a backward pass clears the granule planes of ALL its persistent launches, the BPTT ones
        # included, in one launch in front of the first layer (`_clear_planes`; a memset node in front of every launch otherwise:
        # 8 x 4.7 us of a WSJ-base step).  False: every launch clears its own (what a pass that saves nothing always does).
        self.preclear = True
        self._side = None
        self._side_pending = False

    def _n(self, i, what):
        return "%s%d.%s" % (self.pfx, i, what)

    def _names(self, i, direction):
        base = "/recognizer/encoder/bidir%d/%s" % (i, direction)
        return dict(Wi=base + "/fork/fork_inputs.W", bi=base + "/fork/fork_inputs.b",
                    Wg=base + "/fork/fork_gate_inputs.W", bg=base + "/fork/fork_gate_inputs.b",
                    Whh=base + "/gatedrecurrent.state_to_state", Whg=base + "/gatedrecurrent.state_to_gates",
                    h0=base + "/gatedrecurrent.initial_state")

    def _packed(self, i):
        """Packed (MFMA operand order) copies of the recurrent weights of layer i.  All layers are refreshed together, in one
        library call, the first time a layer is asked for after the parameters changed (store.version)."""
        if self._packs.get("version") != self.store.version or self.lib.capturing:
            p, lib, ws = self.store.p, self.lib, self.ws
            packs, jobs = dict(version=self.store.version), []
            for li in range(self.d.n_layers):
                H = self.d.Hs[li]
                ent = dict(Whh=[], Whg=[], WhhT=[], WhgT=[])
                for di, direction in enumerate(("forward", "backward")):
                    n = self._names(li, direction)
                    for key, W, trans in (("Whh", p[n["Whh"]], False), ("Whg", p[n["Whg"]], False), ("WhhT", p[n["Whh"]], True)):
                        K, N = (W.shape[1], W.shape[0]) if trans else (W.shape[0], W.shape[1])
                        buf = ws.get("enc%d.%d.%s_p" % (li, di, key), (lib.pack_size(K, N),))
                        jobs.append((W, buf, trans))
                        ent[key].append(buf)
                    # state_to_gates^T as two (K=H,N=H) blocks: update rows, then reset rows
                    sz = lib.pack_size(H, H)
                    buf = ws.get("enc%d.%d.WhgT_p" % (li, di), (2 * sz,))
                    Wg = p[n["Whg"]]
                    jobs.append((Wg[:, :H], buf[:sz], True))
                    jobs.append((Wg[:, H:], buf[sz:], True))
                    ent["WhgT"].append(buf)
                packs[li] = ent
            lib.pack_many(jobs, use_graph=self.use_graph, cache=self._pack_cache)
            self._packs = packs
        return self._packs[i]

    def _fork_cat_pairs(self, i):
        """-> (entry of `_cats`, the copies that fill it): the four input-projection matrices of layer i side by side, (I, 6H) =
        [Wi_f | Wg_f | Wi_b | Wg_b] in the column order of `xg`, and their biases (6H): ONE GEMM per layer produces all input
        projections of both directions (and one its input gradient) instead of four."""
        p, ws = self.store.p, self.ws
        H, I = self.d.Hs[i], self.d.layer_input_dim(i)
        W = ws.get("enc%d.Wcat" % i, (I, 6 * H))
        b = ws.get("enc%d.bcat" % i, (6 * H,))
        pairs = []
        for di, direction in enumerate(("forward", "backward")):
            n = self._names(i, direction)
            o = di * 3 * H
            pairs += [(p[n["Wi"]], W[:, o: o + H]), (p[n["Wg"]], W[:, o + H: o + 3 * H]),
                      (p[n["bi"]], b[o: o + H]), (p[n["bg"]], b[o + H: o + 3 * H])]
        return dict(version=self.store.version, W=W, b=b), pairs

    def _fork_cat(self, i):
        """The concatenated fork weights and biases of layer i (`_fork_cat_pairs`), refreshed when the parameters changed (copies, no
        arithmetic)."""
        ent = self._cats.get(i)
        if ent is None or ent["version"] != self.store.version or self.lib.capturing:
            ent, pairs = self._fork_cat_pairs(i)
            self.lib.copy_many(pairs)                      # one launch instead of eight copy kernels
            self._cats[i] = ent
        return ent["W"], ent["b"]

    def _layer_inputs(self, m, T, B):
        """What the layers of a forward pass copy from the parameters and the input mask, in ONE launch in front of the first layer
        (a launch per layer and a copy kernel per subsampled mask before): the concatenated fork weights of every layer whose copy is
        stale (`_fork_cat`), and the mask of every subsampling layer's output — rows 0, s, 2s, ... of the input mask, s = the product of
        the subsampling factors so far.  -> [that mask or None] per layer."""
        d, ws = self.d, self.ws
        pairs = []
        for i in range(d.n_layers):
            ent = self._cats.get(i)
            if ent is None or ent["version"] != self.store.version or self.lib.capturing:
                self._cats[i], fresh = self._fork_cat_pairs(i)
                pairs += fresh
        masks, stride = [], 1
        for i, s in enumerate(d.subsample):
            T = (T + s - 1) // s
            stride *= s
            masks.append(None)
            if m is not None and s > 1:
                masks[i] = ws.get(self._n(i, "msub"), (T, B))
                pairs.append((m[::stride], masks[i]))
        self.lib.copy_many(pairs)
        return masks

    @contextlib.contextmanager
    def _side_stream(self):
        """Run the enclosed launches on the encoder's second stream (GPU only), ordered after everything already queued
        on the current stream; `join_side_stream()` orders the current stream after them.  Yields the split-K workspace to
        use inside (the two streams must not share one)."""
        if not self.overlap or self.lib.is_emulator or not torch.cuda.is_available():
            yield self.ws.get("gemm_ws", (1 << 22,))
            return
        cur = torch.cuda.current_stream()
        if self._side is None:
            self._side = torch.cuda.Stream(cur.device)
        self._side.wait_stream(cur)
        with torch.cuda.stream(self._side):
            yield self.ws.get("gemm_ws.side", (1 << 22,))
        self._side_pending = True

    def join_side_stream(self):
        if self._side is not None and self._side_pending:
            torch.cuda.current_stream().wait_stream(self._side)
            self._side_pending = False

    def _sync_ws(self, i, B, H, bwd=False):
        """Scratch of the persistent cluster kernel (granule planes + abort word), or None when the layer runs as
        per-step kernels (emulator, or a cluster that does not fit the chip).  bwd: a second one of the same size, the BPTT launch's
        own when the planes are cleared ahead of the step (epochs restart at 1 in every launch: a region cleared once serves one)."""
        if not self.use_persistent:
            return None
        nbytes = int(self.lib._lvsr_bigru_persist_ws_bytes(int(B), int(H)))
        if nbytes <= 0:
            return None
        if self.persist_auto and int(self.lib._lvsr_bigru_persist_rows(int(B), int(H))) > self.PERSIST_MAX_ROWS:
            return None
        return self.ws.get(self._n(i, "sync_bwd" if bwd else "sync"), ((nbytes + 3) // 4,), torch.int32)

    def _clear_planes(self, B):
        """-> {layer: the BPTT launch's workspace} of the layers that run on the persistent kernels, after ONE launch that zeroes
        both workspaces of each behind their first 256 bytes (the sticky abort word).  Nothing else touches them until their launch."""
        own, ranges = {}, []
        for i, H in enumerate(self.d.Hs):
            fwd = self._sync_ws(i, B, H)
            if fwd is not None:
                own[i] = self._sync_ws(i, B, H, bwd=True)
                ranges += [(t.data_ptr() + 256, t.numel() * 4 - 256) for t in (fwd, own[i])]
        if ranges:
            self.lib.clear_many(ranges, own[min(own)])
        return own

    def check_persistent(self):
        """After a synchronisation point: raise if a persistent kernel gave up waiting for its cluster.  The abort word is sticky
        (no launch clears it: a forward cluster that gave up is still reported after the backward pass and after replayed steps, and
        every later launch on the workspace leaves at once); it is cleared here, when the failure has been reported."""
        for k, t in self.ws._bufs.items():
            if k[0].startswith("enc") and k[0].endswith((".sync", ".sync_bwd")) and int(t[0]) != 0:
                t[:64].zero_()
                raise RuntimeError("persistent BiGRU kernel aborted (a work-group of the cluster was not scheduled); results since "
                                   "the last check are invalid")

    # ---- large per-GPU batches: the encoder in passes ---------------------------------------------------------------------
    def _pass_columns(self, B):
        """[(first, last + 1)] utterance columns of the passes, or None when the batch runs in one piece.  Utterances are
        independent in the encoder, so a batch the cluster kernels cannot hold at once (more than PERSIST_MAX_ROWS utterances per
        cluster) runs as ceil(B / PASS_ROWS) passes on them instead of as one pass on the step kernels (round-4 verdict item 8:
        B = 128 78.2 ms on the step kernels against 2 x 29.0 ms at B = 64)."""
        if B <= self.PASS_ROWS or self.pfx != "enc":
            return None
        if not self.force_passes:
            if not (self.persist_auto and self.use_persistent):
                return None
            H = max(self.d.Hs)
            if int(self.lib._lvsr_bigru_persist_ws_bytes(int(B), int(H))) > 0 and \
                    int(self.lib._lvsr_bigru_persist_rows(int(B), int(H))) <= self.PERSIST_MAX_ROWS:
                return None                         # the clusters hold the whole batch
        n = (B + self.PASS_ROWS - 1) // self.PASS_ROWS
        per = (B + n - 1) // n
        return [(lo, min(B, lo + per)) for lo in range(0, B, per)]

    def _pass_encoder(self, k):
        while len(self._passes) <= k:
            child = Encoder(self.d, self.store, self.lib, self.ws, use_graph=self.use_graph, use_persistent=None,
                            pfx="enc.p%d_" % len(self._passes))
            child._cats = self._cats                     # one concatenated copy of the fork weights for all passes
            self._passes.append(child)
        return self._passes[k]

    @staticmethod
    def _cols2d(t, lo, hi):
        """Columns [lo, hi) of a time-major (T, B[, F]) tensor as a 2-D strided view (T, (hi - lo) * F) for lvsr_copy2d_many."""
        T, B = int(t.shape[0]), int(t.shape[1])
        F = int(t.numel() // max(1, T * B))
        return t.view(T, B * F)[:, lo * F: hi * F]

    def _apply_in_passes(self, cols, input_, mask, save_for_backward):
        d, lib, ws = self.d, self.lib, self.ws
        T, B = int(input_.shape[0]), int(input_.shape[1])
        F = int(input_.shape[2])
        x = input_.contiguous()
        m = None if mask is None else mask.contiguous()
        enc = msk = None
        for k, (lo, hi) in enumerate(cols):
            child = self._pass_encoder(k)
            xk = ws.get(child.pfx + ".x", (T, hi - lo, F))
            pairs = [(self._cols2d(x, lo, hi), xk.view(T, (hi - lo) * F))]
            mk = None
            if m is not None:
                mk = ws.get(child.pfx + ".m", (T, hi - lo))
                pairs.append((self._cols2d(m, lo, hi), mk))
            lib.copy_many(pairs)
            ek, emk = child.apply(xk, mk, save_for_backward=save_for_backward)
            if enc is None:
                Te, E = int(ek.shape[0]), int(ek.shape[2])
                enc = ws.get("enc.passes.encoded", (Te, B, E))
                msk = ws.get("enc.passes.mask", (Te, B))
            lib.copy_many([(ek.view(Te, (hi - lo) * E), self._cols2d(enc, lo, hi)), (emk, self._cols2d(msk, lo, hi))])
        if save_for_backward:            # (a forward that saves nothing leaves the branch backward() will take alone)
            self._pass_cols = cols
            self._saved = None
        return enc, msk

    def _encoder_gradient_range(self):
        """(first, count) of the encoder's gradients in the flat gradient buffer (contiguous: spec.parameter_shapes order)."""
        offs = self.store.offsets
        mine = [(o, n) for k, (o, n) in offs.items() if k.startswith("/recognizer/encoder/")]
        lo, hi = min(o for o, n in mine), max(o + (n + 3) // 4 * 4 for o, n in mine)
        assert all(k.startswith("/recognizer/encoder/") == (lo <= o < hi) for k, (o, n) in offs.items()), "encoder parameters are not one range"
        return lo, min(hi, self.store.grad.numel()) - lo

    def _backward_in_passes(self, cols, d_encoded, need_input_grad, group=None):
        """Every pass writes its own encoder gradients (the kernels and products overwrite); they are summed in a side buffer
        between the passes (lvsr_copy2d_many with beta = 1).  Every pass ends with a grouped launch of its own; what the caller's
        `group` already holds (the decoder's weight-gradient products) goes out with the first pass."""
        d, lib, ws = self.d, self.lib, self.ws
        dy = d_encoded.contiguous()
        Te, B, E = int(dy.shape[0]), int(dy.shape[1]), int(dy.shape[2])
        first, count = self._encoder_gradient_range()
        genc = self.store.grad[first: first + count]
        acc = ws.get("enc.passes.gacc", (count,))
        dx = None
        if group is None:
            group = lib.group()
        for k, (lo, hi) in enumerate(cols):
            child = self._passes[k]
            dk = ws.get(child.pfx + ".dy", (Te, hi - lo, E))
            lib.copy_many([(self._cols2d(dy, lo, hi), dk.view(Te, (hi - lo) * E))])
            dxk = child.backward(dk, need_input_grad=need_input_grad, group=group)
            group.flush(ws.get("gemm_ws.grouped", (1 << 26,)))
            child.finish_backward()
            if need_input_grad:
                if dx is None:
                    dx = ws.get("enc.passes.dx", (int(dxk.shape[0]), B, int(dxk.shape[2])))
                lib.copy_many([(dxk.view(int(dxk.shape[0]), -1), self._cols2d(dx, lo, hi))])
            if k + 1 < len(cols):
                lib.copy_many([(genc, acc, 0.0 if k == 0 else 1.0)])
            else:
                lib.copy_many([(acc, genc, 1.0)])
        self._scatter = []
        return dx

    def apply(self, input_, mask=None, save_for_backward=True):
        """input_ (T,B,F) fp32, mask (T,B) fp32 or None -> encoded (T',B,2H_last), encoded_mask (T',B)."""
        d, p, lib, ws = self.d, self.store.p, self.lib, self.ws
        T, B = int(input_.shape[0]), int(input_.shape[1])
        cols = self._pass_columns(B)
        if cols is not None:
            return self._apply_in_passes(cols, input_, mask, save_for_backward)
        if save_for_backward:
            self._pass_cols = None
        x = input_.contiguous()
        m = None if mask is None else mask.contiguous()
        saved = []
        gemm_ws = ws.get("gemm_ws", (1 << 22,))
        # a pass that saves for a backward pass (the training step) copies and clears for all its layers in front of the first;
        # any other caller (analyze, generate, decoding) issues the per-layer launches it always did
        msubs = self._layer_inputs(m, T, B) if save_for_backward else None
        cleared = self._clear_planes(B) if self.preclear and save_for_backward else {}
        for i, (H, s) in enumerate(zip(d.Hs, d.subsample)):
            I = d.layer_input_dim(i)
            Ts = (T + s - 1) // s
            xg = ws.get(self._n(i, "xg"), (T, B, 6 * H))
            y = ws.get(self._n(i, "y"), (T, B, 2 * H))
            ysub = y if s == 1 else ws.get(self._n(i, "ysub"), (Ts, B, 2 * H))
            u = ws.get(self._n(i, "u"), (T, B, 2 * H))
            r = ws.get(self._n(i, "r"), (T, B, 2 * H))
            c = ws.get(self._n(i, "c"), (T, B, 2 * H))
            rh = ws.get(self._n(i, "rh"), (T, B, 2 * H))
            x2, xg2 = x.view(T * B, I), xg.view(T * B, 6 * H)
            sync = self._sync_ws(i, B, H)
            pk = self._packed(i) if sync is None else None     # the persistent kernels read the plain weights
            Wcat, bcat = (self._cats[i]["W"], self._cats[i]["b"]) if msubs is not None else self._fork_cat(i)
            lib.sgemm(x2, Wcat, xg2, bias=bcat)          # all input projections of the layer, both directions
            h0s = [p[self._names(i, direction)["h0"]] for direction in ("forward", "backward")]
            if sync is not None:      # persistent cluster kernel: reads the plain weights and shards them into LDS itself
                nf, nb = self._names(i, "forward"), self._names(i, "backward")
                Whh, Whg = [p[nf["Whh"]], p[nb["Whh"]]], [p[nf["Whg"]], p[nb["Whg"]]]
            else:
                Whh, Whg = [pk["Whh"][0], pk["Whh"][1]], [pk["Whg"][0], pk["Whg"][1]]
            # (a persistent layer is a memset + one launch: no graph to build, and no host wait for a time-loop graph to drain)
            lib.run("lvsr_bigru_fwd", "lvsr_bigru_fwd_args", y, self.use_graph and sync is None, xg=xg, mask=m, Whh_p=Whh, Whg_p=Whg, h0=h0s,
                    y=y, ysub=(ysub if s > 1 else None), u=u, r=r, c=c, rh=rh, sub=s, T=T, B=B, H=H,
                    persistent=(0 if sync is None else 5 if i in cleared else 1), sync_ws=sync)
            saved.append(dict(x=x, mask=m, T=T, y=y, u=u, r=r, c=c, rh=rh, sync_bwd=cleared.get(i)))
            x = ysub
            if m is not None and s > 1:
                if msubs is not None:
                    m = msubs[i]
                else:
                    mm = ws.get(self._n(i, "msub"), (Ts, B))
                    mm.copy_(m[::s])
                    m = mm
            T = Ts
        if m is None:
            m = ws.get(self.pfx + ".ones_mask", (T, B))
            m.fill_(1.0)
        if save_for_backward:
            self._saved = saved
        return x, m

    def backward(self, d_encoded, need_input_grad=False, group=None):
        """d_encoded (T',B,2H_last): gradient wrt `encoded`.  Writes the encoder parameter gradients; returns the gradient
        wrt the encoder input when `need_input_grad` (a bottom MLP sits in front), else None.  With a `group` (native.GemmGroup)
        the recurrent weight-gradient products and the fork column sums join it: the caller flushes it and then calls
        finish_backward().  Without one everything launches here."""
        d, p, g, lib, ws = self.d, self.store.p, self.store.g, self.lib, self.ws
        if self._pass_cols is not None:
            return self._backward_in_passes(self._pass_cols, d_encoded, need_input_grad, group)
        assert self._saved is not None, "apply() must run first"
        gemm_ws = ws.get("gemm_ws", (1 << 22,))
        self._scatter = []
        h0_sums = []          # (dh, Bp, H, dh0 forward, dh0 backward) of the persistent layers: summed in one launch behind the loop
        dy = d_encoded.contiguous()
        B = int(dy.shape[1])
        for i in reversed(range(d.n_layers)):
            H, s, I = d.Hs[i], d.subsample[i], d.layer_input_dim(i)
            sv = self._saved[i]
            T = sv["T"]
            dxg = ws.get(self._n(i, "dxg"), (T, B, 6 * H))
            Bp = (B + 15) // 16 * 16
            dh_ws = ws.get(self._n(i, "dh"), (12 * Bp * H,))
            nf, nb = self._names(i, "forward"), self._names(i, "backward")
            sync = self._sync_ws(i, B, H)
            # planes the forward pass cleared for this launch: good for ONE launch (a second backward() clears its own)
            own = sv.pop("sync_bwd", None) if sync is not None else None
            if own is not None:
                sync = own
            pk = self._packed(i) if sync is None else None
            if sync is not None:
                WhhT, WhgT = [p[nf["Whh"]], p[nb["Whh"]]], [p[nf["Whg"]], p[nb["Whg"]]]
            else:
                WhhT, WhgT = [pk["WhhT"][0], pk["WhhT"][1]], [pk["WhgT"][0], pk["WhgT"][1]]
            lib.run("lvsr_bigru_bwd", "lvsr_bigru_bwd_args", dxg, self.use_graph and sync is None, mask=sv["mask"], y=sv["y"],
                    u=sv["u"], r=sv["r"], c=sv["c"], WhhT_p=WhhT, WhgT_p=WhgT, h0=[p[nf["h0"]], p[nb["h0"]]], dy=dy,
                    dxg=dxg, dh_ws=dh_ws, dh0=[g[nf["h0"]], g[nb["h0"]]], sub=s, T=T, B=B, H=H,
                    persistent=(0 if sync is None else 7 if own is not None else 3), sync_ws=sync)
            if sync is not None:      # (every layer has a dh workspace of its own: nothing overwrites it before the sum)
                h0_sums.append((dh_ws, Bp, H, g[nf["h0"]], g[nb["h0"]]))
            x2 = sv["x"].view(T * B, I)
            dxg2 = dxg.view(T * B, 6 * H)
            y2 = sv["y"].view(T * B, 2 * H)
            rh2 = sv["rh"].view(T * B, 2 * H)
            dx = None
            if i > 0 or need_input_grad:
                dx = ws.get(self._n(i, "dx"), (T, B, I))
            # critical path first: the gradient wrt this layer's input is what the next (lower) layer's recurrence waits for
            if dx is not None:      # the concatenated copy the forward pass of this step made (parameters have not moved since)
                lib.sgemm(dxg2, self._cats[i]["W"], dx.view(T * B, I), transB=True)
            # weight gradients are off the critical path; with `self.overlap = True` they go to a second stream and overlap the next
            # layer's recurrence (see __init__ for why this is not the default)
            with self._side_stream() as side_ws:
                wgrad, colsum = lib.weight_grad_calls(group, side_ws)
                for di, direction in enumerate(("forward", "backward")):
                    n = self._names(i, direction)
                    dc = dxg2[:, di * 3 * H: di * 3 * H + H]
                    dg = dxg2[:, di * 3 * H + H: di * 3 * H + 3 * H]
                    hcol = slice(di * H, (di + 1) * H)
                    wgrad(rh2[:, hcol], dc, g[n["Whh"]])
                    if T > 1:
                        if di == 0:     # h_{t-1} = y[t-1]
                            wgrad(y2[: (T - 1) * B, hcol], dg[B:], g[n["Whg"]])
                        else:           # backward direction: previous state in scan order is y[t+1]
                            wgrad(y2[B:, hcol], dg[: (T - 1) * B], g[n["Whg"]])
                        beta = 1.0
                    else:
                        beta = 0.0
                    # the first scan step starts from the (broadcast) initial state: rank-B update with lda = 0, onto the product above
                    first = dg[:B] if di == 0 else dg[(T - 1) * B:]
                    if group is not None:
                        group.add_after(p[n["h0"]], first, g[n["Whg"]], beta=beta, M=H, K=B, lda=0)
                    else:
                        lib.sgemm(p[n["h0"]], first, g[n["Whg"]], transA=True, beta=beta, M=H, K=B, lda=0)
                # fork gradients of both directions: one (I, 6H) product and one column sum, scattered into the four matrices
                gW = ws.get("enc%d.gWcat" % i, (I, 6 * H))
                gb = ws.get("enc%d.gbcat" % i, (6 * H,))
                # (not a member of the grouped launch: with 48 output tiles it fills the chip alone, and the group's common ~1024-deep
                # k-chunks would cost it 13 instead of 5 partial copies of its 3 MB output; as a member with a depth of its own it
                # measured 886 us for the one launch against 381 + 528 us apart — nothing)
                lib.sgemm(x2, dxg2, gW, transA=True, ws=side_ws)
                colsum(dxg2, gb)
                for di, direction in enumerate(("forward", "backward")):
                    n = self._names(i, direction)
                    o = di * 3 * H
                    self._scatter += [(gW[:, o: o + H], g[n["Wi"]]), (gW[:, o + H: o + 3 * H], g[n["Wg"]]),
                                      (gb[o: o + H], g[n["bi"]]), (gb[o + H: o + 3 * H], g[n["bg"]])]
                if self.overlap and group is not None:
                    # second-stream probes: the grouped products collected so far (this layer's, and — for the top layer — the
                    # decoder's) run NOW on the side stream, beside the next layer's recurrence, not in one launch at the end
                    group.flush(ws.get("gemm_ws.grouped.side", (1 << 26,)))
            dy = dx
        if h0_sums:
            arr = (lib.structs["lvsr_h0_desc"] * len(h0_sums))()
            for e, (dh, Bp, H, out_f, out_b) in zip(arr, h0_sums):
                e.dh, e.out_f, e.out_b, e.Bp, e.B, e.H = dh.data_ptr(), out_f.data_ptr(), out_b.data_ptr(), Bp, B, H
            lib.call("lvsr_bigru_h0_many", lib.stream_for(h0_sums[0][0]), arr, len(h0_sums))
        self.join_side_stream()
        if group is None:      # nothing was deferred: the fork gradients are there
            self.finish_backward()
        return dy

    def finish_backward(self):
        """Scatter the concatenated fork gradients of all layers into the four parameters each (one launch per 64 pieces).
        backward(group=...) leaves this to its caller: it must follow the group's flush, which runs the fork column sums."""
        self.lib.copy_many(self._scatter)
        self._scatter = []
