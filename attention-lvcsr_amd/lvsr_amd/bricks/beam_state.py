"""Device state of one set of G >= 1 beam searches of beam K (csrc/beam.hip): the buffers, the argument blocks of the launches of
a position, the key of the step graph, and the launches themselves.  `SequenceGenerator.beam_begin` makes one per search set over
the contexts `init_generation` left; `lvsr_amd/search.py` drives it.  A single search (G = 1) and a batch differ only in kernel
arguments: broadcast context strides and `group_rows = 0` against `groups` / `group_Tp` with every search's own limit in its
control block, the merge products through `lvsr_readout_merge` (`force_merge`, or from `MERGE_ROWS` rows on), `lvsr_fst_lm_step`
against `lvsr_fst_lm_step_groups`, the history capacity rounded up to a multiple of 32 for a batch.  The bookkeeping buffers carry
the group dimension either way.  A generator serves one search set at a time — contexts and workspace buffers are shared — so
`beam_begin` stamps its state as the generator's `current_search` and every launch of an older state raises.  The graph regions
stay with the generator: captured graphs survive from search to search."""
import ctypes

import numpy
import torch

from ..native import ptr

# words of a search's control block (csrc/beam.hip); limit: the search's own position limit (batched searches), reuse: raised by
# the select launch when pass B's glimpses would repeat pass A's row by row, reused: the positions at which that happened
CTL = dict(nlive=0, pos=1, done=2, nfin=3, patience=4, nsel=5, err=6, steps=7, limit=8, reuse=9, reused=10)
CTL_WORDS = 16
HOST_TABLES = ("fin_pos", "fin_col", "hist_parent", "hist_char", "hist_cost")      # what following the back-pointers reads


class BeamState(object):
    def __init__(self, gen, K, eol, max_length, ignore_first_eol=False, char_discount=0.0, round_to_inf=1e9, stop_on="patience",
                 force_merge=False):
        """Allocate (once per (K, G, T', max_length)) and reset the state: hypothesis 0 of every search = initial state / initial
        glimpses (search.py:287-299), every other row a copy.  After `init_generation` on a batch of N utterances: N searches side
        by side (`max_length` = one limit per utterance), search g in rows [g K, g K + K) of every state buffer and block g of the
        bookkeeping buffers (lvsr_beam_args.groups).  `force_merge`: the readout's merge products through lvsr_readout_merge
        whatever the number of rows (every batched decode, so that an utterance's hypotheses do not depend on how many others share
        its launches: a row of that kernel is summed in the same order in any batch)."""
        d, p, n_, lib, ws, g = gen.d, gen.store.p, gen.n, gen.lib, gen.ws, gen._gen
        lm = gen.language_model
        on_dev_lm = lm is not None and lm.on_device
        G = int(g.get("N", 1))
        limits = None
        if G > 1:
            limits = [int(m) for m in max_length]
            assert len(limits) == G
            assert lm is None or on_dev_lm, "batched search: language model on the device"
            # capacity of the history buffers (and part of the step graph's key): the largest limit, rounded up so that batches of
            # slightly different lengths share buffers and graph; every search stops at its own limit (ctl word `limit`)
            max_length, force_merge = (max(limits) + 31) // 32 * 32, True
        max_length = int(max_length)
        Tp, R = g["Tp"], K * G                   # R rows of the state buffers
        tag = ".K%d" % K if G == 1 else ".K%dx%d" % (K, G)
        i32, i64, f64 = torch.int32, torch.int64, torch.float64
        fin_cap = 2 * K if stop_on == "patience" else K * (max_length + 1)
        pos_needed = gen._pos_needed()
        SW = gen._state_width()
        stacked = d.n_dec > 1          # bricks/generator_stack.py: pass B is the attention block and one GRU block per layer

        def attbufs(which, fork):
            t = tag + which
            return gen._attdec_bufs("bs.", t, 1, R, Tp, xg=ws.get("bs.xg" + t, (R, 3 * d.D)) if fork else None, ymask=None)

        def buf(name, *shape, **kw):
            return ws.get("bs." + name + tag, shape, kw.get("dtype", torch.float32))
        self.gen, self.K, self.rows, self.groups, self.Tp, self.max_length, self.limits = gen, K, R, G, Tp, max_length, limits
        self.fin_cap, self.stop_on, self.on_dev_lm = fin_cap, stop_on, on_dev_lm
        A_, B_ = self.A, self.B = attbufs("a", False), attbufs("b", True)
        self.ctl, self.fctl = buf("ctl", G, CTL_WORDS, dtype=i32), buf("fctl", G, 4)
        self.neglogp, self.running, self.live_col = buf("neglogp", R, d.V), buf("running", R), buf("live_col", R, dtype=i32)
        self.hist_parent, self.hist_char = buf("hist_parent", G, max_length, K, dtype=i32), buf("hist_char", G, max_length, K, dtype=i32)
        self.hist_cost = buf("hist_cost", G, max_length, K)
        self.fin_pos, self.fin_col = buf("fin_pos", G, fin_cap, dtype=i32), buf("fin_col", G, fin_cap, dtype=i32)
        self.fin_cost, self.fin_score = buf("fin_cost", G, fin_cap), buf("fin_score", G, fin_cap)
        self.keep, self.chars, self.parents = buf("keep", R, dtype=i32), buf("chars", R, dtype=i64), buf("parents", R, dtype=i32)
        self.fb = buf("fb", R, d.FB) if d.embed else None
        L = self.lm = {}               # the language model's rows: look-ahead costs, and with the device walk the state sets
        if lm is not None:
            L["add_live"] = buf("lm_add_live", R, d.V)
            if on_dev_lm:
                L.update(states_live=buf("lm_sl", R, 7, dtype=i64), weights_live=buf("lm_wl", R, 7, dtype=f64),
                         states_sel=buf("lm_ss", R, 7, dtype=i64), weights_sel=buf("lm_ws", R, 7, dtype=f64),
                         states_new=buf("lm_sn", R, 7, dtype=i64), weights_new=buf("lm_wn", R, 7, dtype=f64),
                         add_new=buf("lm_add_new", R, d.V))
        pk = gen._packed()
        # window centres travel with the rows (select / compact move them), so neither pass recomputes slot 0: phases bit 2
        skip_pos = 4 if pos_needed else 0
        grp = dict(groups=G, group_Tp=g["lengths"]) if G > 1 else {}
        fa = gen._attdec_fields(pk, g["A"], g["PA"], g["Am"], 1, R, A_, phases=1 | skip_pos, step0=0, broadcast=True, **grp)
        words = self.ctl.view(-1)
        pos_word = words[CTL["pos"]:]
        self.argsA = lib.make("lvsr_attdec_args", step_dev=pos_word, **fa)
        self.argsB = self.stepB = None
        if stacked:
            self.stepB = gen._beam_step_blocks(pk, g, R, B_, skip_pos, pos_word, tag, **grp)
        else:
            fb_ = gen._attdec_fields(pk, g["A"], g["PA"], g["Am"], 1, R, B_, phases=3 | skip_pos, step0=-1, broadcast=True, **grp)
            # runs after the select kernel moved the position counter on: step0 = -1; skipped where the select launch raised the
            # search's `reuse` word (and copied pass A's glimpses): lvsr_beam_args.WA_live
            self.argsB = lib.make("lvsr_attdec_args", step_dev=pos_word, skip=words[CTL["reuse"]:], skip_stride=CTL_WORDS, **fb_)
        host_fork = d.embed or stacked      # the fork of the chosen characters as separate launches of pass B
        pos = (lambda bufs, slot: bufs["pos"][slot]) if pos_needed else (lambda bufs, slot: None)
        self.args = lib.make(
            "lvsr_beam_args", K=K, groups=G, V=d.V, eol=int(eol), ignore_first_eol=int(bool(ignore_first_eol)),
            stop_on={"patience": 0, "optimistic_future_cost": 1}[stop_on], max_length=max_length, fin_cap=fin_cap, D=SW, Tp=Tp,
            round_to_inf=float(numpy.float32(min(float(round_to_inf), 3.0e38))), char_discount=float(char_discount),
            ctl=self.ctl, fctl=self.fctl, neglogp=self.neglogp, running=self.running, live_col=self.live_col,
            hist_parent=self.hist_parent, hist_char=self.hist_char, hist_cost=self.hist_cost, fin_pos=self.fin_pos,
            fin_col=self.fin_col, fin_cost=self.fin_cost, fin_score=self.fin_score, keep=self.keep, chars=self.chars,
            parents=self.parents, S_live=A_["S"][0], W_live=A_["W"][0], S_sel=B_["S"][0], W_sel=B_["W"][0],
            lm_states_live=L.get("states_live"), lm_weights_live=L.get("weights_live"), lm_states_sel=L.get("states_sel"),
            lm_weights_sel=L.get("weights_sel"), S_new=B_["S"][1], W_new=B_["W"][1], S_live_out=A_["S"][0], W_live_out=A_["W"][0],
            lm_states_new=L.get("states_new"), lm_weights_new=L.get("weights_new"), lm_add_new=L.get("add_new"),
            lm_states_live_out=L.get("states_live"), lm_weights_live_out=L.get("weights_live"),
            lm_add_live_out=L.get("add_live") if on_dev_lm else None,
            pos_live=pos(A_, 0), pos_sel=pos(B_, 0), pos_new=pos(B_, 1), pos_live_out=pos(A_, 0),
            # one-hot feedback: the fork of the chosen characters is a row gather the select launch does itself
            fork_xg=None if host_fork else B_["xg"], fork_Wi=None if host_fork else p[n_["Wfi"]],
            fork_Wg=None if host_fork else p[n_["Wfg"]], fork_bi=None if host_fork else p[n_["bfi"]],
            fork_bg=None if host_fork else p[n_["bfg"]], fork_rows=0 if host_fork else d.FB,
            **({} if stacked else dict(WA_live=A_["WA"][0], WA_sel=B_["WA"][0], W1_live=A_["W"][1], W1_sel=B_["W"][1], E=d.E,
                                       pos1_live=pos(A_, 1), pos1_sel=pos(B_, 1))))
        # many rows (batched search): the merge products as 16-row tiles in a launch of their own (lvsr_readout_merge)
        R1 = buf("R1", R, d.P) if (R >= gen.MERGE_ROWS or force_merge) else None
        self.merge = None
        if R1 is not None:
            ro = gen._readout_packs()
            self.merge = (ptr(A_["S"][0]), int(A_["S"][0].stride(0)), ptr(A_["WA"][0]), int(A_["WA"][0].stride(0)), R, SW, d.E, d.P,
                          ptr(ro["Wms"]), ptr(ro["Wmw"]), ptr(p[n_["bpm"]] if d.post_merge else p[n_["bro"]]), ptr(R1), int(R1.stride(0)))
        self.readout = gen._readout_step_args(A_["S"][0], A_["WA"][0], R, neglogp=self.neglogp, lm_add=L.get("add_live"), R1=R1)
        # ---- reset: one live hypothesis per search, replicated over its K rows
        ctl0 = numpy.zeros((G, CTL_WORDS), numpy.int32)
        ctl0[:, CTL["nlive"]], ctl0[:, CTL["patience"]] = 1, -1
        if G > 1:
            ctl0[:, CTL["limit"]] = limits
        self.ctl.copy_(torch.from_numpy(ctl0))
        self.fctl.copy_(torch.tensor([1000.0, 0.0, 0.0, 0.0]).repeat(G, 1))
        self.running.zero_()
        self.live_col.zero_()
        A_["S"][0].copy_(gen._initial_state().unsqueeze(0).expand(R, SW))
        A_["W"][0].zero_()
        if d.conv:
            A_["W"][0][:, 0] = 1.0
        if pos_needed:
            A_["pos"].zero_()         # centre of the initial glimpses [1, 0, ...]: mean 0, no median crossing -> 0
        if on_dev_lm:
            first = lm.initial_states(R)
            L["states_live"].copy_(first["states"])
            L["weights_live"].copy_(first["weights"])
            L["add_live"].copy_(first["add"])
        # everything the captured launches depend on belongs to the key: the language model's weighting and normalisation flags are
        # kernel arguments of the readout, its tables and error word are pointers inside the FST walk's argument block
        lm_key = None if lm is None else (float(lm.lm_weight), float(lm.am_beta), tuple(bool(v) for v in lm.norm), float(getattr(lm, "no_transition_cost", 0.0)))
        lm_ptrs = () if not on_dev_lm else tuple(sorted((k, t.data_ptr()) for k, t in lm._dev.items())) + (lm._err.data_ptr(),)
        self.key = ("beam_step", K, G, Tp, max_length, stop_on, int(bool(ignore_first_eol)), int(eol), float(char_discount),
                    float(round_to_inf), lm is not None, on_dev_lm, lm_key, R1 is not None, gen.criterion)
        self.volatile = (g["A"].data_ptr(), g["PA"].data_ptr(), g["Am"].data_ptr(), ws.generation, id(pk), gen.store.version, lm_ptrs)

    def check_current(self):
        """Raise if the generator has begun another search set since: this one's buffers and contexts are no longer its own."""
        if self.gen.current_search is not self:
            raise RuntimeError("beam search: the generator has begun another search since this one (a generator serves one search "
                               "set at a time: contexts and workspace buffers are shared); this search cannot go on")

    # ---- the launches of a position ---------------------------------------------------------------------------------------
    def costs(self):
        """Pass A of a position: glimpses of the live hypotheses -> readout -> step costs `neglogp` (rows,V)
        (logprobs_computer, search.py:126-134; with a language model ShallowFusionReadout + LMEmitter)."""
        self.check_current()
        lib = self.gen.lib
        lib.call("lvsr_attdec_fwd", lib.stream_for(self.A["S"]), ctypes.byref(self.argsA), 0)
        if self.merge is not None:
            lib.call("lvsr_readout_merge", lib.stream_for(self.neglogp), *self.merge)
        lib.call("lvsr_readout_step", lib.stream_for(self.neglogp), ctypes.byref(self.readout))

    def select(self):
        """Stopping rules, the beam_size best continuations, finished hypotheses, back-pointers; gathers the rows of pass B."""
        self.check_current()
        self.gen.lib.call("lvsr_beam_select", self.gen.lib.stream_for(self.ctl), ctypes.byref(self.args))

    def advance(self):
        """Pass B: glimpses AGAIN on the re-arranged hypotheses (the window of the location prior depends on the batch it is
        computed for) + compute_states with the chosen characters (next_state_computer, search.py:112-124), language-model
        transition, then the surviving rows become the new beam."""
        self.check_current()
        gen, lib = self.gen, self.gen.lib
        # (The language-model walk and pass B need nothing of each other.  Side by side on two streams — two branches of the step's
        # graph — they were slower, 0.94 -> 1.12 ms per utterance at 64 x 4: a fork and a join per position cost more than the 18 us
        # of pointer chasing they take off the chain; serial.)
        if self.stepB is not None:
            gen._beam_step_run(self)
        else:
            if gen.d.embed:          # lookup feedback needs the fork's GEMMs; one-hot feedback was gathered by the select launch
                gen._feedback_forks(self.chars, self.rows, [(gen.n, self.B["xg"])], self.fb)
            lib.call("lvsr_attdec_fwd", lib.stream_for(self.B["S"]), ctypes.byref(self.argsB), 0)
        if self.on_dev_lm:
            # language-model transition on the chosen characters + look-ahead costs of the new state sets (lvsr_fst_lm_step*)
            L, lm = self.lm, gen.language_model
            grouped = self.groups > 1       # the rows of finished searches are skipped (their characters are stale)
            args = [ctypes.byref(lm._fst), ptr(L["states_sel"]), ptr(L["weights_sel"]), ptr(self.chars), self.rows, ptr(L["states_new"]),
                    ptr(L["weights_new"]), ptr(L["add_new"]), ptr(lm._err)] + ([ptr(self.ctl), self.K] if grouped else [])
            lib.call("lvsr_fst_lm_step_groups" if grouped else "lvsr_fst_lm_step", lib.stream_for(L["states_sel"]), *args)
        lib.call("lvsr_beam_compact", lib.stream_for(self.ctl), ctypes.byref(self.args))

    def steps(self, n=1):
        """n consecutive positions as ONE replayed hipGraph (the position counter lives on the device, so the graph does not
        depend on where the search stands; captured on the second run of a search shape): the driver looks at the control block
        every n positions anyway."""
        self.check_current()
        gen = self.gen

        def enqueue():
            for _ in range(n):
                self.costs()
                self.select()
                self.advance()
        key = self.key if n == 1 else (self.key, "x%d" % n)
        gen.lib.region(gen, key, self.ctl, enabled=gen.use_graph, volatile=self.volatile, drain=False).run(enqueue)
