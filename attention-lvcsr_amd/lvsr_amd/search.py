"""Beam search driver over the device-resident beam step (csrc/beam.hip, bricks/beam_state.py `BeamState`).

The reference's `BeamSearch.search` (libs/blocks/blocks/search.py:244-407, as modified by lvsr) is a host loop around two
compiled functions; here the whole position — step costs of every continuation, choice of the `beam_size` best, finished
hypotheses, stopping rules, next states, language-model transition — is device work replayed as one hipGraph, and the
host's part shrinks to: start the search, replay steps, look at the `done` word every few steps, and at the end follow the
back-pointers of the finished hypotheses.  The RESULT (hypotheses, costs, the CandidateNotFoundError contract) is what has
to agree with the reference, bit for bit on its golden fixtures; the rules that produce it are listed in csrc/beam.hip.

Two things need the host inside the loop and switch the driver to one synchronisation per position: a
`validate_solution_function` (a Python callback that may veto a finished hypothesis, search.py:372-374) and a language
model whose walk runs on the host (`FSTLanguageModel` without the device tables).
"""
import numpy
import torch

from .bricks.beam_state import CTL, HOST_TABLES

POLL_EVERY = 8          # positions between two looks at the `done` word (a look is the only host<->device round trip)
STOP_ON = ("patience", "optimistic_future_cost")


class CandidateNotFoundError(Exception):
    """search.py:15-16"""


# what a search raises in place of a result (`_raise_device_errors`, `_collect`); a batch reports them utterance by utterance
SEARCH_ERRORS = (CandidateNotFoundError, AssertionError, RuntimeError, UnboundLocalError)


class SearchRun(object):
    """Handle of a set of searches in flight (`BeamSearch.begin` / `begin_batch`): its device state, how far it has been driven,
    and the last look at the control blocks (`ctl`, through the pinned block `host` and `event` on a GPU)."""
    def __init__(self, state, limits, host, first_token, char_discount):
        self.state, self.limits, self.host, self.first_token, self.char_discount = state, limits, host, first_token, char_discount
        self.max_length = max(limits)                 # positions to enqueue at the most; every search stops at its own limit
        self.positions, self.done, self.ctl, self.event = 0, False, None, None


class BeamSearch(object):
    def __init__(self, beam_size, recognizer):
        self.beam_size = beam_size
        self.rec = recognizer
        self.last_stats = {}

    # ---- the reference's `_smallest` on the device (kept for callers / tests of the selection rule) -----------------
    def _smallest(self, matrix, k):
        """Indices (row, column) and values of the k smallest entries of a 2-D array, ascending, equal values in flat-index
        order (lvsr_topk_smallest)."""
        from .native import ptr
        lib, dev = self.rec.lib, self.rec.device
        m = torch.as_tensor(numpy.ascontiguousarray(matrix, dtype=numpy.float32)).to(dev).contiguous()
        n, k = int(m.numel()), int(min(k, m.numel()))
        idx = torch.empty(k, dtype=torch.int64, device=dev)
        val = torch.empty(k, dtype=torch.float32, device=dev)
        lib.call("lvsr_topk_smallest", lib.stream_for(m), ptr(m), n, k, ptr(idx), ptr(val))
        return numpy.unravel_index(idx.cpu().numpy(), matrix.shape), val.cpu().numpy()

    # ---- driver ---------------------------------------------------------------------------------------------------
    def search(self, input_values, eol_symbol, max_length, ignore_first_eol=False, as_arrays=False, char_discount=0,
               round_to_inf=1e9, stop_on="patience", validate_solution_function=None):
        """`input_values` = {'recordings': (T,F) ndarray}.  Returns (outputs, costs) lists, best first, or the padded
        (outputs, mask, step costs) arrays with `as_arrays`."""
        if stop_on not in STOP_ON:
            raise ValueError("Unknown stopping criterion {}".format(stop_on))
        lm = self.rec.generator.language_model
        host_lm = lm if lm is not None and not lm.on_device else None
        stepping = host_lm is not None or validate_solution_function is not None
        if int(max_length) <= 0:
            raise CandidateNotFoundError()
        run = self._begin(lambda: self.rec.compute_contexts(input_values["recordings"]), [max_length], eol_symbol, ignore_first_eol,
                          char_discount, round_to_inf, stop_on, False, stepping)
        if stepping:
            with self.rec._on_stream():
                self._search_stepping(run.state, input_values, host_lm, validate_solution_function, run.first_token)
            run.done = True
        while not run.done:
            self.advance(run, POLL_EVERY, wait=True)
        return self.finish(run, as_arrays=as_arrays)

    def search_batch(self, recordings, eol_symbol, max_lengths, ignore_first_eol=False, char_discount=0, round_to_inf=1e9,
                     stop_on="patience", as_arrays=False, validate_solution_function=None):
        """The searches of N utterances side by side: one encoder pass over the padded batch, then every launch of a position
        serves the N beams at once (rows [g K, g K + K) of the state buffers belong to utterance g; windows, position counters,
        stopping rules and finished lists stay per utterance: lvsr_attdec_args.group_rows, lvsr_beam_args.groups).  A beam step
        is dispatch bound for one utterance (13 launches of 5-14 us per position); here the launches are shared.
        -> list of N results, each what `search` returns for that utterance alone — or the exception it would raise.
        A language model walked on the host or a `validate_solution_function` put the host inside every position (module
        docstring): there is nothing to share then, and the utterances are searched one after the other."""
        lm = self.rec.generator.language_model
        if validate_solution_function is not None or (lm is not None and not lm.on_device):
            out = []
            for x, limit in zip(recordings, max_lengths):
                try:
                    out.append(self.search({"recordings": numpy.asarray(x, numpy.float32)[:, None, :]}, eol_symbol, limit,
                                           ignore_first_eol=ignore_first_eol, as_arrays=as_arrays, char_discount=char_discount,
                                           round_to_inf=round_to_inf, stop_on=stop_on, validate_solution_function=validate_solution_function))
                except SEARCH_ERRORS as e:
                    out.append(e)
            return out
        run = self.begin_batch(recordings, eol_symbol, max_lengths, ignore_first_eol=ignore_first_eol, char_discount=char_discount,
                               round_to_inf=round_to_inf, stop_on=stop_on)
        while not run.done:
            self.advance(run, POLL_EVERY, wait=True)
        return self.finish_batch(run, as_arrays=as_arrays)

    # ---- the same searches in pieces that never block the host: several search sets (one recognizer + stream each) can be kept
    #      in flight from one thread (tools/bench_decode.py: decoding is "replicas only", also within a GPU) ----------------------
    def begin(self, input_values, eol_symbol, max_length, ignore_first_eol=False, char_discount=0, round_to_inf=1e9,
              stop_on="patience", force_merge=False):
        """Enqueue the encoder pass and the reset of the beam state; returns the handle of the running search."""
        return self._begin(lambda: self.rec.compute_contexts(input_values["recordings"]), [max_length], eol_symbol, ignore_first_eol,
                           char_discount, round_to_inf, stop_on, force_merge)

    def begin_batch(self, recordings, eol_symbol, max_lengths, ignore_first_eol=False, char_discount=0, round_to_inf=1e9,
                    stop_on="patience"):
        """`begin` for N utterances side by side.  A batch of one is the single search with the kernels of the batched one
        (`force_merge`): the same hypotheses in any batch."""
        if len(recordings) == 1:
            return self.begin({"recordings": numpy.asarray(recordings[0], numpy.float32)}, eol_symbol, max_lengths[0], ignore_first_eol,
                              char_discount, round_to_inf, stop_on, force_merge=True)
        return self._begin(lambda: self.rec.compute_contexts_batch(recordings), max_lengths, eol_symbol, ignore_first_eol,
                           char_discount, round_to_inf, stop_on, False)

    def _refuse_host_work(self, validate_solution_function, where):
        lm = self.rec.generator.language_model
        if validate_solution_function is not None or (lm is not None and not lm.on_device):
            raise ValueError("%s: a language model walked on the host or a validate_solution_function put the host inside every "
                             "position, one utterance at a time, from host recordings: use beam_search_batch" % where)

    def begin_staged(self, x, mask, max_lengths, eol_symbol, lengths=None, ignore_first_eol=False, char_discount=0, round_to_inf=1e9,
                     stop_on="patience"):
        """`begin_batch` for a batch that is already on the device: x (T,N,F), mask (T,N) (SpeechRecognizer.compute_contexts_staged).
        A batch of one is again the single search with the kernels of the batched one (`force_merge`); with `lengths` (the frames of
        every utterance, host integers) its encoder pass runs over its own frames without a mask, as `begin_batch` runs it."""
        self._refuse_host_work(None, "begin_staged")
        n = int(x.shape[1])
        if len(max_lengths) != n or (lengths is not None and len(lengths) != n):
            raise ValueError("begin_staged: %d utterances, %d length limits" % (n, len(max_lengths)))
        if n == 1 and lengths is not None and 0 < int(lengths[0]) <= int(x.shape[0]):
            x, mask = x[: int(lengths[0])], None
        return self._begin(lambda: self.rec.compute_contexts_staged(x, mask), max_lengths, eol_symbol, ignore_first_eol, char_discount,
                           round_to_inf, stop_on, n == 1)

    def search_staged(self, x, mask, max_lengths, eol_symbol, lengths=None, ignore_first_eol=False, char_discount=0, round_to_inf=1e9,
                      stop_on="patience", as_arrays=False, validate_solution_function=None):
        """`search_batch` over a staged batch -> list of N results or exceptions.  The fallbacks of `search_batch` are refusals here."""
        self._refuse_host_work(validate_solution_function, "search_staged")
        run = self.begin_staged(x, mask, max_lengths, eol_symbol, lengths=lengths, ignore_first_eol=ignore_first_eol,
                                char_discount=char_discount, round_to_inf=round_to_inf, stop_on=stop_on)
        while not run.done:
            self.advance(run, POLL_EVERY, wait=True)
        return self.finish_batch(run, as_arrays=as_arrays)

    def _begin(self, compute_contexts, limits, eol_symbol, ignore_first_eol, char_discount, round_to_inf, stop_on, force_merge,
               stepping=False):
        """`stepping`: the host drives every position itself (`_search_stepping`); it takes no looks through a pinned block."""
        rec, gen = self.rec, self.rec.generator
        if stop_on not in STOP_ON:
            raise ValueError("Unknown stopping criterion {}".format(stop_on))
        lm = gen.language_model
        assert stepping or lm is None or lm.on_device, "the free-running search needs the device language model"
        limits = [int(m) for m in limits]
        with rec._on_stream():
            compute_contexts()
            st = gen.beam_begin(self.beam_size, eol_symbol, limits[0] if len(limits) == 1 else [max(m, 1) for m in limits],
                                ignore_first_eol, char_discount, round_to_inf, stop_on, force_merge=force_merge)
        host = torch.empty(tuple(st.ctl.shape), dtype=torch.int32).pin_memory() if rec.device.type == "cuda" and not stepping else None
        # first token: the LMEmitter's / SoftmaxEmitter's initial outputs
        return SearchRun(st, limits, host, 0 if lm is not None else gen.d.V, char_discount)

    def advance(self, run, positions=POLL_EVERY, wait=False):
        """Enqueue up to `positions` more positions and a look at the control block.  wait=False returns at once; the look is
        picked up by the next call (or by `ready`)."""
        rec, st = self.rec, run.state
        if run.done:
            return True
        st.check_current()
        if run.event is not None:                          # a look is in flight
            if not wait and not run.event.query():
                return False
            run.event.synchronize()
            run.event = None
            run.ctl = run.host.numpy().copy()
            if self._all_done(run.ctl) or run.positions >= run.max_length:
                run.done = True
                return True
        if positions <= 0:
            return False
        with rec._on_stream():
            n = min(int(positions), run.max_length - run.positions)
            if n == POLL_EVERY:
                st.steps(n)                                # one graph launch for the whole stretch between two looks
            else:
                for _ in range(n):
                    st.steps(1)
            run.positions += n
            if run.host is None:                           # CPU emulator: plain synchronous look
                run.ctl = st.ctl.cpu().numpy()
                run.done = self._all_done(run.ctl) or run.positions >= run.max_length
                return run.done
            run.host.copy_(st.ctl, non_blocking=True)
            run.event = torch.cuda.Event()
            run.event.record(torch.cuda.current_stream(rec.device))
        if wait:
            return self.advance(run, 0, wait=True) if run.event is not None else run.done
        return False

    @staticmethod
    def _all_done(ctl):          # ctl: the control blocks of a search set, (G, 16)
        return bool(numpy.all(ctl[:, CTL["done"]] != 0))

    def finish(self, run, as_arrays=False):
        """Collect the result of a search whose `advance` reported done; `last_stats` then carries its `finished` and `done` too."""
        entry = self._finish(run, as_arrays)[0]
        self.last_stats.update(finished=self.last_stats["per_utterance"][0]["finished"], done=self.last_stats["per_utterance"][0]["done"])
        if isinstance(entry, Exception):
            raise entry
        return entry

    def finish_batch(self, run, as_arrays=False):
        """-> one entry per utterance: the result, or the exception the single search raises in its place."""
        return self._finish(run, as_arrays)

    def _finish(self, run, as_arrays):
        rec, st, lm = self.rec, run.state, self.rec.generator.language_model
        st.check_current()
        assert run.done
        with rec._on_stream():
            if lm is not None and lm.on_device:
                lm.check_error()
            rec.encoder.check_persistent()
            ctl = st.ctl.cpu().numpy()
            host = {k: getattr(st, k).cpu().numpy() for k in HOST_TABLES}
        out, stats = [], []
        for g in range(st.groups):
            try:
                if run.limits[g] <= 0:
                    raise CandidateNotFoundError()
                self._raise_device_errors(ctl[g])
                out.append(self._collect({k: v[g] for k, v in host.items()}, ctl[g], run.first_token, run.char_discount, as_arrays))
            except SEARCH_ERRORS as e:
                out.append(e)
            # reused: positions whose second attention pass was the first one's results
            stats.append(dict(positions=int(ctl[g][CTL["steps"]]), finished=int(ctl[g][CTL["nfin"]]), done=int(ctl[g][CTL["done"]]),
                              reused=int(ctl[g][CTL["reused"]])))
        self.last_stats = dict(positions=max(s["positions"] for s in stats), reused=sum(s["reused"] for s in stats), per_utterance=stats)
        return out

    @staticmethod
    def _raise_device_errors(ctl):
        err = int(ctl[CTL["err"]])
        if err == 1:
            raise AssertionError("non-finite step costs in beam search")             # search.py:345 `assert numpy.isfinite`
        if err == 2:
            raise RuntimeError("beam search: the finished-hypothesis list overflowed its device buffer")
        if err == 3:       # the reference decrements `patience` before it ever assigns it (first finished score >= 1000)
            raise UnboundLocalError("local variable 'patience' referenced before assignment")

    def _search_stepping(self, st, input_values, host_lm, validate, first_token):
        """One synchronisation per position: the host language-model walk feeds the fusion costs of the live hypotheses,
        and/or a Python callback vetoes finished hypotheses (search.py:372-374).  One search: group 0 of the state."""
        gen, dev = self.rec.generator, self.rec.device
        K = st.K
        lm_states = host_lm.initial_states(1) if host_lm is not None else None
        hist_p, hist_c = [], []
        ctl = st.ctl[0].cpu().numpy()
        for position in range(st.max_length):
            if host_lm is not None:
                n = int(ctl[CTL["nlive"]])
                add = numpy.zeros((K, gen.d.V), numpy.float32)
                if n:
                    add[:n] = lm_states["add"][:n]
                    add[n:] = add[0]
                st.lm["add_live"].copy_(torch.from_numpy(add))
            # where this position's finished hypotheses will land: in patience mode the kernel first sorts the list and cuts it to K
            nfin_before = int(ctl[CTL["nfin"]])
            if st.stop_on == "patience" and int(ctl[CTL["nlive"]]) > 0:
                nfin_before = min(nfin_before, K)
            st.costs()
            st.select()
            ctl = st.ctl[0].cpu().numpy()
            if ctl[CTL["done"]] in (1, 2):
                break                                         # a stopping rule fired: nothing was selected at this position
            nsel, nlive = int(ctl[CTL["nsel"]]), int(ctl[CTL["nlive"]])
            parents = st.parents.cpu().numpy()[:nsel]
            chars = st.chars.cpu().numpy()[:nsel]
            keep = st.keep.cpu().numpy()[:nlive]
            if validate is not None:
                hist_p.append(st.hist_parent[0, position].cpu().numpy().copy())
                hist_c.append(st.hist_char[0, position].cpu().numpy().copy())
                nfin = int(ctl[CTL["nfin"]])
                if nfin > nfin_before:
                    cols = st.fin_col[0].cpu().numpy()
                    ok = [i for i in range(nfin_before, nfin)
                          if validate(input_values, self._tokens_of(hist_p, hist_c, position, int(cols[i]), first_token))]
                    if len(ok) != nfin - nfin_before:
                        for t in (st.fin_pos[0], st.fin_col[0], st.fin_cost[0], st.fin_score[0]):
                            kept = t[torch.as_tensor(ok, dtype=torch.int64, device=dev)].clone() if ok else t[:0]
                            t[nfin_before: nfin_before + len(ok)] = kept
                        st.ctl[0, CTL["nfin"]] = nfin_before + len(ok)
                        ctl[CTL["nfin"]] = nfin_before + len(ok)
            if host_lm is not None:
                lm_states = host_lm.take(lm_states, parents)
                lm_states = host_lm.transition(lm_states, chars)
                lm_states = host_lm.take(lm_states, keep)
            st.advance()
            if ctl[CTL["done"]]:
                break

    @staticmethod
    def _tokens_of(hist_p, hist_c, position, col, first_token):
        toks = []
        for p in range(position, -1, -1):
            toks.append(int(hist_c[p][col]))
            col = int(hist_p[p][col])
        return numpy.array([first_token] + toks[::-1])

    def _collect(self, host, ctl, first_token, char_discount, as_arrays):
        """Follow the back-pointers of the finished hypotheses of one search and rank them (search.py:378-407).  `host`: host
        copies of its `HOST_TABLES`, `ctl`: of its control block."""
        nfin, npos = int(ctl[CTL["nfin"]]), int(ctl[CTL["steps"]])
        if nfin == 0:
            raise CandidateNotFoundError()
        fin_pos, fin_col = host["fin_pos"][:nfin], host["fin_col"][:nfin]
        hp, hc, hcost = host["hist_parent"][:npos], host["hist_char"][:npos], host["hist_cost"][:npos]
        hyps = []
        for p, col in zip(fin_pos, fin_col):
            toks, run = [], []
            for q in range(int(p), -1, -1):
                toks.append(hc[q, col])
                run.append(hcost[q, col])
                col = hp[q, col]
            tokens = numpy.array([first_token] + toks[::-1], dtype=numpy.int64)
            running = numpy.array([numpy.float32(0)] + run[::-1], dtype=numpy.float32)
            hyps.append((tokens, running))
        # final ranking: cumulative cost minus the discount per row of the cost column; Python's sort is stable, so equal
        # scores keep the order of completion (patience mode: of the truncated, sorted list)
        # (float64, as numpy.float32 - Python float was under the numpy the reference was written for, and as csrc/beam.hip ranks)
        hyps.sort(key=lambda h: float(h[1][-1]) - float(char_discount) * len(h[1]))
        longest = max(len(t) for t, _ in hyps)
        out_tokens = numpy.zeros((longest, len(hyps)))
        out_mask = numpy.zeros((longest, len(hyps)))
        out_running = numpy.zeros((longest, len(hyps)))
        for col, (tokens, running) in enumerate(hyps):
            n = len(tokens)
            out_tokens[:n, col] = tokens
            out_mask[:n, col] = 1
            out_running[:n, col] = running
            out_running[n:, col] = running[-1]
        # drop the initial pseudo-token; step costs = differences of the running costs
        result = out_tokens[1:], out_mask[1:], out_running[1:] - out_running[:-1]
        return result if as_arrays else self.result_to_lists(result)

    @staticmethod
    def result_to_lists(result):
        """(outputs, mask, step costs) arrays -> ([tokens of hypothesis k], [total cost of hypothesis k])."""
        tokens, mask, step_costs = result
        lengths = mask.sum(axis=0).astype(int)
        outputs = [list(tokens[:n, k]) for k, n in enumerate(lengths)]
        return outputs, list(step_costs.sum(axis=0))
