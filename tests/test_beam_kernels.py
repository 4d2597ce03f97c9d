"""The beam-search step of csrc/beam.hip (lvsr_beam_select, lvsr_beam_compact, lvsr_topk_smallest) called directly and driven in
lock-step with a plain Python / NumPy restatement of the reference's search loop (libs/blocks/blocks/search.py:299-377 with the
choices csrc/beam.hip and include/lvsr_hip.h document).  No recognizer: the step costs of a hypothesis are a deterministic function
of (seed, position, its tokens), so that every situation a trained-looking network rarely produces can be staged: equal float32
candidates across the cut, more than K finished hypotheses with equal scores at a loop head, scores that differ only in double,
`round_to_inf` and `ignore_first_eol`, an emptying beam, the three error words, the capacity of the LDS arrays (K = 256,
K * V = 8192), grouped launches whose searches stop at different positions, and both values of the attention-reuse flag.

After every lvsr_beam_select the WHOLE of every buffer the launch may write is compared with the model's mirror of it (integers equal,
float32 / float64 bit for bit): what a step must write and what it must leave alone (sentinels, rows of earlier positions, the blocks
of searches that are done) are checked by the same comparison.  Rows of the inputs no live hypothesis owns hold NaN.  At the end the
host's own BeamSearch._collect runs on the device state and must return the model's ranking.

There are no tolerances.  The model does the kernel's float32 additions and its double subtraction; every `char_discount` used here is
a dyadic rational of few bits, so that discount * (position + 2) is exact in double and the score is the same number whether or not a
compiler fuses the multiplication into the subtraction.

Every scenario first asserts ON THE MODEL ALONE that it produces the situation it is named for; the `*_control` tests show that the
scenario set tells the true rules from nine near misses."""
import collections
import ctypes
import zlib

import numpy
import pytest
import torch

from lvsr_amd import native
from lvsr_amd.native import ptr

F32, F64, I32, I64 = numpy.float32, numpy.float64, numpy.int32, numpy.int64
SENT = -777.25            # the sentinel float outputs are pre-filled with
SENT_I = -7               # ... integer outputs (row indices a later launch reads are pre-filled with K - 1 instead: in bounds)
PATIENCE = 30
FIRST_TOKEN = 99          # the initial pseudo-token of BeamSearch._collect

Hyp = collections.namedtuple("Hyp", "tokens runs")                   # a live hypothesis: its characters, its cumulative costs (float32)
Fin = collections.namedtuple("Fin", "pos col cost tokens runs")      # a finished one: where the device keeps it + what it spells


def bits(a):
    a = numpy.ascontiguousarray(a)
    return a.view({4: numpy.uint32, 8: numpy.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(got, ref, what):
    got, ref = numpy.ascontiguousarray(got), numpy.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, "%s: %s %s != %s %s" % (what, got.dtype, got.shape, ref.dtype, ref.shape)
    bad = numpy.flatnonzero(bits(got).ravel() != bits(ref).ravel())
    assert bad.size == 0, "%s: %d entries differ, first at %d: %r != %r" % (what, bad.size, bad[0], got.ravel()[bad[0]], ref.ravel()[bad[0]])


# ---- the model ------------------------------------------------------------------------------------------------------------------
class BeamModel(object):
    """One search.  `step(costs)` is one lvsr_beam_select: the loop head on the state the previous step left, then one position.
    Beside the reference's own variables (`live`, `finished`, `min_cost`, `patience`) it keeps a mirror of every device buffer of
    the search, stale entries included.  `mutant` replaces one rule by a near miss (controls)."""

    def __init__(self, K, V, eol, limit, stop_on, char_discount=0.0, round_to_inf=1e9, ignore_first_eol=False, fin_cap=None,
                 cap=None, mutant=None):
        self.K, self.V, self.eol, self.limit, self.stop_on = K, V, eol, limit, stop_on
        self.cd, self.rti, self.ife, self.mutant = float(char_discount), F32(min(round_to_inf, 3.0e38)), bool(ignore_first_eol), mutant
        self.fin_cap = fin_cap if fin_cap is not None else (2 * K if stop_on == 0 else K * (limit + 1))
        self.cap = cap if cap is not None else limit
        self.live = [Hyp((), (F32(0),))]
        self.finished = []
        self.min_cost, self.patience = 1000.0, None
        self.pos = self.done = self.err = self.steps = self.nsel = 0
        self.facts = collections.Counter()
        slack = 0 if mutant is None else 64 * K            # (a mutant may keep more than the device could)
        self.m = dict(
            running=numpy.full(K, SENT, F32), live_col=numpy.full(K, SENT_I, I32),
            hist_parent=numpy.full((self.cap, K), SENT_I, I32), hist_char=numpy.full((self.cap, K), SENT_I, I32),
            hist_cost=numpy.full((self.cap, K), SENT, F32),
            fin_pos=numpy.full(self.fin_cap + slack, SENT_I, I32), fin_col=numpy.full(self.fin_cap + slack, SENT_I, I32),
            fin_cost=numpy.full(self.fin_cap + slack, SENT, F32), fin_score=numpy.full(self.fin_cap + slack, SENT, F32),
            keep=numpy.full(K, K - 1, I32), parents=numpy.full(K, K - 1, I32), chars=numpy.full(K, SENT_I, I64),
            fctl=numpy.array([1000.0, 0.0, 0.0, 0.0], F32))
        self.m["running"][0], self.m["live_col"][0] = 0, 0

    def score(self, cost, pos):
        return float(F64(cost) - self.cd * F64(pos + 2))

    def ctl(self):
        return numpy.array([len(self.live), self.pos, self.done, len(self.finished), -1 if self.patience is None else self.patience,
                            self.nsel, self.err, self.steps], I32)

    def _store_fctl(self):
        self.m["fctl"][0] = F32(self.min_cost)
        self.m["fctl"][2:4] = numpy.array([self.min_cost], F64).view(F32)

    def _store_finished(self, first=0):
        for r in range(first, len(self.finished)):
            e = self.finished[r]
            self.m["fin_pos"][r], self.m["fin_col"][r], self.m["fin_cost"][r] = e.pos, e.col, e.cost
            self.m["fin_score"][r] = F32(self.score(e.cost, e.pos))

    def snapshot(self):
        """Everything that is compared after a step (of the finished list what the device holds: a mutant's slack is left out, so
        that traces differ by what the rules did and never by their length)."""
        return (self.ctl().tobytes(),) + tuple(bits(self.m[k][:self.fin_cap] if k.startswith("fin_") else self.m[k]).tobytes()
                                               for k in sorted(self.m))

    def step(self, costs):
        """costs: (n_live, V) float32.  -> did the search advance by a position?"""
        K, V, M, facts = self.K, self.V, self.mutant, self.facts
        if self.done:
            return False
        n, p = len(self.live), self.pos
        # ---- the loop head
        moved_up = False
        if self.stop_on == 0 and (n > 0 or M == "cut_on_empty"):
            before = self.finished
            key = (lambda e: self.score(e.cost, e.pos)) if M != "f32_rank" else (lambda e: F32(self.score(e.cost, e.pos)))
            ranked = sorted(before, key=key)
            facts["nfin_max"] = max(facts["nfin_max"], len(before))
            if len(before) > K:
                facts["cuts"] += 1
                facts["cuts_through_equal_scores"] += key(ranked[K - 1]) == key(ranked[K])
                moved_up = ranked[K] is not before[K]          # slot K keeps a stale copy of an entry that moved below rank K
            if [id(e) for e in ranked] != [id(e) for e in sorted(before, key=lambda e: F32(self.score(e.cost, e.pos)))]:
                facts["double_order_differs_from_float32"] += 1
            self.finished = ranked if M == "no_cut" else ranked[:K]
            self._store_finished()
        stop = 0
        if n == 0:
            stop = 2
        elif self.stop_on == 0:
            if self.finished:
                leader = self.score(self.finished[0].cost, self.finished[0].pos)
                if leader < self.min_cost or (M == "reset_le" and leader == self.min_cost):
                    self.min_cost, self.patience = leader, PATIENCE
                    facts["resets"] += 1
                elif self.patience is None:
                    self.err, stop = 3, 1
                else:
                    self.patience -= 1
                    if self.patience == 0:
                        stop = 1
        else:
            facts["nfin_max"] = max(facts["nfin_max"], len(self.finished))
            if len(self.finished) >= K:
                last = self.finished[K - 1]
                lowest = min(h.runs[-1] for h in self.live)
                bound = float(F64(lowest) - self.cd * F64(p if M == "bound_pos" else self.limit))
                if self.score(last.cost, last.pos) < bound:
                    stop = 1
        if stop:
            self.done = stop
            self._store_fctl()
            return False
        # ---- candidates
        costs = numpy.asarray(costs, F32).reshape(n, V)
        if not numpy.isfinite(costs).all():
            assert self.stop_on == 1 or not self.finished, "the model stages non-finite costs only where the loop head changes nothing"
            self.err, self.done = 1, 1
            return False
        facts["live_max"], facts["candidates_max"] = max(facts["live_max"], n), max(facts["candidates_max"], n * V)
        run = numpy.array([h.runs[-1] for h in self.live], F32)
        cand = (run[:, None] + costs).ravel()
        assert cand.dtype == F32 and not numpy.signbit(cand[cand == 0]).any()
        flat = numpy.arange(n * V)
        order = numpy.lexsort((flat if M != "ties_descending" else -flat, cand))
        nsel = min(K, n * V)
        if n * V > K and cand[order[K - 1]] == cand[order[K]]:
            tied = flat[cand == cand[order[K]]]
            inside = set(order[:K].tolist())
            if any(a // V != b // V for a in tied if a in inside for b in tied if b not in inside):
                facts["ties_across_the_cut"] += 1
        sel = order[:nsel]
        par, ch, cost = sel // V, sel % V, cand[sel]
        m = self.m
        m["parents"][:nsel], m["parents"][nsel:] = par, par[0]
        m["chars"][:nsel], m["chars"][nsel:] = ch, ch[0]
        m["hist_parent"][p, :nsel] = m["live_col"][par]
        m["hist_char"][p, :nsel], m["hist_cost"][p, :nsel] = ch, cost
        # ---- finished hypotheses, the new beam
        keep_all = self.ife and p == 0 and M != "no_ife"
        live, keep, first_new = [], [], len(self.finished)
        for k in range(nsel):
            h = self.live[par[k]]
            h = Hyp(h.tokens + (int(ch[k]),), h.runs + (cost[k],))
            ended = ch[k] == self.eol
            if ended:
                if F32(cost[k] - run[par[k]]) < self.rti or M == "no_rti":
                    facts["eol_recorded"] += 1
                    if len(self.finished) < self.fin_cap:
                        self.finished.append(Fin(p, k, cost[k], h.tokens, h.runs))
                    else:
                        self.err = 2
                        facts["overflows"] += 1
                else:
                    facts["eol_rejected"] += 1
                facts["first_eol_kept"] += keep_all
            if not ended or keep_all:
                keep.append(k)
                live.append(h)
        self._store_finished(first_new)
        facts["stale_slot_K_survives_a_step"] += moved_up and len(self.finished) == first_new
        self.live = live
        nl = len(live)
        m["keep"][:nl], m["keep"][nl:] = keep, (keep[0] if nl else 0)
        m["live_col"][:nl], m["running"][:nl] = keep, cost[keep] if nl else []
        self.pos, self.steps, self.nsel = p + 1, self.steps + 1, nsel
        if self.pos >= self.limit:
            self.done = 3
        self._store_fctl()
        return True

    def result(self):
        """What the host reads back at the end: hypotheses and costs, best first, equal scores in the order of the list."""
        ranked = sorted(self.finished, key=lambda e: self.score(e.cost, e.pos))
        return [list(e.tokens) for e in ranked], [float(e.cost) for e in ranked]


# ---- step costs: a deterministic function of (seed, position, token history) -----------------------------------------------------
def step_costs(spec, pos, tokens):
    """(V) float32, strictly positive before `eol_bias` / `offset` (Gamma(2)); `grid` rounds up to a multiple (ties)."""
    if "fixed" in spec:
        return numpy.array(spec["fixed"], F32)
    seed = zlib.crc32(numpy.array((spec["seed"], pos) + tuple(tokens), I64).tobytes())
    c = numpy.random.RandomState(seed).gamma(2.0, 1.0, spec["V"])
    if spec.get("grid"):
        c = numpy.ceil(c / spec["grid"]) * spec["grid"]
    c = c.astype(F32)
    bias = spec.get("eol_bias", 0.0)
    if isinstance(bias, tuple):
        bias = bias[min(pos, len(bias) - 1)]
    c[spec["eol"]] += F32(bias)
    return c + F32(spec.get("offset", 0.0))


def costs_of(spec, model):
    c = numpy.array([step_costs(spec, model.pos, h.tokens) for h in model.live], F32).reshape(len(model.live), spec["V"])
    if "bad" in spec and model.pos == spec["bad"][0] and len(c):             # a non-finite step cost in the last live row
        c[-1, 1] = spec["bad"][1]
    return c


def new_model(spec, mutant=None, limit=None, cap=None):
    return BeamModel(spec["K"], spec["V"], spec["eol"], spec["limit"] if limit is None else limit, spec["stop_on"],
                     spec.get("char_discount", 0.0), spec.get("round_to_inf", 1e9), spec.get("ignore_first_eol", False),
                     spec.get("fin_cap"), cap, mutant)


def simulate(spec, mutant=None):
    """The model alone.  -> (model at the end, the snapshots after every step)"""
    model, trace = new_model(spec, mutant), []
    while not model.done:
        model.step(costs_of(spec, model))
        trace.append(model.snapshot())
    return model, trace


# ---- scenarios --------------------------------------------------------------------------------------------------------------------
def scenario(K, V, limit, stop_on, seed, eol=None, **kw):
    return dict(K=K, V=V, limit=limit, stop_on=stop_on, seed=seed, eol=V - 1 if eol is None else eol, **kw)


SINGLE = {
    # (groups: 0 and 1 both mean one search; Tp = 300: more than one trip of the 256 threads of a row copy; an <eol> bias of 50 keeps
    # every hypothesis alive for a position, so that the beam fills: K live rows, K * V candidates)
    "plain_patience": scenario(4, 7, 24, 0, 1, eol=2, char_discount=0.125, groups=0, Tp=300),
    "plain_optimistic": scenario(4, 7, 12, 1, 1, eol=2, char_discount=0.5),
    "patience_runs_out": scenario(4, 5, 60, 0, 166, eol_bias=3.0, char_discount=0.0, groups=0),
    "optimistic_stop": scenario(12, 5, 16, 1, 2, char_discount=0.5),
    "ties_across_the_cut": scenario(5, 6, 10, 0, 0, grid=1.0, eol_bias=2.0),
    "ties_across_the_cut_optimistic": scenario(5, 6, 10, 1, 0, grid=1.0, eol_bias=2.0, char_discount=0.5),
    "cut_through_equal_scores": scenario(3, 6, 40, 0, 6, grid=1.0, char_discount=0.0),
    "cut_leaves_slot_K": scenario(3, 6, 40, 0, 2, char_discount=0.5),
    "double_scores": scenario(4, 6, 40, 0, 0, grid=0.25, char_discount=0.25 + 2.0 ** -30),
    "round_to_inf": scenario(4, 5, 16, 0, 0, round_to_inf=1.0, grid=0.5),
    "ignore_first_eol": scenario(4, 5, 12, 0, 0, ignore_first_eol=True, eol_bias=(-3.0, 1.0), eol=0, groups=0),
    "beam_empties": scenario(3, 5, 20, 0, 2, grid=1.0, eol_bias=(0.0, 0.0, 0.0, -40.0)),
    "beam_empties_v2": scenario(1, 2, 20, 1, 0, eol_bias=-1.0, char_discount=0.5),
    "beam_wider_than_candidates": scenario(200, 40, 3, 0, 0, char_discount=0.25),
    "capacity_continuous": scenario(256, 32, 5, 1, 0, char_discount=0.5, eol_bias=(0.0, 50.0, 50.0, 0.0)),
    "capacity_quantised": scenario(256, 32, 5, 0, 0, grid=1.0, groups=0, eol_bias=(0.0, 50.0, 50.0, 0.0)),
    "capacity_finished": scenario(200, 40, 6, 0, 0, grid=0.5, eol_bias=(-3.0, 50.0, -3.0)),
    "error_2": scenario(2, 2, 12, 1, 0, fin_cap=4, fixed=(0.01, 5.0)),
    "error_3": scenario(3, 5, 12, 0, 0, offset=1000.0, eol_bias=-1.0),
}


def assert_staged(name, model, trace):
    """A scenario must produce the situation it is named for — on the model, before any kernel is asked."""
    f, K = model.facts, model.K
    if name.startswith("plain"):
        assert model.done in (1, 3) and model.finished and model.err == 0
    if name == "patience_runs_out":
        assert model.done == 1 and model.patience == 0 and model.pos < model.limit and f["resets"] >= 2 and model.err == 0
    if name == "optimistic_stop":
        assert model.done == 1 and len(model.finished) >= K and f["nfin_max"] > 2 * K and model.err == 0
    if name.startswith("ties_across_the_cut"):
        assert f["ties_across_the_cut"] >= 1
    if name == "cut_through_equal_scores":
        assert f["cuts"] >= 1 and f["cuts_through_equal_scores"] >= 1 and f["nfin_max"] > K
    if name == "cut_leaves_slot_K":        # (an entry written at rank K too would show: nothing finishes in that step)
        assert f["stale_slot_K_survives_a_step"] >= 1
    if name == "double_scores":
        assert f["double_order_differs_from_float32"] >= 1
    if name == "round_to_inf":
        assert f["eol_rejected"] >= 1 and f["eol_recorded"] >= 1
    if name == "ignore_first_eol":
        assert f["first_eol_kept"] >= 1 and any(e.pos == 0 for e in model.finished)
    if name == "beam_empties":
        assert model.done == 2 and len(model.finished) > K             # (more than K: the list is NOT cut on an empty beam)
    if name == "beam_empties_v2":
        assert model.done == 2
    if name == "beam_wider_than_candidates":
        assert numpy.frombuffer(trace[0][0], I32)[5] == model.V < K          # ctl[5] after position 0
    if name.startswith("capacity"):
        assert f["live_max"] == K and f["candidates_max"] == K * model.V >= 8000          # a position the kernel runs, not the spec alone
    if name in ("capacity_continuous", "capacity_quantised"):
        assert f["candidates_max"] == 8192 and f["eol_recorded"] > 1
    if name == "capacity_finished":
        assert f["nfin_max"] > K and f["cuts"] >= 1
    if name == "error_2":
        assert model.err == 2 and f["overflows"] >= 1 and model.done == 3 and len(model.finished) == model.fin_cap
    if name == "error_3":
        assert model.err == 3 and model.done == 1 and model.patience is None


# ---- the lock-step driver ---------------------------------------------------------------------------------------------------------
STATE_OUT = ("fctl", "running", "live_col", "hist_parent", "hist_char", "hist_cost", "fin_pos", "fin_col", "fin_cost", "fin_score",
             "keep", "parents", "chars")


class Driver(object):
    """G searches (one spec each; what the argument block shares — K, V, <eol>, the stopping rule and its constants — from the first)
    on the device, each next to its BeamModel.  Optional blocks: `pos` (window centres), `lm` (language-model state rows), `reuse`
    (the WA / W1 / pos1 block, E = 3), `fork` (one-hot feedback rows; fork_rows characters have a row)."""

    def __init__(self, lib, device, specs, groups=None, pos=True, lm=True, reuse=False, fork=False, fork_rows=None, D=None, Tp=5):
        s0 = specs[0]
        self.lib, self.device, self.specs, self.G = lib, device, specs, len(specs)
        G, K, V = self.G, s0["K"], s0["V"]
        self.K, self.V, self.R = K, V, G * K
        self.groups = G if groups is None else groups
        assert (self.groups if self.groups > 1 else 1) == G
        limits = [s["limit"] for s in specs]
        self.cap = limits[0] if G == 1 else (max(limits) + 31) // 32 * 32           # (as SequenceGenerator.beam_begin sizes the history)
        self.models = [new_model(s, cap=self.cap) for s in specs]
        self.H = max(limits) + 1                                                      # columns of S that spell the tokens
        self.D = D if D is not None else self.H + 3
        assert self.D >= self.H
        self.Tp, self.E, self.pos, self.lm, self.reuse, self.fork = Tp, 3, pos, lm, reuse, fork
        self.fork_rows = V if fork_rows is None else fork_rows
        self.fin_cap = self.models[0].fin_cap
        self.rng = numpy.random.RandomState(zlib.crc32(repr(sorted(s0.items())).encode()))
        R, D, E = self.R, self.D, self.E
        self.t, self.dtypes = {}, {}
        new = self._new
        ctl = numpy.zeros((G, 16), I32)
        ctl[:, 0], ctl[:, 4] = 1, -1
        if G > 1:
            ctl[:, 8] = limits
        new("ctl", ctl)
        new("neglogp", numpy.full((R, V), numpy.nan, F32))
        for name in STATE_OUT:                       # the model's mirrors are the initial contents: reset values and sentinels
            new(name, self.mirror(name))
        rows = dict(S=(D, F32), W=(Tp, F32))
        if pos:
            rows["pos"] = ((), F32)
        if lm:
            rows.update(lm_states=(7, I64), lm_weights=(7, F64))
        for name, (w, dt) in rows.items():
            shape = (R,) + ((w,) if w != () else ())
            for suffix in ("_live", "_sel", "_new", "_live_out"):
                new(name + suffix, numpy.full(shape, SENT if dt != I64 else SENT_I, dt))
        if lm:
            new("lm_add_new", numpy.full((R, V), SENT, F32))
            new("lm_add_live_out", numpy.full((R, V), SENT, F32))
        if reuse:
            for name, w in (("WA", (E,)), ("W1", (Tp,))) + ((("pos1", ()),) if pos else ()):
                new(name + "_live", numpy.full((R,) + w, SENT, F32))
                new(name + "_sel", numpy.full((R,) + w, SENT, F32))
        if fork:
            new("fork_xg", numpy.full((R, 3 * D), SENT, F32))
            new("fork_Wi", self.rng.standard_normal((self.fork_rows, D)).astype(F32))
            new("fork_Wg", self.rng.standard_normal((self.fork_rows, 2 * D)).astype(F32))
            new("fork_bi", self.rng.standard_normal(D).astype(F32))
            new("fork_bg", self.rng.standard_normal(2 * D).astype(F32))
        # hypothesis 0 of every search: the pseudo-token, no characters yet
        self.S = numpy.full((R, D), numpy.nan, F32)
        self.S[::K, :self.H] = -1
        self.S[::K, 0] = FIRST_TOKEN
        self.S[::K, self.H:] = self.rng.standard_normal((G, D - self.H))
        self.ctl9, self.ctl10 = numpy.zeros(G, I32), numpy.zeros(G, I32)
        self.seen9, self.fork_outside = set(), 0
        self.args = self.make_args()

    # ---- buffers
    def _new(self, name, array):
        array = numpy.ascontiguousarray(array)
        self.dtypes[name] = array.dtype
        self.t[name] = torch.from_numpy(array.copy()).to(self.device)

    def up(self, name, array):
        self.t[name].copy_(torch.from_numpy(numpy.ascontiguousarray(array)))

    def down(self, name):
        return self.t[name].cpu().numpy()

    def mirror(self, name):
        """The models' mirrors of a state buffer, search after search as the header lays them out."""
        return numpy.stack([m.m[name][:self.fin_cap] if name.startswith("fin_") else m.m[name] for m in self.models]).reshape(
            (-1,) if name in ("running", "live_col", "keep", "parents", "chars") else (self.G,) + self.models[0].m[name].shape[:-1] + (-1,))

    def make_args(self, **override):
        t, s0 = self.t, self.specs[0]
        kw = dict(K=self.K, V=self.V, eol=s0["eol"], ignore_first_eol=int(s0.get("ignore_first_eol", False)), stop_on=s0["stop_on"],
                  max_length=self.cap, fin_cap=self.fin_cap, D=self.D, Tp=self.Tp, groups=self.groups,
                  round_to_inf=float(F32(min(s0.get("round_to_inf", 1e9), 3.0e38))), char_discount=float(s0.get("char_discount", 0.0)),
                  E=self.E if self.reuse else 0, fork_rows=self.fork_rows if self.fork else 0)
        fields = dict(self.lib.structs["lvsr_beam_args"]._fields_)
        kw.update({name: buf for name, buf in t.items() if name in fields})
        kw.update(override)
        return self.lib.make("lvsr_beam_args", **kw)

    def select(self, args=None):
        self.lib.call("lvsr_beam_select", self.lib.stream_for(self.t["ctl"]), ctypes.byref(self.args if args is None else args))

    def compact(self):
        self.lib.call("lvsr_beam_compact", self.lib.stream_for(self.t["ctl"]), ctypes.byref(self.args))

    # ---- one position
    def random_rows(self, name, live_rows):
        """Fresh values in the rows of live hypotheses, NaN (integers: a poison) in every other row."""
        shape, dt = tuple(self.t[name].shape), self.dtypes[name]
        if dt == I64:
            a = self.rng.randint(-2 ** 40, 2 ** 40, shape).astype(I64)
            a[~live_rows] = -2 ** 62
        else:
            a = self.rng.standard_normal(shape).astype(dt)
            a[~live_rows] = numpy.nan
        self.up(name, a)
        return a

    def gathered(self, live, index):
        """live[index] with the indices local to their search."""
        base = numpy.repeat(numpy.arange(self.G) * self.K, self.K)
        return live[base + index.astype(I64)]

    def position(self):
        """Inputs of a position, one lvsr_beam_select, the comparison; then, if a search advanced, the next-state rows and one
        lvsr_beam_compact.  -> did any search advance?"""
        G, K, V, R, rng = self.G, self.K, self.V, self.R, self.rng
        n_live = numpy.array([0 if m.done else len(m.live) for m in self.models])
        live_rows = (numpy.arange(R) % K) < numpy.repeat(n_live, K)
        neglogp = numpy.full((R, V), numpy.nan, F32)
        costs = []
        for g, (spec, m) in enumerate(zip(self.specs, self.models)):
            c = None
            if not m.done:
                c = costs_of(spec, m)
                neglogp[g * K: g * K + len(m.live)] = c
            costs.append(c)
        self.up("neglogp", neglogp)
        S_live = self.S.copy()
        S_live[~live_rows] = numpy.nan
        self.up("S_live", S_live)
        live = dict(S=S_live, W=self.random_rows("W_live", live_rows))
        if self.lm:
            live["lm_states"] = self.random_rows("lm_states_live", live_rows)
            live["lm_weights"] = self.random_rows("lm_weights_live", live_rows)
        if self.pos:          # window centres: every row counts for the reuse flag, and rows beyond the beam are copies of row 0
            rare = min(1.0 / 3, 1.5 / K)           # (in a wide beam an extreme centre must be rare, or some selected row always has it)
            centres = rng.choice([0.0, 1.0, 2.0], R, p=[rare, 1 - 2 * rare, rare]).astype(F32)
            centres = numpy.where(live_rows, centres, numpy.repeat(centres[::K], K))
            self.up("pos_live", centres)
            live["pos"] = centres
        if self.reuse:
            live["WA"], live["W1"] = self.random_rows("WA_live", live_rows), self.random_rows("W1_live", live_rows)
            if self.pos:
                live["pos1"] = self.random_rows("pos1_live", live_rows)
        kept = {name: self.down(name + "_sel") for name in ("WA", "W1", "pos1") if name in live}
        positions = [m.pos for m in self.models]
        advanced = [m.step(c) for m, c in zip(self.models, costs)]
        parents = self.mirror("parents")
        for g in range(G):
            if self.reuse and advanced[g]:
                rows = slice(g * K, g * K + K)
                a, b = (live["pos"][rows], self.gathered(live["pos"], parents)[rows]) if self.pos else (0, 0)
                self.ctl9[g] = int(numpy.min(a) == numpy.min(b) and numpy.max(a) == numpy.max(b))
                self.ctl10[g] += self.ctl9[g]
                self.seen9.add(int(self.ctl9[g]))
        self.select()
        self.check_state("position %s" % positions)
        # ---- the rows of the next-state pass
        for name in ("S", "W", "pos", "lm_states", "lm_weights"):
            if name in live:
                same(self.down(name + "_sel"), self.gathered(live[name], parents), name + "_sel == live[parents]")
        flag = numpy.repeat(self.ctl9, K).astype(bool)
        for name in kept:                       # copied where the search's flag is up, else left alone
            f = flag.reshape((R,) + (1,) * (kept[name].ndim - 1))
            same(self.down(name + "_sel"), numpy.where(f, self.gathered(live[name], parents), kept[name]), name + "_sel (reuse)")
        chars = self.mirror("chars")
        if self.fork:
            Wi, Wg, bi, bg = (self.down("fork_" + n) for n in ("Wi", "Wg", "bi", "bg"))
            known = (chars >= 0) & (chars < self.fork_rows)
            row = numpy.where(known, chars, 0)
            xi = bi[None, :] + numpy.where(known[:, None], Wi[row], F32(0))
            xg = bg[None, :] + numpy.where(known[:, None], Wg[row], F32(0))
            same(self.down("fork_xg"), numpy.concatenate([xi, xg], axis=1).astype(F32), "fork_xg")
            self.fork_outside += int((~known[numpy.repeat(advanced, K)]).sum())
        if not any(advanced):
            return False
        # ---- next states (the test's own: the chosen character appended to the spelling), then the compaction
        S_new = self.gathered(S_live, parents).copy()
        S_new[:, self.H:] = rng.standard_normal((R, self.D - self.H))
        for g in range(G):
            if advanced[g]:
                S_new[g * K: g * K + K, positions[g] + 1] = chars[g * K: g * K + K]
        every = numpy.ones(R, bool)
        self.up("S_new", S_new)
        new = dict(S=S_new, W=self.random_rows("W_new", every))
        if self.pos:
            new["pos"] = self.random_rows("pos_new", every)
        if self.lm:
            for name in ("lm_states", "lm_weights", "lm_add"):
                new[name] = self.random_rows(name + "_new", every)
        self.compact()
        keep = self.mirror("keep")
        for name in new:
            same(self.down(name + "_live_out"), self.gathered(new[name], keep), name + "_live_out == new[keep]")
        self.S = self.gathered(S_new, keep)
        for g, m in enumerate(self.models):
            if advanced[g]:
                for i, h in enumerate(m.live):
                    spelled = [FIRST_TOKEN] + list(h.tokens) + [-1] * (self.H - 1 - len(h.tokens))
                    assert self.S[g * K + i, :self.H].tolist() == spelled[:self.H], "S of search %d row %d" % (g, i)
        self.check_state("after the compaction")
        return True

    def check_state(self, when):
        ctl = numpy.zeros((self.G, 16), I32)
        for g, m in enumerate(self.models):
            ctl[g, :8] = m.ctl()
            ctl[g, 8] = m.limit if self.G > 1 else 0
        if self.reuse:
            ctl[:, 9], ctl[:, 10] = self.ctl9, self.ctl10
        same(self.down("ctl").reshape(self.G, 16), ctl, "ctl, " + when)
        for name in STATE_OUT:
            same(self.down(name).reshape(-1), self.mirror(name).reshape(-1), name + ", " + when)

    def run(self):
        while not all(m.done for m in self.models):
            self.position()
        self.position()                     # one launch more: searches that are done are left alone
        self.check_results()
        return self

    def check_results(self):
        """The host's own walk over the back-pointers, on the device state."""
        from lvsr_amd.search import BeamSearch, CandidateNotFoundError
        ctl = self.down("ctl").reshape(self.G, 16)
        host = {k: self.down(k).reshape((self.G,) + self.models[0].m[k].shape) for k in ("fin_pos", "fin_col", "hist_parent", "hist_char", "hist_cost")}
        for g, m in enumerate(self.models):
            st = {k: torch.from_numpy(v[g]) for k, v in host.items()}
            collect = lambda: BeamSearch(self.K, None)._collect(st, ctl[g], FIRST_TOKEN, self.specs[0].get("char_discount", 0.0), False)
            if not m.finished:
                with pytest.raises(CandidateNotFoundError):
                    collect()
                continue
            outputs, costs = collect()
            want_outputs, want_costs = m.result()
            assert [[int(c) for c in o] for o in outputs] == want_outputs and len(costs) == len(want_costs), "hypotheses of search %d" % g
            same(numpy.array(costs, F64), numpy.array(want_costs, F64), "costs of search %d" % g)


def run_single(device, lib, name):
    spec = SINGLE[name]
    model, trace = simulate(spec)
    assert_staged(name, model, trace)
    d = Driver(lib, device, [spec], groups=spec.get("groups", 1), Tp=spec.get("Tp", 5)).run()
    assert d.models[0].snapshot() == trace[-1]
    return d


def bad_cost_spec(value, at):
    return scenario(4, 5, 8, 1, 3, char_discount=0.5, bad=(at, value))


def run_error_1(device, lib):
    for value in (numpy.inf, -numpy.inf, numpy.nan):
        for at in (0, 2):
            m = Driver(lib, device, [bad_cost_spec(value, at)]).run().models[0]
            assert (m.err, m.done, m.pos, m.steps) == (1, 1, at, at)


# ---- grouped launches ---------------------------------------------------------------------------------------------------------------
def grouped_specs(name):
    if name == "three_ends":          # limits (5, 40, 17): the limit, the patience rule and an emptied beam end one search each
        shared = dict(K=6, V=9, eol=8, stop_on=0, char_discount=0.0)
        return [dict(shared, limit=5, seed=0), dict(shared, limit=40, seed=10, eol_bias=3.0),
                dict(shared, limit=17, seed=3, grid=1.0, eol_bias=(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -40.0))]
    if name == "optimistic_wide":
        shared = dict(K=70, V=29, eol=0, stop_on=1, char_discount=0.5, fin_cap=70 * 33)        # (K * (history capacity + 1))
        return [dict(shared, limit=limit, seed=seed, eol_bias=-2.0) for seed, limit in ((0, 3), (2, 9), (0, 1), (1, 6))]
    raise KeyError(name)


GROUPED = {"three_ends": dict(D=90, Tp=259, fork_rows=8), "optimistic_wide": dict(D=12, Tp=5, fork_rows=None)}


def run_grouped(device, lib, name):
    specs = grouped_specs(name)
    ends = [simulate(s)[0] for s in specs]
    if name == "three_ends":
        assert sorted(m.done for m in ends) == [1, 2, 3] and len(set(m.steps for m in ends)) == 3
    else:          # two searches stop by the optimistic rule, two at their limits, all at different positions
        assert sorted(m.done for m in ends) == [1, 1, 3, 3] and len(set(m.steps for m in ends)) == len(specs)
    d = Driver(lib, device, specs, reuse=True, fork=True, **GROUPED[name]).run()
    assert d.seen9 == {0, 1}, "the reuse flag must take both values"
    assert [m.snapshot()[0] for m in d.models] == [m.snapshot()[0] for m in ends]
    if GROUPED[name]["fork_rows"] is not None:
        assert d.fork_outside > 0, "no chosen character lay outside the fork's rows"
    return d


def run_reuse_without_centres(device, lib):
    """Expanding prior (no window centres): the second attention pass always repeats the first."""
    d = Driver(lib, device, [SINGLE["plain_patience"]], pos=False, reuse=True).run()
    m = d.models[0]
    assert d.seen9 == {1} and d.ctl10[0] == m.steps > 0


# ---- lvsr_topk_smallest alone -------------------------------------------------------------------------------------------------------
TOPK_N = (1, 255, 256, 257, 8191, 8192)
TOPK_K = (1, 2, 63, 64, 65, 255, 256)


def topk_keys(kind, n, rng):
    if kind == "normal":
        return rng.standard_normal(n).astype(F32)
    if kind == "all_equal":
        return numpy.full(n, 1.5, F32)
    if kind == "two_values":
        return numpy.where(rng.randint(0, 2, n) == 1, F32(2.0), F32(-3.0)).astype(F32)
    if kind == "low_8_bits":
        return (numpy.uint32(0x3f800000) + rng.randint(0, 1 << 8, n).astype(numpy.uint32)).view(F32)
    if kind == "low_16_bits":
        return (numpy.uint32(0x3f800000) + rng.randint(0, 1 << 16, n).astype(numpy.uint32)).view(F32)
    if kind == "mixed_signs":
        return (rng.randint(1, 50, n) * rng.choice([-0.5, 0.5], n)).astype(F32)
    if kind == "extremes":
        pool = numpy.array([1e-45, -1e-45, 3e-39, -3e-39, numpy.inf, -numpy.inf, 1e30, -1e30, 2e30, 1.0, -1.0, 1e-38], F32)
        return pool[rng.randint(0, len(pool), n)]
    raise KeyError(kind)


TOPK_KINDS = ("normal", "all_equal", "two_values", "low_8_bits", "low_16_bits", "mixed_signs", "extremes")


def call_topk(lib, device, keys, k):
    x = torch.from_numpy(keys).to(device)
    idx = torch.full((k + 3,), SENT_I, dtype=torch.int64, device=device)
    val = torch.full((k + 3,), SENT, dtype=torch.float32, device=device)
    lib.call("lvsr_topk_smallest", lib.stream_for(x), ptr(x), len(keys), k, ptr(idx), ptr(val))
    return idx.cpu().numpy(), val.cpu().numpy()


def run_topk(device, lib):
    cases = 0
    for kind in TOPK_KINDS:
        for n in TOPK_N:
            rng = numpy.random.RandomState(zlib.crc32(("%s %d" % (kind, n)).encode()))
            keys = topk_keys(kind, n, rng)
            assert not numpy.signbit(keys[keys == 0]).any() and not numpy.isnan(keys).any()
            order = numpy.lexsort((numpy.arange(n), keys))
            for k in TOPK_K:
                if kind != "normal" and n > 257 and k not in (1, 64, 255, 256):          # (the full grid for one distribution)
                    continue
                idx, val = call_topk(lib, device, keys, k)
                nsel = min(k, n)
                same(idx[:nsel], order[:nsel].astype(I64), "top-k indices, %s n=%d k=%d" % (kind, n, k))
                same(val[:nsel], keys[order[:nsel]], "top-k values, %s n=%d k=%d" % (kind, n, k))
                assert (idx[nsel:] == SENT_I).all() and (val[nsel:] == SENT).all(), "written beyond min(k, n)"
                cases += 1
    assert cases > 150
    # both zeros: -0.0 sorts before +0.0 only in the bit pattern; what test_emu_beam.check_smallest asserts for it, no more
    keys = numpy.zeros(300, F32)
    keys[::2] = -0.0
    keys[7::20] = 0.5
    idx, val = call_topk(lib, device, keys, 40)
    assert numpy.allclose(val[:40], numpy.sort(keys)[:40]) and len(set(idx[:40].tolist())) == 40 and (keys[idx[:40]] == val[:40]).all()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def run_refusals(lib):
    def refused(message, spec=None, topk=None, drop=(), **override):
        if topk is not None:
            n, k = topk
            x = torch.zeros(max(n, 1))
            idx, val = torch.full((300,), SENT_I, dtype=torch.int64), torch.full((300,), SENT, dtype=torch.float32)
            with pytest.raises(native.NativeError, match=message):
                lib.call("lvsr_topk_smallest", lib.stream_for(x), ptr(x), n, k, ptr(idx), ptr(val))
            assert (idx == SENT_I).all() and (val == SENT).all()
            return
        d = Driver(lib, "cpu", [spec or SINGLE["plain_patience"]], reuse=True, fork=True)
        args = d.make_args(**dict(override, **{name: None for name in drop}))
        with pytest.raises(native.NativeError, match=message):
            d.select(args)
        d.check_state("after a refused launch")                   # nothing ran: reset values and sentinels everywhere
        for name in ("S_sel", "W_sel", "fork_xg", "WA_sel"):
            assert (d.down(name) == SENT).all(), name

    small = dict(limit=4, stop_on=0, seed=0, eol=0)
    refused("lvsr_beam_select: beam 257 x 3 characters exceeds the kernel's capacity", dict(small, K=257, V=3))
    assert 3 * 2731 == 8193
    refused("lvsr_beam_select: beam 3 x 2731 characters exceeds the kernel's capacity", dict(small, K=3, V=2731))
    refused("lvsr_beam_select: finished list shorter than 2 \\* beam", fin_cap=2 * 4 - 1)
    refused("lvsr_beam_select: unknown stopping criterion 2", stop_on=2)
    refused("lvsr_beam_select: null state buffer", drop=("hist_cost",))
    refused("lvsr_beam_select: null state buffer", drop=("keep",))
    refused("lvsr_beam_select: null row buffers", drop=("S_sel",))
    refused("lvsr_beam_select: incomplete description of the attention results to reuse", drop=("WA_sel",))
    refused("lvsr_beam_select: incomplete description of the attention results to reuse", drop=("pos1_sel",))
    refused("lvsr_beam_select: incomplete fork description", drop=("fork_Wi",))
    refused("lvsr_beam_select: bad number of searches", groups=65536)
    refused("lvsr_topk_smallest: n <= 8192 and k <= 256", topk=(8193, 4))
    refused("lvsr_topk_smallest: n <= 8192 and k <= 256", topk=(300, 257))
    refused("lvsr_topk_smallest: bad arguments", topk=(0, 4))


# ---- controls: the scenario set tells the rules apart ---------------------------------------------------------------------------
MUTANTS = {          # mutant -> the scenarios of which at least one must tell it from the true model
    "ties_descending": ("ties_across_the_cut", "ties_across_the_cut_optimistic"),
    "no_cut": ("cut_through_equal_scores", "capacity_finished"),
    "f32_rank": ("double_scores",),
    "reset_le": ("patience_runs_out",),
    "cut_on_empty": ("beam_empties",),
    "no_rti": ("round_to_inf",),
    "no_ife": ("ignore_first_eol",),
    "bound_pos": ("optimistic_stop",),
}


# ---- the tests ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SINGLE))
def test_beam_step_emulated(name):
    from emu import emu_lib
    run_single("cpu", emu_lib(), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SINGLE))
def test_beam_step_gpu(gpu_device, name):
    run_single(gpu_device, native.get(), name)


def test_beam_step_error_1_emulated():
    from emu import emu_lib
    run_error_1("cpu", emu_lib())


@pytest.mark.gpu
def test_beam_step_error_1_gpu(gpu_device):
    run_error_1(gpu_device, native.get())


@pytest.mark.parametrize("name", sorted(GROUPED))
def test_beam_step_grouped_emulated(name):
    from emu import emu_lib
    run_grouped("cpu", emu_lib(), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GROUPED))
def test_beam_step_grouped_gpu(gpu_device, name):
    run_grouped(gpu_device, native.get(), name)


def test_beam_reuse_without_centres_emulated():
    from emu import emu_lib
    run_reuse_without_centres("cpu", emu_lib())


@pytest.mark.gpu
def test_beam_reuse_without_centres_gpu(gpu_device):
    run_reuse_without_centres(gpu_device, native.get())


def test_topk_smallest_emulated():
    from emu import emu_lib
    run_topk("cpu", emu_lib())


@pytest.mark.gpu
def test_topk_smallest_gpu(gpu_device):
    run_topk(gpu_device, native.get())


def test_beam_refusals_emulated():
    from emu import emu_lib
    run_refusals(emu_lib())


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_beam_model_control(mutant):
    """A model with one rule replaced by a near miss leaves a different trace in at least one of the scenarios staged for that rule."""
    told = [name for name in MUTANTS[mutant] if simulate(SINGLE[name], mutant)[1] != simulate(SINGLE[name])[1]]
    assert told, "no scenario tells the mutant %s from the true model" % mutant


def test_beam_model_control_of_the_controls():
    """A mutant name no rule looks at changes nothing: traces differ by what the rules do, not by how a mutant's mirrors are sized."""
    for name in sorted(SINGLE):
        assert simulate(SINGLE[name], "changes_nothing")[1] == simulate(SINGLE[name])[1], name


def test_beam_model_grouped_limit_control():
    """A grouped search that stopped at the capacity of the history buffers instead of its own limit (ctl[16 g + 8]) shows in both
    grouped scenarios."""
    for name in sorted(GROUPED):
        specs = grouped_specs(name)
        cap = (max(s["limit"] for s in specs) + 31) // 32 * 32
        differ = 0
        for s in specs:
            true, wrong = new_model(s, cap=cap), new_model(s, limit=cap, cap=cap)
            while not (true.done and wrong.done):
                true.step(costs_of(s, true)), wrong.step(costs_of(s, wrong))
                if true.snapshot() != wrong.snapshot():
                    differ += 1
                    break
        assert differ >= 1, name


def test_beam_model_topk_control():
    """The top-k reference itself: a sort that is not stable, or one on the values alone, is told apart by the tied distributions."""
    rng = numpy.random.RandomState(0)
    keys = topk_keys("two_values", 257, rng)
    order = numpy.lexsort((numpy.arange(257), keys))
    assert not numpy.array_equal(order[:64], numpy.lexsort((-numpy.arange(257), keys))[:64])
    low = topk_keys("low_8_bits", 8192, rng)
    assert len(set(low.view(numpy.uint32) >> 8)) == 1 and len(set(low.tolist())) == 256
