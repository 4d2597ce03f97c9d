"""The forward attention step kernels (csrc/decoder_fwd.hip, the helpers of csrc/decoder.h, lvsr_attdec_glimpses of
csrc/decoder_persist.hip) called directly, one decoder step at a time, against a NumPy float64 restatement of the reference's step:
window, cut and paste and compute_weights of lvsr/bricks/attention.py:120-213, the true convolution of lvsr/expressions.py:28-54,
ShallowEnergyComputer, compute_weighted_averages and the GatedRecurrent step with the distributed glimpse.  Every intermediate
quantity is a function of its own (`m_*`), and every device buffer is compared with that function evaluated on what the DEVICE
produced one stage earlier (sW and CV for the energies, EN for the alignment, W slot 1 for the glimpse and the next centre, ...): errors
do not compound, and the only discrete quantity — the window centre — is recomputed in float32 from the device's own alignment in
the kernel's documented order (sequential float32 cumulative sum / sum; the expanding prior in double on the float32-rounded speeds).

The shapes are the smallest that cross each regime of the kernels' own tiling: both instantiations of attdec_conv_kernel with every
(begin % 4, end % 4) and c % 4, all four attdec_energy_mfma_kernel instantiations with and without filter padding and windows that end
inside a wave's 16 positions, every `rpw` branch, windows beyond 256 positions and the scalar path of ld4g in attdec_glimpse_kernel,
median crossings at the starts of the 64-position chunks of attdec_pos_of_row_wave, the padding and passes of attdec_group_wa_kernel,
ragged row groups, `skip`, `S_ld`, `label0`, graph replay.

Outputs lie inside larger buffers between sentinel bands and are pre-filled with the sentinel; the whole of every buffer is compared
(what a call must leave alone by the same comparison).  Inputs carry 1e30 in their padding: S_ld columns, and for single-label calls
every position of PA / A / Am outside the window the model expects (positions >= group_Tp[g] among them).  Every case first asserts ON
THE MODEL that it stages the situation it is named for.

Bars.  Exact: copied and integer-valued quantities, median centres, sentinels, pasted zeros, grouped versus single, graph versus eager.
Continuous: |got - ref64| <= c * 2^-24 * scale with scale from the model (energy: sum |w_e| + |e_bias|; sW / CV / WA: max |ref| of the
row; alignment, gates, candidate, state: 1; normaliser Z: max(1, Z): a sum of terms in [0, 1] carries its terms' relative errors; mean
centre: sum alpha[t] t).  c is NOT taken from the kernels: test_bars_from_float32_model evaluates this same model in plain float32
NumPy against float64 over all cases of this file and c = 4 x the largest error / (2^-24 scale) found, rounded up (the kernels add
in another order and use the 1-ulp hardware exp / rcp, 2e-7 absolute by csrc/common.h).  "Plain" means that the model's own sums
(convolution taps, normaliser, glimpse) run term after term: numpy.sum and numpy.convolve add in pairs / through a BLAS dot product,
which loses less than a float32 sum does.  The attended values are drawn around 2, not 0, so that a glimpse is no cancelling sum
whose own size says nothing about its error.  Measured ratio -> c:
    sW 3.29 -> 14     CV 14.7 -> 59 (1 023 taps)     EN 2.27 -> 10     Z 16.2 -> 65     W 7.15 -> 29 (1.7e-6; the alignment atol of
    tests/test_gpu_kernels.py, 2e-6, is the wider one)     WA 22.8 -> 92     mean centre 2.97 -> 12     gates 8.7 -> 35     RH 2 -> 8
    C 15.7 -> 63 (D = 250)     S 4.35 -> 18
Every checker prints its worst error as a share of its bar under `pytest -s`.

The `*_control` tests show that the case set tells the true model from nine near misses, and that a mutant that changes no rule is
not told apart."""
import ctypes
import zlib

import numpy
import pytest
import torch

from lvsr_amd import native

F32, F64, I32 = numpy.float32, numpy.float64, numpy.int32
SENT = F32(-777.25)       # outputs are pre-filled with it, and so are the bands around them
POISON = F32(1e30)        # the padding of inputs
GUARD = 16                # floats of a band
U24 = 2.0 ** -24
# quantity -> c of the bar c * 2^-24 * scale (module docstring; test_bars_from_float32_model keeps them honest)
BARS = dict(sW=14, CV=59, EN=10, ZB=65, W=29, WA=92, pos=12, gate=35, RH=8, C=63, S=18)
WORST = {}                # quantity -> largest error / bar seen since the last report()
OUTPUTS = ("S", "W", "pos", "WA", "EN", "ZB", "sW", "CV", "U", "R", "C", "RH")


def bits(a):
    a = numpy.ascontiguousarray(a)
    return a.view(numpy.uint32) if a.dtype == F32 else a


def same(got, ref, what):
    got, ref = numpy.ascontiguousarray(got), numpy.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, "%s: %s %s != %s %s" % (what, got.dtype, got.shape, ref.dtype, ref.shape)
    bad = numpy.flatnonzero(bits(got).ravel() != bits(ref).ravel())
    assert bad.size == 0, "%s: %d entries differ, first at %d: %r != %r" % (what, bad.size, bad[0], got.ravel()[bad[0]], ref.ravel()[bad[0]])


def report(family, device):
    for what in sorted(WORST):
        print("%-28s %-6s on %s: worst error = %.3g of its bar" % (family, what, device, WORST[what]))
    WORST.clear()


# ---- the model: one function per quantity; `dt` = the precision it is evaluated in, `mutant` = one rule replaced by a near miss ----
def m_centre(w, kind, mutant=None):
    """Window centre of one alignment row (float32, the kernel's documented order): 1 = mean, 2 = median."""
    w = numpy.asarray(w, F32)
    if kind == 1:
        return numpy.cumsum(w * numpy.arange(len(w), dtype=F32), dtype=F32)[-1]
    ge = ((numpy.cumsum(w, dtype=F32) - F32(0.5)) >= 0).astype(numpy.int8)
    d = ge[1:] - ge[:-1]
    if mutant == "no_carry":                 # the chunks of 64 positions do not know of each other: a crossing at 64 k is missed
        d[63::64] = 0
    if len(d) == 0:
        return F32(0)
    return F32(numpy.argmax(d) + (1 if mutant == "median_t" else 0))


def m_window(case, i, g, pos_i, mutant=None):
    """-> (begin, end) of the batch the rows of group g form at label i, (lo, hi) per row for the additional mask (None: expanding)."""
    rows = case.rows_of(g)
    length = case.len_of(g)
    if case.K == 0:
        return 0, length, None
    if case.prior == 0:
        step = float(case.step0 + i + case.word_of(g))
        begin, end = case.p[0] + step * float(F32(case.p[2])), case.p[1] + step * float(F32(case.p[3]))
        begin, end = max(0.0, min(length - 1.0, begin)), max(0.0, min(float(length), end))
        begin, end = int(numpy.floor(begin)), int(numpy.ceil(end))
        if mutant == "end_inclusive":
            end = min(length, end + 1)
        return begin, end, None
    p = numpy.asarray(pos_i, F32)[rows]
    lo, hi = numpy.floor(p - F32(case.p[0])), numpy.ceil(p + F32(case.p[1]))
    begin, end = int(max(0.0, lo.min())), int(min(float(length), hi.max()))
    if mutant == "end_inclusive":
        end = min(length, end + 1)
    return begin, max(end, begin), (lo, hi)


def m_mask(case, g, b, begin, end, lohi):
    """attended_mask_cut * additional_mask of row b (the r-th row of its batch) over the window."""
    m = case.x["Am"][begin:end, case.col(b)].astype(F64)
    if lohi is not None:
        r = b - case.rows_of(g).start
        t = numpy.arange(begin, end, dtype=F64)
        m = m * ((t > lohi[0][r]) & (t < lohi[1][r]))
    return m


def seq_sum(terms, dt):
    """Sum over axis 0, one term after the other (numpy.cumsum is sequential; numpy.sum adds in pairs, which in float32 loses less
    than the plain sum the bars are measured on)."""
    terms = numpy.asarray(terms, dt)
    return numpy.cumsum(terms, axis=0, dtype=dt)[-1] if terms.shape[0] else numpy.zeros(terms.shape[1:], dt)


def m_sW(S, Ws, dt):
    return S.astype(dt) @ Ws.astype(dt)


def m_conv(w_row, filters, c, begin, end, dt, mutant=None):
    """(K, Tp): the true convolution of the CUT alignment — 'full', then [c : c + n] of it: out[t] = sum_e f[e] * cut[t + c - e] —
    pasted into zeros.  Written tap by tap, so that in float32 it is a plain sequential float32 sum (numpy.convolve hands the sum to a
    BLAS dot product, whose blocked accumulation is not what "plain float32" loses)."""
    K, Tp, n, FW = filters.shape[0], len(w_row), end - begin, filters.shape[1]
    out = numpy.zeros((K, Tp), dt)
    if n > 0:
        padded = numpy.zeros(n + 2 * FW, dt)            # cut[j] at padded[FW + j]
        padded[FW:FW + n] = w_row[begin:end].astype(dt)
        for k in range(K):
            f = filters[k].astype(dt)
            if mutant == "correlation":
                f = f[::-1]
            acc = numpy.zeros(n, dt)
            for e in range(FW):
                acc += f[e] * padded[FW + c - e:FW + c - e + n]
            out[k, begin:end] = acc
    return out


def m_energy(PA_col, sW_row, CV_row, handler, w_e, e_bias, begin, end, dt):
    """(Tp): w_e . tanh(PA + sW + conv features @ handler) (+ bias), pasted into zeros."""
    out = numpy.zeros(PA_col.shape[0], dt)
    if end > begin:
        x = PA_col[begin:end].astype(dt) + sW_row.astype(dt)[None, :]
        if CV_row is not None:
            x = x + CV_row[:, begin:end].astype(dt).T @ handler.astype(dt)
        out[begin:end] = numpy.tanh(x) @ w_e.astype(dt) + (dt(e_bias) if e_bias is not None else dt(0))
    return out


def m_weights(EN_row, mask, normalizer, begin, end, dt, mutant=None):
    """-> (alignment pasted into zeros (Tp), Z, the unnormalised weights of the whole row for the `whole_row` mutant)."""
    e, mask = EN_row[begin:end].astype(dt), mask.astype(dt)
    if normalizer == 0:
        if e.size:
            keep = mask != 0 if (mutant == "max_unmasked" and (mask != 0).any()) else numpy.ones(e.size, bool)
            e = e - e[keep].max()
        u = numpy.exp(e)
    elif normalizer == 1:
        u = dt(1) / (dt(1) + numpy.exp(-e))
    else:
        u = numpy.maximum(e / dt(1 if mutant == "relu_no_div" else 1000), dt(0))
    u = u * mask
    Z = seq_sum(u, dt) + dt(0 if mutant == "no_all" else numpy.all(1 - mask))
    out = numpy.zeros(len(EN_row), dt)
    with numpy.errstate(all="ignore"):
        out[begin:end] = u / Z
    return out, Z


def m_wa(W_row, A_col, begin, end, dt):
    return seq_sum(W_row[begin:end].astype(dt)[:, None] * A_col[begin:end].astype(dt), dt)


def m_gates(S, xg, WA, Whg, Wdg, D, dt, mutant=None):
    """-> update, reset (B, D)"""
    g = S.astype(dt) @ Whg.astype(dt) + xg[:, D:].astype(dt) + WA.astype(dt) @ Wdg.astype(dt)
    g = dt(1) / (dt(1) + numpy.exp(-g))
    return (g[:, D:], g[:, :D]) if mutant == "gates_swapped" else (g[:, :D], g[:, D:])


def m_candidate(RH, xg, WA, Whh, Wdi, D, dt):
    return numpy.tanh(RH.astype(dt) @ Whh.astype(dt) + xg[:, :D].astype(dt) + WA.astype(dt) @ Wdi.astype(dt))


def m_state(C, U, S, ymask, dt):
    C, U, S = C.astype(dt), U.astype(dt), S.astype(dt)
    new = C * U + S * (dt(1) - U)
    if ymask is not None:
        m = ymask.astype(dt)[:, None]
        new = m * new + (dt(1) - m) * S
    return new


# ---- a case: sizes, prior, layout, and the inputs drawn for it ------------------------------------------------------------------
class Case(object):
    def __init__(self, name, Tp, B=2, L=1, E=5, D=6, M=7, K=0, c=0, prior=0, p=(0.0, 1e4, 0.0, 0.0), normalizer=0, phases=1,
                 group_rows=0, group_Tp=None, broadcast=False, step0=0, words=None, skip=None, S_ld=0, ymask=None, A_off=0, A_pad=0,
                 W0=None, pos0=None, mask=None, peak=False, label0=0, knob=0, poison_window=True, e_bias=None, staged=None,
                 fn="lvsr_attdec_fwd"):
        self.name, self.Tp, self.B, self.L, self.E, self.D, self.M, self.K, self.c = name, Tp, B, L, E, D, M, K, c
        self.prior, self.p, self.normalizer, self.phases, self.step0, self.label0 = prior, p, normalizer, phases, step0, label0
        self.group_rows, self.group_Tp, self.broadcast, self.words, self.skip = group_rows, group_Tp, broadcast, words, skip
        self.S_ld, self.ymask, self.A_off, self.A_pad, self.pos0, self.knob = S_ld, ymask, A_off, A_pad, pos0, knob
        self.e_bias, self.staged, self.fn = e_bias, staged, fn
        self.groups = B // group_rows if group_rows else 1
        self.ncol = self.groups if group_rows else (1 if broadcast else B)
        self.has_pos = K > 0 and prior != 0
        self.FW = 2 * c + 1
        self.ldS = S_ld or D
        self.ldA = E + A_pad
        rng = numpy.random.RandomState(zlib.crc32(name.encode()))
        f = lambda *shape, s=1.0: (s * rng.standard_normal(shape)).astype(F32)
        x = dict(S0=f(B, D), Ws=f(D, M, s=D ** -0.5), PA=f(Tp, self.ncol, M), A=f(Tp, self.ncol, E) + F32(2.0), Am=numpy.ones((Tp, self.ncol), F32),
                 w_e=f(M), filters=f(max(K, 1), self.FW, s=0.5), handler=f(max(K, 1), M),
                 Whg=f(D, 2 * D, s=D ** -0.5), Whh=f(D, D, s=D ** -0.5), Wdi=f(E, D, s=E ** -0.5), Wdg=f(E, 2 * D, s=E ** -0.5),
                 xg=f(L, B, 3 * D), WA_in=f(L, B, E))
        if normalizer != 0 and e_bias is None:
            self.e_bias = 0.375
        w = rng.gamma(0.3, 1.0, (B, Tp)) + 1e-3
        for b in range(B):
            w[b, self.len_of(self.group(b)):] = 0
        x["W0"] = (w / w.sum(axis=1, keepdims=True)).astype(F32)
        if W0 is not None:
            x["W0"] = numpy.array(W0, F32).reshape(B, Tp)
        if mask is not None:
            x["Am"] = numpy.array(mask, F32).reshape(Tp, self.ncol)
        if fn == "lvsr_attdec_glimpses":          # every slot of W is the caller's
            w = rng.gamma(0.3, 1.0, (L + 1, B, Tp)) + 1e-3
            x["W_all"] = (w / w.sum(axis=2, keepdims=True)).astype(F32)
        x["ymask"] = None if ymask is None else numpy.asarray(ymask, F32).reshape(L, B)
        self.x = x
        self.pos0_model = None
        if self.has_pos:
            self.pos0_model = numpy.asarray(pos0, F32) if pos0 is not None else numpy.array([m_centre(r, prior) for r in x["W0"]], F32)
        if peak:           # the largest energy near +90, at the last position of the (first) window
            x["w_e"] *= F32(90.0 / numpy.abs(x["w_e"]).sum())
            begin, end, _ = m_window(self, label0, 0, self.pos0_model)
            x["PA"][end - 1, :, :] = 20.0 * numpy.sign(x["w_e"])
        # 1e30 wherever PA / A / Am lie outside the window of their utterance (single-label calls: the window is known beforehand)
        self.expected_windows = None
        if poison_window and L == 1 and (phases & 1):
            self.expected_windows = [m_window(self, 0, g, self.pos0_model)[:2] for g in range(self.groups)]
            for col in range(self.ncol):
                begin, end = self.expected_windows[col if group_rows else 0]
                for context in ("PA", "A", "Am"):
                    x[context][:begin, col], x[context][end:, col] = POISON, POISON
                if prior == 0 and K > 0:
                    for b in range(B):
                        if self.col(b) == col:
                            x["W0"][b, :begin], x["W0"][b, end:] = POISON, POISON

    def group(self, b):
        return b // self.group_rows if self.group_rows else 0

    def col(self, b):
        return b // self.group_rows if self.group_rows else (0 if self.broadcast else b)

    def rows_of(self, g):
        return range(g * self.group_rows, (g + 1) * self.group_rows) if self.group_rows else range(self.B)

    def len_of(self, g):
        return self.group_Tp[g] if (self.group_rows and self.group_Tp is not None) else self.Tp

    def word_of(self, g):
        return 0 if self.words is None else self.words[g]

    def skipped(self, b):
        return self.skip is not None and self.skip[self.group(b)] != 0

    def init(self):
        """Every output buffer as the caller hands it over: slot 0 of the state slots filled, the sentinel everywhere else."""
        B, L, D, Tp, K = self.B, self.L, self.D, self.Tp, max(self.K, 1)
        o = dict(S=numpy.full((L + 1, B, self.ldS), POISON, F32), W=numpy.full((L + 1, B, Tp), SENT, F32),
                 pos=numpy.full((L + 1, B), SENT, F32), WA=numpy.full((L, B, self.E), SENT, F32), EN=numpy.full((L, B, Tp), SENT, F32),
                 ZB=numpy.full((L, B), SENT, F32), sW=numpy.full((L, B, self.M), SENT, F32), CV=numpy.full((L, B, K, Tp), SENT, F32))
        for name in ("U", "R", "C", "RH"):
            o[name] = numpy.full((L, B, D), SENT, F32)
        o["S"][:, :, :D] = SENT
        o["S"][0, :, :D] = self.x["S0"]
        o["W"][0] = self.x["W0"]
        if "W_all" in self.x:
            o["W"][:] = self.x["W_all"]
        if self.pos0 is not None:
            o["pos"][0] = self.pos0_model
        if not (self.phases & 1):
            o["WA"][:] = self.x["WA_in"]
        return o


# ---- the whole step on the model alone (the float32 twin that sets the bars, and the mutants of the controls) --------------------
def produce(case, dt=F64, mutant=None):
    """Every output buffer as the model computes it, stage after stage on its own float32-rounded results."""
    x, o, D = case.x, case.init(), case.D
    if case.fn == "lvsr_attdec_glimpses":
        for l in range(case.L):
            for b in range(case.B):
                o["WA"][l, b] = m_wa(o["W"][l + 1, b], x["A"][:, case.col(b)], 0, case.Tp, dt)
        return o
    if case.has_pos and (case.phases & 1) and not (case.phases & 4) and case.label0 == 0:
        o["pos"][0] = [m_centre(r, case.prior, mutant) for r in o["W"][0]]
    for i in range(case.label0, case.L):
        if case.phases & 1:
            for g in range(case.groups):
                begin, end, lohi = m_window(case, i, g, o["pos"][i] if case.has_pos else None, mutant)
                for b in case.rows_of(g):
                    if case.skipped(b):
                        continue
                    o["sW"][i, b] = m_sW(o["S"][i, b, :D], x["Ws"], dt)
                    cv = None
                    if case.K > 0:
                        cv = o["CV"][i, b] = m_conv(o["W"][i, b], x["filters"], case.c, begin, end, dt, mutant)
                    o["EN"][i, b] = m_energy(x["PA"][:, case.col(b)], o["sW"][i, b], cv, x["handler"], x["w_e"], case.e_bias, begin, end, dt)
                    w, Z = m_weights(o["EN"][i, b], m_mask(case, g, b, begin, end, lohi), case.normalizer, begin, end, dt, mutant)
                    o["W"][i + 1, b], o["ZB"][i, b] = w, Z
                    if mutant == "whole_row":       # the sum does not stop at the window: 1 / T' where the paste left nothing
                        full = numpy.full(case.Tp, 1.0 / case.Tp, dt)
                        full[begin:end] = o["W"][i + 1, b, begin:end]
                        o["WA"][i, b] = m_wa(full, x["A"][:, case.col(b)], 0, case.len_of(g), dt)
                    else:
                        o["WA"][i, b] = m_wa(o["W"][i + 1, b], x["A"][:, case.col(b)], begin, end, dt)
                    if case.has_pos:
                        o["pos"][i + 1, b] = m_centre(o["W"][i + 1, b], case.prior, mutant)
        if case.phases & 2:
            S, ym = o["S"][i, :, :D], None if x["ymask"] is None else x["ymask"][i]
            o["U"][i], o["R"][i] = m_gates(S, x["xg"][i], o["WA"][i], x["Whg"], x["Wdg"], D, dt, mutant)
            o["RH"][i] = S.astype(dt) * o["R"][i].astype(dt)
            o["C"][i] = m_candidate(o["RH"][i], x["xg"][i], o["WA"][i], x["Whh"], x["Wdi"], D, dt)
            o["S"][i + 1, :, :D] = m_state(o["C"][i], o["U"][i], S, ym, dt)
    return o


# ---- the comparison: every buffer, in full, each quantity against the model on the buffers one stage earlier ----------------------
def close(what, got, ref, scale, measure):
    """|got - ref| <= BARS[what] * 2^-24 * scale, element by element; `measure` collects error / (2^-24 scale) instead."""
    got, ref = numpy.asarray(got, F64), numpy.asarray(ref, F64)
    assert got.shape == ref.shape and numpy.isfinite(got).all(), "%s: shape or non-finite values" % what
    unit = U24 * numpy.broadcast_to(numpy.asarray(scale, F64), ref.shape)
    err = numpy.abs(got - ref)
    ratio = float(numpy.max(numpy.where(err == 0, 0.0, err / numpy.where(unit > 0, unit, 1e-300)))) if err.size else 0.0
    if measure is not None:
        measure[what] = max(measure.get(what, 0.0), ratio)
        return
    bar = min(BARS[what], 2e-6 / U24) if what == "W" else BARS[what]        # (the suite's own bar where that is the tighter one)
    WORST[what] = max(WORST.get(what, 0.0), ratio / bar)
    assert ratio <= bar, "%s: worst error is %.3g x 2^-24 x scale, the bar %g" % (what, ratio, bar)


def verify(case, o, measure=None):
    """o: every output buffer after the call (payloads).  Raises AssertionError at the first quantity that misses its bar."""
    x, D, init = case.x, case.D, case.init()
    written = {k: numpy.zeros(v.shape, bool) for k, v in init.items()}
    labels = range(case.label0, case.L)
    if case.fn == "lvsr_attdec_glimpses":          # WA of every label, from the alignments the caller holds; nothing else
        for l in range(case.L):
            for b in range(case.B):
                ref = m_wa(o["W"][l + 1, b], x["A"][:, case.col(b)], 0, case.Tp, F64)
                close("WA", o["WA"][l, b], ref, numpy.abs(ref).max(), measure)
        written["WA"][:] = True
        labels = ()
    if case.has_pos and (case.phases & 1) and not (case.phases & 4) and case.label0 == 0 and labels:
        ref = numpy.array([m_centre(r, case.prior) for r in o["W"][0]], F32)
        if case.prior == 2:
            same(o["pos"][0], ref, "pos slot 0 (median)")
        else:
            mean = [float((r.astype(F64) * numpy.arange(case.Tp)).sum()) for r in o["W"][0]]
            close("pos", o["pos"][0], mean, mean, measure)
        written["pos"][0] = True
    for i in labels:
        if case.phases & 1:
            for g in range(case.groups):
                begin, end, lohi = m_window(case, i, g, o["pos"][i] if case.has_pos else None)
                if case.expected_windows is not None:
                    assert (begin, end) == case.expected_windows[g], "the window the poison was laid for"
                for b in case.rows_of(g):
                    written["sW"][i, b] = True
                    if case.skipped(b):
                        continue
                    ref = m_sW(o["S"][i, b, :D], x["Ws"], F64)
                    close("sW", o["sW"][i, b], ref, numpy.abs(ref).max(), measure)
                    cv = None
                    if case.K > 0:
                        cv, ref = o["CV"][i, b], m_conv(o["W"][i, b], x["filters"], case.c, begin, end, F64)
                        close("CV", cv, ref, numpy.abs(ref).max(axis=1, keepdims=True), measure)
                        outside = numpy.ones(case.Tp, bool)
                        outside[begin:end] = False
                        same(cv[:, outside], numpy.zeros((case.K, int(outside.sum())), F32), "CV outside the window")
                        written["CV"][i, b, :case.K] = True
                    ref = m_energy(x["PA"][:, case.col(b)], o["sW"][i, b], cv, x["handler"], x["w_e"], case.e_bias, begin, end, F64)
                    close("EN", o["EN"][i, b], ref, float(numpy.abs(x["w_e"]).sum()) + abs(case.e_bias or 0.0), measure)
                    same(o["EN"][i, b, :begin], numpy.zeros(begin, F32), "EN before the window")
                    same(o["EN"][i, b, end:], numpy.zeros(case.Tp - end, F32), "EN behind the window")
                    ref, Z = m_weights(o["EN"][i, b], m_mask(case, g, b, begin, end, lohi), case.normalizer, begin, end, F64)
                    close("W", o["W"][i + 1, b], ref, 1.0, measure)
                    close("ZB", o["ZB"][i, b], Z, max(1.0, Z), measure)
                    same(o["W"][i + 1, b, :begin], numpy.zeros(begin, F32), "W before the window")
                    same(o["W"][i + 1, b, end:], numpy.zeros(case.Tp - end, F32), "W behind the window")
                    ref = m_wa(o["W"][i + 1, b], x["A"][:, case.col(b)], begin, end, F64)
                    close("WA", o["WA"][i, b], ref, numpy.abs(ref).max(), measure)
                    for name in ("EN", "ZB", "WA"):
                        written[name][i, b] = True
                    written["W"][i + 1, b] = True
                    if case.has_pos:
                        w = o["W"][i + 1, b]
                        if case.prior == 2:
                            same(o["pos"][i + 1, b], m_centre(w, 2), "pos slot %d row %d (median)" % (i + 1, b))
                        else:
                            ref = float((w.astype(F64) * numpy.arange(case.Tp)).sum())
                            close("pos", o["pos"][i + 1, b], ref, ref, measure)
                        written["pos"][i + 1, b] = True
        if case.phases & 2:
            S, ym = o["S"][i, :, :D], None if x["ymask"] is None else x["ymask"][i]
            U, R = m_gates(S, x["xg"][i], o["WA"][i], x["Whg"], x["Wdg"], D, F64)
            close("gate", o["U"][i], U, 1.0, measure)
            close("gate", o["R"][i], R, 1.0, measure)
            close("RH", o["RH"][i], S.astype(F64) * o["R"][i].astype(F64), 1.0, measure)
            close("C", o["C"][i], m_candidate(o["RH"][i], x["xg"][i], o["WA"][i], x["Whh"], x["Wdi"], D, F64), 1.0, measure)
            close("S", o["S"][i + 1, :, :D], m_state(o["C"][i], o["U"][i], S, ym, F64), 1.0, measure)
            if ym is not None:          # a row whose label is masked keeps its state: a copy
                same(o["S"][i + 1, ym == 0, :D], S[ym == 0], "S of masked labels")
            for name in ("U", "R", "C", "RH"):
                written[name][i] = True
            written["S"][i + 1, :, :D] = True
    for name in OUTPUTS:             # what the call had no business with: bit for bit the caller's
        same(o[name][~written[name]], init[name][~written[name]], name + " outside what the call writes")


# ---- the device side ----------------------------------------------------------------------------------------------------------------
class Guarded(object):
    """A payload inside a larger device buffer, a band of sentinels on either side."""

    def __init__(self, payload, device, offset=0):
        payload = numpy.ascontiguousarray(payload)
        self.shape, self.n, self.lo = payload.shape, payload.size, GUARD + offset
        host = numpy.full(self.lo + self.n + GUARD, SENT if payload.dtype == F32 else -7, payload.dtype)
        host[self.lo:self.lo + self.n] = payload.ravel()
        self.before = host.copy()
        self.buf = torch.from_numpy(host).to(device)
        self.t = self.buf[self.lo:self.lo + self.n]

    def get(self, what):
        host = self.buf.cpu().numpy()
        same(host[:self.lo], self.before[:self.lo], what + ": the band before")
        same(host[self.lo + self.n:], self.before[self.lo + self.n:], what + ": the band behind")
        return host[self.lo:self.lo + self.n].reshape(self.shape).copy()

    def unchanged(self, what):
        same(self.buf.cpu().numpy(), self.before, what + " (must not change)")


class Call(object):
    """The argument block of a case over guarded buffers."""

    def __init__(self, lib, device, case, init=None):
        self.lib, self.device, self.case = lib, device, case
        x, B, D, E, M = case.x, case.B, case.D, case.E, case.M
        init = case.init() if init is None else init
        self.out = {name: Guarded(init[name], device) for name in OUTPUTS}
        A = numpy.full((case.Tp, case.ncol, case.ldA), POISON, F32)
        A[:, :, :E] = x["A"]
        self.inp = dict(A=Guarded(A, device, offset=case.A_off), PA=Guarded(x["PA"], device), Am=Guarded(x["Am"], device),
                        w_e=Guarded(x["w_e"], device), filters=Guarded(x["filters"], device), handler=Guarded(x["handler"], device),
                        xg=Guarded(x["xg"], device))
        self.scratch = dict(sg=Guarded(numpy.full((B, 2 * D), SENT, F32), device), xin=Guarded(numpy.full((B, D), SENT, F32), device),
                            ep=Guarded(numpy.full((B, (M + 31) // 32, case.Tp), SENT, F32), device))
        packs = {}
        for name, (K, N) in dict(Ws=(D, M), Whg=(D, 2 * D), Whh=(D, D), Wdi=(E, D), Wdg=(E, 2 * D)).items():
            packs[name] = torch.zeros(lib.pack_size(K, N), device=device)
            lib.pack_b(torch.from_numpy(x[name]).to(device), packs[name])
        self.packs = packs
        bs = 0 if (case.broadcast and not case.group_rows) else 1
        kw = dict(Tp=case.Tp, B=B, L=case.L, E=E, D=D, M=M, K=case.K, c=case.c, prior_type=case.prior, step0=case.step0,
                  phases=case.phases, normalizer=case.normalizer, p0=case.p[0], p1=case.p[1],
                  p2=float(F32(case.p[2])) if case.prior == 0 else 0.0, p3=float(F32(case.p[3])) if case.prior == 0 else 0.0,
                  A=self.inp["A"].t, PA=self.inp["PA"].t, Am=self.inp["Am"].t, A_ts=case.ncol * case.ldA, A_bs=bs * case.ldA,
                  PA_ts=case.ncol * M, PA_bs=bs * M, Am_ts=case.ncol, Am_bs=bs, Ws_p=packs["Ws"], w_e=self.inp["w_e"].t,
                  filters=self.inp["filters"].t if case.K else None, handler=self.inp["handler"].t if case.K else None,
                  Whg_p=packs["Whg"], Whh_p=packs["Whh"], Wdi_p=packs["Wdi"], Wdg_p=packs["Wdg"], xg=self.inp["xg"].t,
                  S=self.out["S"].t, W=self.out["W"].t, pos=self.out["pos"].t if case.has_pos else None, WA=self.out["WA"].t,
                  EN=self.out["EN"].t, ZB=self.out["ZB"].t, sW=self.out["sW"].t, CV=self.out["CV"].t if case.K else None,
                  U=self.out["U"].t, R=self.out["R"].t, C=self.out["C"].t, RH=self.out["RH"].t, sg=self.scratch["sg"].t,
                  xin=self.scratch["xin"].t, ep=self.scratch["ep"].t, S_ld=case.S_ld, label0=case.label0, group_rows=case.group_rows)
        if case.e_bias is not None:
            self.inp["e_bias"] = Guarded(numpy.array([case.e_bias], F32), device)
            kw["e_bias"] = self.inp["e_bias"].t
        if x["ymask"] is not None:
            self.inp["ymask"] = Guarded(x["ymask"], device)
            kw["ymask"] = self.inp["ymask"].t
        for name, words in (("step_dev", case.words), ("skip", case.skip)):        # one word per group, 16 ints apart
            if words is not None:
                a = numpy.full((len(words), 16), 5, I32)
                a[:, 0] = words
                self.inp[name] = Guarded(a, device)
                kw[name], kw[name.split("_")[0] + "_stride"] = self.inp[name].t, 16
        if case.group_rows and case.group_Tp is not None:
            self.inp["group_Tp"] = Guarded(numpy.asarray(case.group_Tp, I32), device)
            kw["group_Tp"] = self.inp["group_Tp"].t
        self.kw = kw

    def launch(self, fn="lvsr_attdec_fwd", use_graph=0, **override):
        args = self.lib.make("lvsr_attdec_args", **dict(self.kw, **override))
        stream = self.lib.stream_for(self.out["S"].t)
        before = self.lib.get_knob("energy_rows")
        if self.case.knob:
            self.lib.set_knob("energy_rows", self.case.knob)
        try:
            if fn == "lvsr_attdec_fwd":
                self.lib.call(fn, stream, ctypes.byref(args), use_graph)
            else:
                self.lib.call(fn, stream, ctypes.byref(args))
        finally:
            self.lib.set_knob("energy_rows", before)
        return self

    def results(self):
        """Every output payload; bands, scratch bands and inputs checked on the way."""
        for name, g in self.inp.items():
            g.unchanged("input " + name)
        for name, g in self.scratch.items():
            g.get("scratch " + name)
        return {name: g.get(name) for name, g in self.out.items()}


def run_cases(lib, device, cases, family):
    for case in cases:
        if case.staged is not None:
            case.staged(case, produce(case))             # the situation, on the model, before any kernel is asked
        try:
            verify(case, Call(lib, device, case).launch(case.fn).results())
        except AssertionError as e:
            raise AssertionError("%s: %s" % (case.name, e))
    report(family, device)


# ---- 1-3. the location convolution ----------------------------------------------------------------------------------------------------
def window_is(begin, end):
    def staged(case, o):
        assert m_window(case, 0, 0, case.pos0_model)[:2] == (begin, end), case.name
    return staged


def conv_alignment_cases():
    """Tp = 23, K = 3: every (begin % 4, end % 4) for every c % 4 (OFF, e_lo, e_hi, q0, nqw of attdec_conv_kernel)."""
    cases, seen = [], set()
    windows = [(b, e) for b in (4, 5, 6, 7) for e in (16, 17, 18, 19)] + [(0, 1), (22, 23), (0, 23)]
    for c in range(6):
        for begin, end in windows:
            seen.add((begin % 4, end % 4))
            cases.append(Case("conv_align c=%d [%d,%d)" % (c, begin, end), 23, K=3, c=c, p=(begin + 0.25, end - 0.25, 0.0, 0.0),
                              staged=window_is(begin, end)))
    assert len(seen) == 16
    return cases


def conv_trim_cases():
    """c = 100, K = 10 at Tp = 200: kf = 5, nkg = 2; the taps that reach the window are a strict subset for most quads."""
    cases = [Case("conv_trim [%d,%d)" % w, 200, K=10, c=100, p=(w[0] + 0.5, w[1] - 0.5, 0.0, 0.0), staged=window_is(*w))
             for w in ((37, 148), (0, 1), (199, 200), (0, 200))]
    for Tp in (100, 101, 104, 105):          # 25, 26, 26 and 27 output quads (nq); kf is 5 at each of them: 1024 / 204 binds
        cases.append(Case("conv_trim Tp=%d" % Tp, Tp, K=10, c=100, p=(37.0, Tp - 3.0, 0.0, 0.0), staged=window_is(37, Tp - 3)))
    return cases


def conv_grid(case):
    """The split attdec_pre_grid documents: (small instantiation?, filters per work-group, filter groups)."""
    fw4 = (case.FW + 3) // 4 * 4
    small = case.Tp + fw4 + 16 <= 1536 and fw4 <= 1024
    kf = max(1, min(case.K, 256 // ((case.Tp + 3) // 4), (1024 if small else 4096) // fw4))
    return small, kf, (case.K + kf - 1) // kf


def conv_switch_cases(big):
    def staged(small, kf=None):
        def check(case, o):
            assert conv_grid(case)[0] == small and (kf is None or conv_grid(case)[1] == kf), (case.name, conv_grid(case))
        return check
    if big:
        return [Case("conv_limit", 4096, B=1, K=4, c=3, p=(5.0, 4093.0, 0.0, 0.0), staged=staged(False, 1))]
    return [Case("conv_switch Tp=1512", 1512, K=2, c=2, p=(5.0, 1509.0, 0.0, 0.0), staged=staged(True, 1)),
            Case("conv_switch Tp=1513", 1513, K=2, c=2, p=(5.0, 1510.0, 0.0, 0.0), staged=staged(False, 1)),
            Case("conv_switch c=511 Tp=496", 496, K=3, c=511, p=(3.0, 490.0, 0.0, 0.0), staged=staged(True, 1)),
            Case("conv_switch c=511 Tp=497", 497, K=3, c=511, p=(3.0, 491.0, 0.0, 0.0), staged=staged(False, 2))]


def test_conv_trim_stages_its_split():
    assert conv_grid(conv_trim_cases()[0]) == (True, 5, 2)


# ---- 4-5. energies ----------------------------------------------------------------------------------------------------------------------
def energy_content_cases():
    return [Case("energy_content Tp=%d M=%d" % (Tp, M), Tp, M=M) for Tp in (1, 63, 64, 65, 130) for M in (1, 31, 32, 33, 70)]


def energy_location_cases():
    """Every K of the four MFMA instantiations x every window length, M / begin % 4 / (end = Tp or not) cycling under them."""
    cases, Ks, lengths = [], (1, 4, 5, 8, 9, 12, 13, 16), (1, 15, 16, 17, 48, 49, 64, 65, 129)
    pairs, combos = set(), set()
    for ik, K in enumerate(Ks):
        for il, n in enumerate(lengths):
            begin, M, at_end = (1, 2, 3, 5, 6, 7)[3 * (il % 2) + ik % 3], (7, 32, 40)[il % 3], (ik + il) % 2 == 0
            combos.add((begin, M, at_end))
            Tp = begin + n + (0 if at_end else 3)
            pairs.add((n, at_end))
            cases.append(Case("energy_loc K=%d n=%d M=%d" % (K, n, M), Tp, B=2, M=M, K=K, c=2, p=(begin + 0.5, begin + n - 0.5, 0.0, 0.0),
                              staged=window_is(begin, begin + n)))
            assert begin % 4 != 0
    assert len(pairs) == 2 * len(lengths)
    assert all(len({x[i] for x in combos if x[j] == v}) > 1 for i in range(3) for j in range(3) if i != j for v in {x[j] for x in combos})
    return cases


# ---- 6. row groups ------------------------------------------------------------------------------------------------------------------------
def group_cases():
    """Three utterances of lengths (70, 37, 1), a position counter each: windows [2, 20), [5, 25), [0, 1)."""
    cases = []
    for rows in (1, 3, 8, 9, 16, 17, 70):
        for knob in ((0, 2, 32) if rows in (9, 70) else (0,)):
            cases.append(Case("groups rows=%d knob=%d" % (rows, knob), 70, B=3 * rows, K=2, c=2, M=33, group_rows=rows, group_Tp=(70, 37, 1),
                              p=(2.0, 20.0, 1.0, 1.5), step0=0, words=(0, 3, 7), knob=knob, staged=group_windows([(2, 20), (5, 25), (0, 1)])))
    return cases


def group_windows(want):
    def staged(case, o):
        assert [m_window(case, 0, g, case.pos0_model)[:2] for g in range(case.groups)] == want, case.name
    return staged


GROUP_SPANS = (1, 32, 33, 128, 129, 800)


def group_span_case():
    """attdec_group_wa_kernel: the padded terms per partial (J) and the rows per pass at every span; 17 rows are passes of 16 and 1 up
    to a span of 768, of 13 and 4 at 800."""
    want = [(3, 3 + n) for n in GROUP_SPANS]
    J = [max(4, (((n + 31) >> 5) + 3) & ~3) for n in GROUP_SPANS]
    assert J == [4, 4, 4, 4, 8, 28] and [max(1, min(16, 12288 // (32 * j))) for j in J] == [16, 16, 16, 16, 16, 13]
    return Case("group spans", 803, B=6 * 17, E=70, K=1, c=1, M=7, group_rows=17, group_Tp=tuple(3 + n for n in GROUP_SPANS),
                p=(3.0, 5000.0, 0.0, 0.0), staged=group_windows(want))


def single_of(case, g, i=0):
    """The ungrouped broadcast call (bs = 0) that decodes utterance g of a grouped case alone."""
    n, Tg = case.group_rows, case.len_of(g)
    rows = slice(g * n, (g + 1) * n)
    one = Case(case.name + " utterance %d" % g, Tg, B=n, E=case.E, D=case.D, M=case.M, K=case.K, c=case.c, prior=case.prior, p=case.p,
               normalizer=case.normalizer, broadcast=True, step0=case.step0 + case.word_of(g), poison_window=False, pos0=None if not case.has_pos or case.pos0 is None else case.pos0_model[rows])
    for name in ("Ws", "w_e", "filters", "handler"):
        one.x[name] = case.x[name]
    for name in ("PA", "A", "Am"):
        one.x[name] = numpy.ascontiguousarray(case.x[name][:Tg, g:g + 1])
    one.x["S0"], one.x["W0"] = case.x["S0"][rows], numpy.ascontiguousarray(case.x["W0"][rows, :Tg])
    one.e_bias = case.e_bias
    return one


def run_grouped_equals_single(lib, device, case):
    got = Call(lib, device, case).launch().results()
    verify(case, got)
    n = case.group_rows
    for g in range(case.groups):
        one = single_of(case, g)
        alone = Call(lib, device, one).launch().results()
        Tg, rows = one.Tp, slice(g * n, (g + 1) * n)
        for name in ("W", "EN", "WA"):
            a, b = got[name][-1][rows], alone[name][-1]
            same(a[:, :Tg] if name != "WA" else a, b, "%s of utterance %d: grouped == alone" % (name, g))


def skip_case():
    return Case("skip", 70, B=9, K=2, c=2, M=33, group_rows=3, prior=2, p=(2.5, 3.5, 0, 0), skip=(0, 1, 0), poison_window=False)


def many_workgroups_case():
    """More than 2048 work-groups of the energy kernel (16 slices x 65 groups x 2 tiles): every row of a group in one work-group,
    9 rows = a chunk of EN_RC and a tail of one."""
    case = Case("groups grid>2048", 100, B=65 * 9, M=512, K=1, c=1, E=3, group_rows=9, p=(2.0, 99.0, 0.0, 0.0))
    assert ((case.M + 31) // 32) * case.groups * ((case.Tp + 63) // 64) > 2048
    return case


def rows_per_workgroup(case):
    """The branch of lvsr_attdec_fwd's `rpw` choice a case takes, and its value."""
    rows = case.group_rows or 1
    grid = ((case.M + 31) // 32) * (case.groups if case.group_rows else case.B) * ((case.Tp + 63) // 64)
    if case.knob > 0:
        return "knob", min(case.knob, rows)
    if rows >= 64:
        return "wide", 32
    return ("one round", min(8, rows)) if grid <= 2048 else ("all", rows)


def test_row_group_cases_stage_every_rpw_branch():
    taken = {rows_per_workgroup(c) for c in group_cases() + [many_workgroups_case()]}
    assert {b for b, _ in taken} == {"knob", "wide", "one round", "all"}
    # 9 and 17 rows: whole chunks of EN_RC = 8 rows and a tail of one; 3: less than a chunk; 70 by 32: work-groups of 32, 32 and 6 rows
    assert {("one round", 8), ("one round", 3), ("all", 9), ("wide", 32), ("knob", 2), ("knob", 9), ("knob", 32)} <= taken


# ---- 7. softmax and glimpse ---------------------------------------------------------------------------------------------------------------
def glimpse_cases():
    cases = []
    for E in (1, 31, 32, 33, 100):                                  # 32 with nothing odd: the 16-byte loads of ld4g
        cases.append(Case("glimpse E=%d" % E, 40, B=1 if E == 32 else 2, E=E, broadcast=E == 32))
    cases.append(Case("glimpse A off by one float", 40, B=1, E=32, broadcast=True, A_off=1))
    cases.append(Case("glimpse A_ts % 4 != 0", 40, B=1, E=32, broadcast=True, A_pad=3))
    for n in (256, 257, 600):
        cases.append(Case("glimpse window %d" % n, n + 5, E=33, K=1, c=1, p=(2.0, n + 2.0, 0.0, 0.0), staged=window_is(2, n + 2)))
    for normalizer in (0, 1, 2):
        cases.append(Case("glimpse normalizer %d" % normalizer, 130, normalizer=normalizer, E=9))

    def peaked(case, o):
        begin, end, _ = m_window(case, 0, 0, None)
        assert (o["EN"][0].argmax(axis=1) == end - 1).all() and (o["EN"][0].max(axis=1) > 85).all() and end - begin == 300
    cases.append(Case("glimpse peak", 310, K=1, c=1, M=20, p=(4.0, 304.0, 0.0, 0.0), peak=True, staged=peaked))

    mask = numpy.ones((50, 3), F32)
    mask[:, 1] = 0                       # row 1: nothing attended at all
    mask[30:, 2] = 0                     # row 2: its utterance ends inside the window

    def masked(case, o):
        begin, end, _ = m_window(case, 0, 0, None)
        assert (begin, end) == (10, 44) and o["ZB"][0, 1] == 1 and (o["W"][1, 1] == 0).all() and (o["WA"][0, 1] == 0).all()
        assert (o["W"][1, 2, 30:] == 0).all() and o["W"][1, 2, 29] > 0 and o["EN"][0, 2].argmax() == 40
    cases.append(Case("glimpse masks", 50, B=3, K=1, c=1, p=(10.0, 44.0, 0.0, 0.0), mask=mask, staged=masked))
    cases[-1].x["PA"][40, 2, :] = 20.0 * numpy.sign(cases[-1].x["w_e"])        # row 2: the largest energy where its mask is 0

    def masked_centre(case, o):
        assert o["ZB"][0, 1] == 1 and (o["W"][1, 1] == 0).all() and o["pos"][1, 1] == 0
    cases.append(Case("glimpse all-masked centre", 50, B=3, K=1, c=1, prior=2, p=(20.5, 30.5, 0, 0), mask=mask, poison_window=False, staged=masked_centre))
    return cases


# ---- 8. window centres --------------------------------------------------------------------------------------------------------------------
def crossing_row(Tp, t):
    """cumsum < 0.5 before position t, >= 0.5 from it on."""
    w = numpy.zeros(Tp, F32)
    w[t] = 0.5
    w[:t] = 0.25 / max(t, 1)
    w[t + 1:] = 0.25 / max(Tp - t - 1, 1)
    return w


def centre_rows(Tp):
    """-> rows, the centres the reference's rule gives them."""
    rows, want = [], []
    for t in (1, 2, 63, 64, 65, 127, 128, 129, Tp - 1):
        rows.append(crossing_row(Tp, t)), want.append(t - 1)
    first = crossing_row(Tp, 5)
    first[0] = 0.625                             # alpha[0] >= 0.5: no crossing, argmax of zeros
    rows.append(first), want.append(0)
    rows.append(numpy.zeros(Tp, F32)), want.append(0)
    dyadic = numpy.zeros(Tp, F32)
    dyadic[[3, 7, 70]] = 0.25, 0.25, 0.5         # the sum equals 0.5 exactly at position 7
    rows.append(dyadic), want.append(6)
    f32 = numpy.zeros(Tp, F32)                   # 0.5 - 2^-25, then four quarter-ulps float32 drops and float64 keeps
    f32[0], f32[1:5], f32[5] = 0.5 - 2.0 ** -25, 2.0 ** -27, 0.25
    rows.append(f32), want.append(4)
    return numpy.array(rows, F32), want


def centre_cases():
    cases = []
    for Tp in (130, 200):
        rows, want = centre_rows(Tp)

        def staged(case, o, rows=rows, want=want):
            assert [int(m_centre(r, 2)) for r in rows] == want
            assert numpy.cumsum(rows[11], dtype=F32)[7] == 0.5                             # the dyadic row
            c64 = numpy.cumsum(rows[12].astype(F64))
            assert int(numpy.argmax(c64 >= 0.5)) - 1 == 3 and want[12] == 4                # float64 would put the centre at 3
            assert {int(m_centre(r, 2)) + 1 for r in rows} >= {64, 128}                    # crossings at the chunk starts
        cases.append(Case("centres median Tp=%d" % Tp, Tp, B=len(rows), K=1, c=1, prior=2, p=(2.5, 3.5, 0, 0), W0=rows, staged=staged))

    def margins(case, o):          # floor and ceil of the mean centres are 0.01 and more from a jump, at both labels' inputs
        for p in (case.pos0_model, o["pos"][1]):
            for edge in (p - F32(case.p[0]), p + F32(case.p[1])):
                assert (numpy.abs(edge - numpy.round(edge)) >= 0.01).all(), edge
    for seed in range(40):                       # the first draw that keeps the margins
        case = Case("centres mean %d" % seed, 130, B=3, K=1, c=1, prior=1, p=(6.5, 9.25, 0, 0), poison_window=False)
        try:
            margins(case, produce(case))
        except AssertionError:
            continue
        case.staged = margins
        cases.append(case)
        break
    assert cases[-1].prior == 1
    # windows that follow from the centres: the batch-wide window is the min / max over rows; each row's own mask is narrower
    rows = numpy.array([crossing_row(130, t) for t in (31, 64, 50)], F32)

    def narrow(case, o):
        assert m_window(case, 0, 0, case.pos0_model)[:2] == (27, 67) and list(case.pos0_model) == [30, 63, 49]
        assert (o["W"][1, 0, 35:] == 0).all() and (o["W"][1, 1, :60] == 0).all()
    cases.append(Case("centres windows", 130, B=3, K=2, c=3, prior=2, p=(2.5, 3.5, 0, 0), W0=rows, staged=narrow))

    def callers(case, o):          # phases bit 2: the caller's centres, not the alignment's
        assert list(case.pos0_model) == [17, 40, 100] and [int(m_centre(r, 2)) for r in case.x["W0"]] == [30, 63, 49]
        assert m_window(case, 0, 0, case.pos0_model)[:2] == (14, 104)
    cases.append(Case("centres from the caller", 130, B=3, K=2, c=3, prior=2, p=(2.5, 3.5, 0, 0), W0=rows, pos0=(17, 40, 100), phases=5, staged=callers))

    def empty(case, o):
        begin, end, _ = m_window(case, 0, 0, case.pos0_model)
        assert begin == end == 14 and (o["W"][1] == 0).all() and (o["ZB"][0] == 1).all() and (o["WA"][0] == 0).all()
    cases.append(Case("centres empty window", 40, B=2, K=1, c=1, prior=2, p=(-5.5, 2.5, 0, 0),
                      W0=numpy.array([crossing_row(40, 10)] * 2, F32), staged=empty))
    return cases


# ---- 9. the GRU part ------------------------------------------------------------------------------------------------------------------------
def gru_cases():
    cases, n = [], 0
    for B in (1, 16, 17, 33):
        for D in (4, 16, 20, 250):
            E = (3, 64, 70)[n % 3]
            ymask = None
            if n % 2:
                ymask = numpy.ones(B, F32)
                ymask[::3] = 0
            cases.append(Case("gru B=%d D=%d E=%d" % (B, D, E), 3, B=B, D=D, E=E, phases=2, S_ld=D + 3, ymask=ymask))
            n += 1
    assert {c.E for c in cases} == {3, 64, 70} and any(c.ymask is None for c in cases) and any(c.ymask is not None for c in cases)
    return cases


# ---- 10. chaining ---------------------------------------------------------------------------------------------------------------------------
def chain_cases():
    ymask = numpy.ones((4, 3), F32)
    ymask[2:, 1] = 0
    return [Case("chain expanding", 60, B=3, L=4, K=3, c=2, phases=3, p=(1.0, 12.0, 2.0, 9.5), ymask=ymask),
            Case("chain mean", 60, B=3, L=4, K=3, c=2, phases=3, prior=1, p=(8.5, 11.5, 0, 0), ymask=ymask),
            Case("chain median", 60, B=3, L=4, K=3, c=2, phases=3, prior=2, p=(8.5, 11.5, 0, 0), ymask=ymask, S_ld=9)]


def run_chain(lib, device, case, graph):
    eager = Call(lib, device, case).launch().results()
    verify(case, eager)
    # labels [0, 2) and [2, 4) in two calls on the same slots
    two = Call(lib, device, case)
    two.launch(L=2)
    two.launch(label0=2)
    halves = two.results()
    for name in OUTPUTS:
        same(halves[name], eager[name], "%s: label0 = 2 after an L = 2 call == one call" % name)
    if graph:
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            replayed = None
            for turn in ("capture", "replay"):
                call = Call(lib, device, case) if replayed is None else replayed
                if turn == "replay":          # the same buffers, handed over afresh
                    for name, g in call.out.items():
                        g.buf.copy_(torch.from_numpy(g.before))
                call.launch(use_graph=1)
                side.synchronize()
                replayed = call
                got = call.results()
                for name in OUTPUTS:
                    same(got[name], eager[name], "%s: graph (%s) == eager" % (name, turn))
        torch.cuda.current_stream(device).wait_stream(side)


# ---- 11. lvsr_attdec_glimpses ------------------------------------------------------------------------------------------------------------------
def glimpses_cases():
    """GL_LAB = 16 labels per work-group, 256 columns per work-group, the four-position unroll and its tail."""
    return [Case("glimpses L=%d E=%d Tp=%d" % (L, E, Tp), Tp, B=2, L=L, E=E, A_pad=1, fn="lvsr_attdec_glimpses")
            for Tp in (1, 512) for L in (1, 16, 17) for E in (1, 255, 256, 257)]


# ---- 12. refusals ---------------------------------------------------------------------------------------------------------------------------
def run_refusals(lib, device):
    def refused(message, case, fn="lvsr_attdec_fwd", **override):
        call = Call(lib, device, case)
        with pytest.raises(native.NativeError, match=message):
            call.launch(fn, **override)
        got, init = call.results(), case.init()
        for name in OUTPUTS:
            same(got[name], init[name], "%s after a refused call" % name)

    small = dict(B=1, E=2, D=2, M=2, poison_window=False)
    refused("lvsr_attdec_fwd: attended length 4097 > 4096", Case("r1", 4097, **small))
    refused("lvsr_attdec_fwd: match dim / conv filters / attended length exceed the LDS budget", Case("r2", 8, K=17, c=1, **small))
    assert 5 * 3277 == 16385
    refused("lvsr_attdec_fwd: match dim / conv filters / attended length exceed the LDS budget", Case("r3", 3277, K=5, c=1, **small))
    refused("lvsr_attdec_fwd: match dim / conv filters / attended length exceed the LDS budget", Case("r4", 8, **dict(small, M=1025)))
    refused("lvsr_attdec_fwd: conv filter too wide", Case("r5", 8, K=1, c=512, **small))
    refused("lvsr_attdec_fwd: window_around_\\* priors need pos", Case("r6", 8, K=1, c=1, prior=2, p=(2.5, 3.5, 0, 0), **small), pos=None)
    refused("lvsr_attdec_fwd: skip is for single-step", Case("r7", 8, L=2, skip=(0,), **small))
    refused("lvsr_attdec_fwd: the rows must be whole groups \\(B = 5, group_rows = 2\\)", Case("r8", 8, **dict(small, B=5)), group_rows=2)
    refused("lvsr_attdec_fwd: phases must select attention and/or GRU", Case("r9", 8, **small), phases=4)
    refused("lvsr_attdec_fwd: label0 outside \\[0, L\\)", Case("r10", 8, L=2, **small), label0=2)
    refused("lvsr_attdec_fwd: S_ld < D", Case("r11", 8, **small), S_ld=1)
    refused("lvsr_attdec_glimpses: attended length 513 > 512", Case("r12", 513, **small), fn="lvsr_attdec_glimpses")


# ---- the families ---------------------------------------------------------------------------------------------------------------------------
FAMILIES = {
    "conv_alignment": conv_alignment_cases, "conv_trim": conv_trim_cases, "conv_switch": lambda: conv_switch_cases(False),
    "conv_limit": lambda: conv_switch_cases(True), "energy_content": energy_content_cases, "energy_location": energy_location_cases,
    "groups": group_cases, "group_spans": lambda: [group_span_case()], "skip": lambda: [skip_case()], "glimpse": glimpse_cases,
    "centres": centre_cases, "gru": gru_cases, "chain": chain_cases, "glimpses": glimpses_cases,
}
GPU_ONLY = {"many_workgroups": lambda: [many_workgroups_case()]}            # (a minute and a half on the emulator: 2 080 work-groups)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_attention_step_emulated(family):
    from emu import emu_lib
    run_cases(emu_lib(), "cpu", FAMILIES[family](), family)


@pytest.mark.slow
@pytest.mark.parametrize("family", sorted(GPU_ONLY))
def test_attention_step_large_emulated(family):
    from emu import emu_lib
    run_cases(emu_lib(), "cpu", GPU_ONLY[family](), family)


@pytest.mark.gpu
@pytest.mark.parametrize("family", sorted(FAMILIES) + sorted(GPU_ONLY))
def test_attention_step_gpu(gpu_device, family):
    run_cases(native.get(), gpu_device, dict(FAMILIES, **GPU_ONLY)[family](), family)


def grouped_equals_single_cases():
    return [c for c in group_cases() if c.group_rows in (3, 17) and c.knob == 0] + [group_span_case()]


def test_grouped_equals_single_emulated():
    from emu import emu_lib
    for case in grouped_equals_single_cases():
        run_grouped_equals_single(emu_lib(), "cpu", case)


@pytest.mark.gpu
def test_grouped_equals_single_gpu(gpu_device):
    for case in grouped_equals_single_cases():
        run_grouped_equals_single(native.get(), gpu_device, case)


@pytest.mark.parametrize("name", [c.name for c in chain_cases()])
def test_chain_label0_emulated(name):
    from emu import emu_lib
    run_chain(emu_lib(), "cpu", [c for c in chain_cases() if c.name == name][0], graph=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in chain_cases()])
def test_chain_label0_and_graph_gpu(gpu_device, name):
    run_chain(native.get(), gpu_device, [c for c in chain_cases() if c.name == name][0], graph=True)


def test_refusals_emulated():
    from emu import emu_lib
    run_refusals(emu_lib(), "cpu")


@pytest.mark.gpu
def test_refusals_gpu(gpu_device):
    run_refusals(native.get(), gpu_device)


# ---- the bars and the controls: CPU only, the model alone ---------------------------------------------------------------------------------------
def all_cases():
    every = dict(FAMILIES, **GPU_ONLY)
    return [c for family in sorted(every) for c in every[family]()]


def test_bars_from_float32_model():
    """c of every bar is (at least) 4 x what plain float32 NumPy loses on this model over all cases, and the model in float64 passes
    its own comparison."""
    measure = {}
    for case in all_cases():
        verify(case, produce(case, F32), measure)
        verify(case, produce(case, F64))
    WORST.clear()
    print("float32 model, worst error / (2^-24 scale): " + ", ".join("%s %.3g" % kv for kv in sorted(measure.items())))
    for what, ratio in measure.items():
        assert 4 * ratio <= BARS[what], "%s: float32 NumPy alone is %.3g x 2^-24 x scale off, c = %g" % (what, ratio, BARS[what])


MUTANTS = {          # mutant -> the families of which at least one case must tell it from the true model
    "correlation": ("conv_alignment",), "end_inclusive": ("conv_alignment", "energy_location"), "max_unmasked": ("glimpse",),
    "no_all": ("glimpse",), "median_t": ("centres",), "no_carry": ("centres",), "relu_no_div": ("glimpse",), "whole_row": ("glimpse",),
    "gates_swapped": ("gru",),
}


def told_apart(mutant, families):
    told = []
    for family in families:
        for case in FAMILIES[family]():
            try:
                verify(case, produce(case, F64, mutant))
            except AssertionError:
                told.append(case.name)
    WORST.clear()
    return told


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_model_control(mutant):
    assert told_apart(mutant, MUTANTS[mutant]), "no case tells the mutant %s from the true model" % mutant


def test_model_control_of_the_controls():
    assert not told_apart("changes_nothing", sorted(set(f for fs in MUTANTS.values() for f in fs)))
