"""lvsr_opt_step: the default sequence (the rules and max-norm kernels test their steps for RemoveNotFinite as they go, the norm kernel
clears the flags, the apply kernel runs on a wider grid) against the sequence with a test pass of its own (knob opt_unfused = 1), BIT for
bit on everything the step writes.  Direct calls on a segment table of this file's own: the bodies run on the CPU emulator (same
sources) and, under the `gpu` marker, on the device."""
import ctypes

import numpy
import pytest
import torch

from emu import emu_lib

# (rows, cols, max-norm flag): whole 64-column blocks and 16-row groups; ragged in both; one row; fewer rows than row groups with more
# than one column block; 1-D tensors of 1 and 257 elements (walked flat); a 2-D tensor without the flag
SEGMENTS = [(16, 64, 1), (17, 65, 1), (1, 33, 1), (5, 200, 1), (1, 1, 0), (1, 257, 0), (9, 70, 0)]
MAX_NORM = 0.9
BASE = dict(use_momentum=1, use_adadelta=1, remove_not_finite=1, clip_threshold=2.0, learning_rate=0.5, momentum=0.3, decay_rate=0.9,
            epsilon=1e-6, max_norm=MAX_NORM, nonfinite_scaler=0.1, grad_scale=0.25)


def _layout():
    """-> (segment table rows [offset, rows, cols, flag], total): every tensor 16-byte aligned, as ParameterStore lays them out."""
    table, total = [], 0
    for rows, cols, flag in SEGMENTS:
        table.append([total, rows, cols, flag])
        total += (rows * cols + 3) // 4 * 4
    return table, total


def _initial(seed):
    """Parameters, the gradients of two steps and rule state.  Column 0 of every flagged segment (small values, small gradients) ends
    far below max_norm, column 1 far above, the others near it; the padding between tensors holds zero gradients, as in a training
    step, and rule state, which the rules move."""
    table, n = _layout()
    rng = numpy.random.RandomState(seed)
    param = numpy.zeros(n, numpy.float32)
    grads = numpy.zeros((2, n), numpy.float32)
    for off, rows, cols, flag in table:
        p = rng.normal(0, MAX_NORM / numpy.sqrt(rows), size=(rows, cols)).astype(numpy.float32)
        if flag:
            p[:, 0] *= 0.01
            if cols > 1:
                p[:, 1] *= 10.0
        param[off: off + rows * cols] = p.ravel()
        g = rng.normal(0, 1.0, size=(2, rows, cols))
        if flag:
            g[:, :, 0] *= 0.01
        grads[:, off: off + rows * cols] = g.reshape(2, rows * cols)
    state = dict(param=param, velocity=rng.normal(0, 0.1, n).astype(numpy.float32),
                 ms_step=rng.uniform(0, 0.1, n).astype(numpy.float32), ms_dx=rng.uniform(0, 0.1, n).astype(numpy.float32),
                 step=rng.normal(0, 1.0, n).astype(numpy.float32))
    return table, n, state, grads


def _run(device, lib, unfused, conf, poison=None, poison_param=None, guard=None, clip_state=None, seed=5):
    """Two consecutive optimiser steps -> [everything the steps wrote, after each]."""
    table, n, state, grads = _initial(seed)
    for seg, value in poison_param or ():
        state["param"][table[seg][0] + 5] = value
    if poison:
        for seg, value in poison:
            grads[0, table[seg][0] + 2 % (table[seg][1] * table[seg][2])] = value
    t = {k: torch.tensor(v, device=device) for k, v in state.items()}
    segments = torch.tensor(table, dtype=torch.int64, device=device)
    segflag = torch.full((len(table),), 7, dtype=torch.int32, device=device)
    scratch = torch.zeros(2 + 256, dtype=torch.float32, device=device)
    cs = None if clip_state is None else torch.tensor(clip_state, dtype=torch.float64, device=device)
    gw = None if guard is None else torch.tensor([guard], dtype=torch.float32, device=device)
    max_cols = max(cols for _, cols, flag in SEGMENTS if flag)
    out = []
    lib.set_knob("opt_unfused", int(unfused))
    try:
        for it in range(2):
            grad = torch.tensor(grads[it], device=device)
            a = lib.make("lvsr_opt_args", param=t["param"], grad=grad, velocity=t["velocity"] if conf["use_momentum"] else None,
                         ms_step=t["ms_step"] if conf["use_adadelta"] else None, ms_dx=t["ms_dx"] if conf["use_adadelta"] else None,
                         step=t["step"], segments=segments, segflag=segflag, scratch=scratch, n=n, nseg=len(table), max_cols=max_cols,
                         clip_state=cs, guard=gw, **conf)
            lib.call("lvsr_opt_step", lib.stream_for(t["param"]), ctypes.byref(a))
            got = {k: v.cpu().numpy().copy() for k, v in t.items()}
            got.update(segflag=segflag.cpu().numpy().copy(), scratch=scratch.cpu().numpy().copy())
            if cs is not None:
                got["clip_state"] = cs.cpu().numpy().copy()
            out.append(got)
    finally:
        lib.set_knob("opt_unfused", 0)
    return out


def _same(a, b, what):
    for it, (x, y) in enumerate(zip(a, b)):
        assert sorted(x) == sorted(y)
        for k in x:
            # (bit patterns: NaNs compare too)
            bx, by = x[k].view(numpy.uint8), y[k].view(numpy.uint8)
            assert (bx == by).all(), "%s: %s differs after step %d (%d elements)" % (what, k, it, int((x[k] != y[k]).sum()))


ADAPTIVE = dict(BASE, clip_threshold=30.0, adaptive_clipping=1, adaptive_burnin=4, adaptive_decay=0.9)
CASES = {
    "momentum_adadelta": dict(conf=BASE),
    "adadelta_only": dict(conf=dict(BASE, use_momentum=0)),
    "momentum_only": dict(conf=dict(BASE, use_adadelta=0)),
    "plain": dict(conf=dict(BASE, use_momentum=0, use_adadelta=0)),
    # (no StepClipping: a non-finite gradient stays in its own tensor) a NaN in a flagged segment, an inf in a flat one
    "nan_and_inf": dict(conf=dict(BASE, clip_threshold=0.0), poison=[(1, numpy.nan), (5, numpy.inf)]),
    "nan_without_remove_not_finite": dict(conf=dict(BASE, clip_threshold=0.0, remove_not_finite=0), poison=[(3, numpy.nan)]),
    # a parameter that is not finite: its column norm is not, the max-norm rescaling makes the column's steps NaN
    "inf_parameter": dict(conf=dict(BASE, clip_threshold=0.0), poison_param=[(0, numpy.inf)]),
    "guarded": dict(conf=BASE, guard=1.0),
    "burn_in": dict(conf=ADAPTIVE, clip_state=[30.0, 0, 0, 0, 1.0, 0, 0, 0]),
    "adaptive_clipping": dict(conf=ADAPTIVE, clip_state=[30.0, 0, 0, 0, 0, 0, 0, 0]),
}


def run_case(device, lib, name):
    case = CASES[name]
    fused, unfused = _run(device, lib, False, **case), _run(device, lib, True, **case)
    _same(fused, unfused, name)
    table, n, state, _ = _initial(5)
    first = fused[0]
    if name == "guarded":               # nothing may change, the flags included
        for k, v in state.items():
            assert (first[k] == v).all(), k
        assert (first["segflag"] == 7).all() and first["scratch"][3] == 1.0
        return
    assert first["scratch"][3] == 0.0
    if name == "nan_and_inf":           # the poisoned tensors are flagged and scaled, the others stepped
        assert first["segflag"].tolist() == [0, 1, 0, 0, 0, 1, 0]
        for seg in (1, 5):
            off, rows, cols, _ = table[seg]
            want = state["param"][off: off + rows * cols] - numpy.float32(1.0 - 0.1) * state["param"][off: off + rows * cols]
            numpy.testing.assert_allclose(first["param"][off: off + rows * cols], want, rtol=1e-6)
        assert numpy.isfinite(fused[1]["param"]).all()
        return
    if name == "inf_parameter":
        assert first["segflag"].tolist() == [1, 0, 0, 0, 0, 0, 0]
        return
    if name == "nan_without_remove_not_finite":
        assert (first["segflag"] == 0).all() and numpy.isnan(first["param"]).any()
        return
    assert (first["segflag"] == 0).all()
    if name == "burn_in":               # the first step is multiplied by zero (rule state moves), the second applies
        assert (first["param"] == state["param"]).all() and not (first["ms_step"] == state["ms_step"]).all()
        assert not (fused[1]["param"] == state["param"]).all() and first["clip_state"][4] == 0.0
        return
    # max-norm did its work: column 1 of every flagged segment sits at max_norm, column 0 far below, and both kinds occur elsewhere
    for off, rows, cols, flag in table:
        if flag:
            norms = numpy.sqrt((first["param"][off: off + rows * cols].reshape(rows, cols).astype(numpy.float64) ** 2).sum(0))
            assert norms.max() <= MAX_NORM * (1 + 1e-4) and norms[0] < 0.5 * MAX_NORM
            if cols > 1:
                assert abs(norms[1] - MAX_NORM) < 1e-4 * MAX_NORM
    if name == "adaptive_clipping":
        assert first["clip_state"][3] == 1.0 and fused[1]["clip_state"][3] == 2.0 and fused[1]["clip_state"][0] != 30.0


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_equals_unfused_emulated(name):
    run_case("cpu", emu_lib(), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_equals_unfused_gpu(gpu_device, name):
    from lvsr_amd import native
    run_case(gpu_device, native.get(), name)
