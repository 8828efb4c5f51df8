"""The window's profiling entry points (sage_window_set_profiling / _get_kernel_time / _get_phase_time) on the GPU: what
bench.py and sage_window_tune_runs read.  Levels 1, 2 and 0 on the smoke window; reads drain.  The expected launch and
iteration counts follow from the LM sequence's code (one evaluation per step); they have not yet been read off the library
as it was before the profiler got a file of its own (profiles/window_state_refactor_ab.txt)."""
import math

import pytest

from sage_slam_amd import synth

pytestmark = pytest.mark.gpu

STEPS = 2
# level 1, two lm_step calls of the classic sequence with one evaluation each: one photometric and one geometric linearize
# per step; one error pass per step, in which the photometric kernel evaluates the geometric edges too (no geometric error
# launch).  One iteration of phase marks per step
LAUNCHES_LEVEL1 = {0: STEPS, 1: STEPS, 2: STEPS, 3: 0}
ITERATIONS_LEVEL1 = STEPS
LAUNCHES_LEVEL2 = {0: STEPS, 1: 0, 2: 0, 3: 0}  # the photometric linearize only, no phase marks


def _steps(capi, win, n):
    st, cfg = capi.SageLmState(), capi.lm_config_default()
    cfg.max_inner_evals = 1     # one evaluation per step, accepted or not: the counts below do not depend on the decisions
    for _ in range(n):
        win.lm_step(st, cfg)
    return st


def _read_all(win):
    kernels = {which: win.kernel_time(which) for which in range(4)}
    ms4, iters = win.phase_time()
    return kernels, ms4, iters


def _assert_drained(win):
    kernels, ms4, iters = _read_all(win)
    assert all(n == 0 and ms == 0.0 for ms, n in kernels.values()), kernels
    assert iters == 0 and all(v == 0.0 for v in ms4.values())


def test_profiling_levels_and_draining_reads():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from sage_slam_amd import capi
    w = synth.make_window(K=3, H=64, W=80, FS=16, CS=32, L=4, seed=3)
    win = capi.Window(w)

    win.set_profiling(1)
    _steps(capi, win, STEPS)
    kernels, ms4, iters = _read_all(win)
    print("level 1:", kernels, ms4, iters)
    assert {which: n for which, (_, n) in kernels.items()} == LAUNCHES_LEVEL1
    assert iters == ITERATIONS_LEVEL1
    for ms, n in kernels.values():
        assert math.isfinite(ms) and ms >= 0.0 and (ms > 0.0) == (n > 0)
    assert sorted(ms4) == ["allreduce", "error_pass", "linearize", "solve"]
    assert all(math.isfinite(v) and v >= 0.0 for v in ms4.values())
    assert ms4["linearize"] > 0.0 and ms4["solve"] > 0.0 and ms4["error_pass"] > 0.0   # (no all-reduce on one rank)
    _assert_drained(win)                                    # an immediate second read: nothing left

    win.set_profiling(2)
    _steps(capi, win, STEPS)
    kernels, ms4, iters = _read_all(win)
    print("level 2:", kernels, ms4, iters)
    assert {which: n for which, (_, n) in kernels.items()} == LAUNCHES_LEVEL2
    assert math.isfinite(kernels[0][0]) and kernels[0][0] > 0.0
    assert iters == 0 and all(v == 0.0 for v in ms4.values())
    _assert_drained(win)

    win.set_profiling(0)
    _steps(capi, win, STEPS)
    _assert_drained(win)
    win.close()
