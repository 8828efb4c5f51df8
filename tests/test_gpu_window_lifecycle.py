"""A destroyed window returns its device memory, and a rebuilt window behaves like the first: four create -> finalize ->
lm_step -> destroy cycles of the smoke window (with a reprojection and a match-geometry term on link 0, profiling on) in one
process, free device memory read after each."""
import numpy as np
import pytest

from sage_slam_amd import synth

pytestmark = pytest.mark.gpu

CYCLES = 4
# bytes of free device memory a cycle may cost once the process is warm (cycle 4 against cycle 2).  Every buffer has an
# owner that releases it, so the expectation is zero (the figure of the library before the owners existed is not measured
# yet: profiles/window_state_refactor_ab.txt)
MAX_DROP_BYTES = 0


def _terms(w):
    """one reprojection term (N = 96) and one match-geometry term (N = 64) on link 0's first direction"""
    a, b = w.links[0]
    rep = synth.make_reprojection_matches(w, a, b, 96, 0)
    rep.update(edge=0, weight=5.0, loss_param=0.1 * w.W * w.W)
    mg = synth.make_match_geometry_matches(w, a, b, 64, 0)
    mg.update(edge=0, weight=5.0, loss="fair", loss_param=float(0.1 * np.mean(np.square(w.keyframes[a].bias, dtype=np.float64))))
    return [rep, mg]


def test_destroyed_windows_return_their_memory():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from sage_slam_amd import capi
    w = synth.make_window(K=3, H=64, W=80, FS=16, CS=32, L=4, seed=3)
    terms = _terms(w)
    idle = capi.Window(w)     # keeps the host threads' last-window shutdown out of the cycles
    free, results = [], []
    for _ in range(CYCLES):
        win = capi.Window(w, keypoint_terms=terms)
        win.set_profiling(1)
        st, cfg = capi.SageLmState(), capi.lm_config_default()
        win.lm_step(st, cfg)
        results.append((st.error, st.candidate_error, int(st.accepted)))
        win.close()
        del win
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    idle.close()
    print("free bytes after each cycle:", free, "drop cycle 2 -> 4:", free[1] - free[3])
    print("lm_step (error, candidate_error, accepted) per cycle:", results)
    assert results[1] == results[3]
    assert np.isfinite(results[3][0])
    assert free[1] - free[3] <= MAX_DROP_BYTES
