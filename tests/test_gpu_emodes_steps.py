"""elliptic_modes on the device, one iteration at a time: what csrc/lsm_elliptic.hip adds to csrc/lobpcg.h's iteration (the block
apply on X and on W's slots, the V-cycle or 1/D on the residual's slot, the start) seen per iterate, as tests/test_gpu_modes_edges.py
sees the elastic glue.

A solve with max_iters = k returns X_k (k = 0: rtol 1e300, the Rayleigh–Ritz rotation of the start).  Each X_k and λ is compared column by
column, after sign alignment, with the long-double run (tests/_emodes_ref.lobpcg_ld): the bar is 16 × the float64 restatement's own
distance from it (with eigh and with the device's Jacobi, the larger), floored at 2⁻⁵³·max|x| — the yardstick is the restatement's own
rounding, 16 covers that the device sums the Gram entries in another order.  The active set, the iteration count and `stats` equal the
restatement's.  tests/test_emodes_host.py asserts on the CPU that every step used here is defined to rounding (the decisions equal in
the three restatements, every relres a decade from rtol, the M-Gram's smallest eigenvalue ≥ 1e-9 of its largest, the yardstick
≤ 1e-10·max|x|).

The two locked cases (one 2-D, one 3-D) start from exact eigenvectors in some columns, so the active set is not all columns: slot j
against column act[j] in the preconditioner and in P's coefficients."""
import numpy as np
import pytest

import _emodes_ref as M
import _modes_ref as R
from test_gpu_emodes import _lsm, _modes, _operator

pytestmark = pytest.mark.gpu

FACTOR = 16
STEPS = [(name, k) for name, cs in M.step_cases().items() for k in cs["ks"]]


@pytest.mark.parametrize("name,k", STEPS)
def test_the_iterate_after_k_iterations_is_the_long_double_restatements(name, k):
    lsm = _lsm()
    cs = M.step_cases()[name]
    m = cs["m"]
    dev = _operator(lsm, cs)
    r = M.step_ref(name)
    assert r["hier"].levels == dev.levels
    s = r["steps"][k]
    ld = s["ld"]
    rtol = 1e300 if k == 0 else M.STEP_RTOL
    try:
        md, raised = _modes(dev, cs, x0=r["x0"], rtol=rtol, max_iters=max(k, 1)), False
    except lsm.LsmNotConvergedError as e:
        md, raised = e.modes, True
    X = md.vectors()
    ax = tuple(range(1, X.ndim))
    dx = np.abs(R._aligned(X.astype(M.LD), ld["X"]) - ld["X"]).max(axis=ax)
    rx = (dx / s["yard_x"]).astype(np.float64)
    rl = (np.abs(md.eigenvalues.astype(M.LD) - ld["lam"]) / s["yard_lam"]).astype(np.float64)
    print(f"{name} k = {k}: stats {md.stats} (restatement: active {ld['act']}, V-cycles {ld['applies']}), relres {np.array2string(md.relres, precision=2)} "
          f"(restatement {np.array2string(ld['relres'].astype(np.float64), precision=2)}), |x_dev − x_ld| in max|x| "
          f"{np.array2string((dx / s['scale']).astype(np.float64), precision=1)}, ratio x {np.array2string(rx, precision=2)} λ {np.array2string(rl, precision=2)}")
    assert raised == (k > 0) and md.iterations == k
    want_act = () if k == 0 else ld["act"]
    assert tuple(j for j in range(m) if not md.relres[j] <= rtol) == want_act
    assert md.stats == (k, ld["applies"], ld["dropped"], len(want_act))
    assert not np.any(X[:, r["hier"].ops[0].fixed])
    assert np.all(rx <= FACTOR) and np.all(rl <= FACTOR)
    md.close()
    dev.close()
