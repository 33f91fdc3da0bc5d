"""elasticity_modes on the device one iteration at a time (csrc/lsm_elastic.hip "elasticity_modes"): what tests/test_gpu_modes.py, which
looks at a solve where it ends, cannot see.  LOBPCG corrects itself: a wrong search direction still converges, a few iterations later
and within the margin that file allows its counts.

The iterates.  On LSM_ERR_NOT_CONVERGED X is the last iterate, so a solve with max_iters = k returns X_k, and one at rtol = 1e300 returns
X_0, the start after its Rayleigh–Ritz step, with no iteration.  Cold solves are bit-reproducible, so the runs at k = 0, 1, 2, … are views
of one trajectory.  Each is compared with the restatement in long double (tests/_modes_ref.py, lobpcg_ld) on the device's own K0 and
dampings, column by column after sign alignment:
    |x_dev − x_ld|∞ ≤ 16·max(|x_eigh − x_ld|∞, |x_jacobi − x_ld|∞, 2⁻⁵³·|x_ld|∞)
and λ_k in the same form, where x_eigh and x_jacobi are the float64 restatement with numpy's eigh and with the device's cyclic Jacobi
restated: the yardstick is the restatement's own rounding, 16 covers that the device sums in another order (the factor of
tests/test_gpu_elliptic_edges.py and tests/test_gpu_elastic_edges.py).  Also equal to the restatement's: the iteration count k, the set
of columns with relres ≤ rtol, stats (V-cycle applications, dropped directions, active columns at exit); X is zero on the fixed
components.  tests/test_modes_host.py asserts on the CPU what makes a step usable (test_the_step_cases_are_well_defined): the three
restatements take the same decisions, every relres is a decade from rtol, the M-Gram's smallest eigenvalue is ≥ 1e-9 of its largest, the
yardstick is ≤ 1e-10·max|x|.  Three cases of the plan failed that there and were replaced: 9x12 m = 3 (k = 3: 8e-9, yardstick 2e-10) by
12x9; 5x5 one level stops at k = 2 (k = 3: relres 7.6e-6); 190x180 observes k = 1 in place of k = 2 (5e-10).

The cases (_modes_ref.step_cases): locked starts (exact eigenvectors in the locked columns, v_k + 0.3·v_{m+k} + 0.1·v_{m+k−1} in the others) make
the active set a non-prefix one from the first iteration — (1, 3), (0, 3), (1) and, in 3-D, (1, 2) then (0, 2) — so W's source slot
differs from its target slot and P's coefficient columns are act[j]; default starts with m = 8, 3 and 5 reach every column of the
start kernel, all 21 Gram tiles and the partial tiles (q = 3, 6, 9 and 5, 10, 15); one hierarchy of one level; the diagonal
preconditioner under the same slot mapping; 33x33 with several workgroups per tile; 190x180 and 30x29x27 with more than 256
workgroups in the residual and Gram passes (the strided second pass of the ordered reduction).

Observed on the MI355X, 40 runs: |x_dev − x_ld| 2.2e-16 … 3.2e-13 of max|x| per run (the largest: 9x12 m = 8 at k = 3), 0.009 … 4.07
yardsticks (9x12 m = 8, k = 3); λ at 0.04 … 9.01 yardsticks (9x12 m = 5, k = 2; 8.18 on 9x12 locked {0, 2} at k = 4: a locked column,
whose yardstick is the 2⁻⁵³ floor or little more).  Every count, locked set and stats entry equal to the restatement's.

The other tests: the start kernel's values through m = 1 at k = 0, where the Rayleigh–Ritz step only normalises (1.19 yardsticks); a start
with two equal columns is refused with no iteration and one dropped direction, and the next default solve on the same object gives
a fresh object's bits; max_iters equal to the count converges, one less overruns with that count, and a solve after an overrun of one
iteration gives a fresh object's bits (9x12 m = 4: 18 iterations, the restatement's count).

Deliberate defects, each tried once on a scratch build of the library, never committed (tests/test_gpu_modes.py without its two large
shapes run beside this file):
  1. P's coefficient columns j for act[j] (em_gram_rr): 7 of the step tests fail — every locked case from k = 3 on (9x12 {0,2} at 3 and
     4, its Jacobi twin and {1,2} at 3, 6x5x7 at 3 and 4, 33x33 at 4); k ≤ 2 cannot see it, since the misplaced columns of the first P still
     span the first W.  test_gpu_modes.py fails 5 (the counts of 33x33 at both tolerances, 24x33x10_m4, 5x5_one_level; the 300 iterations of
     the modes() call around op.solve) and passes the rest.
  2. the preconditioner's source slot j for act[j]: 19 fail — every locked case at every k ≥ 1, and the exact budget.  test_gpu_modes.py
     fails 17 of 29.
  3. P stored for k < m in place of k < na (em_update_kernel): nothing fails, here or there, and nothing can: Cp's columns na … 7 are
     zero, so the extra stores put zeros into slots that neither the Gram pass nor the next update reads (both take np = na columns).
     The change is not a defect.  In its place:
  3b. P stored for k < np (so never by the first iteration): 22 fail — every case at every k ≥ 2 (5x5 and 30x29x27 included), the refusal's
      clean state and the exact budget; k = 1 does not read P.  test_gpu_modes.py fails 26 of 29: the stale slots reach the Gram pass."""
import numpy as np
import pytest

import _elastic_ref as E
import _modes_ref as R
from test_gpu_modes import _bits, _lsm, _modes, _operator

pytestmark = pytest.mark.gpu

FACTOR = 16
STEPS = [(name, k) for name, cs in R.step_cases().items() for k in cs["ks"]]


def _device_ref(dev, name):
    """the step references on the device's K0 and dampings (computed once per case)"""
    k0s = [dev.stiffness(l) for l in range(dev.levels)]
    r = R.step_ref(name, k0s, E.device_omegas(k0s, len(R.step_cases()[name]["n"])))
    assert r["hier"].levels == dev.levels
    return r


def _run(lsm, dev, cs, **kw):
    """(the modes object, whether the solve raised LsmNotConvergedError)"""
    try:
        return _modes(dev, cs, **kw), False
    except lsm.LsmNotConvergedError as e:
        return e.modes, True


def _ratios(X, lam, ref_X, ref_lam, yard_x, yard_lam):
    """per column: |x − ref|∞ and |λ − ref| in their yardsticks, in long double, after sign alignment"""
    ax = tuple(range(1, ref_X.ndim))
    dx = np.abs(R._aligned(X.astype(R.LD), ref_X) - ref_X).max(axis=ax)
    return (dx / yard_x).astype(np.float64), (np.abs(lam.astype(R.LD) - ref_lam) / yard_lam).astype(np.float64), dx


@pytest.mark.parametrize("name,k", STEPS)
def test_the_iterate_after_k_iterations_is_the_long_double_restatements(name, k):
    lsm = _lsm()
    cs = R.step_cases()[name]
    m = cs["m"]
    dev = _operator(lsm, cs)
    r = _device_ref(dev, name)
    s = r["steps"][k]
    ld = s["ld"]
    rtol = 1e300 if k == 0 else R.STEP_RTOL
    md, raised = _run(lsm, dev, cs, x0=r["x0"], rtol=rtol, max_iters=max(k, 1))
    X = md.vectors()
    rx, rl, dx = _ratios(X, md.eigenvalues, ld["X"], ld["lam"], s["yard_x"], s["yard_lam"])
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


def test_the_default_start_of_one_column_is_splitmix64_normalised():
    """m = 1 at k = 0: the Rayleigh–Ritz step of one column only scales it, X_0 = x0/√(x0ᵀM x0) with the sign kept — the one direct check of
    the start kernel's values on the device"""
    lsm = _lsm()
    cs = dict(R.step_cases()["9x12_m8"], m=1)
    dev = _operator(lsm, cs)
    md = _modes(dev, cs, rtol=1e300, max_iters=1)
    op = R.build_case(cs, [dev.stiffness(l) for l in range(dev.levels)])[0].ops[0]
    Mn = md.mass()
    x0 = R.default_start(op, 1)[0]
    assert np.count_nonzero(x0) == 2 * 8 * 12
    want = x0.astype(R.LD) / np.sqrt(np.sum(Mn.astype(R.LD)[None] * x0.astype(R.LD) ** 2))
    f64 = x0 / np.sqrt(np.sum(Mn[None] * x0 * x0))
    yard = max(float(np.abs(f64 - want).max()), 2.0 ** -53 * float(np.abs(want).max()))
    err = float(np.abs(md.vectors()[0] - want).max())
    print(f"9x12 m = 1: |x_dev − x0/‖x0‖_M| {err / float(np.abs(want).max()):.2e}·max|x|, ratio {err / yard:.2f}, stats {md.stats}")
    assert md.iterations == 0 and md.stats == (0, 0, 0, 0)
    assert err <= FACTOR * yard
    md.close()
    dev.close()


def test_a_rank_deficient_start_is_refused_and_leaves_the_object_clean():
    lsm = _lsm()
    cs = R.base("5x5_one_level_m2")["case"]
    hier, Mn = R.base("5x5_one_level_m2")["hier"], R.base("5x5_one_level_m2")["mass"]
    col = R.default_start(hier.ops[0], 1)[0]
    x0 = np.stack([col, col])
    with pytest.raises(R.NotPositive):
        R.lobpcg(hier, Mn, 2, x0)
    dev = _operator(lsm, cs)
    fresh = _modes(dev, cs)
    X, lam, it, stats = fresh.vectors(), fresh.eigenvalues.copy(), fresh.iterations, fresh.stats
    fresh.close()
    with pytest.raises(lsm.LsmNotConvergedError, match="not positive") as e:
        _modes(dev, cs, x0=x0)
    md = e.value.modes
    print(f"two equal columns: iterations {e.value.iterations}, stats {md.stats}")
    assert e.value.iterations == 0 and md.stats[0] == 0 and md.stats[1] == 0 and md.stats[2] >= 1
    md.solve(max_iters=600)
    assert md.iterations == it and md.stats == stats
    assert np.array_equal(_bits(md.eigenvalues), _bits(lam)) and np.array_equal(_bits(md.vectors()), _bits(X))
    md.close()
    dev.close()


def test_an_exact_iteration_budget_converges_one_less_does_not_and_the_object_is_reusable_after():
    lsm = _lsm()
    cs = R.step_cases()["9x12_m4_lock02"]
    dev = _operator(lsm, cs)
    r = _device_ref(dev, "9x12_m4_lock02")
    c = R.lobpcg(r["hier"], r["mass"], 4, None, R.STEP_RTOL, 600)
    assert c["converged"]
    c = c["iters"]
    fresh = _modes(dev, cs)
    X, lam, it = fresh.vectors(), fresh.eigenvalues.copy(), fresh.iterations
    fresh.close()
    print(f"9x12 m = 4 from the default start: {it} iterations (restatement {c})")
    assert 2 <= it <= c + max(3, c / 10)
    md = _modes(dev, cs, max_iters=it)
    assert md.iterations == it and md.stats[3] == 0
    assert np.array_equal(_bits(md.eigenvalues), _bits(lam)) and np.array_equal(_bits(md.vectors()), _bits(X))
    with pytest.raises(lsm.LsmNotConvergedError, match=f" {it - 1} iterations") as e:
        md.solve(max_iters=it - 1)
    assert e.value.iterations == it - 1 and md.stats[0] == it - 1 and md.stats[3] >= 1 and md.relres.max() > R.STEP_RTOL
    # after an overrun of one iteration the same object solves as a fresh one does
    with pytest.raises(lsm.LsmNotConvergedError) as e:
        md.solve(max_iters=1)
    assert e.value.iterations == 1 and md.stats[3] == 4
    md.solve(max_iters=600)
    assert md.iterations == it
    assert np.array_equal(_bits(md.eigenvalues), _bits(lam)) and np.array_equal(_bits(md.vectors()), _bits(X))
    md.close()
    dev.close()
