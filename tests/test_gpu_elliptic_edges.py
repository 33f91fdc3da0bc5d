"""elliptic_solve on the device where tests/test_gpu_elliptic.py's ten small cases do not reach (csrc/lsm_elliptic.hip): the V-cycle
node by node, c per node on every level, hierarchies of one level, launches beyond the reduction's and the grid-stride loop's
thresholds, and the smaller branches of the solve.  Every comparison is with the restatement (tests/_elliptic_ref.py);
tests/test_elliptic_host.py establishes on the CPU what is relied on here (its docstrings carry the restatement's numbers).

The first iterate.  From u0 = 0 with zero Dirichlet values r₀ = b and u₁ = α·M b, α = (b·Mb)/(Mb·A Mb): a solve at rtol = 0.95 that
stops after one iteration returns M b, up to a scalar that M b fixes, at every node.  For b = e_j that is column j of the V-cycle.
|u_dev − u_ld|∞ ≤ 16·max(|u_f64 − u_ld|∞, 2⁻⁵³·|u_ld|∞), where u_ld is the restatement in long double and u_f64 the restatement in
float64: the yardstick is the restatement's own rounding (0.4e-16 … 6.4e-16 of max|u|); 16 covers that the device gathers,
prolongs and reduces in another order.  One wrong restriction or prolongation weight moves u₁ by 1e-3 … 1 of max|u|.
Observed on the MI355X: one iteration on all 71 runs; |u_dev − u_ld| 0.4e-16 … 6.4e-16 of max|u|, 0.19 … 2.92 yardsticks for the
V-cycle (the largest: 6x5_face, the impulse at n − 2) and 0.01 … 1.00 for Jacobi.

The cases of _elliptic_ref.edge_cases() run through the bodies of tests/test_gpu_elliptic.py (check_bits, check_solve) unchanged.
A device handle needs at least 4 nodes per dimension (lsm_create), so the smallest grid is 4x4 and the strip whose short axis never
coarsens is 4x40; axes of 3 nodes occur on the coarse levels (6x5, 6x6x6, 24x33x10, 45x41x37, 83x81x79).
Observed: iterations equal to the restatement's on 36 of the 40 solves (65x20_aniso_h_guess mg 24 against 23; jacobi
33x33_face_guess 195 against 197, 65x20_aniso_h_guess 234 against 235, 17c_f32_guess 159 against 158); |u − direct| 1.0× the
restatement's on every case; 45x41x37, which has no direct solve: |u − restatement| 1.8e-15 (mg) and 5.3e-15 (jacobi) against the
restatement's 1.9e-9 and 6.2e-10 to its own solve at rtol/100.  True residuals at the large shapes, in ‖b‖: 300x230 8.8e-9 (mg, 25
iterations) and 9.9e-9 (jacobi, 1529); 45x41x37 2.8e-9 (18) and 1.0e-8 (339); 1000x530 3.5e-9 (28); 83x81x79 7.7e-9 (24)."""
import numpy as np
import pytest

import _elliptic_ref as R
import test_gpu_elliptic as T
from test_gpu_elliptic import RTOL, _bits, _field, _kwargs, _lsm

pytestmark = pytest.mark.gpu

SMALL = R.edge_case_names(big=False)
BIG = R.edge_case_names(big=True)
BOTH = [k for k in SMALL if R.edge_cases()[k].get("solve", "both") == "both"]

# ---- A. the first PCG iterate pins the V-cycle
@pytest.mark.parametrize("name,precond", R.FIRST_ITERATE_PAIRS)
def test_the_first_iterate_is_the_restatements_to_rounding(name, precond):
    lsm = _lsm()
    s = R.any_solved(name)
    cs, hier = s["case"], s["hier"]
    op = hier.ops[0]
    phi = _field(lsm, cs)
    kw = _kwargs(cs)
    if cs["fixed"] is not None:
        kw["dirichlet"] = (cs["fixed"], 0.0)
    dev = lsm.EllipticOperator(phi, precond=precond, **kw)
    for fname, f in R.first_iterate_rhs(op).items():
        sol = dev.solve(f, rtol=0.95)
        u = sol.u.values()
        uld = R.first_iterate_ld(hier, f, precond)
        uref = R.pcg(hier, f, np.zeros(cs["n"]), 0.95, 1, precond)[0]
        scale = float(np.abs(uld).max())
        yard = max(float(np.abs(uref - uld).max()), 2.0 ** -53 * scale)
        err = float(np.abs(u - uld).max())
        print(f"{name} {precond} {fname}: {sol.iterations} iteration(s), relres {sol.relres:.3f}, |u_dev − u_ld| {err / scale:.2e}·max|u|, "
              f"yardstick {yard / scale:.2e}·max|u|, ratio {err / yard:.2f}")
        assert sol.iterations == 1
        assert err <= 16 * yard
    dev.close()


# ---- B, C, D (to 270 workgroups), E: the bit-for-bit set and the solve of the existing file
@pytest.mark.parametrize("name", SMALL)
def test_cells_apply_and_energy_are_the_restatements_bits(name):
    T.check_bits(_lsm(), R.edge_solved(name))


@pytest.mark.parametrize("name,precond", [(k, "mg") for k in SMALL] + [(k, "jacobi") for k in BOTH])
def test_solve_against_the_restatement(name, precond):
    T.check_solve(_lsm(), R.edge_solved(name), name, precond)


@pytest.mark.parametrize("name", BOTH)
def test_mg_needs_fewer_iterations_than_jacobi(name):
    lsm = _lsm()
    s = R.edge_solved(name)
    cs = s["case"]
    phi = _field(lsm, cs)
    it = {}
    for pc in ("mg", "jacobi"):
        sol = lsm.elliptic_solve(phi, T._rhs(lsm, cs, s["f"]), u0=T._guess(s), rtol=RTOL, max_iters=cs.get("max_iters", 2000), precond=pc, **_kwargs(cs, lsm))
        it[pc] = sol.iterations
        sol.operator.close()
    print(name, it)
    assert it["mg"] < it["jacobi"]


def test_c_on_the_device_is_refused_for_a_negative_entry_and_for_a_nan():
    """given as device fields, so that only el_setup_kernel's count on the array can see them; neither is first or last in memory"""
    lsm = _lsm()
    cs = R.edge_cases()["64x48_cn_devicefield"]
    phi = _field(lsm, cs)
    for bad in (-0.25, np.nan):
        c = cs["c"].copy()
        c[37, 29] = bad
        with pytest.raises(ValueError, match="c must be finite and not negative"):
            lsm.elliptic_solve(phi, cs["f"], c=_field(lsm, cs, c), dirichlet=(cs["fixed"], cs["g"]))


# ---- D. beyond MG_MAXB workgroups: the second trip of the grid-stride loop, with a ragged tail
@pytest.mark.parametrize("name", BIG)
def test_beyond_the_grid_stride_threshold(name):
    lsm = _lsm()
    s = R.edge_solved(name)
    cs, op = s["case"], s["hier"].ops[0]
    assert op.free.size > 2048 * 256
    phi = _field(lsm, cs)
    dev = lsm.EllipticOperator(phi, **_kwargs(cs))
    assert dev.levels == s["hier"].levels
    assert dev.fixed_nodes == int(op.fixed.sum()) and dev.free_nodes == int(op.free.sum())
    assert np.array_equal(_bits(dev.cells()), _bits(op.a))
    rng = np.random.default_rng(23)
    x = np.asfortranarray(rng.standard_normal(cs["n"]))
    assert np.array_equal(_bits(dev.apply(x)), _bits(op.apply(x)))
    v = np.asfortranarray(rng.standard_normal(cs["n"]))
    e = lsm.EllipticSolution(dev, _field(lsm, cs, v), None, 0, 0.0).energy_density().values()
    assert np.array_equal(_bits(e), _bits(op.energy(v)))
    sol = dev.solve(s["f"], rtol=RTOL)
    u = sol.u.values()
    g = np.broadcast_to(np.asarray(cs["g"], dtype=cs["dtype"]), cs["n"])
    assert np.array_equal(_bits(u[cs["fixed"]]), _bits(g[cs["fixed"]]))
    tr, bn = R.true_residual(op, s["f"], u)
    itref = s["mg"][1]
    print(f"{name} mg: {sol.iterations} iterations (restatement {itref}), relres {sol.relres:.3e}, true residual {tr / bn:.3e}·‖b‖, levels {sol.levels}")
    assert sol.relres <= RTOL
    assert tr <= 2 * RTOL * bn
    assert sol.iterations <= itref + 2
    want_c = R.compliance(op, s["f"], u)
    assert abs(sol.compliance() - want_c) <= 1e-12 * max(abs(want_c), float(np.prod(cs["h"])) * float(np.abs(R.rhs(op, s["f"]) * u).sum()))
    dev.close()


# ---- E. the remaining branches
def test_a_zero_problem_converges_at_once_to_zero_bits():
    lsm = _lsm()
    cs = R.cases()["33x33_face"]
    phi = _field(lsm, cs)
    for pc in ("mg", "jacobi"):
        sol = lsm.elliptic_solve(phi, 0.0, dirichlet=(cs["fixed"], 0.0), precond=pc)
        assert sol.iterations == 0 and sol.relres == 0.0
        assert not _bits(sol.u.values()).any()
        sol.operator.close()


@pytest.mark.parametrize("precond", ["mg", "jacobi"])
@pytest.mark.parametrize("name", ["24x33x10_patch", "64x48_blob"])
def test_an_exact_iteration_budget_converges_and_one_less_does_not(name, precond):
    """K2 reports CONVERGED before MAXITER; the host loop stops enqueueing at max_iters, whatever the first chunk's length"""
    lsm = _lsm()
    s = R.solved(name)
    cs = s["case"]
    phi = _field(lsm, cs)
    kw = dict(precond=precond, **_kwargs(cs))
    first = lsm.elliptic_solve(phi, s["f"], rtol=RTOL, max_iters=2000, **kw)
    it = first.iterations
    bits = _bits(first.u.values())
    print(f"{name} {precond}: {it} iterations (restatement {s[precond][1]})")
    assert 2 <= it <= s[precond][1] + 2
    kept = first.operator
    kept.solve(s["f"], rtol=1e-2 * RTOL, max_iters=2000)           # a longer solve: the next first chunk is longer than max_iters
    for fresh in (True, False):
        op = lsm.EllipticOperator(phi, **kw) if fresh else kept
        sol = op.solve(s["f"], rtol=RTOL, max_iters=it)
        assert sol.iterations == it
        assert np.array_equal(_bits(sol.u.values()), bits)
        if fresh:
            op.close()
            op = lsm.EllipticOperator(phi, **kw)
        with pytest.raises(lsm.LsmNotConvergedError, match=f" {it - 1} iterations"):
            op.solve(s["f"], rtol=RTOL, max_iters=it - 1)
        op.close()
