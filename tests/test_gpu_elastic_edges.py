"""elasticity_solve on the device where tests/test_gpu_elastic.py's nine small cases do not reach (csrc/lsm_elastic.hip): the V-cycle
component by component and node by node, the per-level damping, hierarchies of one level, coarse levels without a fixed component,
launches beyond the reduction's and the per-unknown kernels' thresholds, and the smaller branches of the solve.  Every comparison
is with the restatement (tests/_elastic_ref.py) on the device's own K0 and with the dampings min(0.6, 1.9/λ) of the host code's
power iteration restated (symbol_lambda_power); tests/test_elastic_host.py establishes on the CPU what is relied on here (its
docstrings carry the restatement's numbers).

The first iterate.  From u0 = 0 with zero prescribed values r₀ = b and u₁ = α·M b, α = (b·Mb)/(Mb·A Mb): a solve at rtol = 0.97
that stops after one iteration returns M b, up to a scalar that M b fixes, at every node and component.  For b = e_(i,j) that is a
column of the V-cycle.  A right-hand side is used if the restatement's relative residual after one iteration is ≤ 0.95; at most
two of a case may fail that, never the normal one.  |u_dev − u_ld|∞ ≤ 16·max(|u_f64 − u_ld|∞, 2⁻⁵³·|u_ld|∞), where u_ld is the
restatement in long double and u_f64 the restatement in float64: the yardstick is the restatement's own rounding; 16 covers that
the device gathers, prolongs and reduces in another order (tests/test_gpu_elliptic_edges.py's factor).  One wrong restriction
weight, coarse fixed bit or damping moves u₁ by 1e-3 … 1 of max|u|.
Observed on the MI355X: one iteration on all 152 runs (138 V-cycle, 14 Jacobi; no right-hand side was left out);
|u_dev − u_ld| 0.2e-16 … 2.6e-15 of max|u|, 0.05 … 6.05 yardsticks for the V-cycle (the largest: 9x12_pin, the impulse of component 1
at the odd interior node) and 0.06 … 1.00 for Jacobi.  With the restriction weight ½ for the unpaired last node the largest
difference is 3.1e-3 (24x10_far_clamp), 0.30 (4x6x21_clamp) and 0.25 (9x12_pin) of max|u|; with SAFE = 1.8 it is 2.9e-2 on
4x6x21_clamp (the two others have ω = 0.6 on every level and pass); with the coarse bits of fine node 2J+1 2.1e-2, 0.22 and 0.43.

The small cases of _elastic_ref.edge_cases() run through the bodies of tests/test_gpu_elastic.py (check_bits, check_solve)
unchanged.  A device handle needs at least 4 nodes per dimension, so the smallest grid is 4x4 (16 nodes in the coarsest kernel's
128 threads); axes of 3 nodes occur on the coarse levels.
Observed: iterations equal to the restatement's on 36 of the 40 solves (mg: 64x48_level 28 against 27, 6x6x6_far_clamp 26 against
25; jacobi: 17c_f32_guess 294 against 295, 5x5x5_flat_clamp 57 against 58); |u − direct| at most 1.3× the restatement's.

The launch shapes (the prototype problem): 300x230 and 45x41x37 have more than 256 workgroups per node, so the second pass of the
ordered reduction strides; 600x500 has 2344 workgroups per unknown, capped at 2048: a second grid-stride trip in the direction
kernel and K2 only.
Observed, mg iterations (restatement's) and true residuals in ‖b‖ (restatement's): 300x230 31 (32), 9.6e-9 (6.9e-9); 45x41x37
25 (25), 3.5e-9 (3.5e-9); 600x500 40 (40), 7.4e-9 (7.4e-9)."""
import numpy as np
import pytest

import _elastic_ref as R
import test_gpu_elastic as T
from test_gpu_elastic import RTOL, _bits, _field, _kwargs, _lsm, _values

pytestmark = pytest.mark.gpu

SMALL = R.edge_case_names(big=False)
BIG = R.edge_case_names(big=True)
BOTH = [k for k in SMALL if R.edge_cases()[k].get("solve", "both") == "both"]


def _device_hierarchy(dev, s, cs=None):
    """the restatement's hierarchy of a solved case on the device's K0 and the device's dampings"""
    cs = s["case"] if cs is None else cs
    assert dev.levels == s["hier"].levels
    k0s = [dev.stiffness(l) for l in range(dev.levels)]
    return R.build_case(cs, k0s, R.device_omegas(k0s, len(cs["n"])))[0]


# ---- B. the first PCG iterate pins the V-cycle
@pytest.mark.parametrize("name,precond", R.FIRST_ITERATE_PAIRS)
def test_the_first_iterate_is_the_restatements_to_rounding(name, precond):
    lsm = _lsm()
    s = R.any_solved(name)
    cs = dict(s["case"], g=np.zeros(len(s["case"]["n"])))
    assert cs["dtype"] == np.float64
    phi = _field(lsm, cs)
    dev = lsm.ElasticityOperator(phi, precond=precond, **_kwargs(cs))
    hier = _device_hierarchy(dev, s, cs)
    runs, left_out = R.first_iterate_runs(hier, precond)
    print(f"{name} {precond}: dampings {[float(hier.omega(l)) for l in range(hier.levels)]}, left out {left_out}")
    assert len(left_out) <= R.FIRST_LEFT_OUT and runs[0][0] == "normal"
    for fname, f, uref, rel in runs:
        sol = dev.solve(f, rtol=R.FIRST_RTOL)
        u = _values(sol.u)
        uld = R.first_iterate_ld(hier, f, precond)
        scale = float(np.abs(uld).max())
        yard = max(float(np.abs(uref - uld).max()), 2.0 ** -53 * scale)
        err = float(np.abs(u - uld).max())
        print(f"{name} {precond} {fname}: {sol.iterations} iteration(s), relres {sol.relres:.3f} (restatement {rel:.3f}), |u_dev − u_ld| {err / scale:.2e}·max|u|, "
              f"yardstick {yard / scale:.2e}·max|u|, ratio {err / yard:.2f}")
        assert sol.iterations == 1
        assert err <= 16 * yard
    dev.close()


# ---- C. the small edge cases through the bodies of the existing file
@pytest.mark.parametrize("name", SMALL)
def test_k0_cells_apply_and_energy_are_the_restatements_bits(name):
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
        sol = lsm.elasticity_solve(phi, s["f"], u0=T._guess(cs), rtol=RTOL, max_iters=3000, precond=pc, **_kwargs(cs))
        it[pc] = sol.iterations
        sol.operator.close()
    print(name, it, "restatement", {pc: s[pc][1] for pc in it})
    assert it["mg"] < it["jacobi"]


def test_f_and_u0_as_device_fields_give_the_bits_of_the_host_arrays():
    lsm = _lsm()
    s = R.edge_solved("64x48_devfield")
    cs = s["case"]
    assert cs["devfield"]
    N = len(cs["n"])
    phi = _field(lsm, cs)

    def on_device(v):
        return [lsm.ROCMeshField(phi.backend, phi.mesh, phi.bcs).copy_(np.asfortranarray(v[i])) for i in range(N)]

    for pc in ("mg", "jacobi"):
        dev = lsm.ElasticityOperator(phi, precond=pc, **_kwargs(cs))
        host = dev.solve(s["f"], u0=cs["u0"], rtol=RTOL, max_iters=3000)
        f, u0 = on_device(s["f"]), on_device(cs["u0"])
        before = [c.values() for c in u0]
        sol = dev.solve(f, u0=u0, rtol=RTOL, max_iters=3000)
        print(f"64x48_devfield {pc}: {sol.iterations} iterations (restatement {s[pc][1]})")
        assert sol.iterations == host.iterations and sol.relres == host.relres
        assert np.array_equal(_bits(_values(sol.u)), _bits(_values(host.u)))
        assert sol.compliance() == host.compliance()
        for c, b in zip(u0, before):          # the guess is copied, not solved in place
            assert np.array_equal(_bits(c.values()), _bits(b))
        dev.close()


# ---- D. launch shapes between "tiny" and "capped"
@pytest.mark.parametrize("name", BIG)
def test_launch_shapes(name):
    lsm = _lsm()
    s = R.edge_solved(name)
    cs, f, u0 = s["case"], s["f"], s["u0"]
    n = cs["n"]
    N = len(n)
    phi = _field(lsm, cs)
    dev = lsm.ElasticityOperator(phi, **_kwargs(cs))
    hier = _device_hierarchy(dev, s)
    op = hier.ops[0]
    assert dev.fixed_dofs == int(op.fixed.sum()) and dev.free_dofs == int(op.free.sum())
    assert np.array_equal(_bits(dev.cells()), _bits(op.E))
    x = np.random.default_rng(11).standard_normal((N,) + n)
    assert np.array_equal(_bits(dev.apply(x)), _bits(op.apply(x)))
    sol = dev.solve(f, rtol=RTOL)
    u = _values(sol.u)
    assert np.array_equal(_bits(sol.energy_density().values()), _bits(op.energy(u)))
    assert np.array_equal(_bits(u[op.fixed]), _bits(u0[op.fixed]))
    tr, bn = R.true_residual(op, f, u)
    uref, itref, relref, ok = R.pcg(hier, f, u0, RTOL, 500, "mg")
    assert ok
    print(f"{name} mg: {sol.iterations} iterations (restatement {itref}), levels {sol.levels}, relres {sol.relres:.3e}, true residual {tr / bn:.3e}·‖b‖ "
          f"(restatement {R.true_residual(op, f, uref)[0] / bn:.3e}), |u − restatement| {np.abs(u - uref).max() / np.abs(uref).max():.2e}·max|u|")
    assert sol.relres <= RTOL
    assert tr <= 2 * RTOL * bn
    assert sol.iterations <= itref + 2
    dev.close()


# ---- E. the remaining branches
def test_a_zero_problem_converges_at_once_to_zero_bits():
    lsm = _lsm()
    for name in ("33x33_clamp", "17c_clamp"):
        cs = R.cases()[name]
        phi = _field(lsm, cs)
        for pc in ("mg", "jacobi"):
            sol = lsm.elasticity_solve(phi, 0.0, dirichlet=(T._mask(cs), 0.0), precond=pc)
            assert sol.iterations == 0 and sol.relres == 0.0
            assert not _bits(_values(sol.u)).any()
            sol.operator.close()


@pytest.mark.parametrize("precond", ["mg", "jacobi"])
@pytest.mark.parametrize("name", ["24x33x10_patch", "64x48_upper_patch"])
def test_an_exact_iteration_budget_converges_and_one_less_does_not(name, precond):
    """K2 reports CONVERGED before MAXITER; the host loop stops enqueueing at max_iters, whatever the first chunk's length"""
    lsm = _lsm()
    s = R.solved(name)
    cs = s["case"]
    phi = _field(lsm, cs)
    kw = dict(precond=precond, **_kwargs(cs))
    first = lsm.elasticity_solve(phi, s["f"], rtol=RTOL, max_iters=3000, **kw)
    it = first.iterations
    bits = _bits(_values(first.u))
    print(f"{name} {precond}: {it} iterations (restatement {s[precond][1]})")
    assert 2 <= it <= s[precond][1] + 2
    kept = first.operator
    kept.solve(s["f"], rtol=1e-2 * RTOL, max_iters=3000)           # a longer solve: the next first chunk is longer than max_iters
    for fresh in (True, False):
        op = lsm.ElasticityOperator(phi, **kw) if fresh else kept
        sol = op.solve(s["f"], rtol=RTOL, max_iters=it)
        assert sol.iterations == it
        assert np.array_equal(_bits(_values(sol.u)), bits)
        if fresh:
            op.close()
            op = lsm.ElasticityOperator(phi, **kw)
        with pytest.raises(lsm.LsmNotConvergedError, match=f" {it - 1} iterations"):
            op.solve(s["f"], rtol=RTOL, max_iters=it - 1)
        op.close()
