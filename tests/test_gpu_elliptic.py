"""elliptic_solve on the device (csrc/lsm_elliptic.hip through the Python API) against the restatement (tests/_elliptic_ref.py).

Bit for bit: the cell array, A x for a random x, the energy density, the fixed nodes of u, and two solves of one operator against
two fresh ones.  The solve at rtol = 1e-8, per case and preconditioner:
  * the true residual of the device's u, computed by the restatement, is ≤ 2·rtol·‖b_free‖₂ on the free nodes.  The factor 2
    covers the drift between the recursive and the true residual: the restatement's own drift on these cases is below 1e-4 of
    the residual (tests/test_elliptic_host.py prints it: e.g. 3.890424e-09 recursive against 3.890427e-09 true).  A float32
    handle stores u rounded: its bound grows by ‖ |A|·|u|·2⁻²⁴ ‖₂, what rounding u to float32 can add to the residual at most;
  * |u − direct solve|∞ ≤ 4× what the restatement's own PCG leaves at the same rtol (1e-14 … 2e-9 on these cases; for the
    float32 case both are rounded to float32 first and differ from the direct solve by 1.1e-7); observed: 1.0× on every case;
  * iterations ≤ the restatement's + 2 (the reduction order differs; observed: equal on all twenty runs), and mg strictly fewer
    than jacobi (8–28 against 32–361)."""
import numpy as np
import pytest

import _elliptic_ref as R

pytestmark = pytest.mark.gpu

RTOL = 1e-8
NAMES = sorted(R.cases())


def _lsm():
    import lsm_amd
    return lsm_amd


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _field(lsm, cs, vals=None):
    n = cs["n"]
    vals = cs["phi"] if vals is None else vals
    mf = lsm.MeshField(np.asfortranarray(vals), lsm.CartesianGrid((0.0,) * len(n), cs["hc"], n), dtype=cs["dtype"])
    phi = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=mf, bc=lsm.NeumannBC()).current_state()
    assert tuple(phi.mesh.meshsize()) == tuple(cs["h"])
    return phi


def _kwargs(cs, lsm=None):
    """the operator's keyword arguments; a case with devfield gives c as a device field (lsm is needed for it)"""
    kw = dict(a_in=cs["a_in"], a_out=cs["a_out"], a=cs["a"], c=_field(lsm, cs, cs["c"]) if cs.get("devfield") else cs["c"])
    if cs["fixed"] is not None:
        kw["dirichlet"] = (cs["fixed"], cs["g"])
    if "level" in cs:
        kw["level"] = cs["level"]
    return kw


def _rhs(lsm, cs, f):
    return _field(lsm, cs, f) if cs.get("devfield") else f


def _guess(s):
    return s["u0"] if s["case"].get("u0") is not None else None


def check_bits(lsm, s):
    """the body of test_cells_apply_and_energy_are_the_restatements_bits for a solved case (also tests/test_gpu_elliptic_edges.py's)"""
    cs, op = s["case"], s["hier"].ops[0]
    phi = _field(lsm, cs)
    dev = lsm.EllipticOperator(phi, **_kwargs(cs, lsm))
    assert dev.levels == s["hier"].levels
    assert dev.fixed_nodes == int(op.fixed.sum()) and dev.free_nodes == int(op.free.sum())
    assert np.array_equal(_bits(dev.cells()), _bits(op.a))
    x = np.asfortranarray(np.random.default_rng(11).standard_normal(cs["n"]))
    assert np.array_equal(_bits(dev.apply(x)), _bits(op.apply(x)))
    sol = dev.solve(_rhs(lsm, cs, s["f"]), u0=_guess(s), rtol=RTOL, max_iters=cs.get("max_iters", 500))
    u = sol.u.values()
    assert u.dtype == cs["dtype"]
    want = op.energy(u.astype(np.float64)).astype(cs["dtype"])
    assert np.array_equal(_bits(sol.energy_density().values()), _bits(want))
    want_c = R.compliance(op, s["f"], u.astype(np.float64))
    assert abs(sol.compliance() - want_c) <= 1e-12 * max(abs(want_c), float(np.prod(cs["h"])) * float(np.abs(R.rhs(op, s["f"]) * u).sum()))
    dev.close()


def check_solve(lsm, s, name, precond):
    """the body of test_solve_against_the_restatement for a solved case.  A case without a direct solve (s["direct"] is None) is
    compared with the restatement's u instead, to 4× the restatement's own distance to its solve at rtol/100 (s["tight"])."""
    cs, op = s["case"], s["hier"].ops[0]
    uref, itref, _, _ = s[precond]
    phi = _field(lsm, cs)
    sol = lsm.elliptic_solve(phi, _rhs(lsm, cs, s["f"]), u0=_guess(s), rtol=RTOL, max_iters=cs.get("max_iters", 2000), precond=precond, **_kwargs(cs, lsm))
    u = sol.u.values()
    u64 = u.astype(np.float64)
    if cs["fixed"] is not None:
        g = np.broadcast_to(np.asarray(cs["g"], dtype=cs["dtype"]), cs["n"])
        assert np.array_equal(_bits(u[cs["fixed"]]), _bits(g[cs["fixed"]]))
    tr, bn = R.true_residual(op, s["f"], u64)
    if bn == 0.0:           # f ≡ 0 on the free nodes: relres is relative to ‖r₀‖₂, the norm of the eliminated right-hand side
        bn = R.true_residual(op, s["f"], s["u0"])[0]
    bound = 2 * RTOL * bn
    if cs["dtype"] == np.float32:
        A = op.matrix()
        extra = abs(A) @ (np.abs(u64).reshape(-1, order="F") * 2.0 ** -24)
        bound += float(np.sqrt(np.sum(np.where(op.free.reshape(-1, order="F"), extra, 0.0) ** 2)))
    if s["direct"] is not None:
        what, dref, ddev = "direct", float(np.abs(uref - s["direct"]).max()), float(np.abs(u64 - s["direct"]).max())
    else:
        what, dref, ddev = "restatement", s["tight"][precond], float(np.abs(u64 - uref).max())
    print(f"{name} {precond}: {sol.iterations} iterations (restatement {itref}), relres {sol.relres:.3e}, true residual {tr / bn:.3e}·‖b‖ "
          f"(bound {bound / bn:.3e}), |u − {what}| {ddev:.3e} (restatement {dref:.3e}), levels {sol.levels}")
    assert sol.relres <= RTOL
    assert tr <= bound
    assert ddev <= 4 * dref
    assert sol.iterations <= itref + 2
    sol.operator.close()
    return sol.iterations


@pytest.mark.parametrize("name", NAMES)
def test_cells_apply_and_energy_are_the_restatements_bits(name):
    check_bits(_lsm(), R.solved(name))


@pytest.mark.parametrize("precond", ["mg", "jacobi"])
@pytest.mark.parametrize("name", NAMES)
def test_solve_against_the_restatement(name, precond):
    check_solve(_lsm(), R.solved(name), name, precond)


@pytest.mark.parametrize("name", NAMES)
def test_mg_needs_fewer_iterations_than_jacobi(name):
    lsm = _lsm()
    s = R.solved(name)
    cs = s["case"]
    phi = _field(lsm, cs)
    it = {}
    for pc in ("mg", "jacobi"):
        sol = lsm.elliptic_solve(phi, s["f"], rtol=RTOL, max_iters=2000, precond=pc, **_kwargs(cs))
        it[pc] = sol.iterations
        sol.operator.close()
    print(name, it)
    assert it["mg"] < it["jacobi"]


@pytest.mark.parametrize("name", ["64x48_upper_patch", "24x33x10_patch"])
def test_not_converged_and_refused_data_leave_u_unchanged(name):
    lsm = _lsm()
    s = R.solved(name)
    cs = s["case"]
    phi = _field(lsm, cs)
    op = lsm.EllipticOperator(phi, **_kwargs(cs))
    calls = []
    real = op.backend.elliptic_solve

    def spy(obj, f, u, rtol, max_iters):      # keeps the field the solve was given
        calls.append((u, u.clone()))
        return real(obj, f, u, rtol, max_iters)

    op.backend.elliptic_solve = spy
    u0 = np.asfortranarray(np.random.default_rng(5).standard_normal(cs["n"]))
    try:
        with pytest.raises(lsm.LsmNotConvergedError):
            op.solve(s["f"], u0=u0, rtol=RTOL, max_iters=2)
        bad = s["f"].copy()
        bad[tuple(m // 2 for m in cs["n"])] = np.nan
        with pytest.raises(ValueError, match="finite"):
            op.solve(bad, u0=u0, rtol=RTOL)
    finally:
        op.backend.elliptic_solve = real
    assert len(calls) == 2
    for after, before in calls:
        assert bool((after.view(before.dtype) == before).all()) or np.array_equal(_bits(after.cpu().numpy()), _bits(before.cpu().numpy()))
    op.close()
    # a NaN in ϕ, and c ≡ 0 without a fixed node, are refused before anything is solved
    vals = cs["phi"].copy()
    vals[tuple(m // 3 for m in cs["n"])] = np.nan
    with pytest.raises(ValueError, match="phi must be finite"):
        lsm.elliptic_solve(_field(lsm, cs, vals), s["f"], **_kwargs(cs))
    with pytest.raises(ValueError, match="singular"):
        lsm.elliptic_solve(phi, s["f"], c=lsm.ROCMeshField(phi.backend, phi.mesh, phi.bcs))      # a device field of zeros


def test_an_operator_solved_twice_equals_two_fresh_solves():
    lsm = _lsm()
    s = R.solved("24x33x10_patch")
    cs = s["case"]
    phi = _field(lsm, cs)
    f1 = s["f"]
    f2 = np.asfortranarray(np.random.default_rng(2).standard_normal(cs["n"]))
    op = lsm.EllipticOperator(phi, **_kwargs(cs))
    kept = [op.solve(f, rtol=RTOL) for f in (f1, f2)]
    for f, k in zip((f1, f2), kept):
        fresh = lsm.elliptic_solve(phi, f, rtol=RTOL, **_kwargs(cs))
        assert fresh.iterations == k.iterations
        assert np.array_equal(_bits(fresh.u.values()), _bits(k.u.values()))
        fresh.operator.close()
    op.close()


@pytest.mark.parametrize("n,hc", [((64, 48), (1.0, 0.75)), ((24, 33, 10), (1.0, 0.8, 0.7))])
def test_regularize_meets_the_residual_test(n, hc):
    lsm = _lsm()
    cs = dict(n=n, hc=hc, h=tuple(x / (m - 1) for x, m in zip(hc, n)), dtype=np.float64)
    g0 = np.asfortranarray(np.random.default_rng(9).standard_normal(n))
    g = _field(lsm, cs, g0)
    alpha = 4 * min(cs["h"])
    sol = lsm.regularize_(g, alpha, rtol=RTOL)
    op = R.Operator(np.full(tuple(m - 1 for m in n), alpha * alpha), cs["h"], 1.0)
    v = g.values()
    tr, bn = R.true_residual(op, g0, v)
    print(f"regularize_ {n}: {sol.iterations} iterations, true residual {tr / bn:.3e}·‖b‖")
    assert tr <= 2 * RTOL * bn
    assert np.array_equal(_bits(v), _bits(sol.u.values()))
    assert np.abs(v).max() < np.abs(g0).max()


def test_an_update_func_sets_the_speed_to_the_energy_density_and_a_step_runs():
    lsm = _lsm()
    s = R.solved("33x33_face")
    cs = s["case"]
    n = cs["n"]
    seen = {}

    def update(coeff, phi, t):
        sol = lsm.elliptic_solve(phi, 1.0, dirichlet=(cs["fixed"], 0.0), rtol=RTOL)
        e = sol.energy_density()
        coeff.set_values(e)
        seen["e"] = e.buf.clone()
        seen["speed"] = coeff.fields[0].clone()
        sol.operator.close()

    grid = lsm.CartesianGrid((0.0,) * len(n), cs["hc"], n)
    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(lsm.MeshField(np.zeros(n), grid), update),), ic=lsm.MeshField(cs["phi"], grid), bc=lsm.NeumannBC(),
                              integrator=lsm.RK3())
    before = eq.current_state().values()
    lsm.integrate_(eq, 1e-6)            # one RK3 step: the CFL step of this speed is far longer
    assert "e" in seen and bool((seen["e"] == seen["speed"]).all())
    assert float(seen["speed"].abs().max()) > 0
    after = eq.current_state().values()
    assert np.isfinite(after).all() and not np.array_equal(after, before)
