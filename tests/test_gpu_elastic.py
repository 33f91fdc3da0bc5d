"""elasticity_solve on the device (csrc/lsm_elastic.hip through the Python API) against the restatement (tests/_elastic_ref.py).

K0 of every level equals the restatement's closed form to 8·2⁻⁵²·max|K0|.  With the device's K0 handed to the restatement, bit
for bit: the cell array (also equal to EllipticOperator's for the same ϕ), A x for a random x, the energy density, the fixed
components of u, and two solves of one operator against two fresh ones.  The solve at rtol = 1e-8, per case and preconditioner,
under tests/test_gpu_elliptic.py's bars:
  * relres ≤ rtol; the true residual of the device's u, computed by the restatement in the stated order, is ≤ 2·rtol·‖b_free‖₂
    (the restatement's own drift between the recursive and the true residual is below 1e-5 of it: tests/test_elastic_host.py
    prints both); a float32 handle stores u rounded: its bound grows by ‖ |A|·|u|·2⁻²⁴ ‖₂;
  * |u − direct solve|∞ ≤ 4× what the restatement's own PCG leaves at the same rtol;
  * iterations ≤ the restatement's + 2, and mg strictly fewer than jacobi.
The two shapes beyond 2048 workgroups of 256 threads (1025×600, 96×96×64) check A x and the energy density bit for bit and run one
mg solve under the first two bars.  The restatement's own PCG takes 23 s at 1025×600 and was run once: 37 iterations, so the bar is
37 + 2.  At 96×96×64 (1.8 million unknowns) neither it nor a direct solve is affordable: the bar is the prototype's largest count
on a 3-D grid with an axis that stops coarsening early, as this one's does (24×33×10: 44 in DESIGN.md §7.18), with the same + 2."""
import numpy as np
import pytest

import _elastic_ref as R

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


def _mask(cs):
    N = len(cs["n"])
    return np.stack([(cs["bits"] >> i) & 1 != 0 for i in range(N)], axis=-1)


def _kwargs(cs):
    return dict(E_in=cs["E_in"], E_out=cs["E_out"], E=cs["E"], nu=cs["nu"], plane=cs["plane"], dirichlet=(_mask(cs), tuple(cs["g"])),
                level=cs.get("level", 0.0))


def _guess(cs):
    """the case's guess for u0= (its fixed components are overwritten by the prescribed values), or None"""
    return None if cs.get("u0") is None else np.asarray(cs["u0"], dtype=np.float64)


def _values(u):
    return np.stack([c.values() for c in u])


def _device_hierarchy(dev, cs):
    """the restatement's hierarchy on the device's own K0, after comparing each level's with the closed form"""
    k0s = []
    h = list(cs["h"])
    n = tuple(cs["n"])
    for l in range(dev.levels):
        K = dev.stiffness(l)
        want = R.k0(tuple(h), cs["nu"], cs["plane"])
        assert np.abs(K - want).max() <= 8 * 2.0 ** -52 * np.abs(want).max(), (l, np.abs(K - want).max())
        k0s.append(K)
        nxt = R.coarsen_shape(n)
        if nxt is not None:
            n, co = nxt
            h = [x * 2.0 if c else x for x, c in zip(h, co)]
    with pytest.raises(lsm_error()):
        dev.stiffness(dev.levels)
    return R.build_case(cs, k0s)[0]


def lsm_error():
    return _lsm().LsmError


def check_bits(lsm, s):
    cs = s["case"]
    phi = _field(lsm, cs)
    dev = lsm.ElasticityOperator(phi, **_kwargs(cs))
    assert dev.levels == s["hier"].levels
    hier = _device_hierarchy(dev, cs)
    op = hier.ops[0]
    assert dev.fixed_dofs == int(op.fixed.sum()) and dev.free_dofs == int(op.free.sum())
    assert np.array_equal(_bits(dev.cells()), _bits(op.E))
    if cs["E"] is None:
        scalar = lsm.EllipticOperator(phi, a_in=cs["E_in"], a_out=cs["E_out"], c=1.0, level=cs.get("level", 0.0))
        assert np.array_equal(_bits(dev.cells()), _bits(scalar.cells()))
        scalar.close()
    x = np.random.default_rng(11).standard_normal((len(cs["n"]),) + tuple(cs["n"]))
    assert np.array_equal(_bits(dev.apply(x)), _bits(op.apply(x)))
    sol = dev.solve(s["f"], rtol=RTOL, max_iters=3000)
    u = _values(sol.u)
    assert u.dtype == cs["dtype"]
    want = op.energy(u.astype(np.float64)).astype(cs["dtype"])
    assert np.array_equal(_bits(sol.energy_density().values()), _bits(want))
    want_c = R.compliance(op, s["f"], u.astype(np.float64))
    assert abs(sol.compliance() - want_c) <= 1e-12 * max(abs(want_c), float(np.prod(cs["h"])) * float(np.abs(R.rhs(op, s["f"]) * u).sum()))
    dev.close()


@pytest.mark.parametrize("name", NAMES)
def test_k0_cells_apply_and_energy_are_the_restatements_bits(name):
    check_bits(_lsm(), R.solved(name))


def check_solve(lsm, s, name, precond):
    cs, op = s["case"], s["hier"].ops[0]
    uref, itref, _, _ = s[precond]
    phi = _field(lsm, cs)
    sol = lsm.elasticity_solve(phi, s["f"], u0=_guess(cs), rtol=RTOL, max_iters=3000, precond=precond, **_kwargs(cs))
    u = _values(sol.u)
    u64 = u.astype(np.float64)
    g = s["u0"].astype(cs["dtype"])
    assert np.array_equal(_bits(u[op.fixed]), _bits(g[op.fixed]))
    tr, bn = R.true_residual(op, s["f"], u64)
    bound = 2 * RTOL * bn
    if cs["dtype"] == np.float32:
        extra = abs(op.matrix()) @ (np.abs(op.flat(u64)) * 2.0 ** -24)
        bound += float(np.sqrt(np.sum(np.where(op.flat(op.free), extra, 0.0) ** 2)))
    dref, ddev = float(np.abs(uref - s["direct"]).max()), float(np.abs(u64 - s["direct"]).max())
    print(f"{name} {precond}: {sol.iterations} iterations (restatement {itref}), relres {sol.relres:.3e}, true residual {tr / bn:.3e}·‖b‖ "
          f"(bound {bound / bn:.3e}), |u − direct| {ddev:.3e} (restatement {dref:.3e}), levels {sol.levels}")
    assert sol.relres <= RTOL
    assert tr <= bound
    assert ddev <= 4 * dref
    assert sol.iterations <= itref + 2
    sol.operator.close()
    return sol.iterations


@pytest.mark.parametrize("name", NAMES)
def test_solve_against_the_restatement_and_mg_needs_fewer_iterations(name):
    lsm = _lsm()
    s = R.solved(name)
    it = {pc: check_solve(lsm, s, name, pc) for pc in ("mg", "jacobi")}
    assert it["mg"] < it["jacobi"]


@pytest.mark.parametrize("name", ["64x48_upper_patch", "24x33x10_patch"])
def test_not_converged_and_refused_data_leave_u_unchanged(name):
    lsm = _lsm()
    s = R.solved(name)
    cs = s["case"]
    N = len(cs["n"])
    phi = _field(lsm, cs)
    op = lsm.ElasticityOperator(phi, **_kwargs(cs))
    calls = []
    real = op.backend.elastic_solve

    def spy(obj, f, u, rtol, max_iters):      # keeps the fields the solve was given
        calls.append((u, [c.clone() for c in u]))
        return real(obj, f, u, rtol, max_iters)

    op.backend.elastic_solve = spy
    u0 = np.random.default_rng(5).standard_normal((N,) + tuple(cs["n"]))
    try:
        with pytest.raises(lsm.LsmNotConvergedError):
            op.solve(s["f"], u0=u0, rtol=RTOL, max_iters=2)
        bad = s["f"].copy()
        bad[(N - 1,) + tuple(m // 2 for m in cs["n"])] = np.nan
        with pytest.raises(ValueError, match="finite"):
            op.solve(bad, u0=u0, rtol=RTOL)
    finally:
        op.backend.elastic_solve = real
    assert len(calls) == 2
    for after, before in calls:
        assert len(after) == N
        for a, b in zip(after, before):
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
    op.close()
    vals = cs["phi"].copy()
    vals[tuple(m // 3 for m in cs["n"])] = np.nan
    with pytest.raises(ValueError, match="phi must be finite"):
        lsm.elasticity_solve(_field(lsm, cs, vals), s["f"], **_kwargs(cs))


def test_create_refuses_singular_and_unsupported_problems():
    lsm = _lsm()
    cs = R.cases()["33x33_clamp"]
    phi = _field(lsm, cs)
    b = phi.backend
    t = b.torch
    bits = cs["bits"].copy()

    def create(bits, nu=0.3, plane=0):
        fixed = t.from_numpy(np.array(bits.reshape(-1, order="F"))).to(b.device)
        return b.elastic_create(phi.buf, 0.0, 1.0, 1e-3, None, nu, plane, fixed, 0)

    with pytest.raises(lsm.LsmError) as e:          # component 1 has no fixed bit anywhere
        create(bits & 1)
    assert e.value.reason == 4 and e.value.detail == 1
    with pytest.raises(lsm.LsmError) as e:
        create(np.full_like(bits, 3))
    assert e.value.reason == 5
    for nu in (0.5, -1.0, float("nan")):
        with pytest.raises(lsm.LsmError):
            create(bits, nu=nu)
    with pytest.raises(lsm.LsmError):
        create(bits, plane=2)
    obj, stats = create(bits)
    assert stats[0] == 4 and stats[1] + stats[2] == 2 * 33 * 33 and stats[2] == 2 * 33
    b.elastic_destroy(obj)
    roller = np.zeros(cs["n"] + (2,), dtype=bool)
    roller[0, :, 0] = True
    with pytest.raises(ValueError, match="no fixed"):
        lsm.elasticity_solve(phi, cs["f"], dirichlet=(roller, 0.0))
    # a 1-D grid and a periodic axis
    g1 = lsm.CartesianGrid((0.0,), (1.0,), (33,))
    p1 = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(np.linspace(-1, 1, 33), g1), bc=lsm.NeumannBC()).current_state()
    with pytest.raises(ValueError, match="1 dimensional"):
        lsm.elasticity_solve(p1, (1.0,), dirichlet=(np.ones(33, dtype=bool), 0.0))
    fixed1 = t.zeros(33, dtype=t.uint8, device=p1.backend.device)
    with pytest.raises(lsm.LsmError, match="1-dimensional"):
        p1.backend.elastic_create(p1.buf, 0.0, 1.0, 1e-3, None, 0.3, 0, fixed1, 0)
    g2 = lsm.CartesianGrid((0.0, 0.0), cs["hc"], cs["n"])
    pp = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(cs["phi"], g2), bc=(lsm.PeriodicBC(), lsm.NeumannBC())).current_state()
    with pytest.raises(ValueError, match="PeriodicBC"):
        lsm.elasticity_solve(pp, cs["f"], **_kwargs(cs))
    fixed2 = t.from_numpy(np.array(bits.reshape(-1, order="F"))).to(pp.backend.device)
    with pytest.raises(lsm.LsmError, match="periodic"):
        pp.backend.elastic_create(pp.buf, 0.0, 1.0, 1e-3, None, 0.3, 0, fixed2, 0)


def test_an_operator_solved_twice_equals_two_fresh_solves():
    lsm = _lsm()
    s = R.solved("24x33x10_patch")
    cs = s["case"]
    phi = _field(lsm, cs)
    f1 = s["f"]
    f2 = np.random.default_rng(2).standard_normal(f1.shape)
    op = lsm.ElasticityOperator(phi, **_kwargs(cs))
    kept = [op.solve(f, rtol=RTOL) for f in (f1, f2)]
    for f, k in zip((f1, f2), kept):
        fresh = lsm.elasticity_solve(phi, f, rtol=RTOL, **_kwargs(cs))
        assert fresh.iterations == k.iterations
        assert np.array_equal(_bits(_values(fresh.u)), _bits(_values(k.u)))
        fresh.operator.close()
    op.close()


@pytest.mark.parametrize("n,itref", [((1025, 600), 37), ((96, 96, 64), 44)])
def test_grid_stride_shapes(n, itref):
    """more nodes than 2048 × 256 threads: the second trip of the grid-stride loops and the index arithmetic"""
    lsm = _lsm()
    N = len(n)
    assert int(np.prod(n)) > 2048 * 256
    hier, f, u0 = R.prototype(n)
    ref = hier.ops[0]
    cs = dict(n=n, hc=tuple((m - 1.0) / (max(n) - 1.0) for m in n), h=ref.h, phi=R.two_holes(n, ref.h), dtype=np.float64)
    phi = _field(lsm, cs)
    dev = lsm.ElasticityOperator(phi, dirichlet=(lsm.face_mask(phi.mesh, 0, 0), 0.0))
    op = R.Operator(ref.E, ref.h, dev.stiffness(0), ref.bits)
    assert np.array_equal(_bits(dev.cells()), _bits(op.E))
    x = np.random.default_rng(11).standard_normal((N,) + n)
    assert np.array_equal(_bits(dev.apply(x)), _bits(op.apply(x)))
    sol = dev.solve(f, rtol=RTOL)
    u = _values(sol.u)
    assert np.array_equal(_bits(sol.energy_density().values()), _bits(op.energy(u)))
    assert np.array_equal(_bits(u[op.fixed]), _bits(u0[op.fixed]))
    tr, bn = R.true_residual(op, f, u)
    print(f"{n}: {sol.iterations} iterations, levels {sol.levels}, relres {sol.relres:.3e}, true residual {tr / bn:.3e}·‖b‖")
    assert sol.relres <= RTOL
    assert tr <= 2 * RTOL * bn
    assert sol.iterations <= itref + 2
    dev.close()


def test_an_update_func_sets_the_speed_to_the_energy_density_and_a_step_runs():
    lsm = _lsm()
    cs = R.cases()["33x33_clamp"]
    n = cs["n"]
    seen = {}

    def update(coeff, phi, t):
        sol = lsm.elasticity_solve(phi, cs["f"], rtol=RTOL, **_kwargs(cs))
        e = sol.energy_density()
        coeff.set_values(e)
        seen["e"] = e.buf.clone()
        seen["speed"] = coeff.fields[0].clone()
        sol.operator.close()

    grid = lsm.CartesianGrid((0.0,) * len(n), cs["hc"], n)
    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(lsm.MeshField(np.zeros(n), grid), update),), ic=lsm.MeshField(cs["phi"], grid), bc=lsm.NeumannBC(),
                              integrator=lsm.RK3())
    before = eq.current_state().values()
    lsm.integrate_(eq, 1e-9)
    assert "e" in seen and bool((seen["e"] == seen["speed"]).all())
    assert float(seen["speed"].abs().max()) > 0
    after = eq.current_state().values()
    assert np.isfinite(after).all() and not np.array_equal(after, before)
