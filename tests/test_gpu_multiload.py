"""Multi-load elasticity on the device (lsm_elastic_solve_many, lsm_elastic_energy_many, lsm_elastic_energy_mutual through the Python
API).

The contract of the batched solve needs no restatement of a solver: column k of solve_many is solve of column k, bit for bit — the
displacements, the iteration count and the relative residual.  So the single solves of the same operator run first and the batch is
compared with them.  That the columns end at different times (one at the initial check, one mid-solve, one last) is asserted on the
single solves, so the comparison cannot pass with the skip path unused.  The two new fields are compared bit for bit with
tests/_multiload_ref.py on the device's own K0 and cell moduli.  Reciprocity, the one comparison to rounding, takes its bar from the
restatement's own PCG solutions at the same rtol (×4) plus the worst-case summation error of the reduction; both are printed."""
import numpy as np
import pytest

import _elastic_ref as R
import _multiload_ref as M

pytestmark = pytest.mark.gpu

RTOL = 1e-8


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
    return lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=mf, bc=lsm.NeumannBC()).current_state()


def _mask(cs):
    return np.stack([(cs["bits"] >> i) & 1 != 0 for i in range(len(cs["n"]))], axis=-1)


def _kwargs(cs):
    return dict(E_in=cs["E_in"], E_out=cs["E_out"], E=cs["E"], nu=cs["nu"], plane=cs["plane"], dirichlet=(_mask(cs), tuple(cs["g"])),
                level=cs.get("level", 0.0))


def _values(u):
    return np.stack([c.values() for c in u])


def _same(a, b):
    """two solutions hold the same bits: u per component, the iteration count, the relative residual"""
    assert a.iterations == b.iterations, (a.iterations, b.iterations)
    assert np.float64(a.relres).view(np.uint64) == np.float64(b.relres).view(np.uint64), (a.relres, b.relres)
    for x, y in zip(a.u, b.u):
        assert np.array_equal(_bits(x.values()), _bits(y.values()))


def _check_batch(op, cols, singles, order, **kw):
    """solve_many of the columns `order` (indices into cols = [(f, u0)]) against the single solves"""
    many = op.solve_many([cols[k][0] for k in order], u0=[cols[k][1] for k in order], **kw)
    assert len(many) == len(order) and many.iterations == tuple(singles[k].iterations for k in order)
    for j, k in enumerate(order):
        _same(many[j], singles[k])
    return many


def _columns(op, f, **kw):
    """the four columns of group 1 and their single solves: cold, warm, a random load, the zero load"""
    cold = op.solve(f, **kw)
    warm_guess = (1.0 + 1e-3) * _values(cold.u).astype(np.float64)
    cols = [(f, None), (f, warm_guess), (np.random.default_rng(5).standard_normal(f.shape), None), (np.zeros_like(f), None)]
    return cols, [cold] + [op.solve(c[0], u0=c[1], **kw) for c in cols[1:]]


# ---- 1. columns are the single solves
GROUP1 = ["33x33_clamp", "65x20_aniso_rollers", "17c_clamp", "24x33x10_patch", "17c_f32", "33x33_contrast1_strain"]


@pytest.mark.parametrize("precond", ["mg", "jacobi"])
@pytest.mark.parametrize("name", GROUP1)
def test_columns_are_the_single_solves(name, precond):
    lsm = _lsm()
    cs = R.cases()[name]
    op = lsm.ElasticityOperator(_field(lsm, cs), precond=precond, **_kwargs(cs))
    kw = dict(rtol=RTOL, max_iters=3000)
    cols, singles = _columns(op, cs["f"], **kw)
    it = [s.iterations for s in singles]
    print(f"{name} {precond}: iterations cold {it[0]}, warm {it[1]}, random {it[2]}, zero load {it[3]}")
    if not np.any(cs["g"]):
        assert 0 == it[3] < it[1] < it[0], it      # a column ends at the initial check, one mid-solve and one last
    _check_batch(op, cols, singles, [0, 1, 2, 3], **kw)
    _check_batch(op, cols, singles, [0], **kw)
    _check_batch(op, cols, singles, [3, 1], **kw)
    _check_batch(op, cols, singles, [0, 1, 2, 3, 3, 2, 1, 0], **kw)      # the order of the columns does not matter
    op.close()


# ---- 2. one-level and odd shapes: the coarsest kernel carries r·z with one workgroup per column; an unpaired last node
def _small_case(n, side):
    N = len(n)
    hc = tuple((m - 1.0) / (max(n) - 1.0) for m in n)
    h = tuple(x / (m - 1) for x, m in zip(hc, n))
    t = [0.0] * N
    t[1] = -1.0
    bits = R.face_bits(n, 0, side, (1 << N) - 1)
    cs = dict(n=n, hc=hc, h=h, phi=R.two_holes(n, h), E=None, E_in=1.0, E_out=1e-3, nu=0.3, plane="stress", bits=np.asfortranarray(bits), g=np.zeros(N),
              dtype=np.float64)
    # unit impulses b = e: at the corner that is upper in every axis but the clamped one, where it is the free end, and at the odd interior node
    corner = tuple(m - 1 for m in n) if side == 0 else (0,) + tuple(m - 1 for m in n[1:])
    odd = tuple((m // 2) | 1 for m in n)
    mass = R.Operator(np.ones(tuple(m - 1 for m in n)), h, R.k0(h), bits).m
    loads = [R.traction(n, h, 0, 1 - side, t)]
    for j, i in ((corner, 0), (odd, N - 1)):
        f = np.zeros((N,) + n)
        f[(i,) + j] = 1.0 / mass[j]
        loads.append(f)
    return cs, loads


@pytest.mark.parametrize("precond", ["mg", "jacobi"])
@pytest.mark.parametrize("n,side", [((4, 4), 0), ((5, 5, 5), 0), ((9, 12), 0), ((12, 10, 8), 1)])
def test_one_level_and_odd_shapes(n, side, precond):
    lsm = _lsm()
    cs, loads = _small_case(n, side)
    op = lsm.ElasticityOperator(_field(lsm, cs), precond=precond, **_kwargs(cs))
    kw = dict(rtol=RTOL, max_iters=3000)
    cols = [(f, None) for f in loads]
    singles = [op.solve(f, **kw) for f in loads]
    assert all(s.iterations > 0 for s in singles)
    print(f"{n} {precond}: levels {op.levels}, iterations {[s.iterations for s in singles]}")
    _check_batch(op, cols, singles, [0, 1, 2], **kw)
    op.close()


# ---- 3. launch shapes: the second trip of the grid-stride loops with a column dimension present
@pytest.mark.parametrize("n", [(1025, 600), (96, 96, 64)])
def test_grid_stride_shapes(n):
    lsm = _lsm()
    N = len(n)
    assert int(np.prod(n)) > 2048 * 256
    hc = tuple((m - 1.0) / (max(n) - 1.0) for m in n)
    h = tuple(x / (m - 1) for x, m in zip(hc, n))
    cs = dict(n=n, hc=hc, h=h, phi=R.two_holes(n, h), dtype=np.float64)
    phi = _field(lsm, cs)
    dev = lsm.ElasticityOperator(phi, dirichlet=(lsm.face_mask(phi.mesh, 0, 0), 0.0))
    t1, t2 = [0.0] * N, [0.0] * N
    t1[1], t2[0] = -1.0, 1.0
    cols = [(R.traction(n, h, 0, 1, t1), None), (R.traction(n, h, 0, 1, t2), None)]
    kw = dict(rtol=R.FIRST_RTOL, max_iters=50)
    singles = [dev.solve(c[0], **kw) for c in cols]
    many = _check_batch(dev, cols, singles, [0, 1], **kw)
    print(f"{n}: iterations {many.iterations}")
    w = (0.25, -2.0)
    got_w, got_m = many.energy_density(w).values(), many.mutual_energy_density(0, 1).values()
    us = [_values(s.u) for s in many]
    if N == 2:
        op = R.Operator(dev.cells(), h, dev.stiffness(0), R.face_bits(n, 0, 0, 3))
        assert np.array_equal(_bits(got_w), _bits(M.energy_weighted(op, us, w)))
        assert np.array_equal(_bits(got_m), _bits(M.energy_mutual(op, us[0], us[1])))
    else:
        e = np.zeros(n)
        for k in range(2):
            e = e + w[k] * many[k].energy_density().values()
        assert np.array_equal(_bits(got_w), _bits(e))
        assert np.array_equal(_bits(many.mutual_energy_density(1, 1).values()), _bits(many[1].energy_density().values()))
    dev.close()


# ---- 4. nothing is written on failure
def _raw(op, cols):
    """the flat loads and the K lists of N fields that solve_many hands to the library"""
    b = op.backend
    us = [op._fields(u0) for _, u0 in cols]
    return b.torch.cat([op._load(f) for f, _ in cols]), us


def test_nothing_is_written_on_failure():
    lsm = _lsm()
    cs = R.cases()["33x33_clamp"]
    op = lsm.ElasticityOperator(_field(lsm, cs), **_kwargs(cs))
    b = op.backend
    kw = dict(rtol=RTOL, max_iters=3000)
    cols, singles = _columns(op, cs["f"], **kw)
    cold, warm, zero = 0, 1, 3
    order = [cold, zero, warm]
    limit = singles[warm].iterations + 1
    assert singles[cold].iterations > limit
    f, us = _raw(op, [cols[k] for k in order])
    held = [[c.buf.clone() for c in u] for u in us]
    with pytest.raises(lsm.LsmNotConvergedError) as ei:
        b.elastic_solve_many(op._handle(), f, [[c.buf for c in u] for u in us], RTOL, limit)
    assert ei.value.status == (2, 1, 1) and "column 0" in str(ei.value)
    assert ei.value.iterations == (limit, 0, singles[warm].iterations)
    assert ei.value.relres[2] == singles[warm].relres
    for u, hu in zip(us, held):
        for c, hc in zip(u, hu):
            assert bool(b.torch.equal(c.buf, hc))      # the converged columns included
    with pytest.raises(lsm.LsmNotConvergedError) as ei:
        op.solve_many([cols[k][0] for k in order], u0=[cols[k][1] for k in order], rtol=RTOL, max_iters=limit)
    assert ei.value.status == (2, 1, 1)
    # a NaN in column 1's load
    bad = np.array(cs["f"])
    bad[1][3, 4] = np.nan
    with pytest.raises(ValueError, match="column 1"):
        op.solve_many([cs["f"], bad, cs["f"]], **kw)
    f, us = _raw(op, [(cs["f"], None), (bad, None), (cs["f"], None)])
    held = [[c.buf.clone() for c in u] for u in us]
    with pytest.raises(lsm.LsmError) as ei:
        b.elastic_solve_many(op._handle(), f, [[c.buf for c in u] for u in us], RTOL, 3000)
    assert not isinstance(ei.value, lsm.LsmNotConvergedError) and ei.value.status[1] == -1 and "column 1" in str(ei.value)
    for u, hu in zip(us, held):
        for c, hc in zip(u, hu):
            assert bool(b.torch.equal(c.buf, hc))
    # the refusals
    with pytest.raises(ValueError):
        op.solve_many([], **kw)
    with pytest.raises(ValueError):
        op.solve_many([cs["f"]] * 9, **kw)
    f, us = _raw(op, [(cs["f"], None), (cs["f"], None)])
    with pytest.raises(lsm.LsmError):
        b.elastic_solve_many(op._handle(), f, [[c.buf for c in us[0]], [us[1][0].buf, us[0][1].buf]], RTOL, 3000)      # a repeated field
    e = lsm.ROCMeshField(b, us[0][0].mesh, us[0][0].bcs)
    with pytest.raises(lsm.LsmError):
        b.elastic_energy_many(op._handle(), [[us[0][0].buf, e.buf]], [1.0], e.buf)      # an output that is an input
    with pytest.raises(lsm.LsmError):
        b.elastic_energy_mutual(op._handle(), [us[0][0].buf, us[0][0].buf], [c.buf for c in us[1]], e.buf)      # repeated within u
    many = op.solve_many([cs["f"], cols[2][0]], **kw)
    with pytest.raises(ValueError):
        many.energy_density((1.0, float("inf")))
    other = lsm.ElasticityOperator(_field(lsm, cs), **_kwargs(cs))
    foreign = other.solve(cs["f"], **kw)
    with pytest.raises(ValueError, match="another operator"):
        many[0].mutual_energy_density(foreign)
    other.close()
    op.close()
    with pytest.raises(ValueError, match="closed"):
        op.solve_many([cs["f"]], **kw)
    with pytest.raises(ValueError, match="closed"):
        many.energy_density()
    with pytest.raises(ValueError, match="closed"):
        many.mutual_energy_density(0, 1)


# ---- 5. neighbours are undisturbed
def test_single_solves_and_the_stress_adjoint_are_undisturbed_and_the_workspace_grows():
    lsm = _lsm()
    cs = R.cases()["24x33x10_patch"]
    phi = _field(lsm, cs)
    kw = dict(rtol=RTOL, max_iters=3000)
    rng = np.random.default_rng(23)
    loads = [cs["f"]] + [rng.standard_normal(cs["f"].shape) for _ in range(4)]
    fresh = lsm.ElasticityOperator(phi, **_kwargs(cs))
    want = [fresh.solve(f, **kw) for f in loads[:2]]
    want_s = want[0].stress_sensitivity(p=6.0)
    fresh.close()
    fresh5 = lsm.ElasticityOperator(phi, **_kwargs(cs))
    want5 = fresh5.solve_many(loads, **kw)

    op = lsm.ElasticityOperator(phi, **_kwargs(cs))
    first = op.solve(loads[0], **kw)
    two = op.solve_many(loads[:2], **kw)
    second = op.solve(loads[1], **kw)
    _same(first, want[0])
    _same(second, want[1])
    _same(two[0], want[0])
    _same(two[1], want[1])
    got_s = first.stress_sensitivity(p=6.0)
    assert got_s.iterations == want_s.iterations and got_s.value == want_s.value
    assert np.array_equal(_bits(got_s.field.values()), _bits(want_s.field.values()))
    five = op.solve_many(loads, **kw)      # the workspace grows from 2 to 5 columns
    for a, b in zip(five, want5):
        _same(a, b)
    _same(op.solve(loads[0], **kw), want[0])
    op.close()
    fresh5.close()


# ---- 6. the new fields
@pytest.mark.parametrize("name", ["33x33_clamp", "64x48_blob_roller", "17c_f32", "24x33x10_aniso_given_E"])
def test_weighted_and_mutual_energy_densities_are_the_restatements_bits(name):
    lsm = _lsm()
    cs = R.cases()[name]
    dev = lsm.ElasticityOperator(_field(lsm, cs), **_kwargs(cs))
    op = R.Operator(dev.cells(), cs["h"], dev.stiffness(0), cs["bits"])
    rng = np.random.default_rng(29)
    loads = [cs["f"], rng.standard_normal(cs["f"].shape), rng.standard_normal(cs["f"].shape)]
    kw = dict(rtol=RTOL, max_iters=3000)
    many = dev.solve_many(loads, **kw)
    us = [_values(s.u) for s in many]
    assert us[0].dtype == cs["dtype"]
    us = [u.astype(np.float64) for u in us]
    for w in (None, (1.0, 1.0, 1.0), (0.25, -2.0, 3.0)):
        want = M.energy_weighted(op, us, (1.0, 1.0, 1.0) if w is None else w).astype(cs["dtype"])      # one rounding to the storage type
        assert np.array_equal(_bits(many.energy_density(w).values()), _bits(want)), w
    one = dev.solve_many(loads[:1], **kw)
    assert np.array_equal(_bits(one.energy_density().values()), _bits(one[0].energy_density().values()))
    assert np.array_equal(_bits(one.energy_density((0.25,)).values()), _bits(M.energy_weighted(op, us[:1], (0.25,)).astype(cs["dtype"])))
    for i, j in ((0, 1), (1, 0), (2, 1)):
        want = M.energy_mutual(op, us[i], us[j]).astype(cs["dtype"])
        assert np.array_equal(_bits(many.mutual_energy_density(i, j).values()), _bits(want)), (i, j)
        assert np.array_equal(_bits(many[i].mutual_energy_density(many[j]).values()), _bits(want))
    for i in range(3):
        assert np.array_equal(_bits(many.mutual_energy_density(i, i).values()), _bits(many[i].energy_density().values()))
    c = many.compliances()
    assert c == tuple(s.compliance() for s in many) and many.compliance() == (0.0 + c[0]) + c[1] + c[2]
    assert many.compliance((0.25, -2.0, 3.0)) == (0.0 + 0.25 * c[0]) + -2.0 * c[1] + 3.0 * c[2]
    assert many.cross_compliance(1, 1) == c[1]
    dev.close()


def test_a_homogeneous_column_takes_zero_on_the_fixed_components():
    lsm = _lsm()
    cs = R.cases()["33x33_contrast1_strain"]
    assert np.any(cs["g"])
    many = lsm.elasticity_solve_many(_field(lsm, cs), [cs["f"], np.random.default_rng(31).standard_normal(cs["f"].shape)], homogeneous=(False, True), rtol=RTOL,
                                     **_kwargs(cs))
    fixed = np.stack([(cs["bits"] >> i) & 1 != 0 for i in range(2)])
    u0, u1 = _values(many[0].u), _values(many[1].u)
    g = np.broadcast_to(np.asarray(cs["g"]).reshape(2, 1, 1), u0.shape)
    assert np.array_equal(u0[fixed], g[fixed]) and not np.any(u1[fixed]) and np.any(u1[~fixed])
    many.operator.close()


# ---- 7. reciprocity
@pytest.mark.parametrize("name", ["33x33_clamp", "17c_clamp"])
def test_reciprocity(name):
    lsm = _lsm()
    s = R.solved(name)
    cs, hier = s["case"], s["hier"]
    op = hier.ops[0]
    assert not np.any(cs["g"])
    f0, f1 = s["f"], np.random.default_rng(37).standard_normal(s["f"].shape)
    many = lsm.elasticity_solve_many(_field(lsm, cs), [f0, f1], rtol=RTOL, **_kwargs(cs))
    c01, c10 = many.cross_compliance(0, 1), many.cross_compliance(1, 0)
    r0 = s["mg"][0]
    r1 = R.pcg(hier, f1, s["u0"], RTOL, 3000, "mg")[0]
    ref = abs(R.compliance(op, f0, r1) - R.compliance(op, f1, r0))
    u0, u1 = _values(many[0].u), _values(many[1].u)
    floor = 2.0 ** -53 * u0.size * float(np.prod(op.h)) * float(np.sum(np.abs(R.rhs(op, f0) * u1)) + np.sum(np.abs(R.rhs(op, f1) * u0)))
    print(f"{name}: cross compliances {c01:.17g}, {c10:.17g}: difference {abs(c01 - c10):.3e}; the restatement's {ref:.3e}, summation floor {floor:.3e}")
    assert abs(c01 - c10) <= 4 * ref + floor
    many.operator.close()


# ---- 8. an update_func step whose speed is the weighted energy density of two load cases
def test_an_update_func_sets_the_speed_to_the_weighted_energy_density_and_a_step_runs():
    lsm = _lsm()
    cs = R.cases()["33x33_clamp"]
    n = cs["n"]
    f2 = R.traction(n, cs["h"], 0, 1, (1.0, 0.0))
    seen = {}

    def update(coeff, phi, t):
        many = lsm.elasticity_solve_many(phi, [cs["f"], f2], rtol=RTOL, **_kwargs(cs))
        e = many.energy_density((0.75, 0.25))
        coeff.set_values(e)
        seen["e"] = e.buf.clone()
        seen["speed"] = coeff.fields[0].clone()
        many.operator.close()

    grid = lsm.CartesianGrid((0.0,) * len(n), cs["hc"], n)
    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(lsm.MeshField(np.zeros(n), grid), update),), ic=lsm.MeshField(cs["phi"], grid), bc=lsm.NeumannBC(),
                              integrator=lsm.RK3())
    before = eq.current_state().values()
    lsm.integrate_(eq, 1e-9)
    assert "e" in seen and bool((seen["e"] == seen["speed"]).all())
    assert float(seen["speed"].abs().max()) > 0
    after = eq.current_state().values()
    assert np.all(np.isfinite(after)) and np.any(after != before)
