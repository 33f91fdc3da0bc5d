"""Multi-source elliptic solves on the device (lsm_elliptic_solve_many, lsm_elliptic_energy_many, lsm_elliptic_energy_mutual through the
Python API).

The contract of the batched solve needs no restatement of a solver: column k of solve_many is solve of column k, bit for bit — the
field, the iteration count and the relative residual.  So the single solves of the same operator run first and the batch is compared
with them.  That the columns end at different times (one at the initial check, one mid-solve, one last) is asserted on the single
solves, so the comparison cannot pass with the skip path unused.  The two new fields are compared bit for bit with
tests/_elliptic_many_ref.py on the device's own cell coefficients.  Reciprocity, the one comparison to rounding, takes its bar from the
restatement's own PCG solutions at the same rtol (×4) plus the worst-case summation error of the reduction; both are printed."""
import ctypes as C

import numpy as np
import pytest

import _elliptic_many_ref as M
import _elliptic_ref as R

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


def _kwargs(cs):
    kw = dict(a_in=cs["a_in"], a_out=cs["a_out"], a=cs["a"], c=cs["c"])
    if cs["fixed"] is not None:
        kw["dirichlet"] = (cs["fixed"], cs["g"])
    return kw


def _source(cs):
    return np.asfortranarray(np.broadcast_to(np.asarray(cs["f"], dtype=np.float64), cs["n"]))


def _same(a, b):
    """two solutions hold the same bits: u, the iteration count, the relative residual"""
    assert a.iterations == b.iterations, (a.iterations, b.iterations)
    assert np.float64(a.relres).view(np.uint64) == np.float64(b.relres).view(np.uint64), (a.relres, b.relres)
    assert np.array_equal(_bits(a.u.values()), _bits(b.u.values()))


def _check_batch(op, cols, singles, order, **kw):
    """solve_many of the columns `order` (indices into cols = [(f, u0)]) against the single solves"""
    many = op.solve_many([cols[k][0] for k in order], u0=[cols[k][1] for k in order], **kw)
    assert len(many) == len(order) and many.iterations == tuple(singles[k].iterations for k in order)
    assert many.relres == tuple(singles[k].relres for k in order)
    for j, k in enumerate(order):
        _same(many[j], singles[k])
    return many


def _columns(op, f, **kw):
    """the four columns of group 1 and their single solves: cold, warm, a random source, the zero source"""
    cold = op.solve(f, **kw)
    warm_guess = (1.0 + 1e-3) * cold.u.values().astype(np.float64)
    cols = [(f, None), (f, warm_guess), (np.asfortranarray(np.random.default_rng(5).standard_normal(f.shape)), None), (np.zeros_like(f), None)]
    return cols, [cold] + [op.solve(c[0], u0=c[1], **kw) for c in cols[1:]]


# ---- 1. columns are the single solves
GROUP1 = ["33x33_face", "65x20_aniso_h", "64x48_blob", "65x20_no_fixed", "17c_face", "17c_f32", "24x33x10_patch", "24x33x10_aniso_given_a"]


@pytest.mark.parametrize("precond", ["mg", "jacobi"])
@pytest.mark.parametrize("name", GROUP1)
def test_columns_are_the_single_solves(name, precond):
    lsm = _lsm()
    cs = R.cases()[name]
    op = lsm.EllipticOperator(_field(lsm, cs), precond=precond, **_kwargs(cs))
    kw = dict(rtol=RTOL, max_iters=3000)
    cols, singles = _columns(op, _source(cs), **kw)
    it = [s.iterations for s in singles]
    print(f"{name} {precond}: iterations cold {it[0]}, warm {it[1]}, random {it[2]}, zero source {it[3]}")
    if cs["fixed"] is None or not np.any(cs["g"]):
        assert 0 == it[3] < it[1] < it[0], it      # a column ends at the initial check, one mid-solve and one last
    _check_batch(op, cols, singles, [0, 1, 2, 3], **kw)
    _check_batch(op, cols, singles, [0], **kw)
    _check_batch(op, cols, singles, [3, 1], **kw)
    _check_batch(op, cols, singles, [0, 1, 2, 3, 3, 2, 1, 0], **kw)      # the order of the columns does not matter
    op.close()


# ---- 2. one-level and odd shapes: the coarsest kernel carries r·z with one workgroup per column; an unpaired last node
def _small_case(n):
    hc = tuple((m - 1.0) / (max(n) - 1.0) for m in n)
    h = tuple(x / (m - 1) for x, m in zip(hc, n))
    fixed = R.face_mask(n, 0, 0)
    cs = dict(n=n, hc=hc, h=h, phi=R.two_holes(n, h), a=None, a_in=1.0, a_out=1e-3, c=0.0, fixed=fixed, g=0.0, dtype=np.float64)
    # a uniform source and two unit impulses b = e: at the upper corner (the unpaired last node of an even axis) and at the odd interior node
    mass = R.Operator(np.ones(tuple(m - 1 for m in n)), h).m
    sources = [np.ones(n, order="F")]
    corner, odd = tuple(m - 1 for m in n), tuple((m // 2) | 1 for m in n)
    if odd == corner:      # 4 nodes per axis
        odd = tuple(1 for _ in n)
    for j in (corner, odd):
        assert not fixed[j]
        f = np.zeros(n, order="F")
        f[j] = 1.0 / mass[j]
        sources.append(f)
    return cs, sources


@pytest.mark.parametrize("precond", ["mg", "jacobi"])
@pytest.mark.parametrize("n", [(4, 4), (5, 5, 5), (9, 12), (12, 10, 8)])
def test_one_level_and_odd_shapes(n, precond):
    lsm = _lsm()
    cs, sources = _small_case(n)
    op = lsm.EllipticOperator(_field(lsm, cs), precond=precond, **_kwargs(cs))
    assert (op.levels == 1) == (max(n) <= 5)
    kw = dict(rtol=RTOL, max_iters=3000)
    cols = [(f, None) for f in sources]
    singles = [op.solve(f, **kw) for f in sources]
    assert all(s.iterations > 0 for s in singles)
    print(f"{n} {precond}: levels {op.levels}, iterations {[s.iterations for s in singles]}")
    _check_batch(op, cols, singles, [0, 1, 2], **kw)
    op.close()


# ---- 3. launch shapes: the second trip of the grid-stride loops with a column dimension present
@pytest.mark.parametrize("n", [(1025, 600), (96, 96, 64)])
def test_grid_stride_shapes(n):
    lsm = _lsm()
    assert int(np.prod(n)) > 2048 * 256
    hc = tuple((m - 1.0) / (max(n) - 1.0) for m in n)
    h = tuple(x / (m - 1) for x, m in zip(hc, n))
    fixed = R.face_mask(n, 0, 0)
    cs = dict(n=n, hc=hc, h=h, phi=R.two_holes(n, h), dtype=np.float64)
    dev = lsm.EllipticOperator(_field(lsm, cs), dirichlet=(fixed, 0.0))
    cols = [(np.ones(n, order="F"), None), (np.asfortranarray(np.random.default_rng(41).standard_normal(n)), None)]
    kw = dict(rtol=0.97, max_iters=50)
    singles = [dev.solve(c[0], **kw) for c in cols]
    assert all(s.iterations > 0 for s in singles)
    many = _check_batch(dev, cols, singles, [0, 1], **kw)
    print(f"{n}: iterations {many.iterations}")
    w = (0.25, -2.0)
    got_w, got_m = many.energy_density(w).values(), many.mutual_energy_density(0, 1).values()
    if len(n) == 2:
        op = R.Operator(dev.cells(), h, 0.0, fixed)
        us = [s.u.values() for s in many]
        assert np.array_equal(_bits(got_w), _bits(M.energy_weighted(op, us, w)))
        assert np.array_equal(_bits(got_m), _bits(M.energy_mutual(op, us[0], us[1])))
    else:
        e = np.zeros(n)
        for k in range(2):
            e = e + w[k] * many[k].energy_density().values()
        assert np.array_equal(_bits(got_w), _bits(e))
        assert np.array_equal(_bits(got_m), _bits(many.mutual_energy_density(1, 0).values())) and np.any(got_m != 0.0)
        assert np.array_equal(_bits(many.mutual_energy_density(1, 1).values()), _bits(many[1].energy_density().values()))
    dev.close()


# ---- 4. outcomes: nothing is written on failure, the column is named, the refusals
def _raw(op, cols):
    """the flat sources and the K fields that solve_many hands to the library"""
    b = op.backend
    return b.torch.cat([op._source(f) for f, _ in cols]), [op._field(u0) for _, u0 in cols]


def test_nothing_is_written_on_failure():
    lsm = _lsm()
    cs = R.cases()["33x33_face"]
    op = lsm.EllipticOperator(_field(lsm, cs), **_kwargs(cs))
    b = op.backend
    kw = dict(rtol=RTOL, max_iters=3000)
    f0 = _source(cs)
    cols, singles = _columns(op, f0, **kw)
    cold, warm, zero = 0, 1, 3
    order = [cold, zero, warm]
    limit = singles[warm].iterations + 1
    assert singles[cold].iterations > limit
    f, us = _raw(op, [cols[k] for k in order])
    held = [u.buf.clone() for u in us]
    with pytest.raises(lsm.LsmNotConvergedError) as ei:
        b.elliptic_solve_many(op._handle(), f, [u.buf for u in us], RTOL, limit)
    assert ei.value.status == (2, 1, 1) and "column 0" in str(ei.value)
    assert ei.value.iterations == (limit, 0, singles[warm].iterations)
    assert ei.value.relres[2] == singles[warm].relres
    for u, hu in zip(us, held):
        assert bool(b.torch.equal(u.buf, hu))      # the converged columns included
    with pytest.raises(lsm.LsmNotConvergedError) as ei:
        op.solve_many([cols[k][0] for k in order], u0=[cols[k][1] for k in order], rtol=RTOL, max_iters=limit)
    assert ei.value.status == (2, 1, 1) and ei.value.iterations == (limit, 0, singles[warm].iterations)
    # a NaN in column 1's source
    bad = np.array(f0)
    bad[3, 4] = np.nan
    with pytest.raises(ValueError, match="column 1"):
        op.solve_many([f0, bad, f0], **kw)
    f, us = _raw(op, [(f0, None), (bad, None), (f0, None)])
    held = [u.buf.clone() for u in us]
    with pytest.raises(lsm.LsmError) as ei:
        b.elliptic_solve_many(op._handle(), f, [u.buf for u in us], RTOL, 3000)
    assert not isinstance(ei.value, lsm.LsmNotConvergedError) and ei.value.status[1] == -1 and "column 1" in str(ei.value)
    for u, hu in zip(us, held):
        assert bool(b.torch.equal(u.buf, hu))
    op.close()


def test_the_refusals_of_the_c_abi():
    lsm = _lsm()
    L = lsm._lib
    cs = R.cases()["33x33_face"]
    op = lsm.EllipticOperator(_field(lsm, cs), **_kwargs(cs))
    b = op.backend
    lib, h = b.lib, op._handle()
    f0 = _source(cs)
    f, us = _raw(op, [(f0, None)] * 9)
    e = lsm.ROCMeshField(b, us[0].mesh, us[0].bcs)
    held = [u.buf.clone() for u in us]
    it, rel, stat = (C.c_int * 9)(), (C.c_double * 9)(), (C.c_int * 9)()

    def ptrs(fields):
        return (C.c_void_p * max(len(fields), 1))(*[None if u is None else int(u.buf.data_ptr()) for u in fields])

    def solve(K, fields, rtol=RTOL, max_iters=100, fptr=b.ptr(f)):
        return lib.lsm_elliptic_solve_many(h, K, fptr, ptrs(fields), rtol, max_iters, it, rel, stat, None)

    assert solve(2, us[:2]) == L.OK
    two = [u.buf.clone() for u in us[:2]]
    for code in (solve(0, []), solve(9, us), solve(-1, us[:1]),                                  # K out of range
                 solve(2, [us[0], None]), solve(2, [us[0], us[0]]), solve(3, [us[0], us[1], us[0]]),      # a null or repeated field
                 solve(2, us[:2], rtol=0.0), solve(2, us[:2], rtol=float("nan")), solve(2, us[:2], rtol=float("inf")), solve(2, us[:2], rtol=-1e-8),
                 solve(2, us[:2], max_iters=0), solve(2, us[:2], fptr=None)):
        assert code == L.ERR_INVALID
    assert lib.lsm_elliptic_solve_many(h, 2, b.ptr(f), None, RTOL, 100, it, rel, stat, None) == L.ERR_INVALID
    for u, hu in zip(us, two + held[2:]):
        assert bool(b.torch.equal(u.buf, hu))      # nothing ran

    def energy(K, fields, w, out=e):
        return lib.lsm_elliptic_energy_many(h, K, ptrs(fields), (C.c_double * max(len(w), 1))(*w), b.ptr(out.buf))

    assert energy(2, us[:2], [1.0, 2.0]) == L.OK
    for code in (energy(0, [], []), energy(9, us, [1.0] * 9), energy(2, [us[0], None], [1.0, 1.0]), energy(2, [us[0], us[0]], [1.0, 1.0]),
                 energy(2, [us[0], e], [1.0, 1.0]), energy(2, us[:2], [1.0, float("inf")]), energy(2, us[:2], [float("nan"), 1.0])):
        assert code == L.ERR_INVALID
    assert lib.lsm_elliptic_energy_many(h, 2, ptrs(us[:2]), None, b.ptr(e.buf)) == L.ERR_INVALID
    assert lib.lsm_elliptic_energy_many(h, 2, ptrs(us[:2]), (C.c_double * 2)(1.0, 1.0), None) == L.ERR_INVALID

    def mutual(u, v, out):
        return lib.lsm_elliptic_energy_mutual(h, None if u is None else b.ptr(u.buf), None if v is None else b.ptr(v.buf), None if out is None else b.ptr(out.buf))

    assert mutual(us[0], us[1], e) == L.OK and mutual(us[0], us[0], e) == L.OK      # u and v may be the same field
    for code in (mutual(None, us[1], e), mutual(us[0], None, e), mutual(us[0], us[1], None), mutual(e, us[1], e), mutual(us[0], e, e)):
        assert code == L.ERR_INVALID
    # and through Python
    kw = dict(rtol=RTOL, max_iters=3000)
    with pytest.raises(ValueError):
        op.solve_many([], **kw)
    with pytest.raises(ValueError):
        op.solve_many([f0] * 9, **kw)
    with pytest.raises(TypeError):
        op.solve_many(f0, **kw)
    with pytest.raises(ValueError):
        op.solve_many([f0, f0], u0=[None], **kw)
    with pytest.raises(ValueError):
        op.solve_many([f0, f0], homogeneous=[True], **kw)
    many = op.solve_many([f0, 2.0 * f0], **kw)
    with pytest.raises(ValueError):
        many.energy_density((1.0, float("inf")))
    other = lsm.EllipticOperator(_field(lsm, cs), **_kwargs(cs))
    foreign = other.solve(f0, **kw)
    with pytest.raises(ValueError, match="another operator"):
        many[0].mutual_energy_density(foreign)
    other.close()
    op.close()
    with pytest.raises(ValueError, match="closed"):
        op.solve_many([f0], **kw)
    with pytest.raises(ValueError, match="closed"):
        many.energy_density()
    with pytest.raises(ValueError, match="closed"):
        many.mutual_energy_density(0, 1)


# ---- 5. neighbours are undisturbed
def test_single_solves_and_the_modes_are_undisturbed_and_the_workspace_grows():
    lsm = _lsm()
    cs = R.cases()["24x33x10_patch"]
    phi = _field(lsm, cs)
    kw = dict(rtol=RTOL, max_iters=3000)
    rng = np.random.default_rng(23)
    sources = [_source(cs)] + [np.asfortranarray(rng.standard_normal(cs["n"])) for _ in range(4)]
    fresh = lsm.EllipticOperator(phi, **_kwargs(cs))
    want = [fresh.solve(f, **kw) for f in sources[:2]]
    want_m = fresh.modes(2)
    want_lam, want_it, want_x = np.array(want_m.eigenvalues), want_m.iterations, want_m.vectors()
    want_after = fresh.solve(sources[0], **kw)      # a solve after the modes, which borrow the single workspace
    fresh.close()
    fresh5 = lsm.EllipticOperator(phi, **_kwargs(cs))
    want5 = fresh5.solve_many(sources, **kw)

    op = lsm.EllipticOperator(phi, **_kwargs(cs))
    first = op.solve(sources[0], **kw)
    two = op.solve_many(sources[:2], **kw)
    second = op.solve(sources[1], **kw)
    _same(first, want[0])
    _same(second, want[1])
    _same(two[0], want[0])
    _same(two[1], want[1])
    got_m = op.modes(2)
    assert got_m.iterations == want_it and np.array_equal(_bits(np.array(got_m.eigenvalues)), _bits(want_lam))
    assert np.array_equal(_bits(got_m.vectors()), _bits(want_x))
    _same(op.solve(sources[0], **kw), want_after)
    five = op.solve_many(sources, **kw)      # the workspace grows from 2 to 5 columns
    for a, b in zip(five, want5):
        _same(a, b)
    _same(op.solve(sources[0], **kw), want[0])
    again = op.solve_many(sources[3:], **kw)      # and a smaller batch in the larger workspace
    _same(again[0], want5[3])
    _same(again[1], want5[4])
    op.close()
    fresh5.close()


def test_regularize_is_undisturbed_by_a_batched_call_before_it():
    lsm = _lsm()
    cs = R.cases()["33x33_face"]
    g = np.asfortranarray(np.random.default_rng(43).standard_normal(cs["n"]))
    want = lsm.regularize_(_field(lsm, cs, g), 0.05)
    many = lsm.elliptic_solve_many(_field(lsm, cs), [_source(cs), g], rtol=RTOL, **_kwargs(cs))
    got = lsm.regularize_(_field(lsm, cs, g), 0.05)
    _same(got, want)
    many.operator.close()


# ---- 6. the new fields
@pytest.mark.parametrize("name", ["33x33_face", "64x48_blob", "17c_f32", "24x33x10_aniso_given_a"])
def test_weighted_and_mutual_energy_densities_are_the_restatements_bits(name):
    lsm = _lsm()
    cs = R.cases()[name]
    dev = lsm.EllipticOperator(_field(lsm, cs), **_kwargs(cs))
    op = R.Operator(dev.cells(), cs["h"], cs["c"], cs["fixed"])
    rng = np.random.default_rng(29)
    sources = [_source(cs), np.asfortranarray(rng.standard_normal(cs["n"])), np.asfortranarray(rng.standard_normal(cs["n"]))]
    kw = dict(rtol=RTOL, max_iters=3000)
    many = dev.solve_many(sources, **kw)
    us = [s.u.values() for s in many]
    assert us[0].dtype == cs["dtype"]
    us = [u.astype(np.float64) for u in us]
    for w in (None, (1.0, 1.0, 1.0), (0.25, -2.0, 3.0)):
        want = M.energy_weighted(op, us, (1.0, 1.0, 1.0) if w is None else w).astype(cs["dtype"])      # one rounding to the storage type
        assert np.array_equal(_bits(many.energy_density(w).values()), _bits(want)), w
    one = dev.solve_many(sources[:1], **kw)
    assert np.array_equal(_bits(one.energy_density().values()), _bits(one[0].energy_density().values()))      # w = (1,)
    assert np.array_equal(_bits(one.energy_density((1.0,)).values()), _bits(op.energy(us[0]).astype(cs["dtype"])))
    for i, j in ((0, 1), (1, 0), (2, 1)):
        want = M.energy_mutual(op, us[i], us[j]).astype(cs["dtype"])
        assert np.array_equal(_bits(many.mutual_energy_density(i, j).values()), _bits(want)), (i, j)
        assert np.array_equal(_bits(many.mutual_energy_density(j, i).values()), _bits(want)), (j, i)
        assert np.array_equal(_bits(many[i].mutual_energy_density(many[j]).values()), _bits(want))
    for i in range(3):
        assert np.array_equal(_bits(many.mutual_energy_density(i, i).values()), _bits(many[i].energy_density().values()))
    c = many.compliances()
    assert c == tuple(s.compliance() for s in many) and many.compliance() == (0.0 + c[0]) + c[1] + c[2]
    assert many.compliance((0.25, -2.0, 3.0)) == (0.0 + 0.25 * c[0]) + -2.0 * c[1] + 3.0 * c[2]
    assert many.cross_compliance(1, 1) == c[1]
    dev.close()


def test_a_homogeneous_column_takes_zero_on_the_dirichlet_nodes():
    lsm = _lsm()
    cs = R.cases()["64x48_blob"]
    assert np.any(cs["g"])
    many = lsm.elliptic_solve_many(_field(lsm, cs), [_source(cs), np.asfortranarray(np.random.default_rng(31).standard_normal(cs["n"]))],
                                   homogeneous=(False, True), rtol=RTOL, **_kwargs(cs))
    fixed = cs["fixed"]
    u0, u1 = many[0].u.values(), many[1].u.values()
    assert np.all(u0[fixed] == cs["g"]) and not np.any(u1[fixed]) and np.any(u1[~fixed])
    single = many.operator.solve(_source(cs), rtol=RTOL)
    _same(many[0], single)
    many.operator.close()


# ---- 7. reciprocity
@pytest.mark.parametrize("name", ["33x33_face", "17c_face"])
def test_reciprocity(name):
    lsm = _lsm()
    s = R.solved(name)
    cs, hier = s["case"], s["hier"]
    op = hier.ops[0]
    assert not np.any(cs["g"])
    f0, f1 = s["f"], np.asfortranarray(np.random.default_rng(37).standard_normal(cs["n"]))
    many = lsm.elliptic_solve_many(_field(lsm, cs), [f0, f1], rtol=RTOL, **_kwargs(cs))
    c01, c10 = many.cross_compliance(0, 1), many.cross_compliance(1, 0)
    r0 = s["mg"][0]
    r1 = R.pcg(hier, f1, s["u0"], RTOL, 2000, "mg")[0]
    ref = abs(R.compliance(op, f0, r1) - R.compliance(op, f1, r0))
    u0, u1 = many[0].u.values(), many[1].u.values()
    floor = 2.0 ** -53 * u0.size * float(np.prod(op.h)) * float(np.sum(np.abs(R.rhs(op, f0) * u1)) + np.sum(np.abs(R.rhs(op, f1) * u0)))
    print(f"{name}: cross compliances {c01:.17g}, {c10:.17g}: difference {abs(c01 - c10):.3e}; the restatement's {ref:.3e}, summation floor {floor:.3e}")
    assert abs(c01 - c10) <= 4 * ref + floor
    many.operator.close()


# ---- 8. an update_func step whose speed is the mutual energy density of a state and its adjoint
def test_an_update_func_sets_the_speed_to_the_mutual_energy_density_and_a_step_runs():
    lsm = _lsm()
    cs = R.cases()["33x33_face"]
    n = cs["n"]
    sensor = np.zeros(n, order="F")
    sensor[24:28, 14:19] = 1.0      # l: the mean temperature over a patch
    seen = {}

    def update(coeff, phi, t):
        many = lsm.elliptic_solve_many(phi, [_source(cs), sensor], homogeneous=(False, True), rtol=RTOL, **_kwargs(cs))
        m = many.mutual_energy_density(0, 1)
        coeff.set_values(m)
        seen["m"] = m.buf.clone()
        seen["speed"] = coeff.fields[0].clone()
        many.operator.close()

    grid = lsm.CartesianGrid((0.0,) * len(n), cs["hc"], n)
    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(lsm.MeshField(np.zeros(n), grid), update),), ic=lsm.MeshField(cs["phi"], grid), bc=lsm.NeumannBC(),
                              integrator=lsm.RK3())
    before = eq.current_state().values()
    lsm.integrate_(eq, 1e-9)
    assert "m" in seen and bool((seen["m"] == seen["speed"]).all())
    assert float(seen["speed"].abs().max()) > 0
    after = eq.current_state().values()
    assert np.all(np.isfinite(after)) and np.any(after != before)
