"""elliptic_solve without a device: the restatement (tests/_elliptic_ref.py) has the properties the device tests rely on — a
symmetric operator whose rows sum to c·m, positive definite on the free nodes, exact fill fractions, second-order convergence, a
symmetric positive V-cycle, fewer V-cycle than Jacobi iterations on every case of tests/test_gpu_elliptic.py and of
tests/test_gpu_elliptic_edges.py, a first iterate that shows the preconditioner — and the Python API refuses what needs no device
to refuse."""
import types

import numpy as np
import pytest

import _elliptic_ref as R

EPS = np.finfo(np.float64).eps


def _small_ops():
    rng = np.random.default_rng(3)
    out = []
    for n, h in (((9, 12), (0.1, 0.07)), ((5, 6, 7), (0.2, 0.1, 0.15))):
        phi = R.two_holes(n, h)
        a = R.cell_coefficients(phi, h, 0.0, 1.0, 1e-3)
        fixed = R.face_mask(n, 0, 0)
        fixed[tuple(m // 2 for m in n)] = True
        out.append(R.Operator(a, h, 0.3 + rng.random(n), fixed))
        out.append(R.Operator(a, h, 0.0, fixed))
    return out


def test_the_operator_is_symmetric_and_its_rows_sum_to_c_m():
    for op in _small_ops():
        A = op.matrix()
        assert abs(A - A.T).max() == 0.0
        rows = np.asarray(A.sum(axis=1)).reshape(-1)
        scale = np.asarray(abs(A).sum(axis=1)).reshape(-1)
        assert np.all(np.abs(rows - op.cm.reshape(-1, order="F")) <= 8 * EPS * scale)
        x = np.random.default_rng(0).standard_normal(op.n)
        y = op.apply(x)
        assert np.abs(y - (A @ x.reshape(-1, order="F")).reshape(op.n, order="F")).max() <= 16 * EPS * np.abs(y).max()
        assert np.abs(A.diagonal() - op.D.reshape(-1, order="F")).max() <= 8 * EPS * op.D.max()


def test_the_operator_is_positive_definite_on_the_free_nodes():
    for op in _small_ops():
        free = op.free.reshape(-1, order="F")
        w = np.linalg.eigvalsh(op.matrix()[free][:, free].toarray())
        assert w.min() > 0, w.min()


@pytest.mark.parametrize("x0", [0.25, 0.3125, 0.4, 0.53, 0.9])
def test_theta_is_the_exact_fill_fraction_of_an_axis_aligned_half_space(x0):
    for n, hc, d in (((17, 9), (1.0, 0.5), 0), ((9, 17), (0.5, 1.0), 1), ((9, 6, 17), (0.5, 0.4, 1.0), 2)):
        h = tuple(x / (m - 1) for x, m in zip(hc, n))
        x = np.arange(n[d]) * h[d]
        phi = np.asfortranarray(np.broadcast_to((x - x0).reshape([-1 if e == d else 1 for e in range(len(n))]), n))
        theta = R.cell_coefficients(phi, h, 0.0, 1.0, 0.0)
        vol = float(np.prod(h)) * float(theta.sum())
        exact = x0 * float(np.prod([hc[e] for e in range(len(n)) if e != d]))
        assert abs(vol - exact) <= 64 * EPS * exact * theta.size ** 0.5, (vol, exact)
        # a level other than zero moves the interface with it
        theta2 = R.cell_coefficients(phi + 0.125, h, 0.125, 1.0, 0.0)
        assert np.abs(theta2 - theta).max() <= 64 * EPS


def test_second_order_convergence_with_natural_faces():
    errs = {}
    for m in (17, 33, 65):
        n, h = (m, m), (1.0 / (m - 1),) * 2
        x, y = np.meshgrid(np.arange(m) * h[0], np.arange(m) * h[1], indexing="ij")
        u = np.cos(np.pi * x) * np.cos(2 * np.pi * y)
        op = R.Operator(np.ones((m - 1, m - 1)), h, 1.0)
        got = R.direct(op, (1 + 5 * np.pi ** 2) * u, np.zeros(n))
        errs[m] = np.abs(got - u).max()
    print(errs)
    assert errs[33] / errs[65] > 3 and errs[17] / errs[33] > 3


def test_the_v_cycle_is_a_symmetric_positive_operator():
    n, h = (9, 12), (0.1, 0.07)
    phi = R.two_holes(n, h)
    fixed = R.face_mask(n, 1, 1)
    fixed[:, -1] &= np.arange(9) > 3           # a patch on the upper face of the even axis: it vanishes from the coarse grids
    hier = R.Hierarchy(R.Operator(R.cell_coefficients(phi, h, 0.0, 1.0, 1e-3), h, 0.0, fixed))
    assert [o.n for o in hier.ops] == [(9, 12), (5, 6), (5, 3)]
    free = np.flatnonzero(hier.ops[0].free.reshape(-1, order="F"))
    M = np.zeros((free.size, free.size))
    for k, i in enumerate(free):
        e = np.zeros(int(np.prod(n)))
        e[i] = 1.0
        M[:, k] = hier.vcycle(e.reshape(n, order="F")).reshape(-1, order="F")[free]
    assert np.abs(M - M.T).max() <= 64 * EPS * np.abs(M).max()
    assert np.linalg.eigvalsh(0.5 * (M + M.T)).min() > 0


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_the_v_cycle_needs_fewer_iterations_than_jacobi(name):
    """the condition tests/test_gpu_elliptic.py relies on, established on the CPU; the drift between the recursive and the true
    residual of the restatement is printed (it is below 1e-4 of the residual in every case: the GPU test's factor 2 is ample)"""
    s = R.solved(name)
    op = s["hier"].ops[0]
    for pc in ("mg", "jacobi"):
        u, it, rel, ok = s[pc]
        assert ok
        if s["case"]["dtype"] == np.float64:
            tr, bn = R.true_residual(op, s["f"], u)
            print(f"{name} {pc}: {it} iterations, recursive {rel:.6e}, true {tr / bn:.6e}, |u - direct| {np.abs(u - s['direct']).max():.3e}")
            assert tr <= 1.01 * max(rel, 1e-12) * bn + 1e-12 * bn
    assert s["mg"][1] < s["jacobi"][1]


# ---- what tests/test_gpu_elliptic_edges.py relies on
@pytest.mark.parametrize("name,precond", R.FIRST_ITERATE_PAIRS)
def test_the_first_iterate_shows_the_preconditioner(name, precond):
    """From u0 = 0 with zero Dirichlet values a solve at rtol = 0.95 stops after exactly one iteration, for every right-hand side
    of first_iterate_rhs: the relative residual after iteration 1 is ≤ 0.9 (0.95 would do; the margin is for the device's
    rounding).  Measured, mg: 0.031 … 0.894 over the 63 pairs, the largest 64x48_upper_patch with the corner impulse; jacobi:
    0.407 … 0.707.  4x40_face fails it (1.317 for the impulse at n − 2; 0.442 … 0.633 for the others: point Jacobi smooths a
    strip four nodes wide badly), so the same shape with the lower face of axis 0 fixed, 4x40_side, takes its place (0.071 … 0.243).
    The long-double u₁ (first_iterate_ld, its own apply and transfers) and the float64 one (pcg, scipy's P) agree to
    0.4e-16 … 6.4e-16 of max|u| (jacobi: 0 … 3.0e-16; each pair's figure is printed): that spread is the device test's yardstick, and 64 ε bounds it here —
    two statements of the V-cycle that differed in a weight would differ by 1e-3 of max|u| or more."""
    s = R.any_solved(name)
    hier = s["hier"]
    op = hier.ops[0]
    rhs = R.first_iterate_rhs(op)
    assert "normal" in rhs and len(rhs) >= 3              # an impulse at a fixed node is left out
    for fname, f in rhs.items():
        b = R.rhs(op, f)
        if fname != "normal":
            assert np.count_nonzero(b) == 1 and b.max() == 1.0 and op.free[np.unravel_index(np.argmax(b), op.n)]
        u, it, rel, ok = R.pcg(hier, f, np.zeros(op.n), 0.95, 1, precond)
        uld = R.first_iterate_ld(hier, f, precond)
        assert uld.dtype == np.longdouble and np.finfo(np.longdouble).eps < EPS
        spread = float(np.abs(u - uld).max() / np.abs(uld).max())
        print(f"{name} {precond} {fname}: relative residual after iteration 1: {rel:.3f}, float64 against long double: {spread:.2e}·max|u|")
        assert ok and it == 1
        assert rel <= 0.9
        assert spread <= 64 * EPS


_EDGE_LEVELS = {"24x33x10_cn": [(24, 33, 10), (12, 17, 5), (6, 9, 5), (3, 5, 5)], "6x6x6_cn_sparse": [(6, 6, 6), (3, 3, 3)], "5x5_face": [(5, 5)],
                "4x4_c": [(4, 4)], "5x5x5_laplace": [(5, 5, 5)], "4x5x4_cn": [(4, 5, 4)], "6x5_face": [(6, 5), (3, 5)],
                "4x40_face": [(4, 40), (4, 20), (4, 10), (4, 5)], "4x40_side": [(4, 40), (4, 20), (4, 10), (4, 5)]}


@pytest.mark.parametrize("name", R.edge_case_names())
def test_the_edge_cases_converge_and_the_v_cycle_needs_fewer_iterations(name):
    """the restatement on the cases of tests/test_gpu_elliptic_edges.py, rtol 1e-8: iterations mg / jacobi
      24x33x10_cn 23/227, 6x6x6_cn_sparse 13/49, 64x48_cn_devicefield 19/361 (float32 handle: the same),
      5x5_face 5/19, 4x4_c 5/15, 5x5x5_laplace 6/29, 4x5x4_cn 7/33, 6x5_face 7/22, 4x40_face 17/74, 4x40_side 8/41,
      300x230 25/1529, 45x41x37 18/339 (|u(rtol) − u(rtol/100)|∞ 1.9e-9 / 6.2e-10), 1000x530 28/–, 83x81x79 24/–,
      33x33_face_guess 14/197, 65x20_aniso_h_guess 23/235, 17c_face_guess 12/159, 17c_f32_guess 12/158,
      64x48_level 18/–, 64x48_level_neg 33/–, 33x33_f32_2d 13/189
    so mg < jacobi wherever both run.  A device handle needs at least 4 nodes per dimension (lsm_create), so 4x4 is the smallest
    grid and 4x40 the strip whose short axis never coarsens; axes of 3 nodes occur on the coarse levels.  The one-level shapes have one level, c per node is positive somewhere and zero somewhere in
    6x6x6_cn_sparse, and the two big shapes need a second grid-stride trip of 2048·256 threads."""
    s = R.edge_solved(name)
    cs, hier = s["case"], s["hier"]
    if name in _EDGE_LEVELS:
        assert [o.n for o in hier.ops] == _EDGE_LEVELS[name]
    for lev, op in enumerate(hier.ops[1:], 1):         # c and the fixed mask are injected: coarse J sits on fine 2J of a coarsened axis
        fine = hier.ops[lev - 1]
        sl = tuple(slice(None, None, 2) if a != b else slice(None) for a, b in zip(fine.n, op.n))
        assert np.array_equal(op.c, fine.c[sl]) and np.array_equal(op.fixed, fine.fixed[sl])
    for pc in ("mg", "jacobi"):
        if s[pc] is None:
            assert pc == "jacobi" and cs["solve"] == "mg"
            continue
        u, it, rel, ok = s[pc]
        print(f"{name} {pc}: {it} iterations, relres {rel:.3e}, levels {[o.n for o in hier.ops]}")
        assert ok and it < cs.get("max_iters", 2000)
    if s["jacobi"] is not None:
        assert s["mg"][1] < s["jacobi"][1]
    if name == "6x6x6_cn_sparse":
        assert 0.25 < float((cs["c"] == 0).mean()) < 0.75 and cs["fixed"] is None
    if cs.get("big"):
        assert hier.ops[0].free.size > 2048 * 256
    elif name in ("300x230", "45x41x37"):
        assert 256 * 256 < hier.ops[0].free.size <= 2048 * 256
    if cs.get("u0") is not None:
        assert np.count_nonzero(s["u0"][hier.ops[0].free]) == int(hier.ops[0].free.sum())


def test_the_budget_cases_need_at_least_eight_iterations():
    """test_an_exact_iteration_budget_converges_and_one_less_does_not solves with max_iters = it − 1 ≥ 1"""
    for name in ("24x33x10_patch", "64x48_blob"):
        for pc in ("mg", "jacobi"):
            assert R.solved(name)[pc][1] >= 8


# ---- the refusals that need no device
def _lsm():
    import lsm_amd
    return lsm_amd


def _fake_field(lsm, n, bc=None, slab=None, band=False):
    """a ROCMeshField without a device: enough for the checks that run before anything touches one"""
    grid = lsm.CartesianGrid((0.0,) * len(n), (1.0,) * len(n), n)
    mf = lsm.MeshField(np.zeros(n), grid, bc=bc or lsm.NeumannBC())
    backend = types.SimpleNamespace(slab=slab)
    if band:
        f = object.__new__(lsm.ROCNarrowBandMeshField)
        f.backend, f.mesh, f.bcs, f.buf = backend, grid, mf.bcs, None
        return f
    return lsm.ROCMeshField(backend, grid, mf.bcs, buf=object())


def test_argument_refusals_without_a_device():
    lsm = _lsm()
    ok = _fake_field(lsm, (9, 9))
    for kw in (dict(a_in=0.0), dict(a_in=-1.0), dict(a_out=float("nan")), dict(a_out=float("inf")), dict(a=-1.0), dict(a=np.full((8, 8), np.nan)),
               dict(c=-1.0, dirichlet=(lsm.face_mask(ok.mesh, 0, 0), 0.0)), dict(c=float("nan")), dict(c=np.full((9, 9), -1.0)),
               dict(c=0.0), dict(c=0.0, dirichlet=(np.zeros((9, 9), dtype=bool), 0.0)), dict(c=np.zeros((9, 9))),
               dict(c=1.0, precond="ilu"), dict(c=1.0, level=float("nan")), dict(c=1.0, dirichlet=(np.ones((9, 9), dtype=bool), 0.0)),
               dict(c=1.0, dirichlet=(np.zeros((8, 9), dtype=bool), 0.0)), dict(c=1.0, dirichlet=(lsm.face_mask(ok.mesh, 0, 0), float("nan"))),
               dict(c=1.0, a=np.ones((9, 9))), dict(c=np.ones((8, 9)))):
        with pytest.raises(ValueError):
            lsm.elliptic_solve(ok, 1.0, **kw)
    with pytest.raises(TypeError):
        lsm.elliptic_solve(lsm.MeshField(np.zeros((9, 9)), ok.mesh), 1.0, c=1.0)
    with pytest.raises(TypeError):
        lsm.elliptic_solve(ok, 1.0, c=1.0, dirichlet=(np.zeros((9, 9)), 0.0))
    with pytest.raises(ValueError, match="1 dimensional"):
        lsm.elliptic_solve(_fake_field(lsm, (9,)), 1.0, c=1.0)
    with pytest.raises(ValueError, match="NarrowBandMeshField"):
        lsm.elliptic_solve(_fake_field(lsm, (9, 9), band=True), 1.0, c=1.0)
    with pytest.raises(ValueError, match="slab"):
        lsm.elliptic_solve(_fake_field(lsm, (9, 9), slab=(0, 4)), 1.0, c=1.0)
    with pytest.raises(ValueError, match="PeriodicBC"):
        lsm.elliptic_solve(_fake_field(lsm, (9, 9), bc=lsm.PeriodicBC()), 1.0, c=1.0)
    with pytest.raises(ValueError, match="at least 3 nodes"):
        lsm.elliptic_solve(_fake_field(lsm, (9, 2)), 1.0, c=1.0)
    with pytest.raises(ValueError, match="alpha"):
        lsm.regularize_(ok, 0.0)
    assert lsm.face_mask(ok.mesh, 1, 1).sum() == 9 and lsm.face_mask(ok.mesh, 1, 1)[:, -1].all()
    with pytest.raises(ValueError):
        lsm.face_mask(ok.mesh, 2, 0)


def test_the_library_exports_the_elliptic_entry_points():
    lsm = _lsm()
    names = {"lsm_elliptic_create", "lsm_elliptic_apply", "lsm_elliptic_solve", "lsm_elliptic_energy", "lsm_elliptic_compliance",
             "lsm_elliptic_cells", "lsm_elliptic_destroy"}
    assert names <= set(lsm._lib.EXPORTS)
    lib = lsm._lib.lib()
    for name in names:
        getattr(lib, name)
