"""homogenize_conductivity's restatement (tests/_hcond_ref.py) against closed forms and against itself, on the CPU: what makes it a
yardstick for tests/test_gpu_hcond.py.  DESIGN.md §7.24 quotes the laminate figures and the iteration table printed here."""
import numpy as np
import pytest

import _hcond_ref as R

FLOOR = 64 * 2.0 ** -53


def _tensor(a, h, how="direct"):
    hier = R.Hierarchy(np.asfortranarray(a), h)
    chi, its = R.correctors(hier, how)
    return hier, chi, hier.ops[0].tensor(chi), its


@pytest.mark.parametrize("m", [(6, 5), (4, 3, 5)])
def test_a_uniform_cell_gives_a_times_the_identity_with_zero_loads_and_no_iteration(m):
    h = tuple(1.0 / x for x in m)
    hier, chi, K, its = _tensor(np.full(m, 2.5), h, "pcg")
    op = hier.ops[0]
    for k in range(len(m)):
        assert not op.load(k).any()
    assert its == [0] * len(m) and not chi.any()
    assert np.abs(K - 2.5 * np.eye(len(m))).max() <= FLOOR * 2.5


@pytest.mark.parametrize("m,axis,layers", [((16, 8), 0, 4), ((16, 8), 1, 3), ((8, 6, 4), 0, 2), ((8, 6, 4), 1, 5), ((4, 6, 8), 2, 5)])
def test_the_laminate_has_the_harmonic_mean_across_and_the_arithmetic_mean_along_its_layers(m, axis, layers):
    """observed max|K − closed form|/max|K|: 2.8e-33 and 5.2e-34 (16×8, axes 0 and 1), 8.5e-17, 1.3e-16 and 2.3e-33 in 3-D; the bar is
    64·2⁻⁵³ = 7.1e-15"""
    h = tuple(1.0 / max(m) for _ in m)
    _, _, K, _ = _tensor(R.laminate_cells(m, 1.0, 0.1, layers, axis), h)
    want = R.laminate_tensor(1.0, 0.1, layers / m[axis], len(m), axis)
    print(f"laminate {m} axis {axis}: max|K − closed form| = {np.abs(K - want).max() / np.abs(want).max():.2e}·max|K|")
    assert np.abs(K - want).max() <= FLOOR * np.abs(want).max()


@pytest.mark.parametrize("name", ["13x9", "12x10_given_a", "33x33_soft", "9x5x7"])
def test_the_tensor_is_symmetric_and_between_the_harmonic_and_arithmetic_means(name):
    s = R.solved(name)
    op = s["hier"].ops[0]
    K = op.tensor(s["direct"])
    assert np.array_equal(K, K.T)
    I = np.eye(op.N)
    upper, lower = op.a.mean() * I, I / np.mean(1.0 / op.a)
    tol = 1e-12 * op.a.mean()
    assert np.linalg.eigvalsh(upper - K).min() >= -tol
    assert np.linalg.eigvalsh(K - lower).min() >= -tol
    assert np.linalg.eigvalsh(K).min() > 0


@pytest.mark.parametrize("m,h", [((8, 6), (0.125, 0.2)), ((4, 6, 5), (0.25, 0.2, 0.125))])
def test_swapping_two_axes_swaps_the_tensor(m, h):
    a = 0.2 + np.random.default_rng(3).random(m)
    _, _, K, _ = _tensor(a, h)
    perm = [1, 0] + list(range(2, len(m)))
    _, _, Ks, _ = _tensor(np.swapaxes(a, 0, 1), tuple(h[p] for p in perm))
    assert np.abs(Ks - K[np.ix_(perm, perm)]).max() <= 1e-13 * np.abs(K).max()
    assert abs(K[0, 1]) > 1e-6 * np.abs(K).max()         # a random cell couples the axes: the off-diagonal entries are compared, not zero


def test_sensitivity_against_central_differences_in_single_cell_coefficients():
    """d(W:K^H)/da_C = (Σ_{p≤q} c·W_pq·t^{pq}_C)/(a_C·ncells): the cell sums of sensitivity() are the derivative, by the direct solve"""
    rng = np.random.default_rng(5)
    m, h = (7, 6), (0.125, 0.15)
    a = np.asfortranarray(0.3 + rng.random(m))
    W = rng.standard_normal((2, 2))
    W = W + W.T
    hier, chi, K, _ = _tensor(a, h)
    op = hier.ops[0]
    cell = op.sensitivity_cells(chi, W)
    nc = a.size
    for c in [(0, 0), (3, 2), (6, 5), (4, 0)]:
        d = 1e-5 * a[c]
        vals = []
        for sgn in (1.0, -1.0):
            ap = a.copy()
            ap[c] += sgn * d
            vals.append(float(np.sum(W * _tensor(ap, h)[2])))
        fd = (vals[0] - vals[1]) / (2 * d)
        an = cell[c] / (a[c] * nc)
        assert abs(fd - an) <= 1e-7 * max(abs(an), np.abs(cell).max() / nc), (c, fd, an)
    # the node field is the mean of the cell values around a node, and wraps
    s = op.sensitivity(chi, W)
    assert s.shape == (8, 7) and np.array_equal(s[-1], s[0]) and np.array_equal(s[:, -1], s[:, 0])
    assert abs(s[:-1, :-1].sum() - cell.sum()) <= 1e-12 * np.abs(cell).sum()


def test_the_assembled_matrix_is_the_stated_operator_and_singular_only_on_the_constants():
    rng = np.random.default_rng(7)
    op = R.Operator(0.1 + rng.random((6, 4, 5)), (0.2, 0.25, 0.1))
    x = rng.standard_normal(op.m)
    y = (op.matrix() @ x.reshape(-1, order="F")).reshape(op.m, order="F")
    assert np.abs(y - op.apply(x)).max() <= 1e-13 * np.abs(y).max()
    assert np.abs(op.apply(np.ones(op.m))).max() <= 1e-12 * op.D.max()
    assert np.abs(op.matrix().diagonal().reshape(op.m, order="F") - op.D).max() <= 1e-13 * op.D.max()
    for k in range(3):
        assert abs(op.load(k).sum()) <= 1e-12 * np.abs(op.load(k)).sum()       # the loads are orthogonal to the constants


def test_the_vcycle_is_symmetric_positive_definite():
    rng = np.random.default_rng(9)
    hier = R.Hierarchy(np.asfortranarray(0.01 + rng.random((8, 12))), (1 / 8, 1 / 8))
    assert hier.levels == 3
    Mv = hier.vcycle_matrix()
    assert np.abs(Mv - Mv.T).max() <= 1e-12 * np.abs(Mv).max()
    assert np.linalg.eigvalsh(0.5 * (Mv + Mv.T)).min() > 0


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_pcg_reaches_the_direct_solve_and_mg_needs_fewer_iterations(name):
    s = R.solved(name)
    op = s["hier"].ops[0]
    scale = np.abs(s["direct"]).max()
    for pc in ("mg", "jacobi"):
        chi, its = s[pc]
        print(f"{name} {pc}: iterations {its}, |χ − direct| {np.abs(chi - s['direct']).max() / scale:.2e}·max|χ|, levels {s['hier'].levels}")
        assert np.abs(chi - s["direct"]).max() <= 1e-5 * scale
        Kp, Kd = op.tensor(chi), op.tensor(s["direct"])
        assert np.abs(Kp - Kd).max() <= 1e-10 * np.abs(Kd).max()
    if s["hier"].levels > 1:
        assert max(s["mg"][1]) < min(s["jacobi"][1])


def test_the_first_iterate_runs_keep_the_load_and_an_impulse_at_the_wrap():
    """what tests/test_gpu_hcond.py's V-cycle group runs: per shape the right-hand sides whose first iteration ends a solve at rtol 0.97"""
    for name in R.FIRST_ITERATE:
        runs, left_out = R.first_iterate_runs(R.build_case(R.cases()[name]))
        names = [r[0] for r in runs]
        print(f"{name}: runs {[(k, round(float(r), 3)) for k, _, _, r in runs]}, left out {[(k, round(float(r), 3)) for k, _, _, r in left_out]}")
        assert names[0] == "load0" and len(runs) >= 3 and any(k.startswith("last") for k in names)


def test_argument_refusals_without_a_device():
    import types

    import lsm_amd as lsm

    def fake(n, slab=None, band=False):
        grid = lsm.CartesianGrid((0.0,) * len(n), (1.0,) * len(n), n)
        mf = lsm.MeshField(np.zeros(n), grid, bc=lsm.NeumannBC())
        backend = types.SimpleNamespace(slab=slab)
        if band:
            f = object.__new__(lsm.ROCNarrowBandMeshField)
            f.backend, f.mesh, f.bcs, f.buf = backend, grid, mf.bcs, None
            return f
        return lsm.ROCMeshField(backend, grid, mf.bcs, buf=object())

    ok = fake((9, 9))
    for kw in (dict(a_in=0.0), dict(a_out=float("nan")), dict(a=-1.0), dict(a=np.full((8, 8), np.nan)), dict(a=np.ones((9, 9))), dict(precond="ilu"),
               dict(level=float("inf"))):
        with pytest.raises(ValueError):
            lsm.homogenize_conductivity(ok, **kw)
    with pytest.raises(TypeError):
        lsm.homogenize_conductivity(np.zeros((9, 9)))
    with pytest.raises(ValueError, match="1 dimensional"):
        lsm.homogenize_conductivity(fake((9,)))
    with pytest.raises(ValueError, match="2 cells"):
        lsm.homogenize_conductivity(fake((2, 9)))
    with pytest.raises(ValueError, match="NarrowBandMeshField"):
        lsm.homogenize_conductivity(fake((9, 9), band=True))
    with pytest.raises(ValueError, match="slab"):
        lsm.homogenize_conductivity(fake((9, 9), slab=(0, 4)))


def test_the_iteration_table():
    """the prototype (a soft disc / ball at contrast 1e-3): PCG iterations per corrector at rtol 1e-8, for DESIGN.md §7.24"""
    for n, hc in R.TABLE:
        hier = R.prototype(n, hc)
        _, mg = R.correctors(hier, "pcg", 1e-8, "mg")
        _, jac = R.correctors(hier, "pcg", 1e-8, "jacobi")
        print(f"{'x'.join(map(str, n))}: levels {hier.levels}, mg {mg}, jacobi {jac}")
        if hier.levels > 1:
            assert max(mg) < min(jac)
        assert max(mg) <= 40
