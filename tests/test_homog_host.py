"""homogenize's restatement (tests/_homog_ref.py) against closed forms and against itself, on the CPU: what makes it a yardstick for
tests/test_gpu_homog.py.  DESIGN.md §7.23 quotes the iteration table printed by the last test."""
import numpy as np
import pytest

import _homog_ref as R


def _tensor(E, h, nu=0.3, plane="stress", how="direct"):
    hier = R.Hierarchy(np.asfortranarray(E), h, nu, plane)
    chi, _ = R.correctors(hier, how)
    return hier, chi, hier.ops[0].tensor(chi)


@pytest.mark.parametrize("m,plane", [((6, 5), "stress"), ((6, 5), "strain"), ((4, 3, 5), "stress")])
def test_uniform_moduli_give_E_times_C0(m, plane):
    h = tuple(1.0 / x for x in m)
    hier, chi, C = _tensor(np.full(m, 2.5), h, 0.3, plane)
    op = hier.ops[0]
    for k in range(R.nstrains(len(m))):
        assert np.abs(op.load(k)).max() <= 64 * 2.0 ** -53 * 2.5 * np.abs(op.g[k]).max()
    want = 2.5 * R.c0_tensor(0.3, len(m), plane)
    assert np.abs(C - want).max() <= 64 * 2.0 ** -53 * np.abs(want).max()


@pytest.mark.parametrize("m,axis,layers", [((16, 8), 0, 4), ((16, 8), 1, 3), ((8, 6, 4), 0, 2), ((4, 6, 8), 2, 5)])
def test_the_laminate_has_its_closed_form(m, axis, layers):
    h = tuple(1.0 / max(m) for _ in m)
    E = R.laminate_cells(m, 1.0, 0.1, layers, axis)
    _, _, C = _tensor(E, h)
    want = R.laminate_tensor(1.0, 0.1, layers / m[axis], 0.3, len(m), "stress", axis)
    print(f"laminate {m} axis {axis}: max|C − closed form| = {np.abs(C - want).max():.2e}")
    assert np.abs(C - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("name", ["9x9", "13x9", "9x5x7", "12x10_given_E"])
def test_the_tensor_is_symmetric_and_between_the_reuss_and_voigt_bounds(name):
    s = R.solved(name)
    op = s["hier"].ops[0]
    cs = s["case"]
    C = op.tensor(s["direct"])
    assert np.array_equal(C, C.T)
    C0 = R.c0_tensor(cs["nu"], op.N, cs["plane"])
    voigt = op.E.mean() * C0
    reuss = C0 / np.mean(1.0 / op.E)
    tol = 1e-12 * np.abs(voigt).max()
    assert np.linalg.eigvalsh(voigt - C).min() >= -tol
    assert np.linalg.eigvalsh(C - reuss).min() >= -tol


def test_a_cell_symmetric_under_the_swap_of_axes_gives_a_square_symmetric_tensor():
    rng = np.random.default_rng(3)
    a = 0.2 + rng.random((8, 8))
    _, _, C = _tensor(0.5 * (a + a.T), (0.125, 0.125))          # x↔y swaps ε00 and ε11 and keeps γ01
    scale = np.abs(C).max()
    assert abs(C[0, 0] - C[1, 1]) <= 1e-12 * scale and abs(C[0, 2] - C[1, 2]) <= 1e-12 * scale
    E = 0.25 * (a + a[::-1] + a[:, ::-1] + a[::-1, ::-1])        # with the two mirror symmetries as well: no normal–shear coupling
    _, _, C = _tensor(0.5 * (E + E.T), (0.125, 0.125))
    assert abs(C[0, 0] - C[1, 1]) <= 1e-12 * scale
    assert abs(C[0, 2]) <= 1e-12 * scale and abs(C[1, 2]) <= 1e-12 * scale


def test_sensitivity_against_finite_differences_in_single_cell_moduli():
    """d(W:C^H)/dE_C = (Σ_pq W_pq t^{pq}_C)/(E_C·ncells): the cell sums of sensitivity() are the derivative, by the direct solve"""
    rng = np.random.default_rng(5)
    m, h = (8, 6), (0.125, 0.125)
    E = np.asfortranarray(0.3 + rng.random(m))
    W = rng.standard_normal((3, 3))
    W = W + W.T
    hier, chi, C = _tensor(E, h)
    op = hier.ops[0]
    cell = op.sensitivity_cells(chi, W)
    nc = E.size
    for c in [(0, 0), (3, 2), (7, 5), (4, 0)]:
        d = 1e-5 * E[c]
        vals = []
        for sgn in (1.0, -1.0):
            Ep = E.copy()
            Ep[c] += sgn * d
            vals.append(float(np.sum(W * _tensor(Ep, h)[2])))
        fd = (vals[0] - vals[1]) / (2 * d)
        an = cell[c] / (E[c] * nc)
        assert abs(fd - an) <= 1e-7 * max(abs(an), np.abs(cell).max() / nc), (c, fd, an)
    # the node field is the mean of the cell values around a node, and wraps
    s = op.sensitivity(chi, W)
    assert s.shape == (9, 7) and np.array_equal(s[-1], s[0]) and np.array_equal(s[:, -1], s[:, 0])
    assert abs(s[:-1, :-1].sum() - cell.sum()) <= 1e-12 * np.abs(cell).sum()


def test_the_vcycle_is_symmetric_positive_definite():
    rng = np.random.default_rng(9)
    hier = R.Hierarchy(np.asfortranarray(0.01 + rng.random((8, 12))), (1 / 8, 1 / 8))
    assert hier.levels == 3
    Mv = hier.vcycle_matrix()
    assert np.abs(Mv - Mv.T).max() <= 1e-12 * np.abs(Mv).max()
    assert np.linalg.eigvalsh(0.5 * (Mv + Mv.T)).min() > 0


@pytest.mark.parametrize("name", sorted(k for k, v in R.cases().items() if v["both"]))
def test_pcg_reaches_the_direct_solve_and_mg_needs_fewer_iterations(name):
    s = R.solved(name)
    op = s["hier"].ops[0]
    scale = np.abs(s["direct"]).max()
    for pc in ("mg", "jacobi"):
        chi, its = s[pc]
        print(f"{name} {pc}: iterations {its}, |χ − direct| {np.abs(chi - s['direct']).max() / scale:.2e}·max|χ|, levels {s['hier'].levels}")
        assert np.abs(chi - s["direct"]).max() <= 1e-5 * scale
        Cp, Cd = op.tensor(chi), op.tensor(s["direct"])
        assert np.abs(Cp - Cd).max() <= 1e-10 * np.abs(Cd).max()
    if s["hier"].levels > 1:
        assert max(s["mg"][1]) < min(s["jacobi"][1])


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
    for kw in (dict(E_in=0.0), dict(E_out=float("nan")), dict(E=-1.0), dict(E=np.full((8, 8), np.nan)), dict(E=np.ones((9, 9))), dict(nu=0.5), dict(nu=-1.0),
               dict(plane="shell"), dict(precond="ilu"), dict(level=float("inf"))):
        with pytest.raises(ValueError):
            lsm.homogenize(ok, **kw)
    with pytest.raises(TypeError):
        lsm.homogenize(np.zeros((9, 9)))
    with pytest.raises(ValueError, match="1 dimensional"):
        lsm.homogenize(fake((9,)))
    with pytest.raises(ValueError, match="2 cells"):
        lsm.homogenize(fake((2, 9)))
    with pytest.raises(ValueError, match="NarrowBandMeshField"):
        lsm.homogenize(fake((9, 9), band=True))
    with pytest.raises(ValueError, match="slab"):
        lsm.homogenize(fake((9, 9), slab=(0, 4)))


def test_the_iteration_table():
    """the prototype (a soft disc / ball at contrast 1e-3): PCG iterations per corrector at rtol 1e-8, for DESIGN.md §7.23"""
    for n, hc in R.TABLE:
        hier = R.prototype(n, hc)
        _, mg = R.correctors(hier, "pcg", 1e-8, "mg")
        line = f"{'x'.join(map(str, n))}: levels {hier.levels}, dampings {[round(float(hier.omega(l)), 3) for l in range(hier.levels)]}, mg {mg}"
        if len(n) == 2:
            _, jac = R.correctors(hier, "pcg", 1e-8, "jacobi")
            line += f", jacobi {jac}"
            assert max(mg) < min(jac)
        print(line)
        assert max(mg) <= 40
