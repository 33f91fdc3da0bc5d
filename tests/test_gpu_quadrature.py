"""quadrature on the device (csrc/lsm_quad.hip, lsm_quad_* through the Python API) against the restatement tests/_quad_ref.py
node for node, and the reference's own tests (test/test-quadrature.jl).  The launch shapes and edges these grids do not reach
(several chunks, a second scan round, two cells per workgroup, the depth limit in 3-D, q = 20, bands in 3-D) are in
tests/test_gpu_quadrature_edges.py."""
import math
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _lsm():
    import lsm_amd
    return lsm_amd


def _grid_vals(n, f, lc=None, hc=None):
    lc = lc or (-1.0,) * len(n)
    hc = hc or (1.0,) * len(n)
    ax = [np.linspace(lc[d], hc[d], n[d]) for d in range(len(n))]
    X = np.meshgrid(*ax, indexing="ij")
    return np.asfortranarray(f(X)), lc, hc


def _device(lsm, vals, lc, hc, bc, dtype=None):
    grid = lsm.CartesianGrid(lc, hc, vals.shape)
    mf = lsm.MeshField(vals, grid, dtype=dtype)
    return lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=mf, bc=bc).current_state()


def _ref(vals, lc, hc, P, k):
    from _reinit_ref import ReinitRef
    from test_reinitialize import _dense_getter
    return ReinitRef(_dense_getter(vals, P), vals.shape, lc, hc, order=k, cells=[])


def _lin(cells, n):
    """ascending linear index (x fastest) of (m, N) cell indices on a grid of n nodes"""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, len(n))
    lin, s = np.zeros(len(cells), dtype=np.int64), 1
    for d in range(len(n)):
        lin += cells[:, d] * s
        s *= n[d] - 1
    return lin


def _compare(q, ref, qo, surface, cells=None, restated=None):
    """cells: compare only those cells' slices of the device output (what the restatement gives for them: nodes, a full cell,
    or nothing); restated: Q.quadrature's result if the caller has it already"""
    import _quad_ref as Q
    cut, full, nfb = restated if restated is not None else Q.quadrature(ref, qo, surface, cells=cells)
    if cells is None:
        cells = sorted(cut, key=lambda I: tuple(I[::-1]))
        assert [tuple(int(v) for v in I) for I in q.cells] == cells
        assert [tuple(int(v) for v in I) for I in q.full_cells] == full
        assert q.nfallback == nfb
        counts = [len(cut[I][1]) for I in cells]
        assert list(np.diff(q.offsets)) == counts
        dX, dW = q.coords, q.weights
    else:
        asked = sorted({tuple(int(v) for v in I) for I in cells}, key=lambda I: tuple(I[::-1]))
        dcut, dfull = _lin(q.cells, ref.n), _lin(q.full_cells, ref.n)
        where = np.flatnonzero(np.isin(dcut, _lin(asked, ref.n)))
        assert [asked[i] for i in np.flatnonzero(np.isin(_lin(asked, ref.n), dfull))] == full
        cells = [I for I in asked if I in cut]
        assert [tuple(int(v) for v in q.cells[i]) for i in where] == cells
        assert [int(q.offsets[i + 1] - q.offsets[i]) for i in where] == [len(cut[I][1]) for I in cells]
        sl = [np.arange(q.offsets[i], q.offsets[i + 1]) for i in where]
        dX, dW = (q.coords[np.concatenate(sl)], q.weights[np.concatenate(sl)]) if sl else (q.coords[:0], q.weights[:0])
    if cells:
        X = np.concatenate([cut[I][0] for I in cells])
        W = np.concatenate([cut[I][1] for I in cells])
        print(f"device vs restatement over {len(cells)} cells, {len(W)} nodes: coords {np.abs(dX - X).max():.3e}, "
              f"weights {np.abs(dW - W).max():.3e} (max |w| {np.abs(W).max():.3e})")
        assert np.abs(dX - X).max() <= 1e-12
        assert np.abs(dW - W).max() <= 1e-12 * max(1.0, np.abs(W).max())
    rx, rw = Q.full_rule(qo, ref.N)
    assert np.abs(q.rule.coords - rx).max() <= 1e-12 and np.abs(q.rule.weights - rw).max() <= 1e-12
    return cut, full


# ----------------------------------------------------------------------------- node for node against the restatement

_SHAPES = {
    1: lambda X: np.abs(X[0] - 0.123) - 0.41,
    2: lambda X: np.hypot((X[0] - 0.11) / 0.83, X[1] + 0.07) - 0.53,
    3: lambda X: np.sqrt(((X[0] - 0.05) / 0.9) ** 2 + (X[1] + 0.08) ** 2 + ((X[2] - 0.03) / 1.1) ** 2) - 0.52,
}
_N = {1: (23,), 2: (17, 15), 3: (9, 10, 8)}


@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("qo", [1, 2, 4, 8])
@pytest.mark.parametrize("surface", [False, True])
def test_device_matches_restatement(N, k, qo, surface):
    lsm = _lsm()
    vals, lc, hc = _grid_vals(_N[N], _SHAPES[N])
    phi = _device(lsm, vals, lc, hc, lsm.ExtrapolationBC(k))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        q = lsm.quadrature(phi, interpolation_order=k, quadrature_order=qo, surface=surface)
    _compare(q, _ref(vals, lc, hc, k, k), qo, surface)


@pytest.mark.parametrize("bc,P", [("neumann", 0), ("linear", 1)])
@pytest.mark.parametrize("surface", [False, True])
def test_interface_across_the_boundary(bc, P, surface):
    """the interface leaves the domain: the stencils of boundary cells read the boundary conditions' ghost values"""
    lsm = _lsm()
    vals, lc, hc = _grid_vals((19, 17), lambda X: np.hypot(X[0] - 0.71, X[1] + 0.43) - 0.61)
    phi = _device(lsm, vals, lc, hc, lsm.NeumannBC() if bc == "neumann" else lsm.LinearExtrapolationBC())
    q = lsm.quadrature(phi, interpolation_order=3, quadrature_order=4, surface=surface)
    _compare(q, _ref(vals, lc, hc, P, 3), 4, surface)


def _kinked(X):
    """setdiff of two disks: a crescent whose horns are sharp corners"""
    return np.maximum(np.hypot(X[0] - 0.13, X[1] - 0.07) - 0.55, -(np.hypot(X[0], X[1] - 0.07) - 0.45))


@pytest.mark.parametrize("surface", [False, True])
def test_kinked_set_splits_boxes(surface):
    """the cells at the horns are split, one box reaches the depth limit at 32²; the fallback counts agree"""
    lsm = _lsm()
    vals, lc, hc = _grid_vals((32, 32), _kinked)
    phi = _device(lsm, vals, lc, hc, lsm.ExtrapolationBC(3))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        q = lsm.quadrature(phi, interpolation_order=3, quadrature_order=4, surface=surface)
    assert q.nfallback > 0
    _compare(q, _ref(vals, lc, hc, 3, 3), 4, surface)
    with pytest.warns(UserWarning, match="subdivision limit"):
        lsm.quadrature(phi, interpolation_order=3, quadrature_order=4, surface=surface)


def test_float32_storage():
    lsm = _lsm()
    vals, lc, hc = _grid_vals((21, 19), _SHAPES[2])
    v32 = np.asfortranarray(vals.astype(np.float32))
    phi = _device(lsm, v32, lc, hc, lsm.ExtrapolationBC(3), dtype=np.float32)
    for surface in (False, True):
        q = lsm.quadrature(phi, interpolation_order=3, quadrature_order=4, surface=surface)
        _compare(q, _ref(np.asfortranarray(v32.astype(np.float64)), lc, hc, 3, 3), 4, surface)


# ----------------------------------------------------------------------------- the reference's tests (test/test-quadrature.jl)

def _total(q, f=lambda x: np.ones(len(x))):
    return _lsm().integrate(f, q)


def test_reference_2d_circle_and_convenience_form():
    lsm = _lsm()
    R = 0.5
    vals, lc, hc = _grid_vals((21, 21), lambda X: X[0] ** 2 + X[1] ** 2 - R ** 2)
    phi = _device(lsm, vals, lc, hc, lsm.ExtrapolationBC(3))
    itp = lsm.InterpolatedField(phi, 3)
    assert abs(_total(lsm.quadrature(itp, quadrature_order=4)) - math.pi * R ** 2) < 1e-4
    assert abs(_total(lsm.quadrature(itp, quadrature_order=4, surface=True)) - 2 * math.pi * R) < 1e-3
    a = _total(lsm.quadrature(phi, interpolation_order=3, quadrature_order=4))
    b = _total(lsm.quadrature(itp, quadrature_order=4))
    assert abs(a - b) <= 1e-12 * abs(b)
    with pytest.raises(TypeError):
        lsm.quadrature(itp, interpolation_order=3, quadrature_order=4)


def test_reference_ellipse_sphere_ellipsoid():
    lsm = _lsm()
    a, b = 0.6, 0.3
    vals, lc, hc = _grid_vals((41, 41), lambda X: (X[0] / a) ** 2 + (X[1] / b) ** 2 - 1.0)
    phi = _device(lsm, vals, lc, hc, lsm.ExtrapolationBC(3))
    h = ((a - b) / (a + b)) ** 2
    peri = math.pi * (a + b) * (1 + 3 * h / (10 + math.sqrt(4 - 3 * h)))
    assert _total(lsm.quadrature(phi, interpolation_order=3, quadrature_order=4)) == pytest.approx(math.pi * a * b, rel=1e-3)
    assert _total(lsm.quadrature(phi, interpolation_order=3, quadrature_order=4, surface=True)) == pytest.approx(peri, rel=1e-3)
    R = 0.5
    vals, lc, hc = _grid_vals((11, 11, 11), lambda X: X[0] ** 2 + X[1] ** 2 + X[2] ** 2 - R ** 2)
    phi = _device(lsm, vals, lc, hc, lsm.ExtrapolationBC(3))
    assert abs(_total(lsm.quadrature(phi, interpolation_order=3, quadrature_order=2)) - 4 * math.pi / 3 * R ** 3) < 1e-3
    assert abs(_total(lsm.quadrature(phi, interpolation_order=3, quadrature_order=2, surface=True)) - 4 * math.pi * R ** 2) < 1e-2
    a, b, c = 0.61, 0.37, 0.29
    vals, lc, hc = _grid_vals((21, 21, 21), lambda X: (X[0] / a) ** 2 + (X[1] / b) ** 2 + (X[2] / c) ** 2 - 1.0)
    phi = _device(lsm, vals, lc, hc, lsm.ExtrapolationBC(3))
    q = lsm.quadrature(phi, interpolation_order=3, quadrature_order=3)
    assert _total(q) == pytest.approx(4 / 3 * math.pi * a * b * c, rel=1e-3)
    assert q.total() == pytest.approx(_total(q), rel=1e-12)


@pytest.mark.parametrize("k", [3, 5])
def test_reference_h_convergence(k):
    lsm = _lsm()
    Ns = [10, 20, 40, 80]
    errs = {False: [], True: []}
    for n in Ns:
        vals, lc, hc = _grid_vals((n, n), lambda X: np.hypot(X[0], X[1]) - 0.5)
        phi = _device(lsm, vals, lc, hc, lsm.ExtrapolationBC(k))
        for s, exact in ((False, math.pi * 0.25), (True, math.pi)):
            errs[s].append(abs(lsm.quadrature(phi, interpolation_order=k, quadrature_order=k + 1, surface=s).total() - exact))
    for s in (False, True):
        e = errs[s]
        orders = [math.log(e[i] / e[i + 1]) / math.log(Ns[i + 1] / Ns[i]) for i in range(len(Ns) - 1)]
        assert all(o >= k + 0.5 for o in orders), (s, orders)


def test_reference_narrow_band():
    lsm = _lsm()
    R = 0.5
    vals, lc, hc = _grid_vals((41, 41), lambda X: X[0] ** 2 + X[1] ** 2 - R ** 2)
    grid = lsm.CartesianGrid(lc, hc, vals.shape)
    full = _device(lsm, vals, lc, hc, lsm.ExtrapolationBC(3))
    nb = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.NarrowBandMeshField(lsm.MeshField(vals, grid), nlayers=3),
                              bc=lsm.ExtrapolationBC(3)).current_state()
    with pytest.raises(ValueError, match="volume integrals"):
        lsm.quadrature(nb, interpolation_order=3, quadrature_order=4, surface=False)
    qf = lsm.quadrature(full, interpolation_order=3, quadrature_order=4, surface=True)
    qb = lsm.quadrature(nb, interpolation_order=3, quadrature_order=4, surface=True)
    assert abs(qf.total() - qb.total()) <= 1e-10 * qf.total()


# ----------------------------------------------------------------------------- size, determinism, lifetime, errors

def test_sphere_256_area_and_volume():
    lsm = _lsm()
    R = 0.5
    n = (256, 256, 256)
    vals, lc, hc = _grid_vals(n, lambda X: np.sqrt(X[0] ** 2 + X[1] ** 2 + X[2] ** 2) - R)
    phi = _device(lsm, vals, lc, hc, lsm.ExtrapolationBC(3))
    qv = lsm.quadrature(phi, interpolation_order=3, quadrature_order=4)
    assert qv.total() == pytest.approx(4 / 3 * math.pi * R ** 3, rel=1e-6)
    assert qv.nfull > 1_000_000
    assert _total(qv) == pytest.approx(qv.total(), rel=1e-12)       # integrate() over the full cells in chunks
    qs = lsm.quadrature(phi, interpolation_order=3, quadrature_order=4, surface=True)
    assert qs.total() == pytest.approx(4 * math.pi * R ** 2, rel=1e-6)


def test_bit_identical_and_rebuild_on_the_same_handle():
    lsm = _lsm()
    vals, lc, hc = _grid_vals((9, 10, 8), _SHAPES[3])
    phi = _device(lsm, vals, lc, hc, lsm.ExtrapolationBC(3))
    a = lsm.quadrature(phi, interpolation_order=3, quadrature_order=4)
    arrays = (a.cells.copy(), a.offsets.copy(), a.coords.copy(), a.weights.copy(), a.full_cells.copy())
    del a
    b = lsm.quadrature(phi, interpolation_order=3, quadrature_order=4)
    for x, y in zip(arrays, (b.cells, b.offsets, b.coords, b.weights, b.full_cells)):
        assert np.array_equal(x, y)
    # the mapping: cut and full cells, Quadrature objects
    assert len(b) == len(b.keys()) == b.ncut + b.nfull
    I = tuple(int(v) for v in b.cells[0])
    assert b[I].coords.shape[1] == 3 and len(b[I].weights) == b.offsets[1] - b.offsets[0]
    J = tuple(int(v) for v in b.full_cells[0])
    assert b[J].weights.sum() == pytest.approx(np.prod(phi.mesh.meshsize()), rel=1e-14)
    assert sum(lsm.integrate(lambda x: np.ones(len(x)), Q) for _, Q in b.items()) == pytest.approx(b.total(), rel=1e-12)


def test_errors():
    lsm = _lsm()
    vals, lc, hc = _grid_vals((9, 9), _SHAPES[2])
    phi = _device(lsm, vals, lc, hc, lsm.ExtrapolationBC(3))
    for kw in (dict(interpolation_order=0, quadrature_order=4), dict(interpolation_order=6, quadrature_order=4),
               dict(interpolation_order=3, quadrature_order=0), dict(interpolation_order=3, quadrature_order=21)):
        with pytest.raises(ValueError):
            lsm.quadrature(phi, **kw)
    with pytest.raises(TypeError):
        lsm.quadrature(phi, quadrature_order=4)
