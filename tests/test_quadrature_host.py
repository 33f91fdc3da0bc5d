"""quadrature (src/LevelSetMethods.jl:103-126, ext/ImplicitIntegrationExt.jl): the restatement tests/_quad_ref.py against the
reference's own tests (test/test-quadrature.jl, each with its thresholds), the docs page's disk, exactness, and the Python
API's argument errors.  No GPU."""
import itertools
import math

import numpy as np
import pytest

import _quad_ref as Q
from _reinit_ref import ReinitRef


def _getter(vals, P):
    from test_reinitialize import _dense_getter
    return _dense_getter(vals, P)


def _ref(n, f, k=3, P=None, lc=None, hc=None):
    lc = lc or (-1.0,) * len(n)
    hc = hc or (1.0,) * len(n)
    ax = [np.linspace(lc[d], hc[d], n[d]) for d in range(len(n))]
    vals = np.asfortranarray(f(np.meshgrid(*ax, indexing="ij")))
    return ReinitRef(_getter(vals, k if P is None else P), n, lc, hc, order=k, cells=[]), vals


def test_2d_circle_and_convenience_form():
    R = 0.5
    ref, _ = _ref((21, 21), lambda X: X[0] ** 2 + X[1] ** 2 - R ** 2)
    assert abs(Q.total(ref, 4) - math.pi * R ** 2) < 1e-4
    assert abs(Q.total(ref, 4, surface=True) - 2 * math.pi * R) < 1e-3
    # the convenience form wraps the same interpolant: the same sum to rtol 1e-12
    ref2, _ = _ref((21, 21), lambda X: X[0] ** 2 + X[1] ** 2 - R ** 2)
    assert Q.total(ref2, 4) == pytest.approx(Q.total(ref, 4), rel=1e-12)


def test_2d_ellipse():
    a, b = 0.6, 0.3
    ref, _ = _ref((41, 41), lambda X: (X[0] / a) ** 2 + (X[1] / b) ** 2 - 1.0)
    h = ((a - b) / (a + b)) ** 2
    peri = math.pi * (a + b) * (1 + 3 * h / (10 + math.sqrt(4 - 3 * h)))
    assert Q.total(ref, 4) == pytest.approx(math.pi * a * b, rel=1e-3)
    assert Q.total(ref, 4, surface=True) == pytest.approx(peri, rel=1e-3)


def test_3d_sphere():
    R = 0.5
    ref, _ = _ref((11, 11, 11), lambda X: X[0] ** 2 + X[1] ** 2 + X[2] ** 2 - R ** 2)
    assert abs(Q.total(ref, 2) - 4 * math.pi / 3 * R ** 3) < 1e-3
    assert abs(Q.total(ref, 2, surface=True) - 4 * math.pi * R ** 2) < 1e-2


def test_3d_ellipsoid():
    a, b, c = 0.61, 0.37, 0.29
    ref, _ = _ref((21, 21, 21), lambda X: (X[0] / a) ** 2 + (X[1] / b) ** 2 + (X[2] / c) ** 2 - 1.0)
    assert Q.total(ref, 3) == pytest.approx(4 / 3 * math.pi * a * b * c, rel=1e-3)


@pytest.mark.parametrize("k", [3, 5])
def test_h_convergence(k):
    Ns = [10, 20, 40, 80]
    for surface, exact in ((False, math.pi * 0.25), (True, math.pi)):
        errs = []
        for n in Ns:
            ref, _ = _ref((n, n), lambda X: np.hypot(X[0], X[1]) - 0.5, k=k)
            errs.append(abs(Q.total(ref, k + 1, surface) - exact))
        orders = [math.log(errs[i] / errs[i + 1]) / math.log(Ns[i + 1] / Ns[i]) for i in range(len(Ns) - 1)]
        assert all(o >= k + 0.5 for o in orders), (surface, orders)


def test_narrow_band_surface_equals_dense():
    """the band's active cells (every corner within nlayers = 3 of a cut cell, src/meshfield.jl:364-369) hold every cell the
    dense surface quadrature keeps"""
    R = 0.5
    n = (41, 41)
    ref, vals = _ref(n, lambda X: X[0] ** 2 + X[1] ** 2 - R ** 2)
    cut, _, _ = Q.quadrature(ref, 4, surface=True)
    # the band: nodes within 3 (Chebyshev) of a node of a cell where ϕ changes sign
    sign = vals < 0
    cutn = np.zeros(n, dtype=bool)
    for i, j in itertools.product(range(n[0] - 1), range(n[1] - 1)):
        s = sign[i:i + 2, j:j + 2]
        if s.any() and not s.all():
            cutn[max(i - 3, 0):i + 5, max(j - 3, 0):j + 5] = True
    cells = [I for I in itertools.product(range(n[0] - 1), range(n[1] - 1)) if cutn[I[0]:I[0] + 2, I[1]:I[1] + 2].all()]
    cb, _, _ = Q.quadrature(ref, 4, surface=True, cells=cells)
    dense = sum(w.sum() for _, w in cut.values())
    band = sum(w.sum() for _, w in cb.values())
    assert abs(dense - band) <= 1e-10 * dense


def test_docs_disk_32():
    """docs/src/extension-implicit-integration.md: the 32² disk, area and perimeter to 1e-5 relative"""
    ref, _ = _ref((32, 32), lambda X: np.hypot(X[0], X[1]) - 0.5)
    assert abs(Q.total(ref, 4) - math.pi * 0.25) / (math.pi * 0.25) < 1e-5
    assert abs(Q.total(ref, 4, surface=True) - math.pi) / math.pi < 1e-5


def _halfspace(nrm, off):
    """volume and area of {n·x < off} ∩ [-1, 1]^N (n > 0, |n| = 1): with x = -1 + 2u, Σ a_d u_d < b on the unit cube,
    V_u = Σ_e (-1)^|e| (b - a·e)_+^N / (N! Π a_d); the area is dV/d(off)"""
    N = len(nrm)
    a, b = 2.0 * nrm, off + nrm.sum()
    V = A = 0.0
    for e in itertools.product((0, 1), repeat=N):
        t = b - a @ np.array(e, dtype=float)
        if t > 0:
            V += (-1) ** sum(e) * t ** N
            A += (-1) ** sum(e) * N * t ** (N - 1)
    den = math.factorial(N) * np.prod(a)
    return 2.0 ** N * V / den, 2.0 ** N * A / den


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("k", [1, 3])
def test_linear_cut_is_exact(N, k):
    """a half-plane / half-space cut at an angle: ψ is linear on every cell, its volume and its area are exact"""
    nrm = np.array([0.6, 0.8]) if N == 2 else np.array([0.6, 0.48, 0.64])
    off = 0.137
    ref, _ = _ref((9,) * N, lambda X: sum(nrm[d] * X[d] for d in range(N)) - off, k=k)
    V, A = _halfspace(nrm, off)
    assert abs(Q.total(ref, 3) - V) <= 1e-13
    assert abs(Q.total(ref, 3, surface=True) - A) <= 1e-13


@pytest.mark.parametrize("N", [1, 2, 3])
def test_full_box_integrates_degree_2q_minus_1(N):
    for q in (1, 2, 4):
        x, w = Q.full_rule(q, N)
        for p in range(2 * q):
            f = (x ** p).prod(axis=1)
            assert float(f @ w) == pytest.approx((1.0 / (p + 1)) ** N, rel=1e-13)


def test_restatement_depth_limit_and_fallback():
    """the kinked set of the GPU test (setdiff of two disks, 32²): a box at a horn reaches the depth limit; the fallback
    keeps the area and the perimeter close to the exact ones"""
    f = lambda X: np.maximum(np.hypot(X[0] - 0.13, X[1] - 0.07) - 0.55, -(np.hypot(X[0], X[1] - 0.07) - 0.45))
    ref, _ = _ref((32, 32), f)
    for surface in (False, True):
        cut, full, nfb = Q.quadrature(ref, 4, surface)
        assert nfb == 1
    # the crescent: disk A minus disk B, |AB| = d = 0.13; the lens A ∩ B from the two circular segments
    ra, rb, d = 0.55, 0.45, 0.13
    a = (d * d + ra * ra - rb * rb) / (2 * d)          # from A's centre to the chord
    ha = math.sqrt(ra * ra - a * a)
    lens = ra * ra * math.acos(a / ra) - a * ha + rb * rb * math.acos((d - a) / rb) - (d - a) * ha
    area = math.pi * ra * ra - lens
    assert abs(Q.total(ref, 4) - area) < 2e-3
    # the perimeter (the arc of A outside B plus the arc of B inside A) loses the horns' tips, thinner than the grid resolves
    perim = 2 * ra * (math.pi - math.acos(a / ra)) + 2 * rb * (math.pi - math.acos((a - d) / rb))
    assert 0.85 * perim < Q.total(ref, 4, surface=True) < perim


def test_api_errors_without_a_device():
    import lsm_amd as lsm
    with pytest.raises(TypeError):
        lsm.quadrature(np.zeros((4, 4)), interpolation_order=3, quadrature_order=4)
    with pytest.raises(TypeError):
        lsm.integrate(lambda x: x[:, 0], object())
    q = lsm.Quadrature(np.array([[0.25], [0.75]]), np.array([0.5, 0.5]))
    assert lsm.integrate(lambda x: x[:, 0], q) == pytest.approx(0.5)


# ----------------------------------------------------------------------------- fixtures of tests/test_gpu_quadrature_edges.py
# Fields whose classification is known in closed form or from a row pattern, so that grids far beyond what the restatement
# can sweep (more than 2^20 cut cells) still have an exact expectation.  Each builder is cached: the GPU file shares them.

def _ref_of(vals, lc, hc, k, P=None):
    return ReinitRef(_getter(vals, k if P is None else P), vals.shape, lc, hc, order=k, cells=[])


def _along_axis0(v, n):
    return np.asfortranarray(np.broadcast_to(v.reshape((-1,) + (1,) * (len(n) - 1)), n))


def stripes1(n):
    """k = 1: the sign alternates from node to node along axis 0, so every cell is cut by one plane x = x*"""
    i = np.arange(n[0])
    v = np.where(i % 2 == 0, 1.0, -1.0) * (0.3 + 0.2 * np.sin(1.7 * i))
    return _along_axis0(v, n), (0.25, -0.5, 1.0)[:len(n)], (1.75, 0.4, 2.5)[:len(n)]


def stripes1_closed_form(n, surface):
    """the one node of every cell of stripes1(n) at q = 1, cells in ascending linear order: (coords (ncell, N), weights)"""
    vals, lc, hc = stripes1(n)
    N = len(n)
    h = [(hc[d] - lc[d]) / (n[d] - 1) for d in range(N)]
    v = vals[(slice(None),) + (0,) * (N - 1)]
    a, b = v[:-1], v[1:]
    t = a / (a - b)
    lo0 = lc[0] + np.arange(n[0] - 1) * h[0]
    if surface:
        x0, w0 = lo0 + t * h[0], np.ones(n[0] - 1)
    else:                       # the piece where ψ < 0: [0, t] if a < 0, else [t, 1]
        u, w = np.where(a < 0, 0.0, t), np.where(a < 0, t, 1.0)
        x0, w0 = lo0 + (u + (w - u) * 0.5) * h[0], (w - u) * h[0]
    dims = tuple(k - 1 for k in n)
    idx = np.unravel_index(np.arange(int(np.prod(dims))), dims, order="F")
    X = np.empty((len(idx[0]), N))
    X[:, 0] = x0[idx[0]]
    for d in range(1, N):
        X[:, d] = (lc[d] + idx[d] * h[d]) + 0.5 * h[d]
    return X, w0[idx[0]] * float(np.prod(h[1:]))


def stripes3(ny):
    """k = 3 (ExtrapolationBC(3)), constant along y: per row 18 candidate cells (the Bernstein bound does not exclude 0),
    12 of them with nodes, 6 empty ones (ψ does not vanish in the cell), and 6 full cells"""
    n = (61, ny)
    i = np.arange(61)
    v = np.cos(2 * np.pi * i / 5 + 0.4) + 1.005 - 0.6 * (i % 10 >= 5)
    return _along_axis0(v, n), (0.0, 0.0), (6.0, 0.5)


def row_pattern(ref, j, q, surface):
    """row j of a 2-D field: (columns of the candidate cells, {column: (coords, weights)} of those with nodes, full columns)"""
    cells = [(i, j) for i in range(ref.n[0] - 1)]
    cand, full = [], []
    for I in cells:
        c = ref.coeffs(I)
        m, M = float(c.min()), float(c.max())
        if (m * M > 0.0) if surface else (m > 0.0):
            continue
        (full if not surface and M < 0.0 else cand).append(I[0])
    cut, full2, nfb = Q.quadrature(ref, q, surface, cells=cells)
    assert nfb == 0 and [I[0] for I in full2] == full and {I[0] for I in cut} <= set(cand)
    return cand, {I[0]: xw for I, xw in cut.items()}, full


_KINK3D = lambda X: np.maximum(np.sqrt((X[0] - 0.13) ** 2 + (X[1] - 0.07) ** 2 + (X[2] + 0.04) ** 2) - 0.55,
                               -(np.sqrt(X[0] ** 2 + (X[1] - 0.07) ** 2 + (X[2] + 0.04) ** 2) - 0.45))
_KINK2D = lambda X: np.maximum(np.hypot(X[0] - 0.13, X[1] - 0.07) - 0.55, -(np.hypot(X[0], X[1] - 0.07) - 0.45))
KINKS = {"kink3d": ((10, 9, 8), _KINK3D, 2), "kink2d_aniso": ((47, 32), _KINK2D, 4)}     # shape, field, q


def kink(name):
    """(vals, lc, hc) of a kinked set off the square grid: boxes at the horns reach the depth limit"""
    n, f, _ = KINKS[name]
    lc, hc = (-1.0,) * len(n), (1.0,) * len(n)
    ax = [np.linspace(lc[d], hc[d], n[d]) for d in range(len(n))]
    return np.asfortranarray(f(np.meshgrid(*ax, indexing="ij"))), lc, hc


_CACHE = {}


def restated(key, vals, lc, hc, k, q, surface, P=None):
    """Q.quadrature of the whole grid, computed once per key and shared between the CPU and the GPU tests"""
    if key not in _CACHE:
        _CACHE[key] = Q.quadrature(_ref_of(vals, lc, hc, k, P), q, surface)
    return _CACHE[key]


@pytest.mark.parametrize("n", [(12, 7), (9, 5, 4)])
@pytest.mark.parametrize("surface", [False, True])
def test_stripes1_closed_form(n, surface):
    vals, lc, hc = stripes1(n)
    cut, full, nfb = Q.quadrature(_ref_of(vals, lc, hc, 1), 1, surface)
    dims = tuple(k - 1 for k in n)
    cells = [tuple(int(v) for v in I) for I in zip(*np.unravel_index(np.arange(int(np.prod(dims))), dims, order="F"))]
    assert list(sorted(cut, key=lambda I: I[::-1])) == cells and full == [] and nfb == 0     # every cell is cut
    assert all(len(cut[I][1]) == 1 for I in cells)
    X, W = stripes1_closed_form(n, surface)
    d = max(np.abs(np.concatenate([cut[I][0] for I in cells]) - X).max(), np.abs(np.concatenate([cut[I][1] for I in cells]) - W).max())
    print(f"restatement vs closed form: {d:.3e}")
    assert d <= 1e-12


@pytest.mark.parametrize("surface", [False, True])
def test_stripes3_row_pattern(surface):
    ny = 12
    vals, lc, hc = stripes3(ny)
    ref = _ref_of(vals, lc, hc, 3)
    rows = [0, 1, 5, ny - 3, ny - 2]
    pats = [row_pattern(ref, j, 2, surface) for j in rows]
    hy = 0.5 / (ny - 1)
    worst = 0.0
    for j, (cand, cut, full) in zip(rows, pats):
        assert len(cand) == 18 and len(cut) == 12 and len(full) == (0 if surface else 6)
        assert cand == pats[2][0] and sorted(cut) == sorted(pats[2][1]) and full == pats[2][2]
        for i, (x, w) in cut.items():
            xm, wm = pats[2][1][i]
            assert x.shape == xm.shape
            worst = max(worst, np.abs(x[:, 0] - xm[:, 0]).max(), np.abs(w - wm).max(),
                        np.abs((x[:, 1] - j * hy) - (xm[:, 1] - rows[2] * hy)).max())
    print(f"rows against the middle row: {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("name", sorted(KINKS))
@pytest.mark.parametrize("surface", [False, True])
def test_kinks_reach_the_depth_limit(name, surface):
    vals, lc, hc = kink(name)
    cut, full, nfb = restated((name, surface), vals, lc, hc, 3, KINKS[name][2], surface)
    print(f"{name}: {len(cut)} cut cells, {len(full)} full cells, nfallback = {nfb}")
    assert nfb > 0 and len(cut) > 0
