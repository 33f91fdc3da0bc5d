"""The restatement of isosurface (tests/_iso_ref.py, the contract of csrc/lsm_iso.hip) against facts that do not come from it:
an independent count of the sign-changing edges, closedness and the Euler characteristic, orientation, second-order convergence
of area and volume, exact planes; and the Medit writer of export_surface_mesh on plain numpy input."""
import functools
import math

import numpy as np
import pytest

import _iso_ref as R


def grid_vals(n, f, lc, hc):
    ax = [np.linspace(lc[d], hc[d], n[d]) for d in range(len(n))]
    return np.asfortranarray(f(np.meshgrid(*ax, indexing="ij")))


SPHERE_C, SPHERE_R = (0.05, -0.08, 0.03), 0.52
DISK_C, DISK_R = (0.11, -0.07), 0.53


def sphere(X):
    return np.sqrt(sum((X[d] - SPHERE_C[d]) ** 2 for d in range(3))) - SPHERE_R


def torus(X):
    return np.sqrt((np.sqrt(X[0] ** 2 + X[1] ** 2) - 0.6) ** 2 + X[2] ** 2) - 0.25


def disk(X):
    return np.hypot(X[0] - DISK_C[0], X[1] - DISK_C[1]) - DISK_R


CASES = {
    "sphere9": ((9, 10, 8), sphere, (-1.0,) * 3, (1.0,) * 3),
    "sphere17": ((17, 18, 16), sphere, (-1.0,) * 3, (1.0,) * 3),
    "sphere33": ((33, 34, 32), sphere, (-1.0,) * 3, (1.0,) * 3),
    "torus": ((21, 20, 13), torus, (-1.0, -1.0, -0.5), (1.0, 1.0, 0.5)),
    "disk17": ((17, 15), disk, (-1.0,) * 2, (1.0,) * 2),
    "disk33": ((33, 31), disk, (-1.0,) * 2, (1.0,) * 2),
    "disk65": ((65, 63), disk, (-1.0,) * 2, (1.0,) * 2),
}
CLOSED_3D = ["sphere9", "sphere17", "sphere33", "torus"]
CLOSED_2D = ["disk17", "disk33", "disk65"]


@functools.lru_cache(maxsize=None)
def case(name):
    """(values, lc, hc, vertices, elements) of a named case: computed once, shared, never modified"""
    n, f, lc, hc = CASES[name]
    vals = grid_vals(n, f, lc, hc)
    v, e = R.isosurface(vals, lc, hc)
    for a in (vals, v, e):
        a.setflags(write=False)
    return vals, lc, hc, v, e


# ----------------------------------------------------------------------------- checks that do not come from the restatement

def count_sign_changes(vals, level=0.0):
    """edges (I, I + d), d over the 2^N − 1 directions, whose ends differ in ϕ < level: numpy slicing only"""
    inside = np.asarray(vals, dtype=np.float64) < level
    N, total = inside.ndim, 0
    for d in range(1, 1 << N):
        lo = tuple(slice(0, inside.shape[a] - (d >> a & 1)) for a in range(N))
        hi = tuple(slice(d >> a & 1, None) for a in range(N))
        total += int(np.count_nonzero(inside[lo] != inside[hi]))
    return total


def directed_edges(elems):
    """every directed edge of every triangle as one int64 key (v0 · nvmax + v1)"""
    big = int(elems.max()) + 1 if len(elems) else 1
    e = np.concatenate([elems[:, [0, 1]], elems[:, [1, 2]], elems[:, [2, 0]]])
    return e[:, 0] * big + e[:, 1], e[:, 1] * big + e[:, 0]


def assert_closed_surface(verts, elems, euler):
    fwd, rev = directed_edges(elems)
    assert len(np.unique(fwd)) == len(fwd), "a directed edge occurs twice"
    assert np.array_equal(np.sort(fwd), np.sort(rev)), "a directed edge has no reverse"
    assert np.array_equal(np.unique(elems), np.arange(len(verts))), "an unreferenced vertex"
    assert len(verts) - len(fwd) // 2 + len(elems) == euler


def assert_closed_curve(verts, elems):
    nv = len(verts)
    assert np.array_equal(np.sort(elems[:, 0]), np.arange(nv)), "a vertex is not the start of exactly one segment"
    assert np.array_equal(np.sort(elems[:, 1]), np.arange(nv)), "a vertex is not the end of exactly one segment"


# ----------------------------------------------------------------------------- tests

@pytest.mark.parametrize("name", sorted(CASES))
def test_vertex_count_is_the_number_of_sign_changing_edges(name):
    vals, _, _, v, _ = case(name)
    assert len(v) == count_sign_changes(vals) > 0
    assert np.isfinite(v).all()


@pytest.mark.parametrize("name", CLOSED_3D)
def test_closed_manifold_3d(name):
    _, _, _, v, e = case(name)
    assert_closed_surface(v, e, 0 if name == "torus" else 2)


@pytest.mark.parametrize("name", CLOSED_2D)
def test_closed_manifold_2d(name):
    _, _, _, v, e = case(name)
    assert_closed_curve(v, e)


@pytest.mark.parametrize("name", CLOSED_3D)
def test_orientation_3d(name):
    _, _, _, v, e = case(name)
    assert R.enclosed(v, e) > 0
    if name != "torus":
        p = v[e]
        nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        out = p.mean(axis=1) - np.array(SPHERE_C)
        keep = np.linalg.norm(nrm, axis=1) > 0
        assert keep.any() and ((nrm * out).sum(axis=1)[keep] > 0).all()


@pytest.mark.parametrize("name", CLOSED_2D)
def test_orientation_2d(name):
    _, _, _, v, e = case(name)
    assert R.enclosed(v, e) > 0
    p = v[e]
    d = p[:, 1] - p[:, 0]
    nrm = np.stack([d[:, 1], -d[:, 0]], axis=1)
    out = p.mean(axis=1) - np.array(DISK_C)
    assert ((nrm * out).sum(axis=1) > 0).all()


def test_convergence_3d():
    """the mesh is inscribed (area below 4πr²) and second order: the error at twice the resolution is at most 0.3 of it"""
    area, vol = 4 * math.pi * SPHERE_R ** 2, 4 / 3 * math.pi * SPHERE_R ** 3
    err = {}
    for name in ("sphere17", "sphere33"):
        _, _, _, v, e = case(name)
        err[name] = (R.measure(v, e) / area - 1, R.enclosed(v, e) / vol - 1)
        assert err[name][0] < 0 and err[name][1] < 0
    for k in range(2):
        assert abs(err["sphere33"][k]) <= 0.3 * abs(err["sphere17"][k]), err


def test_convergence_2d():
    length, area = 2 * math.pi * DISK_R, math.pi * DISK_R ** 2
    err = {}
    for name in ("disk33", "disk65"):
        _, _, _, v, e = case(name)
        err[name] = (R.measure(v, e) / length - 1, R.enclosed(v, e) / area - 1)
        assert err[name][0] < 0 and err[name][1] < 0
    for k in range(2):
        assert abs(err["disk65"][k]) <= 0.3 * abs(err["disk33"][k]), err


PLANES = {
    "z": ((9, 8, 7), lambda X: X[2] - 0.3 + 0 * X[0], 1.0),
    "diag147": ((9, 8, 7), lambda X: X[0] + X[1] + X[2] - 1.47, (math.sqrt(3) / 2) * (-2 * 1.47 ** 2 + 6 * 1.47 - 3)),
    "diag15": ((17, 17, 17), lambda X: X[0] + X[1] + X[2] - 1.5, 3 * math.sqrt(3) / 4),
}


@pytest.mark.parametrize("name", sorted(PLANES))
def test_planes_are_exact(name):
    """linear data: the mesh is the plane's section of the unit cube.  diag15: grid nodes lie on the level (outside by the sign
    convention), so some triangles have zero area; every coordinate stays finite"""
    n, f, exact = PLANES[name]
    vals = grid_vals(n, f, (0.0,) * 3, (1.0,) * 3)
    v, e = R.isosurface(vals, (0.0,) * 3, (1.0,) * 3)
    assert np.isfinite(v).all()
    assert abs(R.measure(v, e) - exact) <= 1e-13
    assert np.array_equal(np.unique(e), np.arange(len(v)))
    if name == "diag15":
        p = v[e]
        assert (np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1) == 0).any()


def test_band_holding_every_cut_cell_gives_the_dense_mesh():
    """the premise of the device's band test: |ϕ| < 0.3 on the (17, 18, 16) sphere holds every cell the surface crosses"""
    vals, lc, hc, v, e = case("sphere17")
    vb, eb = R.isosurface(vals, lc, hc, mask=np.abs(vals) < 0.3)
    assert np.array_equal(vb, v) and np.array_equal(eb, e)
    # a thin band drops cells: a mesh with boundary whose vertices are all referenced
    vt, et = R.isosurface(vals, lc, hc, mask=np.abs(vals) < 0.12)
    assert 0 < len(et) < len(e)
    assert np.array_equal(np.unique(et), np.arange(len(vt)))


def test_level_nan_and_float32():
    vals, lc, hc, v, e = case("sphere9")
    for level in (0.1, -0.07):
        vl, el = R.isosurface(vals, lc, hc, level=level)
        assert len(vl) == count_sign_changes(vals, level)
        assert_closed_surface(vl, el, 2)
    v32, e32 = R.isosurface(vals.astype(np.float32), lc, hc)
    vr, er = R.isosurface(vals.astype(np.float32).astype(np.float64), lc, hc)
    assert np.array_equal(v32, vr) and np.array_equal(e32, er)
    bad = np.array(vals)
    bad[4, 5, 4] = np.nan                      # deep inside: the node turns outside, the vertices on its edges are NaN
    vn, en = R.isosurface(bad, lc, hc)
    assert len(vn) == count_sign_changes(bad) and np.isnan(vn).any()
    empty = R.isosurface(np.abs(vals) + 1.0, lc, hc)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3)


# ----------------------------------------------------------------------------- the Medit writer (ext/MMGSurfaceExt.jl:82-102)

_VERTS = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [0.0, 1.0e-5, -0.25], [1.0e6, 1.0, 1.0 / 3.0]])
_TRIS = np.array([[0, 1, 2], [1, 3, 2]])
_EXPECTED = """MeshVersionFormatted 1
Dimension 3

Vertices
4
0.0 0.0 0.0 1
1.0 0.0 0.5 1
0.0 1.0e-5 -0.25 1
1.0e6 1.0 0.3333333333333333 1

Triangles
2
1 2 3 1
2 4 3 1

End
"""


def test_export_surface_mesh_writes_the_reference_file(tmp_path):
    import lsm_amd
    m = lsm_amd.InterfaceMesh(_VERTS, _TRIS)
    assert len(m) == 2 and m.vertices.dtype == np.float64 and m.elements.dtype == np.int64
    out = str(tmp_path / "surface.mesh")
    assert lsm_amd.export_surface_mesh(m, out) == out
    assert open(out).read() == _EXPECTED


def test_export_surface_mesh_refusals(tmp_path):
    import lsm_amd
    out = str(tmp_path / "surface.mesh")
    m = lsm_amd.InterfaceMesh(_VERTS, _TRIS)
    for kw in ("hgrad", "hmin", "hmax", "hausd"):
        with pytest.raises(NotImplementedError, match="mmgs"):
            lsm_amd.export_surface_mesh(m, out, **{kw: 0.1})
    m2 = lsm_amd.InterfaceMesh(_VERTS[:, :2], _TRIS[:, :2])
    with pytest.raises(ValueError, match="export_mesh of 2 dimensional level-set not supported."):
        lsm_amd.export_surface_mesh(m2, out)
    with pytest.raises(TypeError):
        lsm_amd.export_surface_mesh(np.zeros((3, 3, 3)), out)
    with pytest.raises(TypeError):
        lsm_amd.isosurface(np.zeros((3, 3, 3)))


def test_interface_mesh_measure():
    import lsm_amd
    _, _, _, v, e = case("sphere9")
    assert lsm_amd.InterfaceMesh(v, e).measure() == pytest.approx(R.measure(v, e), rel=1e-15)
    _, _, _, v, e = case("disk17")
    assert lsm_amd.InterfaceMesh(v, e).measure() == pytest.approx(R.measure(v, e), rel=1e-15)
    assert lsm_amd.InterfaceMesh(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)).measure() == 0.0
