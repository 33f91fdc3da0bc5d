"""The restatement of mesh_distance (tests/_mdist_ref.py, the contract of csrc/lsm_mdist.hip) against facts that do not come from
it: the sign against the field the mesh was extracted from, the 1-Lipschitz bound of a distance, the analytic distance of a cube,
open and inconsistently oriented meshes; and read_mesh, the host-side Medit reader, against the library's own writers."""
import functools

import numpy as np
import pytest

import _iso_ref as I
import _mdist_ref as R
from test_isosurface_host import disk, grid_vals, torus


def two_spheres(X):
    a = np.sqrt((X[0] + 0.45) ** 2 + (X[1] + 0.1) ** 2 + (X[2] - 0.05) ** 2) - 0.33
    b = np.sqrt((X[0] - 0.4) ** 2 + (X[1] - 0.15) ** 2 + (X[2] + 0.1) ** 2) - 0.41
    return np.minimum(a, b)


def box(X):
    return np.maximum(np.maximum(np.abs(X[0]), np.abs(X[1])), np.abs(X[2])) - 0.5


def two_disks(X):
    return np.minimum(np.hypot(X[0] + 0.5, X[1] + 0.2) - 0.3, np.hypot(X[0] - 0.45, X[1] - 0.3) - 0.36)


# name: (n, field, lc, hc, level)
CASES = {
    "torus": ((20, 18, 16), torus, (-1.0, -1.0, -0.5), (1.0, 1.0, 0.5), 0.0),
    "two_spheres": ((21, 19, 17), two_spheres, (-1.0,) * 3, (1.0,) * 3, 0.0),
    "box_on_planes": ((17, 17, 17), box, (-1.0,) * 3, (1.0,) * 3, 0.0),
    "box_level": ((17, 17, 17), box, (-1.0,) * 3, (1.0,) * 3, 0.125),
    "disk": ((19, 17), disk, (-1.0,) * 2, (1.0,) * 2, 0.0),
    "two_disks": ((23, 18), two_disks, (-1.0,) * 2, (1.0,) * 2, 0.0),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(values, lc, hc, level, vertices, elements, d², flip counters with the skipped count): computed once, shared, read-only"""
    n, f, lc, hc, level = CASES[name]
    vals = grid_vals(n, f, lc, hc)
    v, e = I.isosurface(vals, lc, hc, level=level)
    d2 = R.dist2(v, e, n, lc, hc)
    F = R.flips(v, e, n, lc, hc)
    for a in (vals, v, e, d2, F[0]):
        a.setflags(write=False)
    return vals, lc, hc, level, v, e, d2, F


@pytest.mark.parametrize("name", sorted(CASES))
def test_sign_is_the_side_of_the_level(name):
    """the mesh is the level set of the piecewise-linear interpolant: a node with ϕ != level lies strictly on one side.  Almost
    every grid line passes through mesh vertices and edges here (isosurface vertices sit on grid edges): a crossing counted twice
    or not at all would flip a run of nodes or unbalance the line"""
    vals, lc, hc, level, v, e, d2, F = case(name)
    assert len(e) > 0
    W, tot = R.winding(F[0])
    assert set(np.unique(W).tolist()) <= {0, 1}
    assert not tot.any()
    off = vals != level
    assert np.array_equal((W != 0)[off], (vals < level)[off])
    phi, stats = R.mesh_distance(v, e, vals.shape, lc, hc, d2=d2, F=F)
    assert stats[0] == vals.size and stats[1] == 0 and stats[2] == F[1]
    assert np.array_equal((phi < 0)[off & (d2 > 0)], (vals < level)[off & (d2 > 0)])
    assert np.isfinite(phi).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_distance_is_1_lipschitz(name):
    """|d(x) − d(x + h e_a)| <= h_a for the distance to any set (triangle inequality); 1e-12 relative for the roundings"""
    vals, lc, hc, _, _, _, d2, _ = case(name)
    d = np.sqrt(d2)
    _, h = R.axes(vals.shape, lc, hc)
    for a in range(vals.ndim):
        assert np.abs(np.diff(d, axis=a)).max() <= h[a] * (1 + 1e-12)


def _cube():
    """[−1/2, 1/2]³ as 12 outward-oriented triangles"""
    v = np.array([[x, y, z] for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)])
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]     # −z +z −y +y −x +x
    e = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int64)
    return v, e


def test_cube_against_the_analytic_distance():
    """every coordinate is a dyadic rational (h = 1/4, 1/8, 1/2): products and sums are exact, the divisions of the edge regions
    and the final square root round once each"""
    v, e = _cube()
    assert I.enclosed(v, e) == pytest.approx(1.0, abs=1e-15)
    n, lc, hc = (9, 17, 5), (-1.0,) * 3, (1.0,) * 3
    phi, stats = R.mesh_distance(v, e, n, lc, hc)
    xs, _ = R.axes(n, lc, hc)
    X = np.meshgrid(*xs, indexing="ij")
    q = [np.abs(x) - 0.5 for x in X]
    outside = np.sqrt(sum(np.maximum(c, 0.0) ** 2 for c in q))
    exact = np.where(outside > 0, outside, np.maximum(np.maximum(q[0], q[1]), q[2]))
    assert stats == (phi.size, 0, 8)                       # the 8 triangles of the ±y and ±z faces project to segments
    assert np.abs(phi - exact).max() <= 1e-14 * np.abs(exact).max()
    assert (np.abs(phi - exact) <= 1e-14 * np.abs(exact)).all()
    assert ((phi == 0) == (exact == 0)).all() and (exact == 0).any()
    # cut off: the same values below c, ±sqrt(c·c) beyond
    c = 0.3
    cut, st = R.mesh_distance(v, e, n, lc, hc, cutoff=c)
    near = np.abs(exact) < c
    assert st[0] == int(near.sum()) and np.array_equal(cut[near], phi[near])
    assert np.array_equal(cut[~near], np.sign(phi[~near]) * np.sqrt(np.float64(c) * c))


def test_open_and_flipped_meshes_unbalance_rows():
    vals, lc, hc, _, v, e, _, _ = case("two_spheres")
    # a triangle some grid line passes through (many lie between the lines): the first such by descending projected area
    p = v[e]
    A2 = (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 2] - p[:, 0, 2]) - (p[:, 1, 2] - p[:, 0, 2]) * (p[:, 2, 1] - p[:, 0, 1])
    k = next(int(k) for k in np.argsort(-np.abs(A2)) if R.flips(v, e[k:k + 1], vals.shape, lc, hc)[0].any())
    for broken in (np.delete(e, k, axis=0), np.concatenate([e[:k], e[k:k + 1, [0, 2, 1]], e[k + 1:]])):
        F, _ = R.flips(v, broken, vals.shape, lc, hc)
        _, tot = R.winding(F)
        assert tot.any()
    # 2-D: a segment removed, a segment reversed
    vals, lc, hc, _, v, e, _, _ = case("disk")
    k = next(k for k in range(len(e)) if R.flips(v, e[k:k + 1], vals.shape, lc, hc)[0].any())
    for broken in (np.delete(e, k, axis=0), np.concatenate([e[:k], e[k:k + 1, ::-1], e[k + 1:]])):
        F, _ = R.flips(v, broken, vals.shape, lc, hc)
        assert R.winding(F)[1].any()


def test_a_mesh_leaving_the_grid_along_x_stays_balanced():
    """crossings left of the grid go to slot 0, crossings right of it to slot n0: every line still sums to zero, and the nodes
    between the grid's left face and the mesh's first crossing inside are inside"""
    vals, lc, hc, _, v, e, _, _ = case("two_spheres")
    n = (9, 19, 17)
    sub_lc, sub_hc = (-0.3, -1.0, -1.0), (0.1, 1.0, 1.0)            # cuts both spheres
    F, _ = R.flips(v, e, n, sub_lc, sub_hc)
    W, tot = R.winding(F)
    assert not tot.any() and F[0].any() and F[-1].any()
    xs, _ = R.axes(n, sub_lc, sub_hc)
    ref = two_spheres(np.meshgrid(*xs, indexing="ij"))
    far = np.abs(ref) > 0.05                                        # the mesh is the level set of an interpolant on another grid
    assert np.array_equal((W != 0)[far], (ref < 0)[far])


# ----------------------------------------------------------------------------- read_mesh

def test_read_mesh_round_trip_of_export_surface_mesh(tmp_path):
    import lsm_amd
    _, _, _, _, v, e, _, _ = case("torus")
    out = str(tmp_path / "torus.mesh")
    lsm_amd.export_surface_mesh(lsm_amd.InterfaceMesh(v, e), out)
    m = lsm_amd.read_mesh(out)
    assert isinstance(m, lsm_amd.InterfaceMesh) and m.ndim == 3
    assert m.vertices.dtype == np.float64 and m.elements.dtype == np.int64
    assert np.array_equal(m.vertices, v) and np.array_equal(m.elements, e)


@pytest.mark.parametrize("name", ["disk", "two_spheres"])
def test_read_mesh_takes_the_interface_of_a_volume_file(name, tmp_path):
    """export_volume_mesh's file: the interface is the `Edges` (2-D) / `Triangles` (3-D) section, the elements are skipped"""
    import lsm_amd
    _, _, _, _, v, e, _, _ = case(name)
    N = v.shape[1]
    filler = np.zeros((2, N + 1), dtype=np.int64)
    out = str(tmp_path / "domain.mesh")
    lsm_amd.export_volume_mesh(lsm_amd.DomainMesh(v, filler, e), out)
    m = lsm_amd.read_mesh(out)
    assert m.ndim == N and np.array_equal(m.vertices, v) and np.array_equal(m.elements, e)


def test_read_mesh_refusals(tmp_path):
    import lsm_amd
    p = tmp_path / "bad.mesh"
    p.write_text("MeshVersionFormatted 1\nDimension 3\n\nVertices\n1\n0.0 0.0 0.0 1\n\nTriangles\n1\n1 2 1 1\n\nEnd\n")
    with pytest.raises(ValueError, match="vertex number"):
        lsm_amd.read_mesh(str(p))
    p.write_text("MeshVersionFormatted 1\nDimension 3\n\nTriangles\n0\n\nEnd\n")
    with pytest.raises(ValueError, match="Vertices"):
        lsm_amd.read_mesh(str(p))
    p.write_text("MeshVersionFormatted 1\nDimension 1\n\nVertices\n0\n\nEnd\n")
    with pytest.raises(ValueError, match="Dimension"):
        lsm_amd.read_mesh(str(p))


def test_the_culled_minimum_is_the_brute_force_minimum():
    """dist2 skips pairs that cannot win; the bits are those of every element against every node"""
    from test_isosurface_host import case as iso_case
    _, _, _, v, e = iso_case("sphere9")
    for n, lc, hc in (((5, 7, 6), (-1.0,) * 3, (1.0,) * 3), ((6, 5, 7), (0.2, -0.4, -2.0), (3.0, 0.3, -0.1))):
        a, b = R.dist2(v, e, n, lc, hc), R.dist2(v, e, n, lc, hc, cull=False)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    _, lc, hc, _, v, e, d2, _ = case("two_disks")
    assert np.array_equal(d2.view(np.uint64), R.dist2(v, e, d2.shape, lc, hc, cull=False).view(np.uint64))
