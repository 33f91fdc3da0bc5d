"""mesh_distance on the device (csrc/lsm_mdist.hip, lsm_mesh_distance through the Python API) against the restatement
tests/_mdist_ref.py, bit for bit: rows shorter than a wave and rows whose prefix sum carries across 64-node chunks, cutoffs whose
boxes hold no node, are cut by the grid's faces or take several pieces, meshes leaving the grid, vertices on nodes, float32
storage, 2-D; determinism; the round trip through isosurface; the API and the refusals."""
import functools

import numpy as np
import pytest

import _iso_ref as I
import _mdist_ref as R
from test_isosurface_host import assert_closed_surface, case as iso_case, grid_vals
from test_mesh_distance_host import _cube, case as md_case

pytestmark = pytest.mark.gpu

INF = float("inf")


def _lsm():
    import lsm_amd
    return lsm_amd


def _field(lsm, n, lc, hc, dtype=None, vals=None):
    grid = lsm.CartesianGrid(lc, hc, n)
    v = np.zeros(n, order="F") if vals is None else vals
    mf = lsm.MeshField(v, grid, dtype=dtype)
    return lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=mf, bc=lsm.NeumannBC()).current_state()


def _mesh(name):
    if name == "cube":
        return _cube()
    if name == "sphere9":
        return iso_case(name)[3:5]
    if name == "open_at_x":          # a sphere leaving its box through the face x = 1: isosurface ends on that face
        n, lc, hc = (11, 10, 9), (-1.0,) * 3, (1.0,) * 3
        return I.isosurface(grid_vals(n, lambda X: np.sqrt((X[0] - 0.7) ** 2 + X[1] ** 2 + X[2] ** 2) - 0.6, lc, hc), lc, hc)
    return md_case(name)[4:6]


# name: (mesh, n, lc, hc)
GRIDS = {
    "row_of_5": ("sphere9", (5, 7, 6), (-1.0,) * 3, (1.0,) * 3),                     # a row shorter than a wave
    "row_of_67": ("sphere9", (67, 9, 8), (-1.0,) * 3, (1.0,) * 3),                   # the prefix sum carries across 64-node chunks
    "two_spheres": ("two_spheres", (21, 19, 17), (-1.0,) * 3, (1.0,) * 3),
    "leaving_x": ("two_spheres", (9, 19, 17), (-0.3, -1.0, -1.0), (0.1, 1.0, 1.0)),  # balanced through the outside slots
    "leaving_y": ("two_spheres", (21, 7, 17), (-1.0, -0.3, -1.0), (1.0, 0.2, 1.0)),  # a closed mesh cut by the grid across the rows: balanced
    "open_at_x": ("open_at_x", (11, 10, 9), (-1.0,) * 3, (1.0,) * 3),                # a mesh with a hole in the plane x = 1: unbalanced rows
    "cube_on_nodes": ("cube", (9, 17, 5), (-1.0,) * 3, (1.0,) * 3),                  # every vertex on a node: ϕ = ±0
    "disk": ("disk", (19, 17), (-1.0,) * 2, (1.0,) * 2),
    "two_disks_row_of_67": ("two_disks", (67, 18), (-1.0,) * 2, (1.0,) * 2),
}


@functools.lru_cache(maxsize=None)
def ref(name):
    """(vertices, elements, n, lc, hc, d², flips): the restatement's cutoff-independent parts, computed once, read-only"""
    mesh, n, lc, hc = GRIDS[name]
    if name in ("two_spheres", "disk"):              # the host tests' grid: their arrays
        _, _, _, _, v, e, d2, F = md_case(name)
        return v, e, n, lc, hc, d2, F
    v, e = _mesh(mesh)
    d2 = R.dist2(v, e, n, lc, hc)
    F = R.flips(v, e, n, lc, hc)
    d2.setflags(write=False)
    F[0].setflags(write=False)
    return v, e, n, lc, hc, d2, F


def _same(got, want):
    """ϕ bit for bit, the sign of a zero included"""
    assert got.shape == want.shape and got.dtype == want.dtype
    fin = np.isfinite(want) & np.isfinite(got)
    if fin.any():
        ulp = np.abs(got[fin] - want[fin]) / np.spacing(np.abs(want[fin]).astype(want.dtype))
        print(f"max difference {ulp.max():.1f} ulp over {int(fin.sum())} nodes, sign mismatches {int((np.signbit(got) != np.signbit(want)).sum())}")
    assert np.array_equal(got, want)
    assert np.array_equal(np.signbit(got), np.signbit(want))


def _h0(name):
    _, n, lc, hc = GRIDS[name]
    return (hc[0] - lc[0]) / (n[0] - 1)


CASES = [(name, INF) for name in GRIDS if name != "open_at_x"] + [
    ("two_spheres", 0.5 * _h0("two_spheres")),       # boxes that hold no node
    ("two_spheres", 3 * _h0("two_spheres")),         # boxes of several hundred nodes, cut by the grid's faces near them
    ("leaving_x", 3 * _h0("leaving_x")),
    ("row_of_67", 3 * _h0("row_of_67")),
    ("disk", 3 * _h0("disk")),
]


@pytest.mark.parametrize("name,cutoff", CASES, ids=[f"{n}-{c:.3g}" for n, c in CASES])
def test_device_matches_restatement(name, cutoff):
    lsm = _lsm()
    v, e, n, lc, hc, d2, F = ref(name)
    want, stats = R.mesh_distance(v, e, n, lc, hc, cutoff, d2=d2, F=F)
    assert stats[1] == 0 and (want < 0).any() and (want > 0).any()
    phi = _field(lsm, n, lc, hc)
    assert phi.backend.mesh_distance(phi.buf, v, e, cutoff) == stats
    _same(phi.values(), want)
    if cutoff == INF:
        assert stats[0] == want.size
    else:
        assert 0 < stats[0] < want.size
    if name == "cube_on_nodes":
        assert (want == 0).sum() >= 8


def test_several_pieces_per_element_and_determinism():
    """(67, 9, 8) without a cutoff: every element's box is the whole grid, 4824 nodes in three pieces; a second call, on a field
    holding the first result, gives the same bits (minima and integer sums do not depend on the order of arrival)"""
    lsm = _lsm()
    v, e, n, lc, hc, d2, F = ref("row_of_67")
    assert np.prod(n) > 2 * 2048
    phi = _field(lsm, n, lc, hc)
    assert lsm.mesh_distance_(phi, (v, e)) is phi and phi.ghosts_dirty
    first = phi.values()
    lsm.mesh_distance_(phi, lsm.InterfaceMesh(v, e), cutoff=INF)
    again = phi.values()
    assert np.array_equal(first.view(np.uint64), again.view(np.uint64))
    _same(first, R.mesh_distance(v, e, n, lc, hc, d2=d2, F=F)[0])


def test_float32_storage_rounds_the_fp64_result_once():
    lsm = _lsm()
    v, e, n, lc, hc, d2, F = ref("two_spheres")
    for cutoff in (INF, 3 * _h0("two_spheres")):
        want, _ = R.mesh_distance(v, e, n, lc, hc, cutoff, d2=d2, F=F)
        phi = _field(lsm, n, lc, hc, dtype=np.float32)
        lsm.mesh_distance_(phi, (v, e), cutoff)
        got = phi.values()
        assert got.dtype == np.float32
        _same(got, want.astype(np.float32))


def test_open_and_inconsistently_oriented_meshes_are_refused():
    """a mesh that ends on the plane x = 1: rows see an entry without an exit.  The statistics and the values still equal the
    restatement's; the API raises.  (A closed mesh that sticks out of the grid, along the rows or across them, stays balanced —
    every row that exists sees all its crossings, the outside slots take those beyond the grid: the leaving_x and leaving_y
    cases above.)"""
    lsm = _lsm()
    v, e, n, lc, hc, d2, F = ref("open_at_x")
    want, stats = R.mesh_distance(v, e, n, lc, hc, d2=d2, F=F)
    assert stats[1] > 0
    phi = _field(lsm, n, lc, hc)
    assert phi.backend.mesh_distance(phi.buf, v, e, INF) == stats
    _same(phi.values(), want)
    with pytest.raises(ValueError, match=rf"mesh_distance: the mesh is not closed or not consistently oriented \({stats[1]} grid rows see unbalanced crossings\)"):
        lsm.mesh_distance_(phi, (v, e))
    # one triangle reversed, one removed
    v, e, n, lc, hc, _, _ = ref("two_spheres")
    p = v[e]
    A2 = (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 2] - p[:, 0, 2]) - (p[:, 1, 2] - p[:, 0, 2]) * (p[:, 2, 1] - p[:, 0, 1])
    k = next(int(k) for k in np.argsort(-np.abs(A2)) if R.flips(v, e[k:k + 1], n, lc, hc)[0].any())     # a grid line passes through it
    for broken in (np.delete(e, k, axis=0), np.concatenate([e[:k], e[k:k + 1, [0, 2, 1]], e[k + 1:]])):
        F = R.flips(v, broken, n, lc, hc)
        nbad = int((R.winding(F[0])[1] != 0).sum())
        phi = _field(lsm, n, lc, hc)
        assert nbad > 0 and phi.backend.mesh_distance(phi.buf, v, broken, INF)[1] == nbad
        with pytest.raises(ValueError, match="not closed or not consistently oriented"):
            lsm.mesh_distance_(phi, (v, broken))


def test_round_trip_through_isosurface():
    """isosurface → mesh_distance_ gives back the sign of every node off the level, hence a mesh of the same connectivity: closed,
    two spheres (Euler characteristic 4); the distance is a distance: at most the cutoff, 1-Lipschitz"""
    lsm = _lsm()
    vals, lc, hc, level, _, _, _, _ = md_case("two_spheres")
    src = _field(lsm, vals.shape, lc, hc, vals=vals)
    m = lsm.isosurface(src, level)
    phi = _field(lsm, vals.shape, lc, hc)
    c = 4 * _h0("two_spheres")
    lsm.mesh_distance_(phi, m, cutoff=c)
    got = phi.values()
    off = vals != level
    assert np.array_equal((got < 0)[off], (vals < level)[off])
    assert np.abs(got).max() <= np.sqrt(c * c)
    back = lsm.isosurface(phi)
    assert_closed_surface(back.vertices, back.elements, 4)
    assert I.enclosed(back.vertices, back.elements) == pytest.approx(I.enclosed(m.vertices, m.elements), rel=0.02)
    # through an equation, as reinitialize_ takes one
    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(vals, lsm.CartesianGrid(lc, hc, vals.shape)), bc=lsm.NeumannBC())
    lsm.mesh_distance_(eq, m, cutoff=c)
    assert np.array_equal(eq.current_state().values().view(np.uint64), got.view(np.uint64))


def test_host_entry_point_and_read_mesh(tmp_path):
    """mesh_distance(mesh, grid) builds its own handle and returns a host MeshField usable as ic=; the mesh comes from a file"""
    lsm = _lsm()
    v, e, n, lc, hc, d2, F = ref("row_of_5")
    out = str(tmp_path / "sphere.mesh")
    lsm.export_surface_mesh(lsm.InterfaceMesh(v, e), out)
    grid = lsm.CartesianGrid(lc, hc, n)
    mf = lsm.mesh_distance(lsm.read_mesh(out), grid)
    assert isinstance(mf, lsm.MeshField) and mf.vals.dtype == np.float64
    _same(np.asarray(mf.vals), R.mesh_distance(v, e, n, lc, hc, d2=d2, F=F)[0])
    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=mf, bc=lsm.NeumannBC())
    assert np.array_equal(eq.current_state().values(), mf.vals)
    m32 = lsm.mesh_distance((v, e), grid, cutoff=0.4, dtype=np.float32)
    assert m32.vals.dtype == np.float32
    _same(np.asarray(m32.vals), R.mesh_distance(v, e, n, lc, hc, 0.4, d2=d2, F=F)[0].astype(np.float32))


def test_an_empty_mesh_is_all_outside():
    lsm = _lsm()
    phi = _field(lsm, (5, 7, 6), (-1.0,) * 3, (1.0,) * 3)
    assert phi.backend.mesh_distance(phi.buf, np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64), 0.3) == (0, 0, 0)
    assert (phi.values() == np.sqrt(np.float64(0.3) * 0.3)).all()


def test_refusals():
    lsm = _lsm()
    v, e, n, lc, hc, _, _ = ref("row_of_5")
    phi = _field(lsm, n, lc, hc)
    with pytest.raises(TypeError, match="device field"):
        lsm.mesh_distance_(np.zeros(n), (v, e))
    with pytest.raises(TypeError, match="InterfaceMesh or a"):
        lsm.mesh_distance_(phi, 3.0)
    with pytest.raises(ValueError, match="elements"):
        lsm.mesh_distance_(phi, (v, e[:, :2]))
    for c in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="cutoff must be positive"):
            lsm.mesh_distance_(phi, (v, e), cutoff=c)
        with pytest.raises(lsm.LsmError, match="lsm_mesh_distance: cutoff must be positive"):
            phi.backend.mesh_distance(phi.buf, v, e, c)
    v2, e2, *_ = ref("disk")
    with pytest.raises(ValueError, match="a mesh in 2 dimensions cannot be measured on a 3 dimensional grid"):
        lsm.mesh_distance_(phi, (v2, e2))
    grid = lsm.CartesianGrid((0.0,), (1.0,), (17,))
    one = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(lambda x: x[0] - 0.4, grid), bc=lsm.NeumannBC())
    with pytest.raises(ValueError, match="1 dimensional"):
        lsm.mesh_distance_(one, (v2, e2))
    with pytest.raises(lsm.LsmError, match="1-dimensional"):
        one.backend.mesh_distance(one.current_state().buf, v2, e2, INF)
    grid3 = lsm.CartesianGrid(lc, hc, n)
    fine = lsm.CartesianGrid(lc, hc, (17, 18, 16))
    band = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), bc=lsm.NeumannBC(),
                                ic=lsm.NarrowBandMeshField(lsm.MeshField(lambda x: np.sqrt(x[0] ** 2 + x[1] ** 2 + x[2] ** 2) - 0.5, fine), nlayers=2))
    with pytest.raises(ValueError, match="NarrowBandMeshField"):
        lsm.mesh_distance_(band, (v, e))
    g = lsm.LocalGroup(1)
    slab = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(np.zeros(n, order="F"), grid3), bc=lsm.NeumannBC(), comm=g.rank(0))
    with pytest.raises(ValueError, match="slab"):
        lsm.mesh_distance_(slab, (v, e))
    with pytest.raises(lsm.LsmError, match="slab"):
        slab.backend.mesh_distance(slab.current_state().buf, v, e, INF)
    bad = np.array(v)
    bad[3, 1] = np.inf
    with pytest.raises(lsm.LsmError, match="the vertices must be finite"):
        lsm.mesh_distance_(phi, (bad, e))


def test_a_vertex_number_out_of_range_is_an_error_not_a_fault():
    """validated on the device by a kernel that only reads, before any kernel addresses a vertex with it; the handle stays usable"""
    lsm = _lsm()
    v, e, n, lc, hc, d2, F = ref("row_of_5")
    phi = _field(lsm, n, lc, hc)
    bad = np.array(e)
    bad[len(e) // 2, 1] = len(v)
    bad[len(e) // 3, 2] = -1
    with pytest.raises(lsm.LsmError, match="an element refers to a vertex number outside"):
        lsm.mesh_distance_(phi, (v, bad))
    lsm.mesh_distance_(phi, (v, e))
    _same(phi.values(), R.mesh_distance(v, e, n, lc, hc, d2=d2, F=F)[0])
