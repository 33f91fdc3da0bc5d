"""volume_mesh on the device (csrc/lsm_vol.hip, lsm_vol_* through the Python API) against the restatement tests/_vol_ref.py:
elements and interface exactly, vertices bit for bit; against lsm.isosurface on the same field; launch shapes where rows straddle
waves and chunks are partial or several, checked by facts that do not come from the restatement; the API, export_volume_mesh and
the refusals."""
import ctypes

import numpy as np
import pytest

import _iso_ref as R
import _vol_ref as V
from test_gpu_isosurface import FIELDS, _device
from test_isosurface_host import case, count_sign_changes, disk, grid_vals, sphere
from test_volume_mesh_host import assert_boundary_is, vcase

pytestmark = pytest.mark.gpu


def _lsm():
    import lsm_amd
    return lsm_amd


def _same(m, v, e, f):
    """elements and interface exactly, vertices bit for bit (csrc/lsm_vol.hip is built with -ffp-contract=off: the device rounds as
    numpy does)"""
    assert m.elements.dtype == np.int64 and m.interface.dtype == np.int64 and m.vertices.dtype == np.float64
    assert m.elements.shape == e.shape and m.interface.shape == f.shape and m.vertices.shape == v.shape
    assert np.array_equal(m.elements, e)
    assert np.array_equal(m.interface, f)
    d = np.abs(m.vertices - v).max() if len(v) else 0.0
    print(f"max |vertex difference| = {d:.3e} over {len(v)} vertices, {len(e)} elements")
    assert np.array_equal(m.vertices, v)


@pytest.mark.parametrize("mode", ["fast", "strict"])
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_device_matches_restatement(name, mode):
    lsm = _lsm()
    n, f, lc, hc = FIELDS[name]
    vals = grid_vals(n, f, lc, hc)
    m = lsm.volume_mesh(_device(lsm, vals, lc, hc, mode))
    v, e, i = V.volume_mesh(vals, lc, hc)
    assert len(e) > 0 and len(i) > 0 and m.level == 0.0 and len(m) == len(e) and m.mesh.n == tuple(n) and m.ndim == len(n)
    _same(m, v, e, i)
    assert m.measure() == pytest.approx(V.measure(v, e), rel=1e-14)


@pytest.mark.parametrize("mode", ["fast", "strict"])
@pytest.mark.parametrize("level", [0.1, -0.07])
def test_levels(level, mode):
    lsm = _lsm()
    vals, lc, hc, _, _ = case("sphere9")
    m = lsm.volume_mesh(_device(lsm, vals, lc, hc, mode), level)
    assert m.level == level
    _same(m, *V.volume_mesh(vals, lc, hc, level=level))


@pytest.mark.parametrize("mode", ["fast", "strict"])
def test_float32_storage(mode):
    lsm = _lsm()
    vals, lc, hc, _, _ = case("sphere17")
    v32 = np.asfortranarray(vals.astype(np.float32))
    m = lsm.volume_mesh(_device(lsm, v32, lc, hc, mode, dtype=np.float32))
    _same(m, *V.volume_mesh(v32.astype(np.float64), lc, hc))


# the smallest shapes at which the rows never line up with the 64 lanes and the chunks of 4096 nodes have seams: 19 chunks, the last
# one partial, in 3-D; three in 2-D
SEAMS = {"sphere_67x33x35": ((67, 33, 35), sphere, (-1.0,) * 3, (1.0,) * 3), "disk_131x67": ((131, 67), disk, (-1.0,) * 2, (1.0,) * 2)}


@pytest.mark.parametrize("name", ["sphere17", "disk17", "sphere_leaving", "plane_diag15", *SEAMS])
def test_interface_is_the_isosurface_of_the_same_field(name):
    lsm = _lsm()
    n, f, lc, hc = {**FIELDS, **SEAMS}[name]
    phi = _device(lsm, grid_vals(n, f, lc, hc), lc, hc)
    vol, iso = lsm.volume_mesh(phi), lsm.isosurface(phi)
    assert vol.interface.shape == iso.elements.shape and len(iso) > 0
    assert np.array_equal(vol.vertices[vol.interface], iso.vertices[iso.elements])


# ----------------------------------------------------------------------------- launch shapes

def test_rows_straddling_waves_and_several_chunks():
    """(67, 33, 35): rows of 67 nodes never line up with the 64 lanes, 19 chunks of 4096 nodes, the last one partial"""
    lsm = _lsm()
    n, lc, hc = (67, 33, 35), (-1.0,) * 3, (1.0,) * 3
    vals = grid_vals(n, sphere, lc, hc)
    m = lsm.volume_mesh(_device(lsm, vals, lc, hc))
    _same(m, *V.volume_mesh(vals, lc, hc))


def _face_keys(elems, nv):
    """every face of every element as one integer key over its sorted vertices, and the face oriented as the boundary of its
    element (test_volume_mesh_host.boundary_faces, without np.unique over rows: these meshes have millions of faces)"""
    N1 = elems.shape[1]
    keys, faces = [], []
    for i in range(N1):
        f = np.delete(elems, i, axis=1)
        if i % 2 == 1:
            f = f[:, [1, 0] + list(range(2, N1 - 1))]
        s = np.sort(f, axis=1)
        k = s[:, 0]
        for c in range(1, N1 - 1):
            k = k * nv + s[:, c]
        keys.append(k)
        faces.append(f)
    return np.concatenate(keys), np.concatenate(faces)


def _independent_checks(lsm, phi, vals):
    m = lsm.volume_mesh(phi)
    nv, N = len(m.vertices), vals.ndim
    assert nv == int(np.count_nonzero(vals < 0)) + count_sign_changes(vals)
    assert nv ** N < 2 ** 63
    keys, faces = _face_keys(m.elements, nv)
    uniq, first, cnt = np.unique(keys, return_index=True, return_counts=True)
    assert cnt.max() <= 2, "a face occurs in more than two elements"
    once = faces[first[cnt == 1]]
    rot = lambda f: f if N == 2 else np.take_along_axis(f, (np.argmin(f, axis=1)[:, None] + np.arange(3)[None, :]) % 3, axis=1)
    as_rows = lambda f: np.unique(rot(f), axis=0)
    assert len(once) == len(m.interface)
    assert np.array_equal(as_rows(once), as_rows(m.interface)), "the boundary of the mesh is not its interface, orientation included"
    vol, enclosed = m.measure(), R.enclosed(m.vertices, m.interface)
    print(f"{nv} vertices, {len(m)} elements, {len(m.interface)} interface elements; Σ volumes = {vol!r}, enclosed = {enclosed!r}")
    assert (V.signed_volumes(m.vertices, m.elements) > 0).all()
    assert vol == pytest.approx(enclosed, rel=1e-12)
    again = lsm.volume_mesh(phi)
    assert np.array_equal(again.vertices, m.vertices) and np.array_equal(again.elements, m.elements)
    assert np.array_equal(again.interface, m.interface)


def test_sphere_129_independent_checks_and_determinism():
    """525 chunks; checked without the restatement"""
    lsm = _lsm()
    n, lc, hc = (129, 129, 129), (-1.0,) * 3, (1.0,) * 3
    vals = grid_vals(n, sphere, lc, hc)
    _independent_checks(lsm, _device(lsm, vals, lc, hc), vals)


def test_disk_1030_by_515_independent_checks():
    """rows of 1030 nodes (more than a workgroup's 256 lanes per pass), 130 chunks"""
    lsm = _lsm()
    n, lc, hc = (1030, 515), (-1.0,) * 2, (1.0,) * 2
    vals = grid_vals(n, disk, lc, hc)
    _independent_checks(lsm, _device(lsm, vals, lc, hc), vals)


# ----------------------------------------------------------------------------- degenerate fields

@pytest.mark.parametrize("N", [2, 3])
def test_all_outside_gives_empty_arrays(N):
    lsm = _lsm()
    vals, lc, hc, _, _ = case("sphere9" if N == 3 else "disk17")
    m = lsm.volume_mesh(_device(lsm, np.asfortranarray(np.abs(vals) + 1.0), lc, hc))
    assert m.vertices.shape == (0, N) and m.elements.shape == (0, N + 1) and m.interface.shape == (0, N)
    assert len(m) == 0 and m.measure() == 0.0


def test_all_inside():
    """N!·cells elements, no interface, Σ = the box.  A device handle needs at least 4 nodes per dimension (lsm_create), so the
    (5, 4, 3) field of the host test cannot exist on the device: (6, 5, 4) is the smallest grid with three different extents"""
    lsm = _lsm()
    n, lc, hc = (6, 5, 4), (0.0, -1.0, 2.0), (2.5, 1.0, 2.75)
    vals = np.full(n, -1.0, order="F")
    m = lsm.volume_mesh(_device(lsm, vals, lc, hc))
    assert len(m.vertices) == 120 and len(m) == 6 * 5 * 4 * 3 and m.interface.shape == (0, 3)
    _same(m, *V.volume_mesh(vals, lc, hc))
    assert (V.signed_volumes(m.vertices, m.elements) > 0).all()
    assert m.measure() == pytest.approx(2.5 * 2.0 * 0.75, rel=1e-13)


# ----------------------------------------------------------------------------- through the API

def test_equation_after_steps_and_stale_ghosts():
    """volume_mesh(eq) is volume_mesh(current_state(eq)); after RK3 steps the ghost layers are stale, and only the interior counts"""
    lsm = _lsm()
    n, lc, hc = (41, 37), (-1.0, -1.0), (1.0, 1.0)
    grid = lsm.CartesianGrid(lc, hc, n)
    ic = lsm.MeshField(lambda x: np.hypot(x[0] - 0.3, x[1] + 0.1) - 0.4, grid)
    eq = lsm.LevelSetEquation(terms=(lsm.AdvectionTerm(lsm.RigidRotation(1.0, (0.0, 0.0)), lsm.WENO5()),), ic=ic, bc=lsm.NeumannBC(),
                              integrator=lsm.RK3())
    lsm.integrate_(eq, 3 * 0.5 * eq.compute_cfl(0.0))       # three RK3 steps
    assert eq.current_time() > 0
    a, b = lsm.volume_mesh(eq), lsm.volume_mesh(eq.current_state())
    assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("vertices", "elements", "interface"))
    v, e, i = V.volume_mesh(eq.current_state().values(), lc, hc)
    _same(a, v, e, i)
    assert_boundary_is(v, e, i)
    assert "DomainMesh in ℝ²" in repr(a) and f"{len(e)} triangles" in repr(a)


def _parse_medit(path):
    """{section: int rows} and the vertex rows as text, of a Medit file with one record per line"""
    lines = open(path).read().split("\n")
    assert lines[0] == "MeshVersionFormatted 1" and lines[-3:] == ["", "End", ""]
    dim = int(lines[1].split()[1])
    sections, k = {}, 2
    while lines[k + 1] != "End":
        assert lines[k] == ""
        name, count = lines[k + 1], int(lines[k + 2])
        sections[name] = [ln.split() for ln in lines[k + 3:k + 3 + count]]
        k += 3 + count
    return dim, sections


@pytest.mark.parametrize("name", ["sphere9", "disk17"])
def test_export_volume_mesh_round_trip(tmp_path, name):
    lsm = _lsm()
    vals, lc, hc, v, e, i = vcase(name)
    N = vals.ndim
    out = str(tmp_path / "domain.mesh")
    assert lsm.export_volume_mesh(_device(lsm, vals, lc, hc), out) == out
    dim, sec = _parse_medit(out)
    assert dim == N and list(sec) == (["Vertices", "Triangles", "Edges"] if N == 2 else ["Vertices", "Tetrahedra", "Triangles"])
    rows = sec["Vertices"]
    assert all(len(r) == N + 1 and r[N] == "1" for r in rows)
    assert np.array_equal(np.array([[float(x) for x in r[:N]] for r in rows]), v)       # shortest round-trip digits
    el = np.array(sec["Tetrahedra" if N == 3 else "Triangles"], dtype=np.int64)
    fa = np.array(sec["Triangles" if N == 3 else "Edges"], dtype=np.int64)
    assert el.shape == (len(e), N + 2) and (el[:, -1] == 3).all() and fa.shape == (len(i), N + 1) and (fa[:, -1] == 10).all()
    assert el[:, :-1].min() == 1 and el[:, :-1].max() == len(v)
    assert np.array_equal(el[:, :-1] - 1, e) and np.array_equal(fa[:, :-1] - 1, i)


# ----------------------------------------------------------------------------- refusals

def test_export_volume_mesh_refusals(tmp_path):
    lsm = _lsm()
    out = str(tmp_path / "domain.mesh")
    vals, lc, hc, _, _ = case("disk17")
    phi = _device(lsm, vals, lc, hc)
    for kw in ("hgrad", "hmin", "hmax", "hausd"):
        with pytest.raises(NotImplementedError, match="mmg2d_O3 / mmg3d_O3"):
            lsm.export_volume_mesh(phi, out, **{kw: 0.01})
    grid = lsm.CartesianGrid((0.0,), (1.0,), (17,))
    one = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(lambda x: x[0] - 0.4, grid), bc=lsm.NeumannBC())
    with pytest.raises(ValueError, match="export_mesh of 1 dimensional level-set not supported."):
        lsm.export_volume_mesh(one, out)


def test_refusals():
    lsm = _lsm()
    with pytest.raises(TypeError, match="device field"):
        lsm.volume_mesh(np.zeros((4, 4)))
    vals, lc, hc, _, _ = case("sphere9")
    phi = _device(lsm, vals, lc, hc)
    with pytest.raises(TypeError, match="device buffer"):
        phi.backend.vol_create(vals, None, 0.0)              # a host array never reaches the library
    grid = lsm.CartesianGrid((0.0,), (1.0,), (17,))
    one = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(lambda x: x[0] - 0.4, grid), bc=lsm.NeumannBC())
    with pytest.raises(ValueError, match="1 dimensional"):
        lsm.volume_mesh(one)
    with pytest.raises(lsm.LsmError, match="lsm_vol_create: a 1-dimensional"):
        one.backend.vol_create(one.current_state().buf, None, 0.0)
    for level in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            lsm.volume_mesh(phi, level)
        with pytest.raises(lsm.LsmError, match="lsm_vol_create: level must be finite"):
            phi.backend.vol_create(phi.buf, None, level)
    # a band does not hold the interior
    nb = _device(lsm, vals, lc, hc, band=3)
    assert isinstance(nb, lsm.ROCNarrowBandMeshField)
    with pytest.raises(ValueError, match="does not hold the interior"):
        lsm.volume_mesh(nb)
    with pytest.raises(lsm.LsmError, match="lsm_vol_create: a narrow band"):
        nb.backend.vol_create(nb.buf, nb.mask, 0.0)
    # a slab handle: a rank of an in-process group
    g = lsm.LocalGroup(1)
    grid3 = lsm.CartesianGrid(lc, hc, vals.shape)
    slab = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(vals, grid3), bc=lsm.NeumannBC(), comm=g.rank(0))
    with pytest.raises(ValueError, match="slab"):
        lsm.volume_mesh(slab)
    with pytest.raises(lsm.LsmError, match="slab of a decomposed grid"):
        slab.backend.vol_create(slab.current_state().buf, None, 0.0)


def test_slab_handles_with_a_communicator_are_refused_by_the_library():
    lsm = _lsm()
    from test_gpu_comm import _run_ranks
    vals, lc, hc, _, _ = case("sphere17")
    grid = lsm.CartesianGrid(lc, hc, vals.shape)

    def body(r, comm):
        eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(vals, grid), bc=lsm.NeumannBC(), comm=comm)
        with pytest.raises(ValueError, match="slab"):
            lsm.volume_mesh(eq)
        b, buf = eq.backend, eq.current_state().buf
        with pytest.raises(lsm.LsmError, match="slab of a decomposed grid"):
            b.vol_create(buf, None, 0.0)
        # the library itself refuses a handle with a communicator
        out, cnt = ctypes.c_void_p(), (ctypes.c_int64 * 3)()
        code = b.lib.lsm_vol_create(b.h, b.ptr(buf), None, 0.0, ctypes.byref(out), cnt)
        assert code != 0 and not out.value
        assert b"lsm_vol_create: the handle has a communicator attached" in b.lib.lsm_last_error(b.h)
        return True

    assert _run_ranks(lsm, 2, body, timeout=60) == [True, True]
