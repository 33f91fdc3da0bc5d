"""isosurface on the device (csrc/lsm_iso.hip, lsm_iso_* through the Python API) against the restatement tests/_iso_ref.py:
elements exactly, vertices bit for bit; narrow bands; launch shapes where rows straddle waves and chunks are partial or several,
checked by facts that do not come from the restatement; the API, export_surface_mesh and the refusals."""
import math

import numpy as np
import pytest

import _iso_ref as R
from test_isosurface_host import (CASES, DISK_R, PLANES, SPHERE_R, assert_closed_curve, assert_closed_surface, case,
                                  count_sign_changes, disk, grid_vals, sphere)

pytestmark = pytest.mark.gpu


def _lsm():
    import lsm_amd
    return lsm_amd


def _device(lsm, vals, lc, hc, mode="fast", dtype=None, band=None):
    grid = lsm.CartesianGrid(lc, hc, vals.shape)
    mf = lsm.MeshField(vals, grid, dtype=dtype)
    ic = mf if band is None else lsm.NarrowBandMeshField(mf, nlayers=band)
    return lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=ic, bc=lsm.NeumannBC(), mode=mode).current_state()


def _same(m, v, e):
    """elements exactly, vertices bit for bit (csrc/lsm_iso.hip is built with -ffp-contract=off: the device rounds as numpy does)"""
    assert m.elements.dtype == np.int64 and m.vertices.dtype == np.float64
    assert m.elements.shape == e.shape and m.vertices.shape == v.shape
    assert np.array_equal(m.elements, e)
    d = np.abs(m.vertices - v).max() if len(v) else 0.0
    print(f"max |vertex difference| = {d:.3e} over {len(v)} vertices")
    assert np.array_equal(m.vertices, v)


FIELDS = {
    **{k: CASES[k] for k in ("sphere9", "sphere17", "torus", "disk17")},
    "sphere_leaving": ((11, 10, 9), lambda X: np.sqrt((X[0] - 0.7) ** 2 + X[1] ** 2 + X[2] ** 2) - 0.6, (-1.0,) * 3, (1.0,) * 3),
    "disk_leaving": ((19, 17), lambda X: np.hypot(X[0] - 0.71, X[1] + 0.43) - 0.61, (-1.0,) * 2, (1.0,) * 2),
    **{"plane_" + k: (n, f, (0.0,) * 3, (1.0,) * 3) for k, (n, f, _) in PLANES.items()},
}


@pytest.mark.parametrize("mode", ["fast", "strict"])
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_device_matches_restatement(name, mode):
    lsm = _lsm()
    n, f, lc, hc = FIELDS[name]
    vals = grid_vals(n, f, lc, hc)
    m = lsm.isosurface(_device(lsm, vals, lc, hc, mode))
    v, e = R.isosurface(vals, lc, hc)
    assert len(e) > 0 and m.level == 0.0 and len(m) == len(e) and m.mesh.n == tuple(n)
    _same(m, v, e)
    assert m.measure() == pytest.approx(R.measure(v, e), rel=1e-14)


@pytest.mark.parametrize("mode", ["fast", "strict"])
@pytest.mark.parametrize("level", [0.1, -0.07])
def test_levels(level, mode):
    lsm = _lsm()
    vals, lc, hc, _, _ = case("sphere9")
    m = lsm.isosurface(_device(lsm, vals, lc, hc, mode), level)
    assert m.level == level
    _same(m, *R.isosurface(vals, lc, hc, level=level))


@pytest.mark.parametrize("mode", ["fast", "strict"])
def test_float32_storage(mode):
    lsm = _lsm()
    vals, lc, hc, _, _ = case("sphere17")
    v32 = np.asfortranarray(vals.astype(np.float32))
    m = lsm.isosurface(_device(lsm, v32, lc, hc, mode, dtype=np.float32))
    _same(m, *R.isosurface(v32.astype(np.float64), lc, hc))


@pytest.mark.parametrize("N", [2, 3])
def test_no_interface_gives_empty_arrays(N):
    lsm = _lsm()
    vals, lc, hc, _, _ = case("sphere9" if N == 3 else "disk17")
    m = lsm.isosurface(_device(lsm, np.asfortranarray(np.abs(vals) + 1.0), lc, hc))
    assert m.vertices.shape == (0, N) and m.elements.shape == (0, N) and len(m) == 0 and m.measure() == 0.0


# ----------------------------------------------------------------------------- narrow bands

def _set_band(phi, mask, garbage=None):
    """replace the device band's byte mask by `mask` (interior, bool); garbage: values written off the band"""
    import torch
    b = phi.backend
    lay, n = b.lay, mask.shape
    flat = np.zeros(int(lay.total), dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(flat[int(lay.origin):], shape=n, strides=tuple(int(lay.stride[d]) for d in range(len(n))))
    view[...] = mask
    phi.mask.copy_(torch.from_numpy(flat).to(phi.mask.device))
    if garbage is not None:
        vals = b.download(phi.buf)
        vals[~mask] = garbage[~mask]
        b.upload(phi.buf, vals)


def test_band_holding_every_cut_cell_equals_dense():
    lsm = _lsm()
    vals, lc, hc, v, e = case("sphere17")
    nb = _device(lsm, vals, lc, hc, band=3)
    assert isinstance(nb, lsm.ROCNarrowBandMeshField)
    _same(lsm.isosurface(nb), v, e)
    _set_band(nb, np.abs(vals) < 0.3)
    _same(lsm.isosurface(nb), v, e)


def test_thin_band_reads_band_values_only():
    """|ϕ| < 0.12 drops cells the surface crosses: the mesh of the band's active cells, every vertex referenced; the values off
    the band (scratch on the device) are overwritten and must not matter"""
    lsm = _lsm()
    vals, lc, hc, _, e_dense = case("sphere17")
    mask = np.abs(vals) < 0.12
    nb = _device(lsm, vals, lc, hc, band=3)
    rng = np.random.default_rng(7)
    _set_band(nb, mask, garbage=rng.choice([-7.0, 7.0], size=vals.shape))
    m = lsm.isosurface(nb)
    v, e = R.isosurface(vals, lc, hc, mask=mask)
    assert 0 < len(e) < len(e_dense)
    _same(m, v, e)
    assert np.array_equal(np.unique(m.elements), np.arange(len(m.vertices)))


def test_band_2d():
    lsm = _lsm()
    vals, lc, hc, v, e = case("disk33")
    nb = _device(lsm, vals, lc, hc, band=2)
    _same(lsm.isosurface(nb), v, e)
    mask = np.abs(vals) < 0.05
    _set_band(nb, mask)
    _same(lsm.isosurface(nb), *R.isosurface(vals, lc, hc, mask=mask))


# ----------------------------------------------------------------------------- launch shapes

def test_rows_straddling_waves_and_several_chunks():
    """(67, 33, 35): rows of 67 nodes never line up with the 64 lanes, 19 chunks of 4096 nodes, the last one partial"""
    lsm = _lsm()
    n, lc, hc = (67, 33, 35), (-1.0,) * 3, (1.0,) * 3
    vals = grid_vals(n, sphere, lc, hc)
    m = lsm.isosurface(_device(lsm, vals, lc, hc))
    _same(m, *R.isosurface(vals, lc, hc))


def test_sphere_129_independent_checks_and_determinism():
    """525 chunks; checked without the restatement.  The area error is second order: 0.0037 on the 33-grid (h = 2/32), so at
    h = 2/128 at most 0.0037·(32/128)², with a margin of 1.5"""
    lsm = _lsm()
    n, lc, hc = (129, 129, 129), (-1.0,) * 3, (1.0,) * 3
    vals = grid_vals(n, sphere, lc, hc)
    phi = _device(lsm, vals, lc, hc)
    m = lsm.isosurface(phi)
    assert len(m.vertices) == count_sign_changes(vals)
    assert_closed_surface(m.vertices, m.elements, 2)
    assert R.enclosed(m.vertices, m.elements) > 0
    err = m.measure() / (4 * math.pi * SPHERE_R ** 2) - 1
    print(f"relative area error at 129^3: {err:.3e}")
    assert -0.0037 * (32 / 128) ** 2 * 1.5 <= err < 0
    again = lsm.isosurface(phi)
    assert np.array_equal(again.vertices, m.vertices) and np.array_equal(again.elements, m.elements)


def test_disk_1030_by_515_independent_checks():
    """rows of 1030 nodes (more than a workgroup's 256 lanes per pass), 130 chunks.  The length error is second order in the
    coarser spacing: 7.0e-4 on the 33-grid (h = 2/32), so with h_y = 2/514 at most 7.0e-4·(32/514)², with a margin of 1.5"""
    lsm = _lsm()
    n, lc, hc = (1030, 515), (-1.0,) * 2, (1.0,) * 2
    vals = grid_vals(n, disk, lc, hc)
    phi = _device(lsm, vals, lc, hc)
    m = lsm.isosurface(phi)
    assert len(m.vertices) == count_sign_changes(vals)
    assert_closed_curve(m.vertices, m.elements)
    assert R.enclosed(m.vertices, m.elements) > 0
    err = m.measure() / (2 * math.pi * DISK_R) - 1
    print(f"relative length error at 1030 x 515: {err:.3e}")
    assert -7.0e-4 * (32 / 514) ** 2 * 1.5 <= err < 0
    again = lsm.isosurface(phi)
    assert np.array_equal(again.vertices, m.vertices) and np.array_equal(again.elements, m.elements)


def _loops(elems):
    """the number of cycles of the map start vertex -> end vertex of the segments (a closed curve: a permutation)"""
    nxt = np.empty(len(elems), dtype=np.int64)
    nxt[elems[:, 0]] = elems[:, 1]
    seen, count = np.zeros(len(elems), dtype=bool), 0
    for v in range(len(elems)):
        if not seen[v]:
            count += 1
            while not seen[v]:
                seen[v] = True
                v = nxt[v]
    return count


def test_chunk_sums_of_more_than_8192_chunks():
    """(4097, 8194) nodes, 8197 chunks: the scan of the three rows of chunk sums (csrc/scan.h; volume_mesh shares it) runs a second
    round, which receives a carry.  Two circles of radius 8.48 nodes, one in rows 1..18 and one in rows 8175..8192, on a
    field that is 3 elsewhere (h = 1, float32 storage).  Checked without the restatement: every vertex is the start of one segment
    and the end of one, the segments form two loops, the elements come ascending by their cell, and the length is that of the two
    circles to second order: h/r is the 33-grid's of test_disk_1030_by_515_independent_checks (h = 2/32, r = 0.53), whose 7.0e-4
    with its margin of 1.5 is the bound.  A dropped carry puts the vertices, elements and list entries of chunk 8192 and beyond on
    top of the first circle's, or loses them from the totals."""
    import _chunk_carry as CC
    lsm = _lsm()
    n, r = CC.N, DISK_R / (2 / 32)
    vals = np.full(n, 3.0, dtype=np.float32, order="F")
    windows = []
    for cx, cy in ((1500.3, 9.6), (2901.6, n[1] - 1 - 9.3)):
        i0, i1, j0, j1 = int(cx) - 13, int(cx) + 15, max(int(cy) - 13, 0), min(int(cy) + 15, n[1])
        X, Y = np.meshgrid(np.arange(i0, i1), np.arange(j0, j1), indexing="ij")
        vals[i0:i1, j0:j1] = np.minimum(3.0, np.hypot(X - cx, Y - cy) - r)
        windows.append((i0, i1, j0, j1))
    assert all((vals[a:b, c:d] != 0.0).all() for a, b, c, d in windows)
    m = lsm.isosurface(_device(lsm, vals, (0.0, 0.0), tuple(float(k - 1) for k in n), dtype=np.float32))
    v, e = m.vertices, m.elements
    assert len(v) == sum(count_sign_changes(vals[a:b, c:d]) for a, b, c, d in windows) and len(e) == len(v) > 0
    assert e.min() == 0 and e.max() == len(v) - 1
    assert_closed_curve(v, e)
    assert _loops(e) == 2
    assert R.enclosed(v, e) > 0
    mid = 0.5 * (v[e[:, 0]] + v[e[:, 1]])                 # inside the segment's cell: h = 1, the lower corner at 0
    cell = np.floor(mid).astype(np.int64)
    owner = cell[:, 0] + n[0] * cell[:, 1]
    assert (np.diff(owner) >= 0).all()
    chunk = owner // CC.CHUNK
    print(f"{len(v)} vertices; {int((chunk < 20).sum())} elements in chunks below 20, {int((chunk >= CC.SCAN).sum())} in chunks from {CC.SCAN}")
    assert (chunk < 20).any() and (chunk >= CC.SCAN).any()
    err = m.measure() / (2 * 2 * math.pi * r) - 1
    print(f"relative length error of the two circles: {err:.3e}")
    assert -7.0e-4 * 1.5 <= err < 0


# ----------------------------------------------------------------------------- through the API

def test_equation_after_steps_and_stale_ghosts():
    """isosurface(eq) is isosurface(current_state(eq)); after RK3 steps the ghost layers are stale, and only the interior counts"""
    lsm = _lsm()
    n, lc, hc = (41, 37), (-1.0, -1.0), (1.0, 1.0)
    grid = lsm.CartesianGrid(lc, hc, n)
    ic = lsm.MeshField(lambda x: np.hypot(x[0] - 0.3, x[1] + 0.1) - 0.4, grid)
    eq = lsm.LevelSetEquation(terms=(lsm.AdvectionTerm(lsm.RigidRotation(1.0, (0.0, 0.0)), lsm.WENO5()),), ic=ic, bc=lsm.NeumannBC(),
                              integrator=lsm.RK3())
    lsm.integrate_(eq, 3 * 0.5 * eq.compute_cfl(0.0))       # three RK3 steps
    assert eq.current_time() > 0
    a, b = lsm.isosurface(eq), lsm.isosurface(eq.current_state())
    assert np.array_equal(a.vertices, b.vertices) and np.array_equal(a.elements, b.elements)
    _same(a, *R.isosurface(eq.current_state().values(), lc, hc))
    assert_closed_curve(a.vertices, a.elements)


def test_export_surface_mesh_round_trip(tmp_path):
    lsm = _lsm()
    vals, lc, hc, v, e = case("sphere9")
    phi = _device(lsm, vals, lc, hc)
    out = str(tmp_path / "sphere.mesh")
    assert lsm.export_surface_mesh(phi, out) == out
    lines = open(out).read().split("\n")
    assert lines[:5] == ["MeshVersionFormatted 1", "Dimension 3", "", "Vertices", str(len(v))]
    rows = [ln.split() for ln in lines[5:5 + len(v)]]
    assert all(r[3] == "1" for r in rows)
    assert np.array_equal(np.array([[float(x) for x in r[:3]] for r in rows]), v)       # shortest round-trip digits
    k = 5 + len(v)
    assert lines[k:k + 3] == ["", "Triangles", str(len(e))]
    tri = np.array([[int(x) for x in ln.split()] for ln in lines[k + 3:k + 3 + len(e)]])
    assert tri.shape == (len(e), 4) and (tri[:, 3] == 1).all()
    assert tri[:, :3].min() == 1 and tri[:, :3].max() == len(v)
    assert np.array_equal(tri[:, :3] - 1, e)
    assert lines[k + 3 + len(e):] == ["", "End", ""]
    with pytest.raises(NotImplementedError, match="mmgs"):
        lsm.export_surface_mesh(phi, out, hausd=0.01)
    vals2, lc2, hc2, _, _ = case("disk17")
    with pytest.raises(ValueError, match="export_mesh of 2 dimensional level-set not supported."):
        lsm.export_surface_mesh(_device(lsm, vals2, lc2, hc2), out)


def test_refusals():
    lsm = _lsm()
    with pytest.raises(TypeError, match="device field"):
        lsm.isosurface(np.zeros((4, 4)))
    grid = lsm.CartesianGrid((0.0,), (1.0,), (17,))
    one = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(lambda x: x[0] - 0.4, grid), bc=lsm.NeumannBC())
    with pytest.raises(ValueError, match="1 dimensional"):
        lsm.isosurface(one)
    b = one.backend
    with pytest.raises(lsm.LsmError, match="1-dimensional"):
        b.iso_create(one.current_state().buf, None, 0.0)
    vals, lc, hc, _, _ = case("sphere9")
    phi = _device(lsm, vals, lc, hc)
    for level in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            lsm.isosurface(phi, level)
        with pytest.raises(lsm.LsmError, match="finite"):
            phi.backend.iso_create(phi.buf, None, level)
    # a slab handle: a rank of an in-process group
    g = lsm.LocalGroup(1)
    grid3 = lsm.CartesianGrid(lc, hc, vals.shape)
    slab = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(vals, grid3), bc=lsm.NeumannBC(), comm=g.rank(0))
    with pytest.raises(ValueError, match="slab"):
        lsm.isosurface(slab)


def test_slab_handles_with_a_communicator_are_refused_by_the_library():
    lsm = _lsm()
    from test_gpu_comm import _run_ranks
    vals, lc, hc, _, _ = case("sphere17")
    grid = lsm.CartesianGrid(lc, hc, vals.shape)

    def body(r, comm):
        eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(vals, grid), bc=lsm.NeumannBC(), comm=comm)
        with pytest.raises(ValueError, match="slab"):
            lsm.isosurface(eq)
        with pytest.raises(lsm.LsmError, match="lsm_iso_create"):
            eq.backend.iso_create(eq.current_state().buf, None, 0.0)
        return True

    assert _run_ranks(lsm, 2, body, timeout=60) == [True, True]
