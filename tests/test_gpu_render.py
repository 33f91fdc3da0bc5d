"""render on the device (csrc/lsm_render.hip, lsm_render_* through the Python API) against the restatement tests/_render_ref.py:
hit masks, classes and colours exactly, depths and normals bit for bit; image shapes with partial tiles, a single tile, a single
pixel and rows shorter than a wave; cameras on grid planes, in the box, in the body and looking away; the identity of the picture
with and without brick skipping; narrow bands with garbage off the band; the Renderer, record_ and the refusals."""
import functools

import numpy as np
import pytest

import _render_ref as R
from test_gpu_isosurface import _set_band
from test_isosurface_host import CASES, PLANES, grid_vals
from test_render_host import _decode_png, _sphere

pytestmark = pytest.mark.gpu


def _lsm():
    import lsm_amd
    return lsm_amd


def _device(lsm, vals, lc, hc, mode="fast", dtype=None, band=None):
    grid = lsm.CartesianGrid(lc, hc, vals.shape)
    mf = lsm.MeshField(vals, grid, dtype=dtype)
    ic = mf if band is None else lsm.NarrowBandMeshField(mf, nlayers=band)
    return lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=ic, bc=lsm.NeumannBC(), mode=mode).current_state()


def _vec(cam, W, H):
    return R.camera_vectors(cam.eye, cam.lookat, cam.up, cam.fov, cam.orthographic, W, H)


def _same3(img, ref):
    """hit mask and colours exactly, depth and normal bit for bit (csrc/lsm_render.hip is built with -ffp-contract=off and uses
    only + − × / sqrt and floor: the device rounds as numpy does)"""
    rgba, depth, normal = ref
    assert img.rgba.dtype == np.uint8 and img.depth.dtype == np.float64 and img.normal.dtype == np.float64
    assert img.rgba.shape == rgba.shape and img.depth.shape == depth.shape and img.normal.shape == normal.shape
    hit = np.isfinite(depth)
    assert np.array_equal(np.isfinite(img.depth), hit) and not np.isnan(img.depth).any()
    dd = np.abs(img.depth[hit] - depth[hit]).max() if hit.any() else 0.0
    dn = np.abs(img.normal - normal).max()
    dc = np.abs(img.rgba.astype(int) - rgba.astype(int)).max()
    print(f"{int(hit.sum())} of {hit.size} rays hit; max |depth difference| = {dd:.3e}, |normal difference| = {dn:.3e}, |colour difference| = {dc}")
    assert np.array_equal(img.depth, depth)
    assert np.array_equal(img.normal, normal)
    assert np.array_equal(img.rgba, rgba)


def _same2(img, ref):
    rgba, cls = ref
    assert img.cls.dtype == np.uint8 and img.cls.shape == cls.shape and img.depth is None and img.normal is None
    print(f"classes differ at {int((img.cls != cls).sum())} of {cls.size} pixels")
    assert np.array_equal(img.cls, cls)
    assert np.array_equal(img.rgba, rgba)


UNIT = ((0.0,) * 3, (1.0,) * 3)
FIELDS = {
    **{k: CASES[k] for k in ("sphere17", "torus")},
    "sphere_leaving": ((11, 10, 9), lambda X: np.sqrt((X[0] - 0.7) ** 2 + X[1] ** 2 + X[2] ** 2) - 0.6, (-1.0,) * 3, (1.0,) * 3),
    **{"plane_" + k: (n, f, *UNIT) for k, (n, f, _) in PLANES.items()},
}


@functools.lru_cache(maxsize=None)
def field(name):
    n, f, lc, hc = FIELDS[name]
    vals = grid_vals(n, f, lc, hc)
    vals.setflags(write=False)
    return vals, lc, hc


def _cameras(lsm, lc, hc):
    c = tuple(0.5 * (a + b) for a, b in zip(lc, hc))
    size = max(b - a for a, b in zip(lc, hc))
    eye = tuple(ci + size * e for ci, e in zip(c, (1.0, 0.75, 0.6)))
    return {"perspective": lsm.Camera(eye, c, fov=35.0), "orthographic": lsm.Camera(eye, c, orthographic=1.1 * size)}


@functools.lru_cache(maxsize=None)
def reference(name, kind, W, H, level=0.0):
    """the restatement's picture of a named field: computed once, shared, never modified"""
    vals, lc, hc = field(name)
    ref = R.render3d(vals, lc, hc, _vec(_cameras(_lsm(), lc, hc)[kind], W, H), W, H, level=level)
    for a in ref:
        a.setflags(write=False)
    return ref


@pytest.mark.parametrize("mode", ["fast", "strict"])
@pytest.mark.parametrize("kind", ["perspective", "orthographic"])
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_device_matches_restatement(name, kind, mode):
    lsm = _lsm()
    vals, lc, hc = field(name)
    img = lsm.render(_device(lsm, vals, lc, hc, mode), _cameras(lsm, lc, hc)[kind], (33, 25))
    ref = reference(name, kind, 33, 25)
    assert 0 < np.isfinite(ref[1]).sum() < 33 * 25
    _same3(img, ref)


@pytest.mark.parametrize("size", [(16, 16), (1, 1), (64, 3)])
def test_image_sizes(size):
    lsm = _lsm()
    vals, lc, hc = field("sphere17")
    img = lsm.render(_device(lsm, vals, lc, hc), _cameras(lsm, lc, hc)["perspective"], size)
    assert img.size == size
    _same3(img, reference("sphere17", "perspective", *size))


@pytest.mark.parametrize("mode", ["fast", "strict"])
@pytest.mark.parametrize("level", [0.1, -0.07])
def test_levels(level, mode):
    lsm = _lsm()
    vals, lc, hc = field("sphere17")
    img = lsm.render(_device(lsm, vals, lc, hc, mode), _cameras(lsm, lc, hc)["perspective"], (33, 25), level=level)
    _same3(img, reference("sphere17", "perspective", 33, 25, level))


@pytest.mark.parametrize("mode", ["fast", "strict"])
def test_float32_storage(mode):
    lsm = _lsm()
    vals, lc, hc = field("sphere17")
    v32 = np.asfortranarray(vals.astype(np.float32))
    cam = _cameras(lsm, lc, hc)["perspective"]
    img = lsm.render(_device(lsm, v32, lc, hc, mode, dtype=np.float32), cam, (33, 25))
    _same3(img, R.render3d(v32.astype(np.float64), lc, hc, _vec(cam, 33, 25), 33, 25))


def test_a_nan_node_makes_its_cells_void():
    lsm = _lsm()
    vals, lc, hc = field("sphere17")
    vals = vals.copy(order="F")
    vals[11, 9, 8] = np.nan                 # a node near the surface on the camera's side
    for kind, cam in _cameras(lsm, lc, hc).items():
        ref = R.render3d(vals, lc, hc, _vec(cam, 33, 25), 33, 25)
        assert not np.array_equal(ref[1], reference("sphere17", kind, 33, 25)[1])
        _same3(lsm.render(_device(lsm, vals, lc, hc), cam, (33, 25)), ref)


def test_style_reaches_the_device():
    lsm = _lsm()
    vals, lc, hc = field("torus")
    cam = _cameras(lsm, lc, hc)["perspective"]
    style = dict(color=(200, 90, 10), background=(3, 2, 1), ambient=0.6, step=0.8, bisections=2)
    _same3(lsm.render(_device(lsm, vals, lc, hc), cam, (33, 25), **style), R.render3d(vals, lc, hc, _vec(cam, 33, 25), 33, 25, **style))
    style = dict(step=0.3, bisections=0)
    _same3(lsm.render(_device(lsm, vals, lc, hc), cam, (33, 25), **style), R.render3d(vals, lc, hc, _vec(cam, 33, 25), 33, 25, **style))


# ----------------------------------------------------------------------------- cameras

def test_axis_aligned_orthographic_camera_with_origins_on_grid_planes():
    """d = (0, 0, −1) exactly and ray origins at x = ±0.125·odd, on grid planes of the 17-node axis: zero direction components
    must not make a NaN; a window as wide as the box puts the outermost origins half a pixel inside it"""
    lsm = _lsm()
    vals, lc, hc = field("sphere17")
    cam = lsm.Camera((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), orthographic=2.0)
    v = _vec(cam, 8, 8)
    o, d = R.rays(v, 8, 8)
    assert np.array_equal(d, np.tile((0.0, 0.0, -1.0), (64, 1))) and np.array_equal(np.unique(o[:, 0]), 0.125 * np.arange(-7, 8, 2))
    img = lsm.render(_device(lsm, vals, lc, hc), cam, (8, 8))
    assert not np.isnan(img.depth).any() and not np.isnan(img.normal).any()
    _same3(img, R.render3d(vals, lc, hc, v, 8, 8))
    # origins on the faces of the box
    cam = lsm.Camera((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), orthographic=4.0)
    _same3(lsm.render(_device(lsm, vals, lc, hc), cam, (4, 4)), R.render3d(vals, lc, hc, _vec(cam, 4, 4), 4, 4))


def test_cameras_in_the_box_in_the_body_and_looking_away():
    lsm = _lsm()
    vals, lc, hc = field("sphere17")
    phi = _device(lsm, vals, lc, hc)
    r = lsm.Renderer(phi)
    in_box = lsm.Camera((0.9, 0.8, 0.7), (0.0, 0.0, 0.0))
    img = r.draw(in_box, (33, 25))
    assert 0 < np.isfinite(img.depth).sum()
    _same3(img, R.render3d(vals, lc, hc, _vec(in_box, 33, 25), 33, 25))
    in_body = lsm.Camera((0.05, -0.08, 0.03), (1.0, 0.0, 0.0))
    img = r.draw(in_body, (16, 16))
    assert np.array_equal(img.depth, np.zeros((16, 16)))
    _same3(img, R.render3d(vals, lc, hc, _vec(in_body, 16, 16), 16, 16))
    away = lsm.Camera((3.0, 0.0, 0.0), (5.0, 0.0, 0.0))
    img = r.draw(away, (16, 16))
    assert np.isinf(img.depth).all() and (img.normal == 0).all() and (img.rgba == 255).all()
    r.close()


# ----------------------------------------------------------------------------- skipping

SKIP_FIELDS = {
    "small_sphere": _sphere((0.3, -0.2, 0.1), 0.2),
    "thin_shell": lambda X: np.abs(np.sqrt(X[0] ** 2 + X[1] ** 2 + X[2] ** 2) - 0.5) - 0.03,
}


@pytest.mark.parametrize("kind", ["perspective", "orthographic"])
@pytest.mark.parametrize("name", sorted(SKIP_FIELDS))
def test_the_picture_is_identical_with_and_without_skipping(name, kind):
    """43³: five whole bricks and a partial one per axis.  The identity of the two pictures is the correctness argument of the
    skipping; both equal the restatement, which samples every lattice point"""
    lsm = _lsm()
    lc, hc = (-1.0,) * 3, (1.0,) * 3
    vals = grid_vals((43,) * 3, SKIP_FIELDS[name], lc, hc)
    phi = _device(lsm, vals, lc, hc)
    cam = _cameras(lsm, lc, hc)[kind]
    r = lsm.Renderer(phi)
    state, uniform = r.bricks()
    raw, uni = R.bricks(vals)
    assert state.shape == (6, 6, 6) and np.array_equal(state, raw) and np.array_equal(uniform, uni)
    print(f"{int(uniform.sum())} of {uniform.size} bricks are uniform")
    if name == "small_sphere":
        assert uniform.sum() > uniform.size // 2          # 152 of 216 by the restatement: skipping has something to skip
    else:
        assert uniform.any() and (state == R.IN).sum() == 0
    b = phi.backend
    assert b.get_tuning("LSM_RENDER_SKIP") == 1
    on = r.draw(cam, (33, 25))
    b.set_tuning("LSM_RENDER_SKIP", 0)
    try:
        off = r.draw(cam, (33, 25))
    finally:
        b.set_tuning("LSM_RENDER_SKIP", 1)
    r.close()
    assert np.array_equal(on.depth, off.depth) and np.array_equal(on.normal, off.normal) and np.array_equal(on.rgba, off.rgba)
    ref = R.render3d(vals, lc, hc, _vec(cam, 33, 25), 33, 25)
    assert 0 < np.isfinite(ref[1]).sum() < 33 * 25
    _same3(on, ref)
    _same3(off, ref)


# ----------------------------------------------------------------------------- narrow bands

def _garbage(shape):
    return np.random.default_rng(7).choice([1e30, -1e30, np.nan], size=shape)


def test_band_3d_reads_band_values_only():
    lsm = _lsm()
    vals, lc, hc = field("sphere17")
    cam = _cameras(lsm, lc, hc)["perspective"]
    nb = _device(lsm, vals, lc, hc, band=3)
    assert isinstance(nb, lsm.ROCNarrowBandMeshField)
    mask = np.abs(vals) < 0.3
    _set_band(nb, mask)
    clean = lsm.render(nb, cam, (33, 25))
    _set_band(nb, mask, garbage=_garbage(vals.shape))
    dirty = lsm.render(nb, cam, (33, 25))
    assert np.array_equal(clean.depth, dirty.depth) and np.array_equal(clean.normal, dirty.normal) and np.array_equal(clean.rgba, dirty.rgba)
    _same3(dirty, R.render3d(vals, lc, hc, _vec(cam, 33, 25), 33, 25, mask=mask))
    # the band holds the surface: the rays that hit are the dense field's
    assert np.array_equal(np.isfinite(dirty.depth), np.isfinite(reference("sphere17", "perspective", 33, 25)[1]))
    # a thin band drops cells the surface crosses
    thin = np.abs(vals) < 0.1
    _set_band(nb, thin, garbage=_garbage(vals.shape))
    ref = R.render3d(vals, lc, hc, _vec(cam, 33, 25), 33, 25, mask=thin)
    assert 0 < np.isfinite(ref[1]).sum() < np.isfinite(clean.depth).sum()
    _same3(lsm.render(nb, cam, (33, 25)), ref)


def test_band_2d_reads_band_values_only():
    lsm = _lsm()
    n, f, lc, hc = CASES["disk33"]
    vals = grid_vals(n, f, lc, hc)
    nb = _device(lsm, vals, lc, hc, band=3)
    mask = nb.active_mask()
    ref = R.render2d(vals, lc, hc, 57, 41, mask=mask)
    assert set(np.unique(ref[1])) == {2, 3, 4, 5}
    _same2(lsm.render(nb, size=(57, 41)), ref)
    mask = np.abs(vals) < 0.2
    _set_band(nb, mask, garbage=_garbage(vals.shape))
    _same2(lsm.render(nb, size=(57, 41)), R.render2d(vals, lc, hc, 57, 41, mask=mask))


# ----------------------------------------------------------------------------- 2-D

FIELDS2 = {
    "disk17": CASES["disk17"],
    "disk_leaving": ((19, 17), lambda X: np.hypot(X[0] - 0.71, X[1] + 0.43) - 0.61, (-1.0,) * 2, (1.0,) * 2),
    "wide": ((70, 33), lambda X: np.hypot(X[0] - 0.4, 2.0 * (X[1] - 0.1)) - 0.7, (-2.0, -1.0), (2.0, 1.0)),
}


@pytest.mark.parametrize("mode", ["fast", "strict"])
@pytest.mark.parametrize("name,size", [("disk17", (33, 25)), ("disk_leaving", (33, 25)), ("wide", (33, 25)), ("wide", (130, 7))])
def test_2d_matches_restatement(name, size, mode):
    lsm = _lsm()
    n, f, lc, hc = FIELDS2[name]
    vals = grid_vals(n, f, lc, hc)
    ref = R.render2d(vals, lc, hc, *size)
    assert set(np.unique(ref[1])) == {0, 1, 2}
    _same2(lsm.render(_device(lsm, vals, lc, hc, mode), size=size), ref)


def test_2d_extent_style_level_and_float32():
    lsm = _lsm()
    n, f, lc, hc = FIELDS2["disk17"]
    vals = grid_vals(n, f, lc, hc)
    phi = _device(lsm, vals, lc, hc)
    ext = (-1.5, 1.25, -1.0, 1.75)
    ref = R.render2d(vals, lc, hc, 44, 40, extent=ext)
    assert (ref[1][:, :7] == 3).all() and (ref[1][:10] == 3).all() and set(np.unique(ref[1])) == {0, 1, 2, 3}       # beside the box: void
    _same2(lsm.render(phi, size=(44, 40), extent=ext), ref)
    style = dict(fill=(10, 20, 30), line=(200, 0, 0), linewidth=3.5, background=(9, 9, 9))
    _same2(lsm.render(phi, size=(33, 25), level=0.1, **style), R.render2d(vals, lc, hc, 33, 25, level=0.1, **style))
    v32 = np.asfortranarray(vals.astype(np.float32))
    _same2(lsm.render(_device(lsm, v32, lc, hc, dtype=np.float32), size=(33, 25)), R.render2d(v32.astype(np.float64), lc, hc, 33, 25))
    nan = vals.copy(order="F")
    nan[8, 7] = np.nan
    ref = R.render2d(nan, lc, hc, 33, 25)
    assert (ref[1] == 3).any()
    _same2(lsm.render(_device(lsm, nan, lc, hc), size=(33, 25)), ref)


# ----------------------------------------------------------------------------- the Renderer and the API

def test_renderer_reuse_and_refresh():
    lsm = _lsm()
    vals, lc, hc = field("sphere17")
    phi = _device(lsm, vals, lc, hc)
    cams = _cameras(lsm, lc, hc)
    r = lsm.Renderer(phi)
    for cam in cams.values():
        a, b = r.draw(cam, (33, 25)), lsm.render(phi, cam, (33, 25))
        assert np.array_equal(a.depth, b.depth) and np.array_equal(a.normal, b.normal) and np.array_equal(a.rgba, b.rgba)
    assert "rays hit" in repr(a)
    # the field changes in place: refresh() rebuilds the bricks
    other = np.asfortranarray(vals + 0.2)
    phi.backend.upload(phi.buf, other)
    img = r.refresh().draw(cams["perspective"], (33, 25))
    _same3(img, R.render3d(other, lc, hc, _vec(cams["perspective"], 33, 25), 33, 25))
    state, uniform = r.bricks()
    raw, uni = R.bricks(other)
    assert np.array_equal(state, raw) and np.array_equal(uniform, uni)
    r.close()
    r.close()
    with pytest.raises(ValueError, match="closed"):
        r.draw(cams["perspective"])
    # the default camera sees the whole box: every hit of a closed surface inside it lies off the image's border
    img = lsm.render(phi, size=(40, 30))
    hit = np.isfinite(img.depth)
    assert hit.any() and not hit[0].any() and not hit[-1].any() and not hit[:, 0].any() and not hit[:, -1].any()


def test_record_writes_one_picture_per_step(tmp_path):
    lsm = _lsm()
    grid = lsm.CartesianGrid((-1.0, -1.0), (1.0, 1.0), (33, 33))
    zalesak = lambda x: np.maximum(np.hypot(x[0], x[1] - 0.25) - 0.35, -np.maximum(np.abs(x[0]) - 0.06, x[1] - 0.4))
    eq = lsm.LevelSetEquation(terms=(lsm.AdvectionTerm(lsm.RigidRotation(1.0, (0.0, 0.0)), lsm.WENO5()),), ic=lsm.MeshField(zalesak, grid),
                              bc=lsm.NeumannBC(), integrator=lsm.RK3())
    dt = 0.25 * eq.compute_cfl(0.0)
    pattern = str(tmp_path / "frame_{:03d}.png")
    paths = lsm.record_(eq, 2 * dt, pattern, dt=dt, size=(48, 36), linewidth=1.5)
    assert paths == [pattern.format(1), pattern.format(2)] and eq.current_time() == 2 * dt
    last = lsm.render(eq, size=(48, 36), linewidth=1.5)
    for p in paths:
        got = _decode_png(open(p, "rb").read())
        assert got.shape == (36, 48, 4)
    assert np.array_equal(got, last.rgba)
    _same2(last, R.render2d(eq.current_state().values(), grid.lc, grid.hc, 48, 36, linewidth=1.5))
    assert lsm.record_(eq, eq.current_time() + 2 * dt, pattern, every=2, dt=dt, size=(8, 8)) == [pattern.format(2)]


def test_refusals():
    lsm = _lsm()
    grid = lsm.CartesianGrid((0.0,), (1.0,), (17,))
    one = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(lambda x: x[0] - 0.4, grid), bc=lsm.NeumannBC())
    with pytest.raises(ValueError, match="1 dimensional"):
        lsm.render(one)
    with pytest.raises(lsm.LsmError, match="1-dimensional"):
        one.backend.render_create(one.current_state().buf, None, 0.0)
    vals, lc, hc = field("sphere17")
    phi = _device(lsm, vals, lc, hc)
    for level in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            lsm.render(phi, level=level)
        with pytest.raises(lsm.LsmError, match="finite"):
            phi.backend.render_create(phi.buf, None, level)
    for size in ((0, 4), (4, -1)):
        with pytest.raises(ValueError, match="size"):
            lsm.render(phi, size=size)
    with pytest.raises(ValueError, match="step"):
        lsm.render(phi, step=0.0)
    with pytest.raises(ValueError, match="step"):
        lsm.render(phi, step=-1.0)
    for nb in (-1, 31, 2.5):
        with pytest.raises(ValueError, match="bisections"):
            lsm.render(phi, bisections=nb)
    with pytest.raises(ValueError, match="parallel"):
        lsm.render(phi, lsm.Camera((0.0, 0.0, 3.0), (0.0, 0.0, 0.0)))
    with pytest.raises(TypeError, match="unknown style"):
        lsm.render(phi, linewidth=2.0)
    # the library refuses on its own what the Python layer checks first
    b = phi.backend
    r = b.render_create(phi.buf, None, 0.0)
    cam = _vec(lsm.Camera((3.0, 2.0, 1.0), (0.0, 0.0, 0.0)), 4, 4)
    good = [70, 130, 180, 255, 255, 255, 0.25, 0.5, 6]
    for bad, what in (({7: 0.0}, "step"), ({7: 1e-6}, "step"), ({8: 31}, "bisections"), ({8: 1.5}, "bisections"), ({6: float("nan")}, "finite")):
        with pytest.raises(lsm.LsmError, match=what):
            b.render_draw(r, cam, 4, 4, [bad.get(i, v) for i, v in enumerate(good)])
    with pytest.raises(lsm.LsmError, match="finite"):
        b.render_draw(r, [float("nan")] * 13, 4, 4, good)
    with pytest.raises(lsm.LsmError, match="positive"):
        b.render_draw(r, cam, 0, 4, good)
    b.render_destroy(r)
    # a slab handle: a rank of an in-process group
    g = lsm.LocalGroup(1)
    grid3 = lsm.CartesianGrid(lc, hc, vals.shape)
    slab = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(vals, grid3), bc=lsm.NeumannBC(), comm=g.rank(0))
    with pytest.raises(ValueError, match="slab"):
        lsm.render(slab)
