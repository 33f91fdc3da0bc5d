"""The restatement of render (tests/_render_ref.py, the contract of csrc/lsm_render.hip) against facts that do not come from it:
exact planes, the analytic ray–sphere intersection within the interpolation error, the slab test's corner cases, cameras inside
the box and the body, the 2-D classes against the disk's area and perimeter, bands, the brick table's promise; and the host code
of the Python API: the camera's vectors, Camera.fit, the PNG writer, the refusals that need no device."""
import functools
import math
import struct
import zlib

import numpy as np
import pytest

import _render_ref as R
from test_isosurface_host import grid_vals


def _sphere(c, rad):
    return lambda X: np.sqrt(sum((X[d] - c[d]) ** 2 for d in range(3))) - rad


BOX = ((-1.0,) * 3, (1.0,) * 3)
DOWN = dict(eye=(0.5, 0.5, 2.0), lookat=(0.5, 0.5, 0.0), up=(0.0, 1.0, 0.0))      # forward = (0, 0, −1) exactly


@functools.lru_cache(maxsize=None)
def plane_vals():
    v = grid_vals((11, 10, 9), lambda X: X[2] - 0.3, (0.0,) * 3, (1.0,) * 3)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def sphere_vals(n, c=(0.0, 0.0, 0.0), rad=0.5):
    v = grid_vals((n,) * 3, _sphere(c, rad), *BOX)
    v.setflags(write=False)
    return v


def test_plane_under_an_axis_aligned_orthographic_camera_is_exact():
    cam = R.camera_vectors(**DOWN, orthographic=0.9, width=13, height=11)
    assert np.array_equal(cam[3:6], (0.0, 0.0, -1.0)) and cam[12] == 1.0
    rgba, depth, normal = R.render3d(plane_vals(), (0.0,) * 3, (1.0,) * 3, cam, 13, 11)
    assert np.isfinite(depth).all()
    assert np.abs(depth - (2.0 - 0.3)).max() <= 1e-12
    assert np.abs(normal - (0.0, 0.0, 1.0)).max() <= 1e-12
    # |n·d| = 1: full light
    assert np.array_equal(rgba.reshape(-1, 4), np.tile(np.array([70, 130, 180, 255], dtype=np.uint8), (13 * 11, 1)))


def _ray_sphere(o, d, c, rad):
    """first analytic intersection of unit rays with the sphere: (hit, t, |n·d|)"""
    oc = o - np.asarray(c)
    b = (oc * d).sum(axis=1)
    disc = b * b - ((oc * oc).sum(axis=1) - rad * rad)
    hit = (disc > 0) & (-b - np.sqrt(np.abs(disc)) > 0)
    t = -b - np.sqrt(np.abs(disc))
    nrm = (oc + t[:, None] * d) / rad
    return hit, t, np.abs((nrm * d).sum(axis=1))


@pytest.mark.parametrize("n,rad,c,size", [(17, 0.5, (0.0, 0.0, 0.0), 33), (33, 0.5, (0.0, 0.0, 0.0), 33), (41, 0.3, (0.1, -0.05, 0.2), 40)])
def test_sphere_depth_within_the_interpolation_error(n, rad, c, size):
    """the interpolation error of a distance function is at most Σ h²/8·|∂²ϕ| <= 3h²/(8R); along a ray with |∇ϕ·d| >= 0.5 the
    intersection moves by at most twice that"""
    h = 2.0 / (n - 1)
    cam = R.camera_vectors((2.6, 1.9, 1.7), c, fov=40.0, width=size, height=size)
    _, depth, normal = R.render3d(sphere_vals(n, c, rad), *BOX, cam, size, size)
    o, d = R.rays(cam, size, size)
    assert np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0).max() <= 4e-16
    hit, t, nd = _ray_sphere(o, d, c, rad)
    sel = hit & (nd >= 0.5)
    assert sel.sum() > 50
    got = depth.reshape(-1)
    assert np.isfinite(got[sel]).all()
    err = np.abs(got[sel] - t[sel]).max()
    bound = 2.0 * 3.0 * h * h / (8.0 * rad)
    print(f"n = {n}: max |depth − analytic| = {err:.4f}, bound {bound:.4f}; whole-image hit mismatches: {int((np.isfinite(got) != hit).sum())}")
    assert err <= bound
    nn = np.sqrt((normal.reshape(-1, 3) ** 2).sum(axis=1))
    assert np.abs(nn[np.isfinite(got)] - 1.0).max() <= 1e-14 and (nn[~np.isfinite(got)] == 0).all()


def test_slab_test_with_zero_components_and_origins_on_grid_planes():
    """pixel centres on grid planes (x = 0.125, 0.375, …) and on the faces of the box (x = 0, 1): zero direction components never
    make a NaN, rays on a face are inside"""
    vals = plane_vals()
    for w, size in ((1.0, 4), (2.0, 2)):
        cam = R.camera_vectors(**DOWN, orthographic=w, width=size, height=size)
        o, d = R.rays(cam, size, size)
        assert (d[:, :2] == 0).all() and np.isin(o[:, 0], [0.0, 0.125, 0.375, 0.625, 0.875, 1.0]).all()
        tin, tout, miss = R.clip(o, d, np.zeros(3), np.ones(3))
        assert not miss.any() and np.array_equal(tin, np.full(size * size, 1.0)) and np.array_equal(tout, np.full(size * size, 2.0))
        _, depth, normal = R.render3d(vals, (0.0,) * 3, (1.0,) * 3, cam, size, size)
        assert not np.isnan(depth).any() and not np.isnan(normal).any()
        assert np.abs(depth - 1.7).max() <= 1e-12
    # a window wider than the box: the rays beside it miss
    cam = R.camera_vectors(**DOWN, orthographic=3.0, width=6, height=6)
    _, depth, _ = R.render3d(vals, (0.0,) * 3, (1.0,) * 3, cam, 6, 6)
    inside = np.zeros((6, 6), dtype=bool)
    inside[2:4, 2:4] = True
    assert np.array_equal(np.isfinite(depth), inside)


def test_cameras_inside_the_box_inside_the_body_and_looking_away():
    vals, c, rad = sphere_vals(17), (0.0, 0.0, 0.0), 0.5
    # in the box, outside the body
    cam = R.camera_vectors((0.9, 0.8, 0.7), c, width=16, height=16)
    _, depth, _ = R.render3d(vals, *BOX, cam, 16, 16)
    o, d = R.rays(cam, 16, 16)
    hit, t, nd = _ray_sphere(o, d, c, rad)
    sel = hit & (nd >= 0.5)
    assert sel.any() and np.abs(depth.reshape(-1)[sel] - t[sel]).max() <= 2 * 3 * 0.125 ** 2 / (8 * rad)
    # in the body: every ray hits where it starts
    cam = R.camera_vectors((0.01, 0.02, 0.03), (1.0, 0.0, 0.0), width=8, height=8)
    rgba, depth, normal = R.render3d(vals, *BOX, cam, 8, 8)
    assert np.array_equal(depth, np.zeros((8, 8)))
    assert np.abs(np.sqrt((normal ** 2).sum(axis=2)) - 1.0).max() <= 1e-14
    # looking away from the box
    cam = R.camera_vectors((3.0, 0.0, 0.0), (5.0, 0.0, 0.0), width=8, height=8)
    rgba, depth, normal = R.render3d(vals, *BOX, cam, 8, 8, background=(1, 2, 3))
    assert np.isinf(depth).all() and (normal == 0).all()
    assert np.array_equal(rgba.reshape(-1, 4), np.tile(np.array([1, 2, 3, 255], dtype=np.uint8), (64, 1)))


def _components(m):
    """number of 8-connected components of a boolean image"""
    m, count = m.copy(), 0
    H, W = m.shape
    for s in zip(*np.nonzero(m)):
        if not m[s]:
            continue
        count += 1
        stack = [s]
        m[s] = False
        while stack:
            j, i = stack.pop()
            for q in ((j + a, i + b) for a in (-1, 0, 1) for b in (-1, 0, 1)):
                if 0 <= q[0] < H and 0 <= q[1] < W and m[q]:
                    m[q] = False
                    stack.append(q)
    return count


DISK_C, DISK_R = (0.11, -0.07), 0.53


def _disk(X):
    return np.hypot(X[0] - DISK_C[0], X[1] - DISK_C[1]) - DISK_R


def test_disk_classes_against_area_and_perimeter():
    vals = grid_vals((65, 63), _disk, (-1.0,) * 2, (1.0,) * 2)
    W = H = 120
    lw = 2.0
    rgba, cls = R.render2d(vals, (-1.0,) * 2, (1.0,) * 2, W, H, linewidth=lw)
    assert set(np.unique(cls)) == {0, 1, 2}
    px = 2.0 / W
    ring = 2 * math.pi * DISK_R / px                    # pixels in a ring one pixel wide along the interface
    n_in, n_line = int((cls == 1).sum()), int((cls == 2).sum())
    assert abs(n_line - 2 * math.pi * DISK_R * lw / px) <= ring
    assert abs(n_in + 0.5 * n_line - math.pi * DISK_R ** 2 / px ** 2) <= ring
    # the line is one closed curve: connected, and no inside pixel touches an outside pixel along an edge
    assert _components(cls == 2) == 1
    a, b = cls == 0, cls == 1
    assert not (a[1:] & b[:-1]).any() and not (a[:-1] & b[1:]).any() and not (a[:, 1:] & b[:, :-1]).any() and not (a[:, :-1] & b[:, 1:]).any()
    assert _components(b) == 1 and b[int((1 - DISK_C[1]) / px), int((DISK_C[0] + 1) / px)]
    tab = R.class_table().astype(np.uint8)
    assert np.array_equal(rgba[..., :3], tab[cls]) and (rgba[..., 3] == 255).all()
    # row 0 is the top of the picture: the disk's centre lies below the middle (c_y < 0)
    rows = np.nonzero(b.any(axis=1))[0]
    assert 0.5 * (rows[0] + rows[-1]) > H / 2


def test_band_void_pixels_lie_exactly_off_the_active_cells():
    n, lc, hc = (33, 31), (-1.0,) * 2, (1.0,) * 2
    vals = grid_vals(n, _disk, lc, hc)
    mask = np.abs(vals) < 0.2
    W, H = 57, 41
    garbage = np.where(mask, vals, np.nan)
    _, cls = R.render2d(garbage, lc, hc, W, H, mask=mask)
    h = [(hc[a] - lc[a]) / (n[a] - 1) for a in range(2)]
    X = lc[0] + (np.arange(W) + 0.5) / W * (hc[0] - lc[0])
    Y = hc[1] - (np.arange(H) + 0.5) / H * (hc[1] - lc[1])
    cx, cy = np.floor((X - lc[0]) / h[0]).astype(int), np.floor((Y - lc[1]) / h[1]).astype(int)
    act = mask[:-1, :-1] & mask[1:, :-1] & mask[:-1, 1:] & mask[1:, 1:]
    assert np.array_equal(cls == 3, ~act[cx[None, :], cy[:, None]])
    assert set(np.unique(cls)) == {2, 3, 4, 5}
    assert np.array_equal(cls, R.render2d(vals, lc, hc, W, H, mask=mask)[1])
    # 3-D: the values off the band decide nothing
    v3 = sphere_vals(17)
    m3 = np.abs(v3) < 0.3
    cam = R.camera_vectors((2.6, 1.9, 1.7), (0, 0, 0), width=24, height=20)
    a = R.render3d(v3, *BOX, cam, 24, 20, mask=m3)
    b = R.render3d(np.where(m3, v3, 1e30), *BOX, cam, 24, 20, mask=m3)
    c = R.render3d(np.where(m3, v3, np.nan), *BOX, cam, 24, 20, mask=m3)
    dense = R.render3d(v3, *BOX, cam, 24, 20)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert np.array_equal(np.isfinite(a[1]), np.isfinite(dense[1])) and np.isfinite(a[1]).any()


def test_uniform_bricks_keep_their_promise():
    """every sample in a cell of a uniform brick has the brick's state: what lets the device step over it.  43³ is five whole
    bricks and a partial one per axis; more than half of them are uniform around a small sphere"""
    c, rad = (0.3, -0.2, 0.1), 0.2
    vals = grid_vals((43,) * 3, _sphere(c, rad), *BOX)
    raw, uni = R.bricks(vals)
    assert raw.shape == (6, 6, 6) and uni.sum() > raw.size // 2
    assert set(np.unique(raw)) == {R.OUT, R.MIXED} and not uni[raw == R.MIXED].any()
    rng = np.random.default_rng(3)
    p = rng.uniform(-1.0, 1.0, size=(20000, 3))
    lc, h = np.full(3, -1.0), np.full(3, 2.0 / 42)
    val, void, _, _ = R.sample3(vals, R.active_cells(vals.shape), lc, h, p)
    b = np.minimum(np.floor((p - lc) / h).astype(int), 41) // 8
    u = uni[b[:, 0], b[:, 1], b[:, 2]]
    assert u.sum() > 5000 and not void[u].any() and (val[u] >= 0).all()
    # a level equal to a node value: the margin keeps such cells mixed
    flat = np.zeros((17, 17, 17))
    raw, uni = R.bricks(flat)
    assert (raw == R.MIXED).all() and not uni.any()
    raw, uni = R.bricks(flat + 1.0)
    assert (raw == R.OUT).all() and uni.all()
    nan = flat - 1.0
    nan[3, 3, 3] = np.nan
    raw, uni = R.bricks(nan)
    assert raw[0, 0, 0] == R.MIXED and raw[1, 1, 1] == R.IN and not uni.any()
    raw, uni = R.bricks(flat - 1.0, mask=np.zeros(flat.shape, dtype=bool))
    assert (raw == R.VOID).all() and uni.all()


def test_lattice_samples_are_counted():
    stats = {}
    cam = R.camera_vectors(**DOWN, orthographic=0.9, width=4, height=4)
    R.render3d(plane_vals(), (0.0,) * 3, (1.0,) * 3, cam, 4, 4, level=0.025, stats=stats)
    # dt = 0.5·0.1: z = 1, 0.95, …, 0.35, 0.30, the first below the crossing at z = 0.325: 15 samples per ray
    assert stats["samples"] == 15 * 16


# ----------------------------------------------------------------------------- the host code of the API

def _lsm():
    import lsm_amd
    return lsm_amd


@pytest.mark.parametrize("kw", [dict(fov=40.0), dict(fov=63.0, up=(0.1, 1.0, 0.0)), dict(orthographic=1.7)])
def test_camera_vectors_of_the_api_equal_the_restatement(kw):
    lsm = _lsm()
    cam = lsm.Camera((2.6, 1.9, 1.7), (0.1, 0.0, -0.2), **kw)
    for W, H in ((640, 480), (33, 25), (1, 1)):
        got, want = cam.vectors(W, H), R.camera_vectors((2.6, 1.9, 1.7), (0.1, 0.0, -0.2), width=W, height=H, **kw)
        assert got.dtype == np.float64 and np.array_equal(got, want)
    f, rs, us = want[3:6], want[6:9], want[9:12]
    assert abs(f @ f - 1) < 1e-15 and abs(f @ rs) < 1e-15 and abs(f @ us) < 1e-15 and abs(rs @ us) < 1e-15
    assert "Camera(" in repr(cam)


@pytest.mark.parametrize("direction", [(1, 1, 1), (0, 0, 1), (-2, 0.5, 0.1)])
@pytest.mark.parametrize("size", [(640, 480), (100, 100)])
def test_camera_fit_sees_all_eight_corners(direction, size):
    lsm = _lsm()
    grid = lsm.CartesianGrid((-1.0, 0.0, 2.0), (1.5, 1.0, 2.5), (11, 9, 7))
    cam = lsm.Camera.fit(grid, direction)
    v = cam.vectors(*size)
    eye, f, rs, us = v[0:3], v[3:6], v[6:9], v[9:12]
    for corner in np.ndindex(2, 2, 2):
        p = np.array([(grid.lc[a], grid.hc[a])[corner[a]] for a in range(3)]) - eye
        z = p @ f
        assert z > 0 and abs(p @ rs / (rs @ rs)) < z and abs(p @ us / (us @ us)) < z
    e2, l2, u2 = R.fit_camera(grid.lc, grid.hc, direction)
    assert np.array_equal(e2, cam.eye) and np.array_equal(l2, cam.lookat) and tuple(u2) == cam.up


def _decode_png(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        chunks.append((kind, body))
        pos += 12 + n
    assert [k for k, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 6, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b"".join(b for k, b in chunks if k == b"IDAT")), dtype=np.uint8).reshape(H, 1 + 4 * W)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(H, W, 4)


def test_png_round_trip(tmp_path):
    lsm = _lsm()
    rng = np.random.default_rng(5)
    rgba = rng.integers(0, 256, size=(7, 13, 4), dtype=np.uint8)
    img = lsm.Image(rgba, cls=np.zeros((7, 13), dtype=np.uint8))
    path = str(tmp_path / "a.png")
    assert img.save(path) == path and img.size == (13, 7)
    assert np.array_equal(_decode_png(open(path, "rb").read()), rgba)
    assert repr(img).startswith("Image 13×7")


def test_refusals_that_need_no_device():
    lsm = _lsm()
    with pytest.raises(ValueError, match="parallel"):
        lsm.Camera((0, 0, 3), (0, 0, 0))                       # the default up is z
    with pytest.raises(ValueError, match="parallel"):
        R.camera_vectors((0, 0, 3), (0, 0, 0))
    with pytest.raises(ValueError, match="coincide"):
        lsm.Camera((1, 1, 1), (1, 1, 1))
    with pytest.raises(ValueError, match="fov"):
        lsm.Camera((1, 1, 1), (0, 0, 0), fov=180.0)
    with pytest.raises(ValueError, match="orthographic"):
        lsm.Camera((1, 1, 1), (0, 0, 0), orthographic=0.0)
    with pytest.raises(TypeError, match="device field"):
        lsm.render(np.zeros((4, 4, 4)))
    with pytest.raises(ValueError, match="3-D grid"):
        lsm.Camera.fit(lsm.CartesianGrid((0, 0), (1, 1), (5, 5)))
