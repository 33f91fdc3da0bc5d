"""numpy restatement of render(ϕ, camera) (csrc/lsm_render.hip): what ext/MakieExt.jl draws — in 3-D the first
hit of a ray march through the trilinear interpolant (volume!(…; algorithm = :iso)), in 2-D the filled contour with its line.
The device is tested against this file bit for bit; tests/test_render_host.py checks this file against facts that do not come
from it.  Everything is fp64 (float32 storage widens exactly), every operation below is one correctly rounded IEEE operation out
of + − × / sqrt, floor and comparisons, in the order written.

3-D, pixel (i, j) of W × H, camera = [eye, forward, right_s, up_s, orthographic flag] (camera_vectors):
  * sx = (2·(i + ½))/W − 1, sy = 1 − (2·(j + ½))/H; perspective: o = eye, v = (forward + sx·right_s) + sy·up_s,
    d = v / sqrt((v₀² + v₁²) + v₂²); orthographic: o = (eye + sx·right_s) + sy·up_s, d = forward;
  * slab test against [lc, hc], t_in = 0, t_out = ∞: per axis with d ≠ 0, t₁ = (lc − o)/d, t₂ = (hc − o)/d, t_in = max(t_in,
    min(t₁, t₂)), t_out = min(t_out, max(t₁, t₂)); d = 0: a miss if o < lc or o > hc, no constraint otherwise; a miss unless
    t_in < t_out < ∞;
  * lattice t_k = t_in + k·dt, dt = step·min(h), k = 0, 1, … while t_k <= t_out;
  * sample at t: p = o + t·d, x = (p − lc)/h, cell = clamp(floor(x), 0, n − 2), w = x − cell (unclamped); lerps a + w·(b − a)
    along x, then y, then z; void iff a corner of the cell is off the band or the value is NaN; else inside iff value < level;
  * hit at t_0 if sample 0 is inside; otherwise at the first k whose samples k − 1 and k are both non-void and differ in inside:
    `bisections` halvings m = ½·(a + b) that keep the change (a void midpoint stops them), then
    t = a + ((level − v_a)/(v_b − v_a))·(b − a); depth = t;
  * normal = gradient of the interpolant in the hit's cell / its norm, 0 if the cell is void or the norm is not > 0;
  * rgb = clamp(floor(((255·s)·c)/255 + ½), 0, 255), s = ambient + (1 − ambient)·|((n₀d₀ + n₁d₁) + n₂d₂)|; a miss: background.
2-D: pixel centre X = x0 + ((i + ½)/W)·(x1 − x0), Y = y1 − ((j + ½)/H)·(y1 − y0); outside [lc, hc] void; value and gradient of
the bilinear interpolant; line iff non-void and |v − level| <= ((½·linewidth)·px)·‖g‖, px = max((x1 − x0)/W, (y1 − y0)/H).
Bricks (what the ray kernel may skip, never what it computes): 8 cells per axis; a cell is void (0) if inactive, outside (1) if
min corner > level + m, inside (2) if max corner < level − m, m = 10⁻⁶·max(|min|, |max|, |level|), mixed (3) otherwise (NaN
included); a brick has its cells' common state or 3; it is uniform iff not 3 and its 3 × 3 × 3 neighbours in the grid agree."""
import numpy as np

VOID, OUT, IN, MIXED = 0, 1, 2, 3
BRICK = 8
STYLE3 = dict(color=(70, 130, 180), background=(255, 255, 255), ambient=0.25, step=0.5, bisections=6)
STYLE2 = dict(fill=(233, 233, 233), line=(0, 0, 0), linewidth=2.0, cell=(198, 217, 234), background=(255, 255, 255), extent=None)


# ----------------------------------------------------------------------------- the camera (host side, fp64)

def camera_vectors(eye, lookat, up=(0.0, 0.0, 1.0), fov=40.0, orthographic=None, width=640, height=480):
    """the 13 doubles the library sees: eye, forward (unit), right·s_x, up·s_y, orthographic flag.  s_y = tan(fov/2) for a
    perspective camera and w/2 for an orthographic window w high; s_x = s_y·W/H."""
    eye, lookat, up = (np.asarray(a, dtype=np.float64) for a in (eye, lookat, up))
    f = lookat - eye
    nf = np.sqrt(f @ f)
    if not nf > 0:
        raise ValueError("Camera: eye and lookat coincide")
    f = f / nf
    r = np.cross(f, up)
    nr = np.sqrt(r @ r)
    if not nr > 1e-12 * np.sqrt(up @ up):
        raise ValueError("Camera: up is parallel to the view direction")
    r = r / nr
    u = np.cross(r, f)
    sy = np.tan(np.radians(float(fov)) / 2.0) if orthographic is None else 0.5 * float(orthographic)
    sx = sy * (float(width) / float(height))
    return np.concatenate([eye, f, r * sx, u * sy, [0.0 if orthographic is None else 1.0]])


def fit_camera(lc, hc, direction=(1.0, 1.0, 1.0), fov=40.0):
    """(eye, lookat, up) of a perspective camera on the ray centre + s·direction that sees the box's bounding sphere in an image
    at least as wide as high"""
    lc, hc, dirn = (np.asarray(a, dtype=np.float64) for a in (lc, hc, direction))
    c = 0.5 * (lc + hc)
    rad = 0.5 * np.sqrt(((hc - lc) ** 2).sum())
    dirn = dirn / np.sqrt(dirn @ dirn)
    dist = 1.05 * rad / np.sin(np.radians(float(fov)) / 2.0)
    up = (0.0, 0.0, 1.0) if abs(dirn[2]) < 0.99 else (0.0, 1.0, 0.0)
    return c + dist * dirn, c, up


# ----------------------------------------------------------------------------- cells and samples

def active_cells(shape, mask=None):
    nc = tuple(k - 1 for k in shape)
    act = np.ones(nc, dtype=bool)
    if mask is not None:
        m = np.asarray(mask, dtype=bool)
        for c in range(1 << len(shape)):
            act &= m[tuple(slice((c >> a) & 1, ((c >> a) & 1) + nc[a]) for a in range(len(shape)))]
    return act


def _cell(p, lc, h, n):
    """per axis: clamped cell index (int64) and unclamped weight of the positions p (npts, N)"""
    cs, ws = [], []
    for a in range(len(n)):
        x = (p[:, a] - lc[a]) / h[a]
        cf = np.floor(x)
        cf = np.where(cf < 0.0, 0.0, np.where(cf > n[a] - 2.0, n[a] - 2.0, cf))
        cs.append(cf.astype(np.int64))
        ws.append(x - cf)
    return cs, ws


def sample3(v, act, lc, h, p):
    """value, void flag and gradient of the trilinear interpolant at the positions p (npts, 3)"""
    n = v.shape
    (cx, cy, cz), (wx, wy, wz) = _cell(p, lc, h, n)
    with np.errstate(all="ignore"):
        c = [[[v[cx + i, cy + j, cz + k] for k in (0, 1)] for j in (0, 1)] for i in (0, 1)]
        c00 = c[0][0][0] + wx * (c[1][0][0] - c[0][0][0])
        c10 = c[0][1][0] + wx * (c[1][1][0] - c[0][1][0])
        c01 = c[0][0][1] + wx * (c[1][0][1] - c[0][0][1])
        c11 = c[0][1][1] + wx * (c[1][1][1] - c[0][1][1])
        c0 = c00 + wy * (c10 - c00)
        c1 = c01 + wy * (c11 - c01)
        val = c0 + wz * (c1 - c0)
        dx00, dx10 = c[1][0][0] - c[0][0][0], c[1][1][0] - c[0][1][0]
        dx01, dx11 = c[1][0][1] - c[0][0][1], c[1][1][1] - c[0][1][1]
        gx0 = dx00 + wy * (dx10 - dx00)
        gx1 = dx01 + wy * (dx11 - dx01)
        gx = (gx0 + wz * (gx1 - gx0)) / h[0]
        dy0, dy1 = c10 - c00, c11 - c01
        gy = (dy0 + wz * (dy1 - dy0)) / h[1]
        gz = (c1 - c0) / h[2]
    inactive = ~act[cx, cy, cz]
    return val, inactive | np.isnan(val), np.stack([gx, gy, gz], axis=1), inactive


def _grid(vals, lc, hc):
    v = np.asarray(vals).astype(np.float64)
    lc, hc = np.asarray(lc, dtype=np.float64), np.asarray(hc, dtype=np.float64)
    return v, lc, hc, (hc - lc) / (np.array(v.shape, dtype=np.float64) - 1.0)


def rays(camera, W, H):
    """origins and directions (H·W, 3), row-major over (j, i)"""
    cam = np.asarray(camera, dtype=np.float64)
    eye, f, rs, us, ortho = cam[0:3], cam[3:6], cam[6:9], cam[9:12], cam[12] != 0.0
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    sx = ((2.0 * (ii + 0.5)) / float(W) - 1.0).reshape(-1)
    sy = (1.0 - (2.0 * (jj + 0.5)) / float(H)).reshape(-1)
    if ortho:
        o = np.stack([(eye[a] + sx * rs[a]) + sy * us[a] for a in range(3)], axis=1)
        d = np.broadcast_to(f, o.shape).copy()
    else:
        vv = np.stack([(f[a] + sx * rs[a]) + sy * us[a] for a in range(3)], axis=1)
        nn = np.sqrt((vv[:, 0] * vv[:, 0] + vv[:, 1] * vv[:, 1]) + vv[:, 2] * vv[:, 2])
        d = vv / nn[:, None]
        o = np.broadcast_to(eye, d.shape).copy()
    return o, d


def clip(o, d, lc, hc):
    """(t_in, t_out, miss) of the slab test"""
    P = len(o)
    tin, tout, miss = np.zeros(P), np.full(P, np.inf), np.zeros(P, dtype=bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            z = d[:, a] == 0.0
            miss |= z & ((o[:, a] < lc[a]) | (o[:, a] > hc[a]))
            t1, t2 = (lc[a] - o[:, a]) / d[:, a], (hc[a] - o[:, a]) / d[:, a]
            tn, tf = np.where(t1 < t2, t1, t2), np.where(t1 < t2, t2, t1)
            tin = np.where(~z & (tn > tin), tn, tin)
            tout = np.where(~z & (tf < tout), tf, tout)
    miss |= ~((tout > tin) & (tout < np.inf))
    return tin, tout, miss


def _shade(s, c):
    q = np.floor(((255.0 * s) * float(c)) / 255.0 + 0.5)
    return np.where(q < 0.0, 0.0, np.where(q > 255.0, 255.0, q)).astype(np.uint8)


def render3d(vals, lc, hc, camera, W, H, level=0.0, mask=None, color=(70, 130, 180), background=(255, 255, 255), ambient=0.25,
             step=0.5, bisections=6, stats=None):
    """(rgba (H, W, 4) uint8, depth (H, W), normal (H, W, 3)); stats: a dict that receives the number of lattice samples"""
    v, lc, hc, h = _grid(vals, lc, hc)
    act = active_cells(v.shape, mask)
    level, ambient = float(level), float(ambient)
    dt = float(step) * h.min()
    o, d = rays(camera, W, H)
    tin, tout, miss = clip(o, d, lc, hc)
    P = W * H
    t_hit = np.full(P, np.inf)
    hit = np.zeros(P, dtype=bool)
    alive = ~miss
    prev_st, prev_v = np.zeros(P, dtype=np.int8), np.zeros(P)
    br = {k: [] for k in ("idx", "a", "b", "va", "vb")}
    k, nsamples = 0, 0
    while alive.any():
        idx = np.nonzero(alive)[0]
        t = tin[idx] + float(k) * dt
        over = ~(t <= tout[idx])
        alive[idx[over]] = False
        idx, t = idx[~over], t[~over]
        nsamples += len(idx)
        val, void, _, _ = sample3(v, act, lc, h, o[idx] + t[:, None] * d[idx])
        st = np.where(void, VOID, np.where(val < level, IN, OUT)).astype(np.int8)
        if k == 0:
            now = st == IN
            t_hit[idx[now]] = t[now]
        else:
            now = (prev_st[idx] != VOID) & (st != VOID) & (prev_st[idx] != st)
            br["idx"].append(idx[now])
            br["a"].append(tin[idx[now]] + float(k - 1) * dt)
            br["b"].append(t[now])
            br["va"].append(prev_v[idx[now]])
            br["vb"].append(val[now])
        hit[idx[now]] = True
        alive[idx[now]] = False
        prev_st[idx], prev_v[idx] = st, val
        k += 1
    if stats is not None:
        stats["samples"] = nsamples
    idx, a, b, va, vb = (np.concatenate(br[q]) if br[q] else np.zeros(0, dtype=np.int64 if q == "idx" else np.float64)
                         for q in ("idx", "a", "b", "va", "vb"))
    going = np.ones(len(idx), dtype=bool)
    for _ in range(int(bisections)):
        g = np.nonzero(going)[0]
        if not len(g):
            break
        m = 0.5 * (a[g] + b[g])
        vm, void, _, _ = sample3(v, act, lc, h, o[idx[g]] + m[:, None] * d[idx[g]])
        going[g[void]] = False
        g, m, vm = g[~void], m[~void], vm[~void]
        same = (vm < level) == (va[g] < level)
        a[g[same]], va[g[same]] = m[same], vm[same]
        b[g[~same]], vb[g[~same]] = m[~same], vm[~same]
    t_hit[idx] = a + ((level - va) / (vb - va)) * (b - a)
    depth = np.full(P, np.inf)
    normal = np.zeros((P, 3))
    rgba = np.empty((P, 4), dtype=np.uint8)
    rgba[:, :3], rgba[:, 3] = np.asarray(background, dtype=np.uint8), 255
    hi = np.nonzero(hit)[0]
    if len(hi):
        th = t_hit[hi]
        _, _, g, inactive = sample3(v, act, lc, h, o[hi] + th[:, None] * d[hi])
        with np.errstate(all="ignore"):
            nn = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
            ok = ~inactive & (nn > 0.0)
            nrm = np.where(ok[:, None], g / nn[:, None], 0.0)
        dd = d[hi]
        s = ambient + (1.0 - ambient) * np.abs((nrm[:, 0] * dd[:, 0] + nrm[:, 1] * dd[:, 1]) + nrm[:, 2] * dd[:, 2])
        depth[hi], normal[hi] = th, nrm
        for c in range(3):
            rgba[hi, c] = _shade(s, color[c])
    return rgba.reshape(H, W, 4), depth.reshape(H, W), normal.reshape(H, W, 3)


# ----------------------------------------------------------------------------- 2-D

def class_table(fill=(233, 233, 233), line=(0, 0, 0), cell=(198, 217, 234), background=(255, 255, 255)):
    """rgb of the classes 0 outside, 1 inside, 2 line, 3 void, 4 active band cell outside, 5 active band cell inside (the
    cell colour over the fill: their product / 255, rounded)"""
    both = tuple(int(np.floor(float(c) * float(f) / 255.0 + 0.5)) for c, f in zip(cell, fill))
    return np.array([background, fill, line, background, cell, both], dtype=np.float64)


def render2d(vals, lc, hc, W, H, level=0.0, mask=None, fill=(233, 233, 233), line=(0, 0, 0), linewidth=2.0, cell=(198, 217, 234),
             background=(255, 255, 255), extent=None):
    """(rgba (H, W, 4) uint8, cls (H, W) uint8)"""
    v, lc, hc, h = _grid(vals, lc, hc)
    act = active_cells(v.shape, mask)
    x0, x1, y0, y1 = (float(lc[0]), float(hc[0]), float(lc[1]), float(hc[1])) if extent is None else (float(e) for e in extent)
    level = float(level)
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    X = (x0 + ((ii + 0.5) / float(W)) * (x1 - x0)).reshape(-1)
    Y = (y1 - ((jj + 0.5) / float(H)) * (y1 - y0)).reshape(-1)
    pw, ph = (x1 - x0) / float(W), (y1 - y0) / float(H)
    px = pw if pw > ph else ph
    (cx, cy), (wx, wy) = _cell(np.stack([X, Y], axis=1), lc, h, v.shape)
    with np.errstate(all="ignore"):
        v00, v10, v01, v11 = v[cx, cy], v[cx + 1, cy], v[cx, cy + 1], v[cx + 1, cy + 1]
        c0 = v00 + wx * (v10 - v00)
        c1 = v01 + wx * (v11 - v01)
        val = c0 + wy * (c1 - c0)
        dx0, dx1 = v10 - v00, v11 - v01
        gx = (dx0 + wy * (dx1 - dx0)) / h[0]
        gy = (c1 - c0) / h[1]
        nn = np.sqrt(gx * gx + gy * gy)
        off = (X < lc[0]) | (X > hc[0]) | (Y < lc[1]) | (Y > hc[1])
        void = off | ~act[cx, cy] | np.isnan(val)
        is_line = ~void & (np.abs(val - level) <= ((0.5 * float(linewidth)) * px) * nn)
    inside = val < level
    cls = np.where(void, 3, np.where(is_line, 2, np.where(inside, 1, 0) + (0 if mask is None else 4))).astype(np.uint8)
    tab = class_table(fill, line, cell, background).astype(np.uint8)
    rgba = np.empty((W * H, 4), dtype=np.uint8)
    rgba[:, :3], rgba[:, 3] = tab[cls], 255
    return rgba.reshape(H, W, 4), cls.reshape(H, W)


# ----------------------------------------------------------------------------- bricks

def bricks(vals, level=0.0, mask=None):
    """(raw states, uniform flags) of the bricks, each of shape ceil((n − 1)/8) per axis"""
    v = np.asarray(vals).astype(np.float64)
    n, level = v.shape, float(level)
    nc = tuple(k - 1 for k in n)
    act = active_cells(n, mask)
    corners = np.stack([v[tuple(slice((c >> a) & 1, ((c >> a) & 1) + nc[a]) for a in range(3))] for c in range(8)])
    with np.errstate(all="ignore"):
        mn, mx = corners.min(axis=0), corners.max(axis=0)      # NaN propagates
        m = 1e-6 * np.maximum(np.maximum(np.abs(mn), np.abs(mx)), abs(level))
        st = np.where(mn > level + m, OUT, np.where(mx < level - m, IN, MIXED))
    st = np.where(act, st, VOID).astype(np.uint8)
    nb = tuple((k + BRICK - 1) // BRICK for k in nc)
    raw = np.zeros(nb, dtype=np.uint8)
    for b in np.ndindex(*nb):
        s = np.unique(st[tuple(slice(BRICK * b[a], BRICK * (b[a] + 1)) for a in range(3))])
        raw[b] = s[0] if len(s) == 1 else MIXED
    uni = raw != MIXED
    pad = np.pad(raw.astype(np.int16), 1, constant_values=-1)
    for off in np.ndindex(3, 3, 3):
        nbr = pad[tuple(slice(off[a], off[a] + nb[a]) for a in range(3))]
        uni &= (nbr == -1) | (nbr == raw)
    return raw, uni
