"""components / remove_components_ restated in numpy (csrc/lsm_cc.hip), and the fixtures of the tests.

The definition: inside(I) := ϕ[I] < level (ϕ == level and NaN are outside); the set is the inside nodes (side "inside") or the
others ("outside"); two set nodes are adjacent iff they differ by ±d, d ∈ {0,1}^N \\ {0} (the Kuhn edges: 6 neighbours in 2-D,
14 in 3-D); components are numbered 0 … K−1 by their smallest linear node index, axis 0 fastest.  labels() does not follow the
device's schedule: it hooks the larger of two root labels under the smaller over all edges at once and jumps pointers until
nothing changes — any correct labelling gives the same arrays, so the comparison with the device is for equality."""
import itertools

import numpy as np

SIDES = ("inside", "outside")


def kuhn_offsets(N):
    """the forward Kuhn edges: {0,1}^N without 0 (3 in 2-D, 7 in 3-D)"""
    return [d for d in itertools.product((0, 1), repeat=N) if any(d)]


def in_set(vals, level=0.0, side="inside"):
    inside = np.asarray(vals, dtype=np.float64) < level          # float32 widens exactly
    return inside if side == "inside" else ~inside


def _roots(p):
    while True:
        q = p[p]
        if np.array_equal(q, p):
            return p
        p = q


def _union_all(size, a, b):
    """the root (smallest member) of every node after joining a[i] ~ b[i]"""
    p = np.arange(size, dtype=np.int64)
    while True:
        ra, rb = p[a], p[b]
        lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
        m = lo != hi
        if not m.any():
            return p
        np.minimum.at(p, hi[m], lo[m])
        p = _roots(p)


def labels(vals, level=0.0, side="inside"):
    """int32 of vals' shape: the component number of every set node, −1 elsewhere"""
    s = in_set(vals, level, side)
    n, N = s.shape, s.ndim
    lin = np.arange(s.size, dtype=np.int64).reshape(n, order="F")
    a, b = [], []
    for d in kuhn_offsets(N):
        lo = tuple(slice(0, n[k] - d[k]) for k in range(N))
        hi = tuple(slice(d[k], n[k]) for k in range(N))
        m = s[lo] & s[hi]
        a.append(lin[lo][m])
        b.append(lin[hi][m])
    p = _union_all(s.size, np.concatenate(a), np.concatenate(b))
    flat = s.reshape(-1, order="F")
    roots = np.flatnonzero(flat & (p == np.arange(s.size)))       # ascending: the numbering
    out = np.full(s.size, -1, dtype=np.int32)
    out[flat] = np.searchsorted(roots, p[flat]).astype(np.int32)
    return out.reshape(n, order="F")


def stats(lab):
    """(K, nodes int64[K], index_sums int64[K, N], bbox int32[K, 2, N]) of a label array"""
    lab = np.asarray(lab)
    N = lab.ndim
    K = int(lab.max()) + 1 if lab.size and lab.max() >= 0 else 0
    on = lab >= 0
    l = lab[on].astype(np.int64)
    nodes = np.bincount(l, minlength=K).astype(np.int64)
    sums = np.zeros((K, N), dtype=np.int64)
    bbox = np.zeros((K, 2, N), dtype=np.int32)
    bbox[:, 0, :] = np.iinfo(np.int32).max
    bbox[:, 1, :] = np.iinfo(np.int32).min
    idx = np.nonzero(on)
    for d in range(N):
        i = idx[d].astype(np.int64)
        np.add.at(sums[:, d], l, i)
        np.minimum.at(bbox[:, 0, d], l, i.astype(np.int32))
        np.maximum.at(bbox[:, 1, d], l, i.astype(np.int32))
    return K, nodes, sums, bbox


def count(vals, level=0.0, side="inside"):
    return stats(labels(vals, level, side))[0]


def flip(vals, lab, which, level=0.0, side="inside", dtype=np.float64):
    """vals after remove_components_: the nodes of the flagged components mirrored at the level, operation by operation.
    vals holds values of `dtype`; returns (new values of dtype, nodes flipped)."""
    dtype = np.dtype(dtype)
    out = np.array(vals, dtype=dtype, order="F")
    which = np.asarray(which, dtype=bool)
    if not which.size:
        return out, 0
    sel = (lab >= 0) & which[np.where(lab >= 0, lab, 0)]
    level = np.float64(level)
    v = out[sel].astype(np.float64)
    with np.errstate(over="ignore"):
        w = level + (level - v)                                   # two roundings
    below = side == "outside"                                     # where the node has to land: below the level, or not below
    if below:
        w = np.where(w < level, w, np.nextafter(level, -np.inf))
    if dtype == np.float32:
        f = w.astype(np.float32)                                  # one rounding
        wrong = (f.astype(np.float64) < level) != below
        f = np.where(wrong, np.nextafter(f, np.float32(-np.inf if below else np.inf)), f).astype(np.float32)
        out[sel] = f
    else:
        out[sel] = w
    return out, int(sel.sum())


def mesh_components(elements, nverts):
    """the number of vertex-connected components of a simplicial mesh, over the vertices its elements use"""
    e = np.asarray(elements, dtype=np.int64)
    if not len(e):
        return 0
    p = _union_all(nverts, np.repeat(e[:, :1], e.shape[1] - 1, axis=1).reshape(-1), e[:, 1:].reshape(-1))
    used = np.zeros(nverts, dtype=bool)
    used[e.reshape(-1)] = True
    return int((used & (p == np.arange(nverts))).sum())


def same_partition(a, b):
    """two label arrays (−1 or 0: background, as given by bg) describe the same partition of the same set"""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    pairs = np.unique(np.stack([a, b]), axis=1)
    return len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))


# ----------------------------------------------------------------------------- fixtures: (values, lc, hc)

def _box(n):
    return tuple(0.0 for _ in n), tuple(1.0 for _ in n)


def random_field(n, fraction, seed):
    """uniform values: the inside fraction is `fraction`"""
    return (np.asfortranarray(np.random.default_rng(seed).random(n) - fraction),) + _box(n)


def from_mask(inside):
    return (np.asfortranarray(np.where(inside, -1.0, 1.0)),) + _box(inside.shape)


def isolated(n=(130, 70)):
    """the nodes with both indices even: one-node components"""
    i, j = np.meshgrid(*[np.arange(k) for k in n], indexing="ij")
    return from_mask((i % 2 == 0) & (j % 2 == 0))


def diagonals(n=(130, 70)):
    """(i − j) % 3 == 0: one component per (1, 1) diagonal"""
    i, j = np.meshgrid(*[np.arange(k) for k in n], indexing="ij")
    return from_mask((i - j) % 3 == 0)


def spiral(n=(67, 41)):
    """a one-node-wide rectangular arm winding inwards, two nodes of gap between its turns"""
    W, H = n
    m = np.zeros(n, dtype=bool)
    x0, x1, y0, y1 = 0, W - 1, 0, H - 1
    x, y = 0, 0
    m[x, y] = True
    while True:
        if x1 - x < 1:
            break
        m[x:x1 + 1, y] = True; x = x1; y0 += 3           # noqa: E702
        if y1 - y < 1:
            break
        m[x, y:y1 + 1] = True; y = y1; x1 -= 3           # noqa: E702
        if x - x0 < 1:
            break
        m[x0:x + 1, y] = True; x = x0; y1 -= 3           # noqa: E702
        if y - y0 < 1:
            break
        m[x, y0:y + 1] = True; y = y0; x0 += 3           # noqa: E702
    return from_mask(m)


CORNER_DIRECTIONS = [d for d in itertools.product((-1, 0, 1), repeat=3) if d > (0, 0, 0)]      # 13: {−1,0,1}³ up to sign


def corner(delta, n=(16, 16, 16)):
    """two inside nodes, c and c + δ, across the tile corner between the indices 7 and 8"""
    c = tuple(7 if d >= 0 else 8 for d in delta)
    m = np.zeros(n, dtype=bool)
    m[c] = True
    m[tuple(ci + d for ci, d in zip(c, delta))] = True
    return from_mask(m)


def corner_count(delta):
    """1 for the Kuhn directions (all components of one sign), 2 for the others"""
    return 1 if all(d >= 0 for d in delta) or all(d <= 0 for d in delta) else 2


def serpentine(n=24):
    """one path: the x-lines at even y and z, joined at alternating ends; the planes swept to and fro"""
    m = np.zeros((n, n, n), dtype=bool)
    end = 0                                # the x-end where the last line stopped
    ys = list(range(0, n, 2))
    for kz, z in enumerate(range(0, n, 2)):
        order = ys if kz % 2 == 0 else ys[::-1]
        for ky, y in enumerate(order):
            m[:, y, z] = True
            end = n - 1 - end
            if ky + 1 < len(order):
                m[end, (y + order[ky + 1]) // 2, z] = True
        if z + 2 < n:
            m[end, order[-1], z + 1] = True
    return from_mask(m)


def bodies(n=(21, 19, 17)):
    """two spheres and a torus in an anisotropic box: 3 inside components, 1 outside; the smaller sphere is the smallest"""
    lc, hc = (-1.0, -0.8, -0.5), (1.0, 1.1, 0.9)
    x, y, z = np.meshgrid(*[np.linspace(a, b, k) for a, b, k in zip(lc, hc, n)], indexing="ij")
    s1 = np.sqrt((x + 0.55) ** 2 + (y + 0.4) ** 2 + (z + 0.1) ** 2) - 0.3
    s2 = np.sqrt((x - 0.7) ** 2 + (y + 0.5) ** 2 + (z - 0.55) ** 2) - 0.2
    tor = np.sqrt((np.sqrt((x - 0.2) ** 2 + (y - 0.5) ** 2) - 0.42) ** 2 + (z - 0.2) ** 2) - 0.14
    return np.asfortranarray(np.minimum(np.minimum(s1, s2), tor)), lc, hc


def shell(n=21):
    """0.3 < r < 0.6 in [−1, 1]³: 1 inside component, 2 outside"""
    lc, hc = (-1.0,) * 3, (1.0,) * 3
    x, y, z = np.meshgrid(*[np.linspace(-1.0, 1.0, n)] * 3, indexing="ij")
    r = np.sqrt(x * x + y * y + z * z)
    return np.asfortranarray(np.maximum(0.3 - r, r - 0.6)), lc, hc


def largest_share(vals, level=0.0, side="inside"):
    """the share of the set held by its largest component"""
    K, nodes, _, _ = stats(labels(vals, level, side))
    return float(nodes.max()) / float(nodes.sum()) if K else 0.0


# many_tiles: a random 3-D field over 12 × 8 × 5 tiles.  The fraction was chosen with this file: the share of the set in the
# largest cluster over the fractions 0.10 … 0.30 (seed 7) is 0.002, 0.002, 0.004, 0.009, 0.12 (0.18), 0.65 (0.20), 0.83 (0.22),
# 0.93 (0.25), 0.98 (0.30): at 0.20 the clusters have every size and the largest holds 65.2 % of the set
MANY_TILES_SHAPE, MANY_TILES_FRACTION, MANY_TILES_SEED, MANY_TILES_SHARE = (96, 64, 40), 0.20, 7, 0.652
