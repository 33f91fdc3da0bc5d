"""TEST-ONLY restatement of the measures (src/levelsetops.jl:27-33,139-149,171-183; the band volume :49-113): the per-node
terms in fp64 NumPy, summed exactly with math.fsum, so that a device value differs from these by the device's own rounding
only.  The ghost values the centred gradient of `perimeter` reads come from the caller (the oracle's ϕ[I])."""
import math

import numpy as np


def heaviside(x, a):
    """smooth_heaviside(x, α), src/levelsetops.jl:171-179; NaN stays NaN (both comparisons fail, as in the reference)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        mid = 0.5 * (1.0 + x / a + 1.0 / np.pi * np.sin(np.pi * x / a))
        return np.where(x > a, 1.0, np.where(x < -a, 0.0, mid))


def delta(x, a):
    """smooth_delta(x, α), src/levelsetops.jl:181-183; NaN stays NaN."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x) > a, 0.0, 0.5 / a * (1.0 + np.cos(np.pi * x / a)))


def volume(vals, h):
    """prod(h) · Σ H(-ϕ, min h) over every node (src/levelsetops.jl:27-33)."""
    return float(np.prod(h)) * math.fsum(heaviside(-np.asarray(vals, dtype=np.float64), min(h)).ravel())


def pad_faces(vals, ghost):
    """vals with one layer of ghosts on every face: ghost(I) is ϕ[I] for an index one node outside the grid in exactly one
    dimension (0-based).  Edges and corners stay NaN: the centred differences never read them."""
    vals = np.asarray(vals, dtype=np.float64)
    n, N = vals.shape, vals.ndim
    p = np.full(tuple(k + 2 for k in n), np.nan)
    p[(slice(1, -1),) * N] = vals
    for d in range(N):
        others = [range(n[k]) for k in range(N) if k != d]
        for J in np.ndindex(*[len(r) for r in others]):
            for out in (-1, n[d]):
                I = J[:d] + (out,) + J[d:]
                p[tuple(i + 1 for i in I)] = ghost(I)
    return p


def perimeter(padded_or_getter, h, n=None):
    """prod(h) · Σ δ(ϕ[I], min h) · ‖D⁰ϕ[I]‖ over every node (src/levelsetops.jl:139-149).  The field comes as the array of
    pad_faces (interior plus one ghost layer), or as a getter I -> ϕ[I] over the grid of size `n` and its face ghosts."""
    if callable(padded_or_getter):
        get = padded_or_getter
        p = pad_faces(np.array([get(I) for I in np.ndindex(*n)], dtype=np.float64).reshape(n), get)
    else:
        p = np.asarray(padded_or_getter, dtype=np.float64)
    N = p.ndim
    inner = (slice(1, -1),) * N
    nrm2 = None
    for d in range(N):
        up = inner[:d] + (slice(2, None),) + inner[d + 1:]
        dn = inner[:d] + (slice(0, -2),) + inner[d + 1:]
        with np.errstate(invalid="ignore"):
            g = (p[up] - p[dn]) / (2 * h[d])
            nrm2 = g * g if nrm2 is None else nrm2 + g * g
    with np.errstate(invalid="ignore"):
        terms = delta(p[inner], min(h)) * np.sqrt(nrm2)
    return float(np.prod(h)) * math.fsum(terms.ravel())


def geometry_padded(p, h, what):
    """curvature / gradient / normal at every node (src/levelsetops.jl:197-226) from an array that carries one complete ghost
    layer (edges and corners included), in the oracle's operation order (oracle/lsm_oracle.c: D0, D2, D2 mixed, curvature).
    For fields whose ghost values are not what the oracle's dense ϕ[I] returns: a float32 field keeps its ghost layers in
    float32 too, so behind a weighted extrapolation face they are the oracle's values rounded once more.
    tests/test_geometry.py checks this restatement against the oracle itself."""
    p = np.asarray(p, dtype=np.float64)
    N = p.ndim

    def at(*offs):
        o = list(offs) + [0] * (N - len(offs))
        return p[tuple(slice(1 + o[d], p.shape[d] - 1 + o[d]) for d in range(N))]

    def e(d, s=1):
        return tuple(s if k == d else 0 for k in range(N))

    def plus(a, b):
        return tuple(x + y for x, y in zip(a, b))
    with np.errstate(invalid="ignore", divide="ignore"):
        c = at()
        g = [(at(*e(d)) - at(*e(d, -1))) / (2 * h[d]) for d in range(N)]
        nrmsq = g[0] * g[0]
        for d in range(1, N):
            nrmsq = nrmsq + g[d] * g[d]
        if what == "gradient":
            return g
        if what == "normal":
            nrm = np.sqrt(nrmsq)
            return [gd / nrm for gd in g]
        H = [[None] * N for _ in range(N)]
        for a in range(N):
            H[a][a] = (at(*e(a)) - 2 * c + at(*e(a, -1))) / (h[a] * h[a])
            for b in range(a + 1, N):
                H[a][b] = ((at(*plus(e(a), e(b))) - at(*plus(e(a), e(b, -1)))) / (2 * h[b]) -
                           (at(*plus(e(a, -1), e(b))) - at(*plus(e(a, -1), e(b, -1)))) / (2 * h[b])) / (2 * h[a])
        lap = H[0][0]
        for d in range(1, N):
            lap = lap + H[d][d]
        r = np.zeros_like(c)
        for j in range(N):
            r = r + g[j] * (H[j][j] * g[j])
            for i in range(j):
                r = r + (g[i] * (H[i][j] * g[j]) + g[j] * (H[i][j] * g[i]))
        return np.where(nrmsq < 2.220446049250313e-16, 0.0, (lap * nrmsq - r) / nrmsq ** 1.5)


def _band_volume_ref(vals_on_band, n, h, dmin):
    """volume(nb) restated literally (src/levelsetops.jl:49-113): dict of band values (0-based indices), scanlines along
    dimension 1, band-free lines by the nearest band node (exact KD-tree query from the line's point n1÷2)."""
    from scipy.spatial import cKDTree
    d = vals_on_band
    if not d:
        return 0.0
    N = len(n)

    def heaviside(x, a):
        return 1.0 if x > a else (0.0 if x < -a else 0.5 * (1.0 + x / a + np.sin(np.pi * x / a) / np.pi))
    interface = sum(heaviside(-v, dmin) for v in d.values())
    ks = sorted(d.keys(), key=lambda I: (tuple(I[1:][::-1]), I[0]))     # by line, then along dimension 1 (any line order will do)
    count, lines = 0, set()
    i, M = 0, len(ks)
    while i < M:
        j = i
        while j + 1 < M and ks[j + 1][1:] == ks[i][1:]:
            j += 1
        lines.add(ks[i][1:])
        first, last = ks[i], ks[j]
        if d[first] < 0:
            count += first[0]                    # 1-based first[1] - 1
        if d[last] < 0:
            count += n[0] - 1 - last[0]          # n1 - last[1]
        for t in range(i, j):
            gap = ks[t + 1][0] - ks[t][0] - 1
            if gap > 0 and d[ks[t]] < 0 and d[ks[t + 1]] < 0:
                count += gap
        i = j + 1
    transverse = list(np.ndindex(*n[1:])) if N > 1 else [()]
    if len(lines) != len(transverse):
        pts = np.array([[I[k] + 1 for k in range(N)] for I in d.keys()], dtype=float)     # 1-based, as the reference
        neg = [v < 0 for v in d.values()]
        tree = cKDTree(pts)
        for t in transverse:
            if t in lines:
                continue
            _, idx = tree.query(np.array([n[0] // 2] + [c + 1 for c in t], dtype=float))
            if neg[idx]:
                count += n[0]
    return float(np.prod(h)) * (interface + count)
