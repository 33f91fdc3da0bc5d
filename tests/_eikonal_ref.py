"""eikonal_ restated in numpy and plain Python (csrc/lsm_eikonal.hip): the first-order Godunov update G in the
form shifted by the smallest neighbour, the two seedings, and three solvers over the same G and the same strict `G < T` rule —
Jacobi passes (what the tile kernel runs in LDS), Gauss–Seidel sweeps in all 2^N directions, heap fast marching.  No device.
Every operation is spelled in the kernel's order (the library is built with -ffp-contract=off: the device rounds as numpy does).
Arrays are n-shaped, axis 0 fastest in memory (order="F"), as a MeshField's."""
import heapq
import itertools
import math

import numpy as np

INF = float("inf")
EPS = float(np.finfo(np.float64).eps)


def meshsize(n, lc, hc):
    return np.array([(hc[d] - lc[d]) / (n[d] - 1) for d in range(len(n))], dtype=np.float64)


def tol(n, tmax):
    """16·Σ_d(n_d − 1)·eps·max T, the bound on what the visiting order can change: G is non-expansive in the sup norm (∂G/∂a_d >= 0,
    Σ_d ∂G/∂a_d = 1), so the rounding error of one evaluation, a few ulps of max T (16 allows for the sqrt, the division and the
    sums), travels along a causal chain of at most Σ_d(n_d − 1) nodes without growing"""
    return 16.0 * sum(int(k) - 1 for k in n) * EPS * float(tmax)


# ---- the update

def G(a, s, h):
    """G of one node, scalars: a[d] = min of the two neighbours' T along axis d (+inf where none exists or none is finite),
    s the node's slowness, h the mesh sizes"""
    ax = sorted(range(len(a)), key=lambda d: (a[d], d))
    a0 = a[ax[0]]
    if a0 == INF:
        return INF
    tau = s * h[ax[0]]
    for k in range(2, len(a) + 1):
        if not a0 + tau > a[ax[k - 1]]:
            break
        A = B = C = 0.0
        for d in ax[:k]:
            w = 1.0 / (h[d] * h[d])
            dl = a[d] - a0
            A = A + w
            B = B + w * dl
            C = C + (w * dl) * dl
        C = C - s * s
        disc = B * B - A * C
        if disc < 0.0:
            break
        tau = (B + math.sqrt(disc)) / A
    return a0 + tau


def G_vec(a, s, h):
    """G of many nodes: a (N, M), s (M,) or a scalar, h (N,) → (M,); the same operations in the same order as G"""
    N = a.shape[0]
    order = np.argsort(a, axis=0, kind="stable")            # by (a_d, d)
    srt = np.take_along_axis(a, order, axis=0)
    hs = np.asarray(h, dtype=np.float64)[order]
    ws = 1.0 / (hs * hs)
    s = np.broadcast_to(np.asarray(s, dtype=np.float64), srt.shape[1:])
    a0 = srt[0]
    tau = s * hs[0]
    alive = np.isfinite(a0)
    with np.errstate(invalid="ignore"):
        for k in range(2, N + 1):
            go = alive & (a0 + tau > srt[k - 1])
            A = np.zeros_like(a0)
            B = np.zeros_like(a0)
            Cc = np.zeros_like(a0)
            for j in range(k):
                dl = np.where(go, srt[j] - a0, 0.0)
                A = A + ws[j]
                B = B + ws[j] * dl
                Cc = Cc + (ws[j] * dl) * dl
            Cc = Cc - s * s
            disc = B * B - A * Cc
            ok = go & ~(disc < 0.0)
            tau = np.where(ok, (B + np.sqrt(np.where(ok, disc, 0.0))) / A, tau)
            alive = ok
        return np.where(np.isfinite(a0), a0 + tau, INF)


def G_textbook(a, s, h):
    """the un-shifted quadratic Σ (T − a_d)²/h_d² = s², for comparison only (it cancels like (a/h)²)"""
    ax = sorted(range(len(a)), key=lambda d: (a[d], d))
    if a[ax[0]] == INF:
        return INF
    T = a[ax[0]] + s * h[ax[0]]
    for k in range(2, len(a) + 1):
        if not T > a[ax[k - 1]]:
            break
        A = B = C = 0.0
        for d in ax[:k]:
            w = 1.0 / (h[d] * h[d])
            A = A + w
            B = B + w * a[d]
            C = C + (w * a[d]) * a[d]
        C = C - s * s
        disc = B * B - A * C
        if disc < 0.0:
            break
        T = (B + math.sqrt(disc)) / A
    return T


# ---- seeding

def _shift(x, d, step, fill):
    """x[I + step·e_d], `fill` where that node does not exist"""
    out = np.full_like(x, fill)
    src = [slice(None)] * x.ndim
    dst = [slice(None)] * x.ndim
    if step > 0:
        src[d], dst[d] = slice(1, None), slice(None, -1)
    else:
        src[d], dst[d] = slice(None, -1), slice(1, None)
    out[tuple(dst)] = x[tuple(src)]
    return out


def seed(phi, h, slowness=None, width=None):
    """(T, frozen): T = +inf at the free nodes.  width=None: the crossing seed; width = w > 0: |ϕ| where |ϕ| <= w and at every
    crossing-adjacent node.  Raises ValueError for what the library refuses."""
    phi = np.asarray(phi, dtype=np.float64)
    if not np.isfinite(phi).all():
        raise ValueError("non-finite phi")
    N = phi.ndim
    s = np.broadcast_to(np.asarray(1.0 if slowness is None else slowness, dtype=np.float64), phi.shape)
    if not (np.isfinite(s).all() and (s > 0).all()):
        raise ValueError("bad speed")
    ap = np.abs(phi)
    pos = phi > 0
    exists = np.ones(phi.shape, dtype=bool)
    adjacent = np.zeros(phi.shape, dtype=bool)
    acc = np.zeros(phi.shape)
    for d in range(N):
        sig = np.full(phi.shape, INF)
        for step in (-1, 1):
            pj = _shift(phi, d, step, 0.0)
            there = _shift(exists, d, step, False)
            cross = there & (phi != 0) & (((pj > 0) != pos) | (pj == 0))
            with np.errstate(invalid="ignore", divide="ignore"):
                sg = h[d] * (ap / (ap + np.abs(pj)))
            sig = np.where(cross & (sg < sig), sg, sig)
            adjacent |= cross
        has = sig < INF
        with np.errstate(divide="ignore"):
            acc = acc + np.where(has, 1.0 / (sig * sig), 0.0)
    T = np.full(phi.shape, INF)
    if width is None:
        frozen = adjacent | (phi == 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            T = np.where(adjacent, s / np.sqrt(acc), T)
        T = np.where(phi == 0, 0.0, T)
    else:
        frozen = adjacent | (ap <= width)
        T = np.where(frozen, ap, T)
    if not frozen.any():
        raise ValueError("no interface")
    return np.asfortranarray(T), np.asfortranarray(frozen)


# ---- the three solvers

def _neighbour_min(T):
    """a (N, *n): per axis the smaller of the two neighbours, +inf where none exists"""
    return np.stack([np.minimum(_shift(T, d, -1, INF), _shift(T, d, 1, INF)) for d in range(T.ndim)])


def solve_jacobi(T0, frozen, h, slowness=None, max_passes=100000):
    """synchronous passes of T ← G where G < T at the free nodes, to a fixed point; returns (T, passes that changed something)"""
    T = np.array(T0, dtype=np.float64, order="F")
    s = np.broadcast_to(np.asarray(1.0 if slowness is None else slowness, dtype=np.float64), T.shape)
    free = ~frozen
    for it in range(max_passes):
        a = _neighbour_min(T)
        g = G_vec(a.reshape(T.ndim, -1), s.reshape(-1), h).reshape(T.shape)
        upd = free & (g < T)
        if not upd.any():
            return T, it
        T[upd] = g[upd]
    raise RuntimeError("solve_jacobi: no fixed point")


def _a_of(T, I, n):
    a = []
    for d in range(len(n)):
        lo = T[I[:d] + (I[d] - 1,) + I[d + 1:]] if I[d] > 0 else INF
        hi = T[I[:d] + (I[d] + 1,) + I[d + 1:]] if I[d] + 1 < n[d] else INF
        a.append(lo if lo < hi else hi)
    return a


def solve_sweep(T0, frozen, h, slowness=None, max_rounds=1000, update=G):
    """Gauss–Seidel in all 2^N sweep directions, repeated until a whole round accepts nothing"""
    T = np.array(T0, dtype=np.float64, order="F")
    n = T.shape
    s = np.broadcast_to(np.asarray(1.0 if slowness is None else slowness, dtype=np.float64), n)
    hh = [float(x) for x in h]
    for rnd in range(max_rounds):
        changed = False
        for dirs in itertools.product((1, -1), repeat=len(n)):
            ranges = [range(n[d]) if dirs[d] > 0 else range(n[d] - 1, -1, -1) for d in range(len(n))]
            for I in itertools.product(*ranges[::-1]):       # axis 0 innermost
                I = I[::-1]
                if frozen[I]:
                    continue
                g = update(_a_of(T, I, n), float(s[I]), hh)
                if g < T[I]:
                    T[I] = g
                    changed = True
        if not changed:
            return T, rnd
    raise RuntimeError("solve_sweep: no fixed point")


def solve_fmm(T0, frozen, h, slowness=None):
    """heap fast marching: pop the smallest value, re-evaluate its free neighbours (lazy deletion of stale entries)"""
    T = np.array(T0, dtype=np.float64, order="F")
    n = T.shape
    s = np.broadcast_to(np.asarray(1.0 if slowness is None else slowness, dtype=np.float64), n)
    hh = [float(x) for x in h]
    heap = [(float(T[I]), I) for I in zip(*np.nonzero(frozen))]
    heap = [(v, tuple(int(i) for i in I)) for v, I in heap]
    heapq.heapify(heap)
    while heap:
        v, I = heapq.heappop(heap)
        if v > T[I]:
            continue
        for d in range(len(n)):
            for step in (-1, 1):
                j = I[d] + step
                if j < 0 or j >= n[d]:
                    continue
                J = I[:d] + (j,) + I[d + 1:]
                if frozen[J]:
                    continue
                g = G(_a_of(T, J, n), float(s[J]), hh)
                if g < T[J]:
                    T[J] = g
                    heapq.heappush(heap, (g, J))
    return T


TILES = {2: (32, 8), 3: (8, 8, 8)}


def solve_tiles(T0, frozen, h, slowness=None, passes=8, cutoff=INF, snapshot=True, max_iters=None):
    """the device's schedule, one tile after the other: the active tiles run `passes` Jacobi passes on the tile and a one-node halo;
    a tile that changed in its last pass stays active, a changed layer at a face wakes the neighbour across it; a change to a
    value >= cutoff counts for neither.  snapshot=True: every tile of a launch reads the halo as it was before the launch;
    False: as the tiles before it left it — the two ends of what concurrent workgroups may see.  Returns (T, launches, visits)."""
    T = np.array(T0, dtype=np.float64, order="F")
    n, N = T.shape, T.ndim
    tile = TILES[N]
    s = np.broadcast_to(np.asarray(1.0 if slowness is None else slowness, dtype=np.float64), n)
    touch = np.zeros(n, dtype=bool)
    for d in range(N):
        for step in (-1, 1):
            touch |= _shift(frozen, d, step, False)
    active = {tuple(int(I[d]) // tile[d] for d in range(N)) for I in zip(*np.nonzero(~frozen & touch))}
    nt = [-(-n[d] // tile[d]) for d in range(N)]
    if max_iters is None:
        max_iters = 2 * sum(n)
    launches = visits = 0
    while active:
        if launches >= max_iters:
            raise RuntimeError("solve_tiles: the active list did not empty within max_iters")
        src = T.copy() if snapshot else T
        nxt = set()
        for b in sorted(active):
            lo = [b[d] * tile[d] for d in range(N)]
            hi = [min(lo[d] + tile[d], n[d]) for d in range(N)]
            P = np.full([hi[d] - lo[d] + 2 for d in range(N)], INF)
            glo = [max(lo[d] - 1, 0) for d in range(N)]
            ghi = [min(hi[d] + 1, n[d]) for d in range(N)]
            P[tuple(slice(glo[d] - lo[d] + 1, ghi[d] - lo[d] + 1) for d in range(N))] = src[tuple(slice(glo[d], ghi[d]) for d in range(N))]
            own = tuple(slice(lo[d], hi[d]) for d in range(N))
            inner = P[tuple(slice(1, -1) for _ in range(N))]
            fr, ss = frozen[own], s[own]
            stay, faces = False, set()
            for _ in range(passes):
                a = np.stack([np.minimum(P[tuple(slice(0, -2) if k == d else slice(1, -1) for k in range(N))],
                                         P[tuple(slice(2, None) if k == d else slice(1, -1) for k in range(N))]) for d in range(N)])
                g = G_vec(a.reshape(N, -1), ss.reshape(-1), h).reshape(inner.shape)
                take = ~fr & (g < inner)
                live = take & (g < cutoff)
                inner[take] = g[take]
                for d in range(N):
                    if np.take(live, 0, axis=d).any():
                        faces.add((d, -1))
                    if hi[d] - lo[d] == tile[d] and np.take(live, tile[d] - 1, axis=d).any():      # a partial tile has no neighbour there
                        faces.add((d, 1))
                stay = bool(live.any())
                if not stay:
                    break
            T[own] = inner
            if stay:
                nxt.add(b)
            for d, side in faces:
                if 0 <= b[d] + side < nt[d]:
                    nxt.add(b[:d] + (b[d] + side,) + b[d + 1:])
        visits += len(active)
        launches += 1
        active = nxt
    return T, launches, visits


def residual(T, frozen, h, slowness=None):
    """max over the free nodes of |G(T's neighbours) − T|"""
    s = np.broadcast_to(np.asarray(1.0 if slowness is None else slowness, dtype=np.float64), T.shape)
    g = G_vec(_neighbour_min(T).reshape(T.ndim, -1), s.reshape(-1), h).reshape(T.shape)
    free = ~frozen
    return float(np.abs(g[free] - T[free]).max()) if free.any() else 0.0


def eikonal(phi, h, speed=None, width=None, cutoff=None, T=None):
    """what eikonal_ writes: copysign(min(T, cutoff), ϕ), T the Jacobi fixed point (or the one given)"""
    phi = np.asarray(phi, dtype=np.float64)
    slow = None if speed is None else 1.0 / np.broadcast_to(np.asarray(speed, dtype=np.float64), phi.shape)
    if T is None:
        T0, frozen = seed(phi, h, slow, width)
        T, _ = solve_jacobi(T0, frozen, h, slow)
    c = INF if cutoff is None else float(cutoff)
    return np.copysign(np.minimum(T, c), phi)


# ---- the fixtures the host and the device tests share

def nodes(n, lc, hc):
    h = meshsize(n, lc, hc)
    return np.meshgrid(*[lc[d] + np.arange(n[d]) * h[d] for d in range(len(n))], indexing="ij")


def spheres(n, lc, hc, balls):
    """min over the balls (centre, radius) of |x − c| − r"""
    X = nodes(n, lc, hc)
    out = None
    for c, r in balls:
        d = np.sqrt(sum((X[k] - c[k]) ** 2 for k in range(len(n)))) - r
        out = d if out is None else np.minimum(out, d)
    return np.asfortranarray(out)


def random_speed(n, seed_=7):
    """speeds whose slowness 1/F is uniform in [0.25, 3.25]"""
    rng = np.random.default_rng(seed_)
    return np.asfortranarray(1.0 / (0.25 + 3.0 * rng.random(n)))


# name: (n, lc, hc, balls, speed or None).  Anisotropic spacing everywhere: the box is not a cube of n − 1 equal cells.
FIXTURES = {
    "one_tile": ((5, 7, 6), (-1.0, -1.1, -0.9), (1.0, 1.2, 1.1), [((0.1, 0.0, 0.1), 0.55)], None),
    "partial_tiles": ((13, 12, 11), (-1.0, -1.1, -0.9), (1.0, 1.2, 1.1), [((0.1, 0.0, 0.1), 0.6)], None),
    "nine_tiles_3d": ((67, 9, 8), (-4.0, -0.5, -0.45), (4.2, 0.55, 0.5), [((-3.3, 0.02, 0.01), 0.3)], None),
    "nine_tiles_2d": ((67, 9), (-4.0, -0.5), (4.2, 0.55), [((-3.3, 0.02), 0.3)], None),
    "two_circles": ((41, 37), (-1.0, -1.0), (1.1, 1.0), [((-0.45, -0.3), 0.3), ((0.5, 0.35), 0.22)], None),
    "two_spheres_speed": ((13, 12, 11), (-1.0, -1.1, -0.9), (1.0, 1.2, 1.1), [((-0.4, -0.4, -0.3), 0.4), ((0.5, 0.5, 0.4), 0.3)], "random"),
    "cut_by_face": ((13, 12, 11), (-1.0, -1.1, -0.9), (1.0, 1.2, 1.1), [((0.9, 0.0, 0.1), 0.5)], None),
    "cut_by_face_2d": ((33, 30), (-1.0, -1.0), (1.0, 1.1), [((0.9, 0.1), 0.45)], None),
    "tiny_h": ((33, 30), (0.0, 0.0), (32 * 0.002, 29 * 0.0021), [((0.03, 0.03), 0.015)], "random"),
}


def fixture(name):
    """(phi, n, lc, hc, h, speed)"""
    n, lc, hc, balls, sp = FIXTURES[name]
    phi = spheres(n, lc, hc, balls)
    speed = random_speed(n) if sp == "random" else None
    return phi, n, lc, hc, meshsize(n, lc, hc), speed
