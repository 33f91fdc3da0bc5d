"""eikonal_ restated in numpy and plain Python (csrc/lsm_eikonal.hip): the first-order Godunov update G in the
form shifted by the smallest neighbour, the two seedings, and three solvers over the same G and the same strict `G < T` rule —
Jacobi passes (what the tile kernel runs in LDS), Gauss–Seidel sweeps in all 2^N directions, heap fast marching.  No device.
Every operation is spelled in the kernel's order (the library is built with -ffp-contract=off: the device rounds as numpy does).
Further down: the device's tile schedule run one tile after the other, what must hold of any of its fixed points (`unsatisfied`,
`residual`), and the fixtures the host and the device tests share — spheres, checkerboards, plane fronts, seed fields.
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

def _G_and_stage(a, s, h):
    ax = sorted(range(len(a)), key=lambda d: (a[d], d))
    a0 = a[ax[0]]
    if a0 == INF:
        return INF, 0
    tau, stage = s * h[ax[0]], 1
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
        tau, stage = (B + math.sqrt(disc)) / A, k
    return a0 + tau, stage


def G(a, s, h):
    """G of one node, scalars: a[d] = min of the two neighbours' T along axis d (+inf where none exists or none is finite),
    s the node's slowness, h the mesh sizes"""
    return _G_and_stage(a, s, h)[0]


def G_stage(a, s, h):
    """which stage of G produced τ: 1 (τ = s·h of the smallest axis: a0 + τ <= a1, or there is no second axis), 2 (the quadratic
    over the two smallest axes) or 3 (over all three); 0 where every a_d is +inf.  The two `disc < 0` guards are not counted as
    a stage of their own because exact arithmetic cannot reach them: stage k is entered only when a0 + τ > a_k with τ the
    solution over the first k − 1 axes, and then the quadratic over k axes has a root >= a_k − a0 (for k = 2: δ1 = a1 − a0 < s·h0
    gives disc = w1·(s² − w0·δ1²) + w0·s² > w0·s² > 0).  No fixture tries to reach them."""
    return _G_and_stage(a, s, h)[1]


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


def unsatisfied(T, frozen, h, slowness=None, where=None):
    """the number of free nodes (of `where`, if given) with G(T's neighbours) < T: 0 at any fixed point of the strict `G < T`
    rule, whatever the visiting order, because the comparison is the solver's own and G here is the solver's G bit for bit.
    Rounding cannot leave such a node; a tile that was not woken after its neighbour's layer fell does."""
    s = np.broadcast_to(np.asarray(1.0 if slowness is None else slowness, dtype=np.float64), T.shape)
    g = G_vec(_neighbour_min(T).reshape(T.ndim, -1), s.reshape(-1), h).reshape(T.shape)
    bad = ~frozen & (g < T)
    if where is not None:
        bad &= where
    return int(bad.sum())


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


# the sizes at which the tile schedule shows: 8·7·6 = 336 tiles of 8×8×8 (the last ones 1, 2 and 3 nodes thick), 10·30 = 300 of
# 32×8; two compaction workgroups.  Kept out of FIXTURES: the host parametrisations over those run pure-Python sweeps and a heap.
LARGE = {
    "many_tiles_3d": ((57, 50, 43), (-1.0, -1.1, -0.9), (1.0, 1.2, 1.1), [((-0.4, -0.4, -0.3), 0.4), ((0.5, 0.5, 0.4), 0.3)], None),
    "many_tiles_3d_speed": ((57, 50, 43), (-1.0, -1.1, -0.9), (1.0, 1.2, 1.1), [((-0.4, -0.4, -0.3), 0.4), ((0.5, 0.5, 0.4), 0.3)], "random"),
    "many_tiles_2d": ((290, 235), (-1.0, -1.0), (1.1, 1.0), [((-0.45, -0.3), 0.3), ((0.5, 0.35), 0.22)], None),
}


def fixture(name):
    """(phi, n, lc, hc, h, speed)"""
    n, lc, hc, balls, sp = FIXTURES[name] if name in FIXTURES else LARGE[name]
    phi = spheres(n, lc, hc, balls)
    speed = random_speed(n) if sp == "random" else None
    return phi, n, lc, hc, meshsize(n, lc, hc), speed


def ntiles(n):
    return int(np.prod([-(-int(k) // e) for k, e in zip(n, TILES[len(n)])]))


# ---- checkerboards: every free node's neighbours are frozen, so its result is G of chosen inputs after one pass, whatever the
# schedule — the update and the launch bookkeeping bit for bit at any number of tiles

# name: (n, nominal h).  The 2-node grids are the smallest lsm_eikonal takes, the 4-node ones the smallest a device handle has
CHECKERBOARDS = {
    "cb_336_tiles": ((57, 50, 43), (0.3, 0.02, 0.11)),
    "cb_300_tiles": ((290, 235), (0.3, 0.02)),
    "cb_one_tile": ((7, 6, 5), (0.3, 0.02, 0.11)),
    "cb_4x4x4": ((4, 4, 4), (0.3, 0.02, 0.11)),
    "cb_4x4": ((4, 4), (0.3, 0.02)),
    "cb_2x2x2": ((2, 2, 2), (0.3, 0.02, 0.11)),
    "cb_2x2": ((2, 2), (0.3, 0.02)),
}
CB_FREE = 1000.0        # |ϕ| of the free nodes: beyond any width
_CB_KINDS = {3: ("tie_small", "tie_large") * 3 + ("dominated",) * 2 + ("close",) * 2, 2: ("tie",) * 6 + ("dominated",) * 2 + ("close",) * 2}


def checkerboard(name, sign=1.0, f32=False):
    """(phi, n, lc, hc, h, speed, w) with one sign of ϕ over the grid, for the width seeding with w = 3·h_max: node I is free iff
    Σ I_d is odd and holds |ϕ| = CB_FREE; every other node holds a value in (0, 0.99·w] and is frozen at it.  The values are
    uniform, except around the free nodes of the lattice 3·J + 1 (no two of them share a neighbour), whose neighbour minima a_d
    are planted in turn: the two smallest equal (`tie_small`), the two largest equal with a0 up to 2·s·h below them
    (`tie_large`: stage 1 or stage 3), the smallest so far below the rest that a0 + s·h <= a1 (`dominated`), all within
    0.2·s·h_min (`close`: stage 3); the minimum sits at the lower or the upper neighbour at random, the other one is equal to
    it one time in four.  f32: the values rounded to float32 (ties stay ties).  The speed is random_speed's."""
    n, hn = CHECKERBOARDS[name]
    N = len(n)
    lc, hc = (0.0,) * N, tuple(hn[d] * (n[d] - 1) for d in range(N))
    h = meshsize(n, lc, hc)
    w = 3.0 * float(h.max())
    rng = np.random.default_rng(11)
    speed = random_speed(n)
    idx = np.indices(n)
    free = idx.sum(axis=0) % 2 == 1
    vals = 0.99 * w * (1.0 - rng.random(n))
    sites = [I for I in itertools.product(*[range(1, n[d] - 1, 3) for d in range(N)]) if sum(I) % 2 == 1]
    kinds = _CB_KINDS[N]
    top = 0.99 * w
    for k, at in enumerate(rng.permutation(len(sites))):
        I = sites[at]
        s = 1.0 / float(speed[I])
        p = [int(x) for x in rng.permutation(N)]
        u = rng.random(4)
        a = [0.0] * N
        kind = kinds[k % len(kinds)]
        if kind in ("tie_small", "tie"):
            v = w * (0.01 + 0.89 * u[0])
            a[p[0]] = a[p[1]] = v
            if N > 2:
                a[p[2]] = v + (top - v) * u[1]
        elif kind == "tie_large":
            v = w * (0.3 + 0.69 * u[0])
            a[p[1]] = a[p[2]] = v
            a[p[0]] = v - u[1] * min(2.0 * s * float(h[p[0]]), 0.9 * v)
        elif kind == "dominated":
            if 1.01 * s * float(h[p[0]]) + 0.01 * w >= 0.98 * w:
                p.remove(int(np.argmin(h)))
                p.insert(0, int(np.argmin(h)))
            a[p[0]] = 0.01 * w * (1.0 - u[0])
            lo = a[p[0]] + 1.01 * s * float(h[p[0]])
            for j in range(1, N):
                a[p[j]] = lo + (top - lo) * u[j]
        else:
            a[p[0]] = w * (0.01 + 0.7 * u[0])
            for j in range(1, N):
                a[p[j]] = a[p[0]] + 0.2 * u[j] * s * float(h.min())
        for d in range(N):
            side = 1 if rng.random() < 0.5 else -1
            other = a[d] if rng.random() < 0.25 else a[d] + (top - a[d]) * rng.random()
            vals[I[:d] + (I[d] + side,) + I[d + 1:]] = a[d]
            vals[I[:d] + (I[d] - side,) + I[d + 1:]] = other
    if f32:
        vals = vals.astype(np.float32).astype(np.float64)
    phi = np.asfortranarray(float(sign) * np.where(free, CB_FREE, vals))
    return phi, n, lc, hc, h, speed, w


def checkerboard_census(phi, h, speed, w):
    """(free, g, stage, ties of the two smallest a_d, ties of the two largest): at every free node of a checkerboard the scalar
    G and G_stage of its neighbour minima (g and stage are n-shaped, 0 at the frozen nodes), and the numbers of free nodes
    whose two smallest, and whose two largest, a_d are exactly equal"""
    T0, frozen = seed(phi, h, 1.0 / speed, w)
    a = _neighbour_min(T0)
    hh = [float(x) for x in h]
    g = np.zeros(phi.shape, order="F")
    stage = np.zeros(phi.shape, dtype=np.int64, order="F")
    for I in zip(*np.nonzero(~frozen)):
        g[I], stage[I] = _G_and_stage([float(x) for x in a[(slice(None),) + I]], 1.0 / float(speed[I]), hh)
    srt = np.sort(a[:, ~frozen], axis=0)
    return ~frozen, g, stage, int((srt[0] == srt[1]).sum()), int((srt[-1] == srt[-2]).sum())


# ---- plane fronts: with s ≡ 1 a front that leaves a face of zeros moves along one axis only.  A node's lateral neighbours hold
# either +inf or exactly fl(a0 + h_d), its own stage-1 value, so stage 2 is never entered and every node is a0 + h_d whatever a
# tile read of its neighbours' layers: values, launches and visits do not depend on the schedule, and the tiles of layer b + 1
# along the axis are reached through the face flag of layer b alone (a lateral wake-up comes one launch later and shows in both
# counts).

def plane(name, axis, end):
    """(phi, n, lc, hc, h) on the grid of LARGE[name]: ϕ = x_axis − its value at the first (end 0: ϕ >= 0) or the last node
    (end 1: ϕ <= 0, the zeros −0.0) of the axis; the crossing seed freezes the face of zeros and the layer next to it"""
    n, lc, hc = LARGE[name][:3]
    h = meshsize(n, lc, hc)
    k = np.indices(n)[axis].astype(np.float64)
    phi = h[axis] * (k - (0 if end == 0 else n[axis] - 1))
    return np.asfortranarray(np.where(phi == 0, -0.0, phi) if end else phi), n, lc, hc, h


# ---- the seeding's edge cases as fields (test_eikonal_host.test_seeding_edge_cases states the rules on the same 2-D ones)

def seed_fields():
    """name → (phi, lc, hc, is a distance): 2-D fields on (5, 4) with h = (0.5, 0.25), 3-D ones on (5, 4, 6) with
    h = (0.5, 0.25, 0.125), and the smallest grids of a device handle with one node of the other sign"""
    lc2, hc2 = (0.0, 0.0), (2.0, 0.75)
    lc3, hc3 = (0.0, 0.0, 0.0), (2.0, 0.75, 0.625)
    line = np.array([[-1.0, -0.5, 0.0, 0.5, 1.0]] * 4).T
    i2, j2 = np.indices((5, 4)).astype(np.float64)
    i3, j3, k3 = np.indices((5, 4, 6)).astype(np.float64)
    out = {
        "zero_line": (line, lc2, hc2, True),                                              # ϕ = 0 on a node, zero neighbours beside it
        "negative_zero_line": (np.where(line == 0, -0.0, line), lc2, hc2, True),          # the sign bit comes back
        "one_zero_node": ((i2 - 2.0) * 0.5 + (j2 - 1.0) * 0.125, lc2, hc2, False),        # ϕ_J = 0 next to ϕ_I != 0, along both axes
        "sliver": (np.array([[1.0, 0.75, -0.05, 0.2, 1.0]] * 4).T, lc2, hc2, False),      # one node thick: crossings on both sides
        "leaves_through_a_face": (i2 * 0.5 - 1.6 + 0.0 * j2, lc2, hc2, True),             # seeded from the neighbours that exist
        "zero_plane": ((i3 - 2.0) * 0.5 + 0.0 * j3, lc3, hc3, True),
        "face_node_one_axis": (k3 * 0.125 - 0.55 + 0.0 * i3, lc3, hc3, True),             # the face k = 5 crosses along axis 2 only
        "corner_4x4": (np.where(i2[:4] + j2[:4] == 0, -0.3, 0.2 + 0.01 * i2[:4] + 0.03 * j2[:4]), lc2, (1.5, 0.75), False),
        "corner_4x4x4": (np.where(i3[:4, :, :4] + j3[:4, :, :4] + k3[:4, :, :4] == 0, -0.3, 0.2 + 0.01 * i3[:4, :, :4] + 0.03 * j3[:4, :, :4] + 0.02 * k3[:4, :, :4]),
                         lc3, (1.5, 0.75, 0.375), False),
        "corner_2x2": (np.array([[-0.3, 0.2], [0.25, 0.4]]), lc2, (0.5, 0.25), False),
        "corner_2x2x2": (np.where(i3[:2, :2, :2] + j3[:2, :2, :2] + k3[:2, :2, :2] == 0, -0.3, 0.2 + 0.05 * i3[:2, :2, :2] + 0.03 * j3[:2, :2, :2] + 0.02 * k3[:2, :2, :2]),
                         lc3, (0.5, 0.25, 0.125), False),
    }
    return {k: (np.asfortranarray(v[0]), v[1], v[2], v[3]) for k, v in out.items()}
