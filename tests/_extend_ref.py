"""extend_from_interface_ restated in numpy and plain Python (csrc/lsm_eikonal.hip, the comment at lsm_extend in include/lsm.h,
DESIGN.md §7.28): the frozen sets, the two seed sources, the cutoff and the orphans, and three solvers of the same triangular
system — the nodes in key order (a stable sort of g = |ϕ|), global Jacobi waves, and the device's tile schedule run one tile after
the other with both halo orders of _eikonal_ref.solve_tiles.  Every entry is computed exactly once from final values, so the three
give the same bits; every operation is spelled in the kernel's order (the library is built with -ffp-contract=off).  No device.
Arrays are n-shaped, axis 0 fastest in memory (order="F"), as a MeshField's."""
import functools

import numpy as np

import _eikonal_ref as R

INF = float("inf")
NAN = float("nan")
PASSES = 8


class Refused(ValueError):
    def __init__(self, reason, offenders, what):
        super().__init__(what)
        self.reason, self.offenders = reason, offenders


# ---- the frozen set and the seeds

def crossings(phi, h):
    """(adjacent, per axis (has, theta, sigma, step)): ek_seed_kernel's crossing test; per axis the crossing neighbour with the
    smaller sigma = h·(|ϕ_I|/(|ϕ_I| + |ϕ_J|)), the − side on a tie; theta = |ϕ_I|/(|ϕ_I| + |ϕ_J|) of that neighbour"""
    ap = np.abs(phi)
    pos = phi > 0
    exists = np.ones(phi.shape, dtype=bool)
    adjacent = np.zeros(phi.shape, dtype=bool)
    axes = []
    for d in range(phi.ndim):
        sig = np.full(phi.shape, INF)
        theta = np.zeros(phi.shape)
        step_of = np.zeros(phi.shape, dtype=np.int64)
        for step in (-1, 1):
            pj = R._shift(phi, d, step, 0.0)
            there = R._shift(exists, d, step, False)
            cross = there & (phi != 0) & (((pj > 0) != pos) | (pj == 0))
            with np.errstate(invalid="ignore", divide="ignore"):
                th = ap / (ap + np.abs(pj))
                sg = h[d] * th
            better = cross & (sg < sig)
            sig = np.where(better, sg, sig)
            theta = np.where(better, th, theta)
            step_of = np.where(better, step, step_of)
            adjacent |= cross
        axes.append((sig < INF, theta, sig, step_of))
    return adjacent, axes


def frozen_nodes(phi, h, rule="rule", width=None, mask=None):
    if rule == "rule":
        adjacent, _ = crossings(phi, h)
        return adjacent | ((phi == 0) if width is None else (np.abs(phi) <= width))
    if rule == "mask":
        return np.asarray(mask) != 0
    if rule == "inside":
        return phi <= 0
    if rule == "outside":
        return phi >= 0
    raise ValueError(rule)


def keys(phi, rule="rule"):
    """g: |ϕ|; under "inside" ϕ and under "outside" −ϕ — the same at the free nodes, but every frozen node lies below every free
    one, so a free node next to the interface depends on its frozen neighbour however far inside that one sits"""
    return phi if rule == "inside" else -phi if rule == "outside" else np.abs(phi)


def _clamp(q, lo, hi):
    r = np.where(q >= lo, q, lo)         # comparisons, not fmin/fmax: the sign of a zero and a NaN go one way only
    return np.where(r <= hi, r, hi)


def reseed(F, phi, h):
    """source="interface": the crossing-adjacent nodes take the value at their crossings, from the input field F"""
    adjacent, axes = crossings(phi, h)
    num = np.zeros(phi.shape)
    den = np.zeros(phi.shape)
    lo = np.full(phi.shape, INF)
    hi = np.full(phi.shape, -INF)
    for d, (has, theta, sig, step_of) in enumerate(axes):
        FJ = np.where(step_of < 0, R._shift(F, d, -1, 0.0), R._shift(F, d, 1, 0.0))
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            Fg = F + theta * (FJ - F)
            u = 1.0 / (sig * sig)
            num = np.where(has, num + Fg * u, num)
            den = np.where(has, den + u, den)
        lo = np.where(has & (Fg < lo), Fg, lo)
        hi = np.where(has & (Fg > hi), Fg, hi)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = _clamp(num / den, lo, hi)
    return np.where(adjacent, v, F)


class Problem:
    """what the init kernel leaves: g, the fixed nodes (frozen, filled at the cutoff, orphans), the participating neighbours and
    their weights, the working copies W[k] (NaN where a value is still to be computed) and the counts"""


def prepare(phi, h, F, rule="rule", width=None, mask=None, source="nodes", cutoff=None, fill=0.0):
    phi = np.asarray(phi, dtype=np.float64)
    F = [np.asarray(f, dtype=np.float64) for f in F]
    n, N = phi.shape, phi.ndim
    if source == "interface" and rule != "rule":
        raise ValueError("source='interface' goes with the rule's frozen set only")
    P = Problem()
    P.n, P.N, P.h = n, N, np.asarray(h, dtype=np.float64)
    bad_phi = int((~np.isfinite(phi)).sum())
    if bad_phi:
        raise Refused(1, bad_phi, "non-finite phi")
    g = np.asfortranarray(keys(phi, rule))
    frozen = frozen_nodes(phi, h, rule, width, mask)
    c_off = INF if cutoff is None else float(cutoff)
    part, take_lo, cs = [], [], []
    for d in range(N):
        lo, hi = R._shift(g, d, -1, INF), R._shift(g, d, 1, INF)
        tl = lo <= hi                                    # a tie: the − side
        a = np.where(tl, lo, hi)
        w = 1.0 / (P.h[d] * P.h[d])
        with np.errstate(invalid="ignore"):
            cs.append(np.asfortranarray(w * (g - a)))
        part.append(np.asfortranarray(a < g))
        take_lo.append(np.asfortranarray(tl))
    anypart = np.logical_or.reduce(part)
    filled = ~frozen & (g >= c_off)
    orphan = ~frozen & ~filled & ~anypart
    kept = frozen | orphan                               # an orphan behaves as frozen, the refusal included
    bad_F = np.zeros(n, dtype=bool)
    for f in F:
        bad_F |= kept & ~np.isfinite(f)
    if bad_F.any():
        raise Refused(2, int(bad_F.sum()), "a non-finite F at a frozen node")
    if not frozen.any():
        raise Refused(3, 0, "no frozen node")
    P.g, P.frozen, P.filled, P.orphan = g, np.asfortranarray(frozen), filled, orphan
    P.fixed = np.asfortranarray(frozen | filled | orphan)
    P.part, P.take_lo, P.c = part, take_lo, cs
    P.W = []
    for f in F:
        seeds = reseed(f, phi, h) if source == "interface" else f
        w = np.where(filled, float(fill), np.where(kept, seeds, NAN))
        P.W.append(np.asfortranarray(w))
    P.stats = {"frozen": int(frozen.sum()), "orphans": int(orphan.sum()), "filled": int(filled.sum())}
    return P


# ---- the update of one entry: (Σ c_d·F_d)/(Σ c_d) over the participating axes, ascending, clamped to their range

def _combine(part, c, FJ):
    """arrays: part[d], c[d], FJ[d] (the chosen neighbour's value) → (value, ready)"""
    shape = part[0].shape
    num, den = np.zeros(shape), np.zeros(shape)
    lo, hi = np.full(shape, INF), np.full(shape, -INF)
    ready = np.ones(shape, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for d in range(len(part)):
            p, f = part[d], FJ[d]
            ready &= ~p | ~np.isnan(f)
            num = np.where(p, num + c[d] * f, num)
            den = np.where(p, den + c[d], den)
            lo = np.where(p & (f < lo), f, lo)
            hi = np.where(p & (f > hi), f, hi)
        return _clamp(num / den, lo, hi), ready


def solve_key_order(P):
    """every free node once, in ascending g (a stable sort over the linear index, axis 0 fastest): scalar Python"""
    n, N = P.n, P.N
    stride = [int(np.prod(n[:d])) for d in range(N)]
    g = P.g.ravel(order="F")
    fixed = P.fixed.ravel(order="F")
    part = [p.ravel(order="F").tolist() for p in P.part]
    off = [np.where(P.take_lo[d], -stride[d], stride[d]).ravel(order="F").tolist() for d in range(N)]
    c = [x.ravel(order="F").tolist() for x in P.c]
    order = np.argsort(g, kind="stable").tolist()
    out = []
    for W in P.W:
        w = W.ravel(order="F").tolist()
        for i in order:
            if fixed[i]:
                continue
            num = den = 0.0
            lo, hi = INF, -INF
            for d in range(N):
                if part[d][i]:
                    f = w[i + off[d][i]]
                    assert f == f, "key order met an unset neighbour"
                    num = num + c[d][i] * f
                    den = den + c[d][i]
                    if f < lo:
                        lo = f
                    if f > hi:
                        hi = f
            q = num / den if den != 0.0 else NAN
            r = q if q >= lo else lo
            w[i] = r if r <= hi else hi
        out.append(np.asfortranarray(np.array(w).reshape(n, order="F")))
    return out


def _neighbour_values(W, take_lo):
    return [np.where(take_lo[d], R._shift(W, d, -1, NAN), R._shift(W, d, 1, NAN)) for d in range(W.ndim)]


def solve_waves(P):
    """global Jacobi passes: every entry whose participating neighbours are all set is computed; returns (fields, passes)"""
    out, passes = [], 0
    for W in P.W:
        W = W.copy(order="F")
        k = 0
        while True:
            todo = np.isnan(W)
            if not todo.any():
                break
            v, ready = _combine(P.part, P.c, _neighbour_values(W, P.take_lo))
            take = todo & ready
            assert take.any(), "no entry is ready: the dependency graph is not acyclic"
            W[take] = v[take]
            k += 1
        passes = max(passes, k)
        out.append(W)
    return out, passes


def solve_tiles(P, snapshot=True, max_iters=None):
    """the device's schedule, one tile after the other (see _eikonal_ref.solve_tiles for `snapshot`): up to PASSES Jacobi passes per
    visit; a tile that set something in its last pass stays listed, an entry set in a face layer wakes the neighbour across it.
    Returns (fields, launches, visits)."""
    n, N = P.n, P.N
    tile = R.TILES[N]
    Ws = [W.copy(order="F") for W in P.W]
    fixed = P.fixed
    touch = np.zeros(n, dtype=bool)
    for d in range(N):
        for step in (-1, 1):
            touch |= R._shift(fixed, d, step, False)
    active = {tuple(int(I[d]) // tile[d] for d in range(N)) for I in zip(*np.nonzero(~fixed & touch))}
    nt = [-(-n[d] // tile[d]) for d in range(N)]
    if max_iters is None:
        max_iters = 2 * sum(n)
    launches = visits = 0
    while active:
        if launches >= max_iters:
            raise RuntimeError("solve_tiles: the active list did not empty within max_iters")
        srcs = [W.copy() for W in Ws] if snapshot else Ws
        nxt = set()
        for b in sorted(active):
            lo = [b[d] * tile[d] for d in range(N)]
            hi = [min(lo[d] + tile[d], n[d]) for d in range(N)]
            own = tuple(slice(lo[d], hi[d]) for d in range(N))
            glo = [max(lo[d] - 1, 0) for d in range(N)]
            ghi = [min(hi[d] + 1, n[d]) for d in range(N)]
            part = [p[own] for p in P.part]
            tl = [t[own] for t in P.take_lo]
            cc = [c[own] for c in P.c]
            fr = fixed[own]
            stay, faces = False, set()
            for W, src in zip(Ws, srcs):
                Pd = np.full([hi[d] - lo[d] + 2 for d in range(N)], NAN)
                Pd[tuple(slice(glo[d] - lo[d] + 1, ghi[d] - lo[d] + 1) for d in range(N))] = src[tuple(slice(glo[d], ghi[d]) for d in range(N))]
                inner = Pd[tuple(slice(1, -1) for _ in range(N))]
                last = False
                for _ in range(PASSES):
                    FJ = [np.where(tl[d], Pd[tuple(slice(0, -2) if k == d else slice(1, -1) for k in range(N))],
                                   Pd[tuple(slice(2, None) if k == d else slice(1, -1) for k in range(N))]) for d in range(N)]
                    v, ready = _combine(part, cc, FJ)
                    take = ~fr & np.isnan(inner) & ready
                    inner[take] = v[take]
                    for d in range(N):
                        if np.take(take, 0, axis=d).any():
                            faces.add((d, -1))
                        if hi[d] - lo[d] == tile[d] and np.take(take, tile[d] - 1, axis=d).any():
                            faces.add((d, 1))
                    last = bool(take.any())
                    if not last:
                        break
                stay = stay or last
                W[own] = inner
            if stay:
                nxt.add(b)
            for d, side in faces:
                if 0 <= b[d] + side < nt[d]:
                    nxt.add(b[:d] + (b[d] + side,) + b[d + 1:])
        visits += len(active)
        launches += 1
        active = nxt
    return Ws, launches, visits


def extend(phi, h, F, rule="rule", width=None, mask=None, source="nodes", cutoff=None, fill=0.0):
    """what extend_from_interface_ writes: (fields, stats); raises Refused for what the library refuses"""
    P = prepare(phi, h, F, rule, width, mask, source, cutoff, fill)
    out, _ = solve_waves(P)
    assert not any(np.isnan(w).any() for w in out)
    return out, P.stats


# ---- fixtures: ϕ = copysign(T_jacobi, ϕ0) of _eikonal_ref's fixtures (a first-order distance: no orphan, see test_extend_host),
# seed fields, planted orphans

def widths(h):
    return (None, 1.5 * float(h.max()))


# beside _eikonal_ref.FIXTURES: a 2-D grid inside one tile, and fronts that must wake tiles along axis 1 and axis 2 in turn
# (nine_tiles_* do along axis 0).  name: (n, lc, hc, balls)
EXTRA = {
    "one_tile_2d": ((5, 4), (-1.0, -1.1), (1.0, 1.2), [((0.1, 0.0), 0.55)]),
    "wake_axis1_3d": ((9, 67, 8), (-0.5, -4.0, -0.45), (0.55, 4.2, 0.5), [((0.02, -3.3, 0.01), 0.3)]),
    "wake_axis2_3d": ((9, 8, 67), (-0.5, -0.45, -4.0), (0.55, 0.5, 4.2), [((0.02, 0.01, -3.3), 0.3)]),
    "wake_axis1_2d": ((40, 67), (-0.5, -4.0), (0.55, 4.2), [((0.02, -3.3), 0.3)]),
}


@functools.lru_cache(maxsize=None)
def distance(name, seeding=0):
    """(ϕ, n, lc, hc, h): ϕ = copysign(T, ϕ0), T the Jacobi fixed point with s ≡ 1 seeded by `seeding`; read-only"""
    if name in EXTRA:
        n, lc, hc, balls = EXTRA[name]
        phi0, h = R.spheres(n, lc, hc, balls), R.meshsize(n, lc, hc)
    else:
        phi0, n, lc, hc, h, _ = R.fixture(name)
    T0, frozen = R.seed(phi0, h, None, widths(h)[seeding])
    T, _ = R.solve_jacobi(T0, frozen, h, None)
    phi = np.asfortranarray(np.copysign(T, phi0))
    phi.setflags(write=False)
    return phi, n, lc, hc, h


def fields(n, lc, hc, K, seed_=5):
    """K seed fields: the first few smooth (a coordinate, a product, the unit normal's first component of the box centre), the
    rest random in [−1, 1]; deterministic"""
    X = R.nodes(n, lc, hc)
    rng = np.random.default_rng(seed_)
    out = []
    for k in range(K):
        if k == 0:
            f = X[0] + 0.5 * X[-1]
        elif k == 1:
            f = np.cos(3.0 * X[0]) * np.sin(2.0 * X[1] + 0.3)
        else:
            f = 2.0 * rng.random(n) - 1.0
        out.append(np.asfortranarray(f))
    return out


def planted_orphans(n=(13, 12, 11), lc=(-1.0, -1.1, -0.9), hc=(1.0, 1.2, 1.1)):
    """(ϕ, n, lc, hc, h): a sphere's exact distance with a pit dug far from the interface — a node whose |ϕ| is below all its
    neighbours' (an orphan), and a plateau of three equal nodes below theirs (orphans by the strict inequality)"""
    phi = np.array(R.spheres(n, lc, hc, [((0.1, 0.0, 0.1)[:len(n)], 0.45)]), order="F")
    h = R.meshsize(n, lc, hc)
    far = [1] * len(n)
    assert phi[tuple(far)] > 4 * h.max()
    phi[tuple(far)] = 0.37 * phi[tuple(far)]
    top = [k - 2 for k in n]
    v = 0.5 * min(float(phi[tuple(top[:1] + top[1:])]), float(phi[tuple([top[0] - 2] + top[1:])]))
    for i in range(3):
        phi[tuple([top[0] - i] + top[1:])] = v
    return np.asfortranarray(phi), n, lc, hc, h


def plane_front(n, lc, hc, axis, x0):
    """ϕ = x_axis − x0"""
    X = R.nodes(n, lc, hc)
    return np.asfortranarray(X[axis] - x0), R.meshsize(n, lc, hc)
