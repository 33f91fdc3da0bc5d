"""numpy restatement of SemiLagrangian, written from the operation order stated there; N = 1, 2, 3.  It does
not import the library.  Arrays are indexed [i1, i2, i3]; every operation is an IEEE double operation in the stated order (numpy
does not contract), so the device kernels — compiled without contraction — must give the same bits.

    bcs      per dimension a pair (left, right) of "periodic" | "neumann" | "linear" | "symmetry" | ("extrapolation", P)
    velocity ("const", (c1, ...)) | ("rotation", w, c1, c2) | ("separable", tables[c][e], tfac_of_t) | ("field", (U1, ...))
"""
import math

import numpy as np

G = 3   # ghost layers (LSM_GHOST)


def meshsize(lc, hc, n):
    return tuple((float(hc[d]) - float(lc[d])) / (n[d] - 1) for d in range(len(n)))


def cos_factor(T):
    """g(t) = cos(π t / T), as the host side of the library evaluates it"""
    return lambda t: math.cos(math.pi * t / T)


# ----------------------------------------------------------------------------- ghost fill (the five boundary kinds)
def _lagrange_w(j, k, P):
    w = 1.0
    for m in range(P + 1):
        if m == j:
            continue
        w *= float(-k - m) / float(j - m)
    return w


def _kind(b):
    if isinstance(b, str):
        return {"periodic": ("periodic", 0), "neumann": ("extrapolation", 0), "linear": ("extrapolation", 1), "symmetry": ("symmetry", 0)}[b]
    return ("extrapolation", int(b[1]))


def fill_ghosts(u, bcs, storage=np.float64):
    """The padded field: dimension 1 first, then 2 over the ghosts of 1, then 3 (acc = 0; acc += w·value per source node).  The
    sums run in fp64; Float32 storage rounds every ghost once, when it is stored."""
    n = u.shape
    N = u.ndim
    p = np.full(tuple(m + 2 * G for m in n), np.nan)
    p[tuple(slice(G, G + m) for m in n)] = u.astype(storage).astype(np.float64)
    for d in range(N):
        # lower dimensions with their ghosts, higher ones interior only
        sl = [slice(None) if e < d else slice(G, G + n[e]) for e in range(N)]

        def at(i):
            s = list(sl)
            s[d] = G + i
            return tuple(s)
        for side in (0, 1):
            kind, P = _kind(bcs[d][side])
            b, dr = (0, 1) if side == 0 else (n[d] - 1, -1)
            for k in range(1, G + 1):
                ig = -k if side == 0 else n[d] - 1 + k
                if kind == "periodic":
                    acc = 0.0 + 1.0 * p[at((n[d] - 1) - k if side == 0 else k)]
                elif kind == "symmetry":
                    acc = 0.0 + 1.0 * p[at(b + dr * k)]
                else:
                    acc = 0.0
                    for j in range(P + 1):
                        acc = acc + _lagrange_w(j, k, P) * p[at(b + dr * j)]
                p[at(ig)] = acc
    if np.dtype(storage) == np.float32:
        p = p.astype(np.float32).astype(np.float64)
    return p


# ----------------------------------------------------------------------------- the map W, cells, velocities
def wrap(xi, n, periodic):
    pd = float(n - 1)
    with np.errstate(invalid="ignore"):
        if periodic:
            return xi - np.floor(xi / pd) * pd
        return np.where(xi < 0.0, 0.0, np.where(xi > pd, pd, xi))


def cell(xi, n):
    """(j, θ): NaN and negative ξ go to cell 0 by the form of the comparisons; the conversion only sees values in range"""
    with np.errstate(invalid="ignore"):
        f = np.floor(xi)
        top = float(n - 2)
        inr = (f >= 0.0) & (f <= top)
        j = np.where(inr, np.where(inr, f, 0.0).astype(np.int64), np.where(f > top, n - 2, 0))
        j = np.clip(j, 0, n - 2)
        return j, xi - j.astype(np.float64)


def _lerp(a, b, th):
    return a + th * (b - a)


def _index_arrays(n):
    return np.meshgrid(*[np.arange(m, dtype=np.float64) for m in n], indexing="ij")


def vel_node(vel, n, lc, h, t):
    N = len(n)
    I = _index_arrays(n)
    kind = vel[0]
    if kind == "const":
        return [np.full(n, float(vel[1][d])) for d in range(N)]
    if kind == "rotation":
        w, c1, c2 = vel[1:]
        u = [-(w * ((lc[1] + I[1] * h[1]) - c2)), w * ((lc[0] + I[0] * h[0]) - c1)]
        return u + ([np.zeros(n)] if N == 3 else [])
    if kind == "separable":
        tabs, g = vel[1], vel[2]
        out = []
        for c in range(N):
            p = np.asarray(tabs[c][0], dtype=np.float64).reshape([-1] + [1] * (N - 1))
            for e in range(1, N):
                shp = [1] * N
                shp[e] = -1
                p = p * np.asarray(tabs[c][e], dtype=np.float64).reshape(shp)
            out.append(np.broadcast_to(p * g(t), n))
        return out
    return [np.asarray(vel[1][d], dtype=np.float64) for d in range(N)]


def vel_at(vel, xi, n, lc, h, t):
    N = len(n)
    kind = vel[0]
    with np.errstate(invalid="ignore"):
        if kind == "const":
            return [np.full(n, float(vel[1][d])) for d in range(N)]
        if kind == "rotation":
            w, c1, c2 = vel[1:]
            u = [-(w * ((lc[1] + xi[1] * h[1]) - c2)), w * ((lc[0] + xi[0] * h[0]) - c1)]
            return u + ([np.zeros(n)] if N == 3 else [])
        cl = [cell(xi[d], n[d]) for d in range(N)]
        if kind == "separable":
            tabs, g = vel[1], vel[2]
            out = []
            for c in range(N):
                p = None
                for e in range(N):
                    T = np.asarray(tabs[c][e], dtype=np.float64)
                    le = _lerp(T[cl[e][0]], T[cl[e][0] + 1], cl[e][1])
                    p = le if p is None else p * le
                out.append(p * g(t))
            return out
        out = []
        for c in range(N):
            F = np.asarray(vel[1][c], dtype=np.float64)

            def corner(k):
                return F[tuple(cl[e][0] + k[e] for e in range(N))]
            if N == 1:
                out.append(_lerp(corner((0,)), corner((1,)), cl[0][1]))
                continue
            z = []
            for kz in range(2 if N > 2 else 1):
                y = []
                for ky in range(2):
                    k = (0, ky, kz)[:N]
                    k1 = (1, ky, kz)[:N]
                    y.append(_lerp(corner(k), corner(k1), cl[0][1]))
                z.append(_lerp(y[0], y[1], cl[1][1]))
            out.append(_lerp(z[0], z[1], cl[2][1]) if N > 2 else z[0])
        return out


def trace(vel, n, lc, hc, bcs, tc, dt, which=2):
    """departure cells [(j, θ) per dimension] and the largest |Δt·u_d/h_d| of the final trace"""
    N = len(n)
    h = meshsize(lc, hc, n)
    per = [_kind(bcs[d][0])[0] == "periodic" for d in range(N)]
    I = _index_arrays(n)
    with np.errstate(invalid="ignore", over="ignore"):
        if which == 1:
            u = vel_node(vel, n, lc, h, tc)
        else:
            th = tc + 0.5 * dt
            hdt = 0.5 * dt
            u = vel_node(vel, n, lc, h, th)
            xm = [wrap(I[d] - (hdt * u[d]) / h[d], n[d], per[d]) for d in range(N)]
            u = vel_at(vel, xm, n, lc, h, th)
        cells, disp = [], 0.0
        for d in range(N):
            s = (dt * u[d]) / h[d]
            m = np.abs(s)
            m = m[~np.isnan(m)]
            disp = max(disp, float(m.max()) if m.size else 0.0)
            cells.append(cell(wrap(I[d] - s, n[d], per[d]), n[d]))
    return cells, disp


# ----------------------------------------------------------------------------- interpolation
def weights(th, r):
    w = []
    for s in range(2 * r):
        num, den = 1.0, 1.0
        for m in range(2 * r):
            if m == s:
                continue
            num = num * (th - float(m - r + 1))
            den = den * float(s - m)
        w.append(num / den)
    return w


def interpolate(p, cells, order=3, limiter=True):
    """the tensor-product Lagrange interpolant of the padded field p at the cells: dimension 1 first, then 2, then 3"""
    N = p.ndim
    r = {1: 1, 3: 2, 5: 3}[order]
    S = 2 * r
    with np.errstate(invalid="ignore", over="ignore"):
        w = [weights(cells[d][1], r) for d in range(N)]
        base = [cells[d][0] - r + 1 + G for d in range(N)]
        lo = hi = None
        az = None
        for sz in range(S if N > 2 else 1):
            ay = None
            for sy in range(S if N > 1 else 1):
                ax = None
                for sx in range(S):
                    idx = (base[0] + sx,) + ((base[1] + sy,) if N > 1 else ()) + ((base[2] + sz,) if N > 2 else ())
                    v = p[idx]
                    ax = w[0][0] * v if sx == 0 else ax + w[0][sx] * v
                    if sx in (r - 1, r) and (N < 2 or sy in (r - 1, r)) and (N < 3 or sz in (r - 1, r)):
                        if lo is None:
                            lo, hi = v, v
                        else:
                            lo = np.where(v < lo, v, lo)
                            hi = np.where(v > hi, v, hi)
                if N > 1:
                    ay = w[1][0] * ax if sy == 0 else ay + w[1][sy] * ax
                else:
                    ay = ax
            if N > 2:
                az = w[2][0] * ay if sz == 0 else az + w[2][sz] * ay
            else:
                az = ay
        if limiter:
            az = np.where(az < lo, lo, np.where(az > hi, hi, az))
    return az


def step(u, vel, lc, hc, bcs, tc, dt, order=3, trace_order=2, limiter=True, storage=np.float64):
    """one SemiLagrangian step of the dense field u (values of the storage type); returns the new field in that type"""
    n = u.shape
    p = fill_ghosts(u, bcs, storage)
    cells, _ = trace(vel, n, lc, hc, bcs, tc, dt, trace_order)
    with np.errstate(invalid="ignore", over="ignore"):
        return interpolate(p, cells, order, limiter).astype(storage)
