"""TEST-ONLY restatement of the reference's SemiImplicitI2OE (src/timestepping.jl:204-426) in numpy.

The global system is assembled as the reference assembles it — per node, dimension by dimension, the lower side before
the upper one, the diagonal last, duplicates summed (`sparse(rows, cols, coeffs)`) — and solved directly with
scipy.sparse.linalg.spsolve.  Without scipy a dense numpy solve stands in for grids of at most 4096 nodes; larger ones
skip.  Boundary conditions per dimension are (left, right) pairs of "periodic", "neumann", "linear" (ExtrapolationBC{0},
ExtrapolationBC{1}); anything else is refused with the reference's message.  Indices are 0-based, arrays are indexed
[i1, i2, i3] like the grid."""
import math

import numpy as np
import pytest

try:
    import scipy.sparse as _sp
    import scipy.sparse.linalg as _spla
except ImportError:   # pragma: no cover - scipy is optional
    _sp = _spla = None

DENSE_MAX = 4096


def relation(bc, i, n, side):
    """_i2oe_neighbor_relation (:364-369) for the neighbour i + side of node i: (α, β, idx, γ)."""
    j = i + side
    if 0 <= j < n:
        return 0.0, 1.0, j, 0.0
    if bc == "periodic":                                   # :390-394, period n - 1
        return 0.0, 1.0, (n - 2 if side < 0 else 1), 0.0
    if bc == "neumann":                                    # :396-400
        return 0.0, 1.0, min(max(j, 0), n - 1), 0.0
    if bc == "linear":                                     # :402-412
        dist = 1
        return 1.0 + dist, -float(dist), (1 if side < 0 else n - 2), 0.0
    raise ValueError(f"boundary condition {bc} is not supported by SemiImplicitI2OE")


def meshsize(lc, hc, n):
    return [(hc[d] - lc[d]) / (n[d] - 1) for d in range(len(n))]


def face_measure(h, dim):
    """_i2oe_face_measure (:421-426)."""
    if len(h) == 1:
        return 1.0
    out = None
    for d in range(len(h)):
        if d != dim:
            out = h[d] if out is None else out * h[d]
    return out


def _relations(shape, bcs):
    """Per (dimension, side): arrays α, β, γ, and the flat (column-major) index of idx, over all nodes."""
    N = len(shape)
    I = np.indices(shape)
    lin = np.arange(int(np.prod(shape))).reshape(shape, order="F")
    out = {}
    for d in range(N):
        n = shape[d]
        for side, bc in ((-1, bcs[d][0]), (+1, bcs[d][1])):
            a = np.zeros(shape)
            b = np.ones(shape)
            g = np.zeros(shape)
            j = I[d] + side
            for i in (0, n - 1):
                if not (0 <= i + side < n):
                    al, be, jj, ga = relation(bc, i, n, side)
                    sl = tuple(slice(None) if e != d else i for e in range(N))
                    a[sl], b[sl], g[sl] = al, be, ga
                    j[sl] = jj
            J = list(I)
            J[d] = j
            out[d, side] = (a, b, g, lin[tuple(J)])
    return out


def assemble(u_old, vel, h, bcs, dt):
    """_i2oe_global_step!'s system (:246-303): (A as scipy CSR or dense ndarray, rhs), flat in column-major order."""
    shape = u_old.shape
    N = len(shape)
    nn = u_old.size
    mp = h[0]
    for d in range(1, N):
        mp = mp * h[d]
    fac = dt / (2 * mp)
    u = np.asarray(u_old, dtype=np.float64).ravel(order="F")
    V = [np.asarray(v, dtype=np.float64).ravel(order="F") for v in vel]
    rel = _relations(shape, bcs)
    diag = np.ones(nn)
    rhs = u.copy()
    rows, cols, vals, keys = [], [], [], []
    order = 0
    for d in range(N):
        area = face_measure(h, d)
        for side in (-1, +1):
            a, b, g, idx = (x.ravel(order="F") for x in rel[d, side])
            ordinary = (a == 0) & (b == 1)
            vface = np.where(ordinary, 0.5 * (V[d] + V[d][idx]), V[d])          # :414-419
            A = area * vface if side < 0 else -area * vface
            ain = np.maximum(A, 0.0)
            aout = np.minimum(A, 0.0)
            inn = ain != 0
            diag = np.where(inn, diag + fac * ain * (1 - a), diag)             # :331-336
            m = inn & (b != 0)
            rows.append(np.nonzero(m)[0])
            cols.append(idx[m])
            vals.append((-fac * ain * b)[m])
            keys.append(np.full(int(m.sum()), order))
            rhs = np.where(inn, rhs + fac * ain * g, rhs)
            uq = a * u + b * u[idx] + g                                          # :349-353
            rhs = np.where(aout != 0, rhs - fac * aout * (u - uq), rhs)         # :340-343
            order += 1
    rows.append(np.arange(nn))
    cols.append(np.arange(nn))
    vals.append(diag)
    keys.append(np.full(nn, order))
    r, c, v, k = (np.concatenate(x) for x in (rows, cols, vals, keys))
    perm = np.lexsort((k, r))                                                    # per row: the reference's push order
    r, c, v = r[perm], c[perm], v[perm]
    if _sp is not None:
        M = _sp.coo_matrix((v, (r, c)), shape=(nn, nn)).tocsr()                  # sums duplicates
        M.sum_duplicates()
        return M, rhs
    if nn > DENSE_MAX:
        pytest.skip("scipy is not installed and the grid is too large for a dense solve")
    M = np.zeros((nn, nn))
    np.add.at(M, (r, c), v)
    return M, rhs


def step(u_old, vel, h, bcs, dt):
    """One _i2oe_global_step!: the new values, shaped like u_old."""
    M, rhs = assemble(u_old, vel, h, bcs, dt)
    x = _spla.spsolve(M.tocsc(), rhs) if _sp is not None else np.linalg.solve(M, rhs)
    return np.asarray(x).reshape(u_old.shape, order="F")


def residual_norms(u_new, u_old, vel, h, bcs, dt):
    """(‖A u_new - rhs‖₂, ‖rhs‖₂) of the reference's system, matrix-free (no assembly, no solve): for large grids."""
    shape = u_old.shape
    N = len(shape)
    mp = h[0]
    for d in range(1, N):
        mp = mp * h[d]
    fac = dt / (2 * mp)
    x = np.asarray(u_new, dtype=np.float64)
    u = np.asarray(u_old, dtype=np.float64)
    Ax = x.copy()
    rhs = u.copy()
    for d in range(N):
        area = face_measure(h, d)
        n = shape[d]
        for side, bc in ((-1, bcs[d][0]), (+1, bcs[d][1])):
            src = np.arange(n) + side
            a = np.zeros(n)
            b = np.ones(n)
            for i in (0, n - 1):
                if not (0 <= i + side < n):
                    a[i], b[i], src[i], _ = relation(bc, i, n, side)
            shp = [1] * N
            shp[d] = n
            a, b = a.reshape(shp), b.reshape(shp)
            take = lambda f: np.take(f, src, axis=d)
            vd = vel[d]
            ordinary = (a == 0) & (b == 1)
            vface = np.where(ordinary, 0.5 * (vd + take(vd)), vd)
            A = area * vface if side < 0 else -area * vface
            ain, aout = np.maximum(A, 0.0), np.minimum(A, 0.0)
            Ax += fac * ain * (x - (a * x + b * take(x)))
            rhs -= fac * aout * (u - (a * u + b * take(u)))
    return float(np.linalg.norm((Ax - rhs).ravel())), float(np.linalg.norm(rhs.ravel()))


def advection_cfl(vel, h):
    """compute_cfl of an AdvectionTerm (src/levelsetterms.jl:90-96): min over nodes of 1 / Σ_d |u_d|/h_d."""
    s = sum(np.abs(np.asarray(v, dtype=np.float64)) / h[d] for d, v in enumerate(vel))
    m = float(np.max(s))
    return math.inf if m == 0 else 1.0 / m


def integrate(u0, lc, hc, bcs, velocity, cfl, tf, t0=0.0, dt_max=math.inf, prehook=None, posthook=None):
    """_integrate!(…, ::SemiImplicitI2OE, …) (:207-233).  velocity(t) -> tuple of node arrays.  Returns (u, steps)."""
    n = u0.shape
    h = meshsize(lc, hc, n)
    for d in range(len(n)):
        if n[d] < 3:
            raise ValueError("SemiImplicitI2OE requires at least 3 grid nodes along each dimension")
    u = np.array(u0, dtype=np.float64)
    tc = t0
    steps = 0
    while tc <= tf - np.spacing(abs(tc)):
        if prehook is not None:
            prehook(tc)
        vel = velocity(tc)
        dt = min(dt_max, cfl * advection_cfl(vel, h), tf - tc)
        u = step(u, vel, h, bcs, dt)
        tc += dt
        steps += 1
        if posthook is not None:
            posthook(tc)
    return u, steps


def node_coords(lc, hc, n):
    h = meshsize(lc, hc, n)
    return [lc[d] + np.arange(n[d]) * h[d] for d in range(len(n))]


def upwind_fe_periodic(u0, lc, hc, vel, cfl, tf):
    """ForwardEuler + Upwind on a periodic grid with a constant velocity (src/timestepping.jl:126-137, first-order
    one-sided differences, period n - 1): the explicit baseline of the reference's tests."""
    n = u0.shape
    h = meshsize(lc, hc, n)
    N = len(n)
    u = np.array(u0, dtype=np.float64)
    tc = 0.0
    dtc = 1.0 / sum(abs(vel[d]) / h[d] for d in range(N))
    while tc <= tf - np.spacing(abs(tc)):
        dt = min(cfl * dtc, tf - tc)
        du = np.zeros_like(u)
        for d in range(N):
            m = n[d]
            lo = np.take(u, np.r_[m - 2, np.arange(m - 1)], axis=d)
            hi = np.take(u, np.r_[np.arange(1, m), 1], axis=d)
            du += vel[d] * ((u - lo) / h[d] if vel[d] > 0 else (hi - u) / h[d])
        u = u - dt * du
        tc += dt
    return u
