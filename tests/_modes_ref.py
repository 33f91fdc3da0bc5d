"""elasticity_modes restated in numpy (csrc/lsm_elastic.hip "elasticity_modes", include/lsm.h "elasticity_modes").

The problem: the m smallest eigenpairs of A x = λ M x on the free components; A is _elastic_ref's operator (scaled by 1/∏h), the
fixed components are zero, M the lumped mass, the same for every component of a node and scaled by 1/∏h like A.

  density    ρ_C = ρ_out + (ρ_in − ρ_out)·θ_C: _elliptic_ref.cell_coefficients with (ρ_in, ρ_out) — the bits of the modulus' θ — or a
             given cell array
  mass       M_I = (Σ of ρ_C over the existing cells around I, ascending, from +0)·2^−N;  ρ̄_I = that sum / (number of those cells)
  start      entry t = k·N·nn + i·nn + id of x0: z = splitmix64(t) (z = t + 0x9E3779B97F4A7C15 mod 2^64, two xor-shift-multiply
             rounds, a last xor-shift), d = (z >> 11)·2^−53, the value 2d − 1; zero on the fixed components
  iteration  LOBPCG with soft locking.  S = [X, W, P]: W = T(R_k) for the columns k that have not converged (T: one V-cycle, or
             1/D), P the previous step's W,P-part of those columns.  Rayleigh–Ritz on span S: the Gram matrices SᵀA S and SᵀM S
             (upper triangle, mirrored), scaled to a unit diagonal of the M-Gram; its eigen-decomposition, directions below 1e-12
             of the largest dropped; the reduced standard problem, ascending.  X, P, A·X, A·P ← S·C: A·X is never recomputed.
  stop       ‖A x_k − λ_k M x_k‖₂ ≤ rtol·λ_k·‖M x_k‖₂ for every k, with the recursive A·X, tested before each iteration
  sensitivity  g_I = e_I − (λ·ρ̄_I)·(Σ_i u_{I,i}², from +0, i ascending), e = Operator.energy(u)

The device sums the Gram entries in workgroup order and solves the small problems by cyclic Jacobi; this file uses numpy's sums
and eigh.  The two agree to rounding, so eigenvalues, residuals and orthonormality are compared against bars, the iteration
counts with a margin, and only the mass, the start vector, the stored mode's rounding and the sensitivity bit for bit.

Single iterations (tests/test_gpu_modes_edges.py) are compared to rounding instead: lobpcg(trace=True) records every iterate, lobpcg_ld
runs the whole iteration in long double, rayleigh_ritz_jacobi restates the device's small problems operation for operation, and the
distance between those restatements is the yardstick (step_ref).
"""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import _elastic_ref as E
from _elliptic_ref import cell_coefficients

DROP = 1e-12
LD = E.LD
MASK64 = (1 << 64) - 1


def density_cells(phi, h, level, rho_in, rho_out):
    return cell_coefficients(phi, h, level, rho_in, rho_out)


def _cell_sum(op, rho):
    w = np.pad(np.asarray(rho, dtype=np.float64), 1)
    acc = np.zeros(op.n)
    for m in range(1 << op.N):
        acc = acc + w[op._cell(m)]
    return acc


def mass(op, rho):
    """the lumped mass of a node (n-shaped), in the stated order"""
    return _cell_sum(op, rho) * 2.0 ** -op.N


def mean_density(op, rho):
    return _cell_sum(op, rho) / op.count


def splitmix64(t):
    z = (np.asarray(t, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def default_start(op, m):
    """(m, N)+n: the default start, zero on the fixed components"""
    nn = int(np.prod(op.n))
    with np.errstate(over="ignore"):
        z = splitmix64(np.arange(m * op.N * nn, dtype=np.uint64))
    v = 2.0 * ((z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53) - 1.0
    x = np.stack([np.stack([v[(k * op.N + i) * nn:(k * op.N + i + 1) * nn].reshape(op.n, order="F") for i in range(op.N)]) for k in range(m)])
    return np.where(op.free[None], x, 0.0)


class NotPositive(Exception):
    pass


def rayleigh_ritz(GA, GM, m, info=None):
    """C (q × m) and the m smallest Ritz values of the pencil (GA, GM) of a basis of q ≥ m vectors; the number of dropped directions.
    info (a dict) receives mu: the smallest and the largest eigenvalue of the scaled M-Gram"""
    GA = np.triu(GA) + np.triu(GA, 1).T
    GM = np.triu(GM) + np.triu(GM, 1).T
    d = np.diag(GM)
    if not (np.all(np.isfinite(GA)) and np.all(np.isfinite(GM)) and np.all(d > 0)):
        raise NotPositive
    s = 1.0 / np.sqrt(d)
    Ms, As = s[:, None] * GM * s[None, :], s[:, None] * GA * s[None, :]
    mu, V = np.linalg.eigh(Ms)
    keep = mu > DROP * mu.max()
    if info is not None:
        info["mu"] = (float(mu.min()), float(mu.max()))
    if keep.sum() < m:
        raise NotPositive(int((~keep).sum()))
    B = V[:, keep] / np.sqrt(mu[keep])
    th, Z = np.linalg.eigh(B.T @ As @ B)
    if not th[0] > 0:
        raise NotPositive
    return s[:, None] * (B @ Z[:, :m]), th[:m], int((~keep).sum())


def lobpcg(hier, Mn, m, x0=None, rtol=1e-6, max_iters=300, precond="mg", trace=False, rr=None):
    """returns dict(lam, X ((m, N)+n), iters, relres (m), converged, dropped, applies).  rr: the Rayleigh–Ritz step (rayleigh_ritz, or
    rayleigh_ritz_jacobi).  trace: also `steps`, one record per k = 0 … iters of what a solve with max_iters = k returns: X, lam, relres,
    act (the columns that have not converged), dropped and applies (so far), dr and mu (the dropped count and the extreme eigenvalues
    of the scaled M-Gram of the Rayleigh–Ritz step that gave X_k)"""
    rr = rayleigh_ritz if rr is None else rr
    info, steps = {}, []
    op = hier.ops[0]
    A = op.matrix()
    free = op.flat(op.free)
    Mv = np.where(free, np.concatenate([np.asarray(Mn).reshape(-1, order="F")] * op.N), 0.0)
    T = (lambda r: op.flat(hier.vcycle(op.unflat(r)))) if precond == "mg" else (lambda r: np.where(free, r / op.flat(op.D), 0.0))

    def apply(V):
        return np.where(free[None], (A @ np.where(free[None], V, 0.0).T).T, 0.0)

    X = default_start(op, m) if x0 is None else np.asarray(x0, dtype=np.float64)
    X = np.where(free[None], np.stack([op.flat(x) for x in X]), 0.0)
    AX = apply(X)
    C, lam, dropped = rr(X @ AX.T, X @ (Mv * X).T, m, info)
    X, AX = C.T @ X, C.T @ AX
    P = AP = np.zeros((0, X.shape[1]))
    it = applies = 0
    dr = dropped
    while True:
        MX = Mv * X
        R = AX - lam[:, None] * MX
        rn, mn = np.sqrt(np.sum(R * R, axis=1)), np.sqrt(np.sum(MX * MX, axis=1))
        relres = rn / (lam * mn)
        act = [k for k in range(m) if not rn[k] <= rtol * lam[k] * mn[k]]
        if trace:
            steps.append(dict(X=np.stack([op.unflat(x) for x in X]), lam=lam.copy(), relres=relres.copy(), act=tuple(act), dropped=dropped, applies=applies,
                              dr=dr, mu=info["mu"]))
        if not act or it == max_iters:
            break
        W = np.stack([T(R[k]) for k in act])
        AW = apply(W)
        applies += len(act)
        S, AS = np.concatenate([X, W, P]), np.concatenate([AX, AW, AP])
        C, lam, dr = rr(S @ AS.T, S @ (Mv * S).T, m, info)
        dropped += dr
        Cp = C.copy()
        Cp[:m] = 0.0
        Cp = Cp[:, act]
        X, AX, P, AP = C.T @ S, C.T @ AS, Cp.T @ S, Cp.T @ AS
        it += 1
    out = dict(lam=lam, X=np.stack([op.unflat(x) for x in X]), iters=it, relres=relres, converged=not act, dropped=dropped, applies=applies)
    if trace:
        out["steps"] = steps
    return out


# ---- the host's small problems operation for operation (em_jacobi, em_rayleigh_ritz of csrc/lsm_elastic.hip), in float64 or in long
# double: numpy's eigh has no long double.  A whole row or column is rotated by one numpy expression: every element sees the
# operations of the C loop.

def _seq_matmul(A, B, dt):
    """A·B with every entry summed from +0 over the inner index ascending"""
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=dt)
    for k in range(A.shape[1]):
        acc = acc + A[:, k, None] * B[None, k, :]
    return acc


def em_jacobi(A, dt=np.float64):
    """cyclic Jacobi on a symmetric matrix: the eigenvalues ascending and the eigenvectors as columns.  The sweeps end when the
    squared off-diagonal part is ≤ 1e-34 of the squared diagonal, as on the device; in long double that bar is scaled by (ε_ld/ε_64)²"""
    A = np.array(A, dtype=dt)
    n = len(A)
    V = np.eye(n, dtype=dt)
    one, two = dt(1), dt(2)
    tol = dt(1e-34) * (dt(np.finfo(dt).eps) / dt(2.0 ** -52)) ** 2
    for _ in range(64):
        off = dia = dt(0)
        for p in range(n):
            dia = dia + A[p, p] * A[p, p]
            for q in range(p + 1, n):
                off = off + A[p, q] * A[p, q]
        if not off > tol * dia:
            break
        for p in range(n):
            for q in range(p + 1, n):
                apq = A[p, q]
                if apq == 0:
                    continue
                theta = (A[q, q] - A[p, p]) / (two * apq)
                t = (one if theta >= 0 else -one) / (abs(theta) + np.sqrt(theta * theta + one))
                c = one / np.sqrt(t * t + one)
                s = t * c
                akp, akq = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * akp - s * akq, s * akp + c * akq
                apk, aqk = A[p, :].copy(), A[q, :].copy()
                A[p, :], A[q, :] = c * apk - s * aqk, s * apk + c * aqk
                vkp, vkq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * vkp - s * vkq, s * vkp + c * vkq
    order = np.argsort(np.diag(A), kind="stable")
    return np.diag(A)[order].copy(), V[:, order].copy()


def rayleigh_ritz_jacobi(GA, GM, m, info=None, dt=np.float64):
    """rayleigh_ritz by em_rayleigh_ritz's operations: the scaling (s_i·G_ij)·s_j, em_jacobi, the directions at or below 1e-12 of the
    largest dropped, B = V·μ^−½, Bᵀ(A_s B) by sequential sums (the upper triangle, mirrored), em_jacobi, C = s·(B Z)"""
    GA, GM = np.array(GA, dtype=dt), np.array(GM, dtype=dt)
    q = len(GA)
    GA = np.triu(GA) + np.triu(GA, 1).T
    GM = np.triu(GM) + np.triu(GM, 1).T
    d = np.diag(GM)
    if not (np.all(np.isfinite(GA)) and np.all(np.isfinite(GM)) and np.all(d > 0)):
        raise NotPositive
    s = dt(1) / np.sqrt(d)
    Ms, As = (s[:, None] * GM) * s[None, :], (s[:, None] * GA) * s[None, :]
    mu, V = em_jacobi(Ms, dt)
    if info is not None:
        info["mu"] = (float(mu[0]), float(mu[-1]))
    if not mu[-1] > 0:
        raise NotPositive
    first = 0
    while first < q and not mu[first] > dt(DROP) * mu[-1]:
        first += 1
    if q - first < m:
        raise NotPositive(first)
    B = V[:, first:] / np.sqrt(mu[first:])[None, :]
    Ar = _seq_matmul(B.T, _seq_matmul(As, B, dt), dt)
    th, Z = em_jacobi(np.triu(Ar) + np.triu(Ar, 1).T, dt)
    if not th[0] > 0:
        raise NotPositive
    return s[:, None] * _seq_matmul(B, Z[:, :m], dt), th[:m], first


def lobpcg_ld(hier, Mn, m, x0=None, rtol=1e-6, max_iters=300, precond="mg"):
    """lobpcg(trace=True) with every operation in np.longdouble: the Gram sums, S·C, the residuals, A·x (Operator.apply's loops on long-double
    arrays, from the float64 coefficients), the V-cycle (_elastic_ref._vcycle_ld) or 1/D, and the small problems (rayleigh_ritz_jacobi).
    x0, the mass and rtol are the float64 values.  The vectors are (columns, N)+n arrays throughout"""
    op = hier.ops[0]
    free = op.free
    Mv = np.where(free, np.asarray(Mn, dtype=LD)[None], LD(0))
    D = op.D.astype(LD)
    T = (lambda r: E._vcycle_ld(hier, r)) if precond == "mg" else (lambda r: np.where(free, r / D, LD(0)))

    def apply(V):
        return np.stack([E._apply_free_ld(op, v) for v in V])

    def gram(S, Y):
        return S.reshape(len(S), -1) @ Y.reshape(len(Y), -1).T

    def combine(C, S):
        return (C.T @ S.reshape(len(S), -1)).reshape((C.shape[1],) + S.shape[1:])

    info, steps = {}, []
    X = (default_start(op, m) if x0 is None else np.asarray(x0, dtype=np.float64)).astype(LD)
    X = np.where(free[None], X, LD(0))
    AX = apply(X)
    C, lam, dropped = rayleigh_ritz_jacobi(gram(X, AX), gram(X, Mv[None] * X), m, info, LD)
    X, AX = combine(C, X), combine(C, AX)
    P = AP = np.zeros((0,) + X.shape[1:], dtype=LD)
    it = applies = 0
    dr = dropped
    ax = tuple(range(1, X.ndim))
    while True:
        MX = Mv[None] * X
        R = AX - lam.reshape((m,) + (1,) * (X.ndim - 1)) * MX
        rn, mn = np.sqrt(np.sum(R * R, axis=ax)), np.sqrt(np.sum(MX * MX, axis=ax))
        relres = rn / (lam * mn)
        act = [k for k in range(m) if not rn[k] <= LD(rtol) * lam[k] * mn[k]]
        steps.append(dict(X=X.copy(), lam=lam.copy(), relres=relres.copy(), act=tuple(act), dropped=dropped, applies=applies, dr=dr, mu=info["mu"]))
        if not act or it == max_iters:
            break
        W = np.stack([T(R[k]) for k in act])
        AW = apply(W)
        applies += len(act)
        S, AS = np.concatenate([X, W, P]), np.concatenate([AX, AW, AP])
        C, lam, dr = rayleigh_ritz_jacobi(gram(S, AS), gram(S, Mv[None] * S), m, info, LD)
        dropped += dr
        Cp = C.copy()
        Cp[:m] = LD(0)
        Cp = Cp[:, act]
        X, AX, P, AP = combine(C, S), combine(C, AS), combine(Cp, S), combine(Cp, AS)
        it += 1
    return dict(lam=lam, X=X, iters=it, relres=relres, converged=not act, dropped=dropped, applies=applies, steps=steps)


def locked_start(op, Mn, m, locked):
    """(m, N)+n: a start whose columns in `locked` are exact eigenvectors v_k (of the dense generalised eigh, the 2m lowest) and whose other
    columns are v_k + 0.3·v_{m+k} + 0.1·v_{m+k−1}: the first are converged from the first residual on, the others are far from it"""
    free = op.flat(op.free)
    A = op.matrix()[free][:, free].toarray()
    Mv = np.concatenate([np.asarray(Mn).reshape(-1, order="F")] * op.N)[free]
    _, V = sla.eigh(A, np.diag(Mv), subset_by_index=(0, 2 * m - 1))
    cols = []
    for k in range(m):
        full = np.zeros(len(free))
        full[free] = V[:, k] if k in locked else V[:, k] + 0.3 * V[:, m + k] + 0.1 * V[:, m + k - 1]
        cols.append(op.unflat(full))
    return np.stack(cols)


def true_residual(op, Mn, x, lam):
    """‖(A x − λ M x)_free‖₂ with A x in the stated order, and ‖M x‖₂ over the free components"""
    x = np.where(op.free, x, 0.0)
    Mx = np.where(op.free, Mn[None] * x, 0.0)
    r = np.where(op.free, op.apply(x) - lam * Mx, 0.0)
    return float(np.sqrt(np.sum(r * r))), float(np.sqrt(np.sum(Mx * Mx)))


def ortho_defect(op, Mn, X):
    """max |XᵀM X − I|"""
    F = np.stack([op.flat(np.where(op.free, x, 0.0)) for x in X])
    Mv = np.concatenate([np.asarray(Mn).reshape(-1, order="F")] * op.N)
    return float(np.abs(F @ (Mv * F).T - np.eye(len(X))).max())


def exact(op, Mn, k):
    """the k smallest eigenvalues: dense below 3000 free components, shift-invert Lanczos above"""
    free = op.flat(op.free)
    A = op.matrix()[free][:, free]
    Mv = np.concatenate([np.asarray(Mn).reshape(-1, order="F")] * op.N)[free]
    if A.shape[0] < 3000:
        return sla.eigh(A.toarray(), np.diag(Mv), eigvals_only=True, subset_by_index=(0, k - 1))
    w = spla.eigsh(A.tocsc(), k=k, M=sp.diags(Mv).tocsc(), sigma=0.0, which="LM", tol=1e-13, return_eigenvectors=False)
    return np.sort(w)


def sensitivity(op, rho, u, lam):
    """g in float64 (the caller rounds to the storage type): u is the stored mode"""
    u = np.asarray(u, dtype=np.float64)
    s = np.zeros(op.n)
    for i in range(op.N):
        s = s + u[i] * u[i]
    return op.energy(u) - (lam * mean_density(op, rho)) * s


# ---- the cases shared by tests/test_modes_host.py and tests/test_gpu_modes.py.  iters / ortho: the restatement's own iteration
# counts at rtol 1e-6 and 1e-8 and its max |XᵀM X − I| at 1e-6 (tests/test_modes_host.py asserts the counts and prints both)

def _clamp(n):
    return E.face_bits(n, 0, 0, (1 << len(n)) - 1)


def cases():
    """name → dict(n, hc, h, phi, bits, m, rho_in, rho_out, rho (cells or None), E_in, E_out, nu, plane, dtype, precond, iters, ortho)"""
    out = {}

    def add(name, n, m, iters, ortho, hc=None, bits=None, plane="stress", nu=0.3, dtype=np.float64, rho=None, shift=0.0, precond="mg"):
        hc = tuple((nd - 1.0) / (max(n) - 1.0) for nd in n) if hc is None else hc
        h = tuple(x / (nd - 1) for x, nd in zip(hc, n))
        bits = _clamp(n) if bits is None else bits
        out[name] = dict(n=n, hc=hc, h=h, phi=E.two_holes(n, h, shift), bits=np.asfortranarray(bits.astype(np.uint8)), m=m, rho_in=1.0, rho_out=1e-6,
                         rho=rho, E_in=1.0, E_out=1e-3, nu=nu, plane=plane, dtype=dtype, precond=precond, iters=iters, ortho=ortho)

    add("33x33_m4", (33, 33), 4, ITERS["33x33_m4"], ORTHO["33x33_m4"])
    add("65x65_m6", (65, 65), 6, ITERS["65x65_m6"], ORTHO["65x65_m6"])
    add("64x48_m4", (64, 48), 4, ITERS["64x48_m4"], ORTHO["64x48_m4"], shift=0.25)
    add("17c_m6", (17, 17, 17), 6, ITERS["17c_m6"], ORTHO["17c_m6"])
    add("24x33x10_m4", (24, 33, 10), 4, ITERS["24x33x10_m4"], ORTHO["24x33x10_m4"], hc=(1.0, 1.2, 0.45))
    add("20x14_m1", (20, 14), 1, ITERS["20x14_m1"], ORTHO["20x14_m1"])
    add("9x12_m8", (9, 12), 8, ITERS["9x12_m8"], ORTHO["9x12_m8"])
    n = (64, 48)
    blob = np.zeros(n, dtype=np.uint8)
    blob[20:25, 30:34] = 3
    add("64x48_blob_roller_m3", n, 3, ITERS["64x48_blob_roller_m3"], ORTHO["64x48_blob_roller_m3"], bits=blob | E.face_bits(n, 1, 0, 2), plane="strain", nu=0.2)
    add("5x5_one_level_m2", (5, 5), 2, ITERS["5x5_one_level_m2"], ORTHO["5x5_one_level_m2"])
    add("17c_f32_m3", (17, 17, 17), 3, ITERS["17c_f32_m3"], ORTHO["17c_f32_m3"], bits=E.face_bits((17, 17, 17), 0, 1, 7), dtype=np.float32)
    n = (24, 33, 10)
    rho = np.asfortranarray(0.25 + np.random.default_rng(5).random(tuple(k - 1 for k in n)))
    add("24x33x10_given_rho_m2", n, 2, ITERS["24x33x10_given_rho_m2"], ORTHO["24x33x10_given_rho_m2"], rho=rho)
    return out


# the restatement's iteration counts (rtol 1e-6, rtol 1e-8) and max |XᵀM X − I| at 1e-6, from tests/test_modes_host.py's print-out
ITERS = {
    "33x33_m4": (22, 28), "65x65_m6": (20, 25), "64x48_m4": (24, 30), "17c_m6": (16, 20), "24x33x10_m4": (157, 189), "20x14_m1": (27, 33),
    "9x12_m8": (20, 25), "64x48_blob_roller_m3": (29, 38), "5x5_one_level_m2": (16, 17), "17c_f32_m3": (16, 20), "24x33x10_given_rho_m2": (63, 83),
}
ORTHO = {
    "33x33_m4": 1.3e-15, "65x65_m6": 7.3e-16, "64x48_m4": 1.8e-15, "17c_m6": 1.8e-15, "24x33x10_m4": 8.9e-16, "20x14_m1": 0.0, "9x12_m8": 1.3e-15,
    "64x48_blob_roller_m3": 4.8e-16, "5x5_one_level_m2": 7.8e-16, "17c_f32_m3": 6.7e-16, "24x33x10_given_rho_m2": 8.9e-16,
}
TIGHT = ("33x33_m4", "17c_m6", "5x5_one_level_m2")      # the cases the device also runs at rtol 1e-8


def build_case(cs, k0s=None, omegas=None):
    """(Hierarchy, ρ cells, node mass) of a case; an f32 case's ϕ is rounded to float32 first, as the handle stores it.  k0s, omegas:
    the levels' K0 and dampings (the device's, _elastic_ref.device_omegas) in place of the restatement's own"""
    phi = cs["phi"].astype(cs["dtype"]).astype(np.float64)
    Ec = cell_coefficients(phi, cs["h"], 0.0, cs["E_in"], cs["E_out"])
    hier = E.Hierarchy(Ec, cs["h"], cs["nu"], cs["plane"], cs["bits"], k0s, omegas=omegas)
    rho = cs["rho"] if cs["rho"] is not None else density_cells(phi, cs["h"], 0.0, cs["rho_in"], cs["rho_out"])
    return hier, rho, mass(hier.ops[0], rho)


_SOLVED = {}


def base(name):
    """a case's reference data, computed once and shared: case, hier, rho, mass, exact (the m smallest eigenvalues)"""
    if (name, None) not in _SOLVED:
        cs = cases()[name]
        hier, rho, Mn = build_case(cs)
        _SOLVED[(name, None)] = dict(case=cs, hier=hier, rho=rho, mass=Mn, exact=exact(hier.ops[0], Mn, cs["m"]))
    return _SOLVED[(name, None)]


def solved(name, rtol=1e-6):
    """base(name) and the restatement's own solve at rtol (lobpcg's dict), computed once"""
    key = (name, rtol)
    if key not in _SOLVED:
        res = dict(base(name))
        res.update(lobpcg(res["hier"], res["mass"], res["case"]["m"], None, rtol, 600, res["case"]["precond"]))
        _SOLVED[key] = res
    return _SOLVED[key]


# ---- single iterations (tests/test_gpu_modes_edges.py; tests/test_modes_host.py asserts the conditions): a solve with max_iters = k
# returns X_k, one at a huge finite rtol X_0, so the device's iterates are compared one by one with lobpcg_ld's.  start: "locked"
# (locked_start with these columns) or "default"; ks: the observed steps

STEP_RTOL = 1e-6


def step_cases():
    """name → the dict of cases() with start, locked, ks; iters and ortho are None"""
    out = {}

    def add(name, n, m, ks, locked=None, precond="mg"):
        hc = tuple((nd - 1.0) / (max(n) - 1.0) for nd in n)
        h = tuple(x / (nd - 1) for x, nd in zip(hc, n))
        out[name] = dict(n=n, hc=hc, h=h, phi=E.two_holes(n, h), bits=np.asfortranarray(_clamp(n).astype(np.uint8)), m=m, rho_in=1.0, rho_out=1e-6, rho=None,
                         E_in=1.0, E_out=1e-3, nu=0.3, plane="stress", dtype=np.float64, precond=precond, iters=None, ortho=None,
                         start="default" if locked is None else "locked", locked=locked, ks=tuple(ks))

    add("9x12_m4_lock02", (9, 12), 4, range(5), (0, 2))             # act (1, 3): the source slot is not the target slot, P's columns act[j]; q = 4, 6, 8
    add("9x12_m4_lock02_jacobi", (9, 12), 4, range(4), (0, 2), precond="jacobi")
    add("9x12_m4_lock12", (9, 12), 4, range(4), (1, 2))             # act (0, 3)
    add("9x12_m8", (9, 12), 8, range(4))                            # the start's columns 1 … 7; q = 8, 16, 24: all 21 tiles
    add("12x9_m3", (12, 9), 3, range(4))                            # partial tiles: q = 3, 6, 9 (9x12: the third Gram's smallest is 8e-9 of its largest)
    add("9x12_m5", (9, 12), 5, range(4))                            # q = 5, 10, 15
    add("5x5_one_level_m2_lock0", (5, 5), 2, range(3), (0,))        # a hierarchy of one level, act (1) (at k = 3 its relres is 7.6e-6, below 10·rtol)
    add("6x5x7_m3_lock1", (6, 5, 7), 3, range(5), (1,))             # N = 3: act (1, 2) at k = 0, the locked column moves to 1, then act (0, 2)
    add("33x33_m4_lock02", (33, 33), 4, (0, 2, 4), (0, 2))          # several workgroups per Gram tile
    # _elastic_ref.prototype's problem: more than 256 workgroups in the residual and Gram passes (nt = 68400, 70470), the strided second pass
    # of the ordered reduction.  2-D stops at k = 1: the second Gram's smallest eigenvalue is 5e-10 of its largest there (and 2e-10 … 1e-9 on
    # 180x190, 200x171, 185x185 and 192x179)
    add("190x180_m2", (190, 180), 2, (0, 1))
    add("30x29x27_m2", (30, 29, 27), 2, (0, 2))
    return out


_STEPS = {}


def _aligned(X, ref):
    """X's columns with the signs of ref's"""
    ax = tuple(range(1, ref.ndim))
    sg = np.where(np.sum(X * ref, axis=ax) < 0, -1, 1).reshape((-1,) + (1,) * (ref.ndim - 1))
    return X * sg


def step_ref(name, k0s=None, omegas=None):
    """a step case's references, computed once per (name, K0): case, hier, mass, x0 (None: the default start), and per k = 0 … max(ks)
    `ld` (lobpcg_ld's record), `eigh` and `jacobi` (the float64 restatement's with either Rayleigh–Ritz step), yard_x and yard_lam (per
    column: max(|x_eigh − x_ld|∞, |x_jacobi − x_ld|∞, 2⁻⁵³·|x_ld|∞) after sign alignment, and the same of λ), scale (|x_ld|∞ per column)"""
    key = (name, None if k0s is None else b"".join(np.ascontiguousarray(k).tobytes() for k in k0s))
    if key in _STEPS:
        return _STEPS[key]
    cs = step_cases()[name]
    hier, _, Mn = build_case(cs, k0s, omegas)
    m, kmax = cs["m"], max(cs["ks"])
    x0 = locked_start(hier.ops[0], Mn, m, cs["locked"]) if cs["start"] == "locked" else None
    runs = dict(eigh=lobpcg(hier, Mn, m, x0, STEP_RTOL, kmax, cs["precond"], trace=True)["steps"],
                jacobi=lobpcg(hier, Mn, m, x0, STEP_RTOL, kmax, cs["precond"], trace=True, rr=rayleigh_ritz_jacobi)["steps"],
                ld=lobpcg_ld(hier, Mn, m, x0, STEP_RTOL, kmax, cs["precond"])["steps"])
    steps = []
    for k in range(kmax + 1):
        if min(len(v) for v in runs.values()) <= k:
            break
        ld = runs["ld"][k]
        ax = tuple(range(1, ld["X"].ndim))
        scale = np.abs(ld["X"]).max(axis=ax)
        dx = [np.abs(_aligned(runs[v][k]["X"].astype(LD), ld["X"]) - ld["X"]).max(axis=ax) for v in ("eigh", "jacobi")]
        dl = [np.abs(runs[v][k]["lam"].astype(LD) - ld["lam"]) for v in ("eigh", "jacobi")]
        steps.append(dict(ld=ld, eigh=runs["eigh"][k], jacobi=runs["jacobi"][k], scale=scale, yard_x=np.maximum(np.maximum(dx[0], dx[1]), LD(2.0 ** -53) * scale),
                          yard_lam=np.maximum(np.maximum(dl[0], dl[1]), LD(2.0 ** -53) * ld["lam"])))
    _STEPS[key] = dict(case=cs, hier=hier, mass=Mn, x0=x0, steps=steps)
    return _STEPS[key]
