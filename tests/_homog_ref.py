"""homogenize restated in numpy and scipy.sparse (csrc/lsm_homog.hip, include/lsm.h "homogenize").

The torus has m = n − 1 nodes and cells per axis (node n − 1 is node 0); vectors are (N,)+m-shaped, component-major.  The functions
the device is compared with bit for bit (Operator.apply, D, load, energy_cells, sensitivity; the cell array is
_elliptic_ref.cell_coefficients) spell their operation order out with np.roll; the assembled matrix, the hierarchy, the V-cycle
and PCG are compared to rounding / by iteration counts.

  operator  _elastic_ref's, over wrapped cells and nodes: cell m of node I is I − 1 + bits(m) mod m, corner b of it one further
  strains   M = N(N+1)/2 in Voigt order: 2-D (00, 11, 01); 3-D (00, 11, 22, 12, 02, 01); engineering shears
  χ0^k      at a cell's corners (corner a at x_d = bit_d(a)·h_d): normal ii: component i = x_i; shear ij: component i = x_j/2, j = x_i/2
  g^k       K0·χ0^k, each row from +0 ascending
  load      f^k_{I,i} = −(Σ_C E_C·g^k[(a,i)]), the cells ascending, from +0
  t^{pq}_C  E_C·(Σ_r w^p_r·(Σ_s K0[r,s]·w^q_s)), w = χ0 + χ at the cell's corners, both sums from +0 ascending
  C^H_pq    (Σ_C t^{pq}_C)/ncells
  sens.     cell_C = Σ_q Σ_{p≤q} (c·W_pq)·t^{pq}_C, c = 2 for p < q, from +0; s_I = (Σ_C around I cell_C, ascending, from +0)·2^−N
  hierarchy axis d coarsens while m_d is even and > 4; coarse cell = mean of cells 2J, 2J+1; R = 2^−k·(½, 1, ½ per axis, wrapped);
            P = Rᵀ·2^k; node 0 pinned on every level; ω_l = min(0.6, 1.9/λ_l); 2 + 2 sweeps, 16 on the coarsest level
"""
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from _elastic_ref import NCOARSE, NPOST, NPRE, OMEGA, SAFE, _bits, k0, level_omega, material, symbol_lambda_power
from _elliptic_ref import LD, cell_coefficients

VOIGT = {2: ((0, 0), (1, 1), (0, 1)), 3: ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))}


def nstrains(N):
    return N * (N + 1) // 2


def chi0(h):
    """(M, 2^N·N): the cell-local affine fields at a cell's corners"""
    N = len(h)
    out = np.zeros((nstrains(N), (1 << N) * N))
    for k, (i, j) in enumerate(VOIGT[N]):
        for a in range(1 << N):
            xi, xj = ((a >> i) & 1) * h[i], ((a >> j) & 1) * h[j]
            if i == j:
                out[k, a * N + i] = xi
            else:
                out[k, a * N + i] = 0.5 * xj
                out[k, a * N + j] = 0.5 * xi
    return out


def unit_loads(K0, c0):
    """g^k = K0·χ0^k, each row from +0 ascending (Python floats)"""
    R = K0.shape[0]
    g = np.zeros_like(c0)
    for k in range(c0.shape[0]):
        for r in range(R):
            t = 0.0
            for s in range(R):
                t = t + float(K0[r, s]) * float(c0[k, s])
            g[k, r] = t
    return g


def c0_tensor(nu, N, plane="stress"):
    """C0(ν) at E = 1 in Voigt order with engineering shears"""
    lam, mu = material(nu, N, plane)
    M = nstrains(N)
    C = np.zeros((M, M))
    C[:N, :N] = lam
    for i in range(N):
        C[i, i] = lam + 2 * mu
    for k in range(N, M):
        C[k, k] = mu
    return C


class Operator:
    """one level of the torus: the cell moduli E (shape m), the mesh sizes h, the level's K0"""

    def __init__(self, E, h, K0):
        self.E = np.asfortranarray(E, dtype=np.float64)
        self.N = N = self.E.ndim
        self.m = self.n = tuple(self.E.shape)
        self.h = tuple(float(x) for x in h)
        self.K0 = np.array(K0, dtype=np.float64)
        self.c0 = chi0(self.h)
        self.g = unit_loads(self.K0, self.c0)
        self.free = np.ones((N,) + self.m, dtype=bool)
        self.free[(slice(None),) + (0,) * N] = False
        D = np.zeros((N,) + self.m)
        for m in range(1 << N):
            a = (~m) & ((1 << N) - 1)
            Ec = self._cell(self.E, m)
            for i in range(N):
                D[i] = D[i] + Ec * self.K0[a * N + i, a * N + i]
        self.D = D
        self._A = None

    def _cell(self, c, m):
        """cell m of every node: index I − 1 + bits(m), wrapped"""
        return np.roll(c, tuple(1 - b for b in _bits(m, self.N)), axis=tuple(range(self.N)))

    def _node(self, v, m, b):
        """corner b of cell m of every node: I − 1 + bits(m) + bits(b), wrapped"""
        return np.roll(v, tuple(1 - x - y for x, y in zip(_bits(m, self.N), _bits(b, self.N))), axis=tuple(range(self.N)))

    def _corner(self, v, b):
        """corner b of every cell: C + bits(b), wrapped"""
        return np.roll(v, tuple(-x for x in _bits(b, self.N)), axis=tuple(range(self.N)))

    def apply(self, u):
        """A u on all components, no pin: _elastic_ref.Operator.apply's order"""
        N, NC = self.N, 1 << self.N
        u = np.asarray(u)
        dt = LD if u.dtype == LD else np.float64
        u = u.astype(dt, copy=False)
        acc = np.zeros((N,) + self.m, dtype=dt)
        for m in range(NC):
            a = (~m) & (NC - 1)
            Ec = self._cell(self.E, m)
            inner = np.zeros((N,) + self.m, dtype=dt)
            for b in range(NC):
                for j in range(N):
                    v = self._node(u[j], m, b)
                    for i in range(N):
                        inner[i] = inner[i] + self.K0[a * N + i, b * N + j] * v
            for i in range(N):
                acc[i] = acc[i] + Ec * inner[i]
        return acc

    def load(self, k):
        N, NC = self.N, 1 << self.N
        acc = np.zeros((N,) + self.m)
        for m in range(NC):
            a = (~m) & (NC - 1)
            Ec = self._cell(self.E, m)
            for i in range(N):
                acc[i] = acc[i] + Ec * self.g[k, a * N + i]
        return -acc

    def _w(self, chi, k):
        """the 2^N·N corner arrays of w^k = χ0^k + χ^k"""
        N = self.N
        return [self.c0[k, r] + self._corner(chi[k][r % N], r // N) for r in range((1 << N) * N)]

    def _kw(self, wq):
        """K0·w^q at every cell, each row from +0 ascending"""
        R = len(wq)
        out = []
        for r in range(R):
            t = np.zeros(self.m)
            for s in range(R):
                t = t + self.K0[r, s] * wq[s]
            out.append(t)
        return out

    def _dot(self, wp, wq, kw=None):
        kw = self._kw(wq) if kw is None else kw
        d = np.zeros(self.m)
        for r in range(len(wp)):
            d = d + wp[r] * kw[r]
        return d

    def energy_cells(self, chi, p, q):
        chi = np.asarray(chi, dtype=np.float64)
        return self.E * self._dot(self._w(chi, p), self._w(chi, q))

    def tensor(self, chi):
        """C^H from the cell integrands with math.fsum, mirrored"""
        M, nc = nstrains(self.N), int(np.prod(self.m))
        C = np.zeros((M, M))
        for q in range(M):
            for p in range(q + 1):
                C[p, q] = C[q, p] = math.fsum(self.energy_cells(chi, p, q).reshape(-1)) / nc
        return C

    def sensitivity_cells(self, chi, W):
        chi = np.asarray(chi, dtype=np.float64)
        M = nstrains(self.N)
        w = [self._w(chi, k) for k in range(M)]
        acc = np.zeros(self.m)
        for q in range(M):
            kw = self._kw(w[q])
            for p in range(q + 1):
                c = 2.0 * W[p, q] if p < q else W[p, q]
                acc = acc + c * (self.E * self._dot(w[p], w[q], kw))
        return acc

    def sensitivity(self, chi, W):
        """the node field on the n = m + 1 nodes of the dense grid (node n − 1 is node 0)"""
        N = self.N
        cell = self.sensitivity_cells(chi, np.asarray(W, dtype=np.float64))
        acc = np.zeros(self.m)
        for m in range(1 << N):
            acc = acc + self._cell(cell, m)
        return image(acc * 2.0 ** -N)

    def matrix(self):
        """the assembled periodic A (csr) over component-major unknowns i·nn + id"""
        if self._A is None:
            N, NC = self.N, 1 << self.N
            nn = int(np.prod(self.m))
            idx = np.arange(nn).reshape(self.m, order="F")
            corner = [self._corner(idx, b).reshape(-1, order="F") for b in range(NC)]
            Ec = self.E.reshape(-1, order="F")
            rows, cols, vals = [], [], []
            for a in range(NC):
                for i in range(N):
                    for b in range(NC):
                        for j in range(N):
                            k = self.K0[a * N + i, b * N + j]
                            if k != 0.0:
                                rows.append(i * nn + corner[a])
                                cols.append(j * nn + corner[b])
                                vals.append(Ec * k)
            self._A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N * nn, N * nn))
        return self._A

    def flat(self, u):
        return np.concatenate([np.asarray(u[i]).reshape(-1, order="F") for i in range(self.N)])

    def unflat(self, x):
        nn = int(np.prod(self.m))
        return np.stack([x[i * nn:(i + 1) * nn].reshape(self.m, order="F") for i in range(self.N)])

    def apply_free(self, x):
        y = self.unflat(self.matrix() @ self.flat(np.where(self.free, x, 0.0)))
        return np.where(self.free, y, 0.0)


def image(v):
    """an m-shaped torus field on the n = m + 1 nodes of the dense grid"""
    return np.pad(v, [(0, 1)] * v.ndim, mode="wrap")


def coarsen_shape(m):
    co = tuple(x % 2 == 0 and x > 4 for x in m)
    return (tuple(x // 2 if c else x for x, c in zip(m, co)), co) if any(co) else None


def coarsen_cells(E, co):
    """mg_cell_average: the cells {2J, 2J+1} per coarsened axis, ascending, the first taken as it is; ·2^−k"""
    N = E.ndim
    s = None
    for m in range(1 << N):
        bits = _bits(m, N)
        if any(b and not c for b, c in zip(bits, co)):
            continue
        v = E[tuple(slice(b, None, 2) if c else slice(None) for b, c in zip(bits, co))]
        s = v.copy() if s is None else s + v
    return np.asfortranarray(s * 2.0 ** -sum(co))


def _p1(mf):
    """the 1-D wrapping prolongation from mf/2 to mf nodes"""
    mc = mf // 2
    P = sp.lil_matrix((mf, mc))
    for J in range(mc):
        P[2 * J, J] = 1.0
        P[(2 * J + 1) % mf, J] += 0.5
        P[(2 * J - 1) % mf, J] += 0.5
    return P.tocsr()


def prolongation(mf, co):
    P = None
    for d in range(len(mf)):
        Pd = _p1(mf[d]) if co[d] else sp.identity(mf[d], format="csr")
        P = Pd if P is None else sp.kron(Pd, P, format="csr")
    return P


class Hierarchy:
    def __init__(self, E, h, nu=0.3, plane="stress", k0s=None, omegas=None):
        self.nu, self.plane, self.omegas, self._om = nu, plane, omegas, {}
        mk = (lambda l, hh: k0(hh, nu, plane)) if k0s is None else (lambda l, hh: k0s[l])
        self.ops, self.P = [Operator(E, h, mk(0, tuple(h)))], []
        while True:
            f = self.ops[-1]
            cs = coarsen_shape(f.m)
            if cs is None:
                break
            mc, co = cs
            hh = tuple(x * 2.0 if c else x for x, c in zip(f.h, co))
            self.ops.append(Operator(coarsen_cells(f.E, co), hh, mk(len(self.ops), hh)))
            self.P.append((prolongation(f.m, co), 2.0 ** -sum(co), co))

    @property
    def levels(self):
        return len(self.ops)

    def omega(self, lev):
        if self.omegas is not None:
            return self.omegas[lev]
        if lev not in self._om:
            self._om[lev] = level_omega(self.ops[lev].K0, self.ops[lev].N, OMEGA)
        return self._om[lev]

    def _smooth(self, op, x, r, sweeps, omega):
        for _ in range(sweeps):
            if x is None:
                x = np.where(op.free, omega * r / op.D, 0.0)
            else:
                x = np.where(op.free, x + omega * (r - op.apply_free(x)) / op.D, 0.0)
        return x

    def vcycle(self, r, lev=0):
        op = self.ops[lev]
        r = np.where(op.free, r, 0.0)
        om = self.omega(lev)
        if lev == self.levels - 1:
            return self._smooth(op, None, r, NCOARSE, om)
        x = self._smooth(op, None, r, NPRE, om)
        P, scale, _ = self.P[lev]
        cop = self.ops[lev + 1]
        res = np.where(op.free, r - op.apply_free(x), 0.0)
        rc = np.stack([(P.T @ res[i].reshape(-1, order="F") * scale).reshape(cop.m, order="F") for i in range(op.N)])
        xc = self.vcycle(np.where(cop.free, rc, 0.0), lev + 1)
        px = np.stack([(P @ xc[i].reshape(-1, order="F")).reshape(op.m, order="F") for i in range(op.N)])
        x = np.where(op.free, x + px, 0.0)
        return self._smooth(op, x, r, NPOST, om)

    def vcycle_matrix(self):
        """M as a dense matrix over the free unknowns of level 0"""
        op = self.ops[0]
        free = op.flat(op.free)
        idx = np.flatnonzero(free)
        out = np.zeros((idx.size, idx.size))
        for c, j in enumerate(idx):
            e = np.zeros(free.size)
            e[j] = 1.0
            out[:, c] = op.flat(self.vcycle(op.unflat(e)))[idx]
        return out


def device_omegas(k0s, N):
    return [min(OMEGA, SAFE / symbol_lambda_power(K, N)) for K in k0s]


def pcg(hier, f, x0=None, rtol=1e-8, max_iters=500, precond="mg"):
    """PCG away from the pin until the recursive ‖r‖₂ ≤ rtol·‖f_free‖₂.  Returns (x, iterations, relres, converged)."""
    op = hier.ops[0]
    M = (lambda r: hier.vcycle(r, 0)) if precond == "mg" else (lambda r: np.where(op.free, r / op.D, 0.0))
    b = np.where(op.free, np.asarray(f, dtype=np.float64), 0.0)
    x = np.zeros_like(b) if x0 is None else np.where(op.free, np.asarray(x0, dtype=np.float64), 0.0)
    r = np.where(op.free, b - op.unflat(op.matrix() @ op.flat(x)), 0.0)
    bb = float(np.sum(b * b))
    rr = float(np.sum(r * r))
    if bb == 0.0:
        bb = rr
    if rr <= rtol * rtol * bb:
        return x, 0, (np.sqrt(rr / bb) if bb > 0 else 0.0), True
    z = M(r)
    rho = float(np.sum(r * z))
    p = z
    for it in range(1, max_iters + 1):
        q = op.apply_free(p)
        alpha = rho / float(np.sum(p * q))
        x = x + alpha * p
        r = r - alpha * q
        rr = float(np.sum(r * r))
        if rr <= rtol * rtol * bb:
            return x, it, np.sqrt(rr / bb), True
        if not np.isfinite(rr):
            break
        z = M(r)
        rho1 = float(np.sum(r * z))
        p = z + (rho1 / rho) * p
        rho = rho1
    return x, max_iters, np.sqrt(rr / bb), False


def direct(op, f):
    """the pinned sparse direct solve; the factorisation is kept on the operator for the M right-hand sides"""
    free = op.flat(op.free)
    if getattr(op, "_lu", None) is None:
        # the matrix is symmetric positive definite: the symmetric ordering factors 17×17×17 five times faster than the default
        op._lu = spla.splu(op.matrix()[free][:, free].tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    x = np.zeros(free.size)
    x[free] = op._lu.solve(op.flat(f)[free])
    return op.unflat(x)


def true_residual(op, f, x):
    """‖(f − A x)_free‖₂ with A x in the stated order, and ‖f_free‖₂"""
    r = np.where(op.free, f - op.apply(x), 0.0)
    return float(np.sqrt(np.sum(r * r))), float(np.sqrt(np.sum(np.where(op.free, f, 0.0) ** 2)))


def correctors(hier, how="direct", rtol=1e-8, precond="mg", max_iters=3000):
    """(χ of shape (M, N)+m, iterations per corrector or None)"""
    op = hier.ops[0]
    M = nstrains(op.N)
    if how == "direct":
        return np.stack([direct(op, op.load(k)) for k in range(M)]), None
    out, its = [], []
    for k in range(M):
        x, it, rel, ok = pcg(hier, op.load(k), None, rtol, max_iters, precond)
        assert ok, (k, it, rel)
        out.append(x)
        its.append(it)
    return np.stack(out), its


# ---- closed forms

def laminate_tensor(E1, E2, theta, nu, N, plane="stress", axis=0):
    """layers normal to `axis`, phases E1 (volume fraction θ) and E2: the exact tensor (Q1 is exact for cell-aligned layers)"""
    lam, mu = material(nu, N, plane)
    Ms = lam + 2 * mu
    mean = theta * E1 + (1 - theta) * E2
    harm = 1.0 / (theta / E1 + (1 - theta) / E2)
    M = nstrains(N)
    C = np.zeros((M, M))
    a = axis
    C[a, a] = harm * Ms
    for i in range(N):
        if i == a:
            continue
        C[a, i] = C[i, a] = (lam / Ms) * C[a, a]
        for j in range(N):
            if j == a:
                continue
            base = (Ms if i == j else lam) - lam * lam / Ms
            C[i, j] = mean * base + (lam / Ms) ** 2 * C[a, a]
    for k, (i, j) in enumerate(VOIGT[N]):
        if i != j:
            C[k, k] = harm * mu if a in (i, j) else mean * mu
    return C


def laminate_cells(m, E1, E2, layers, axis=0):
    """cells of modulus E1 in the first `layers` cells along `axis`, E2 in the rest"""
    E = np.full(m, E2, order="F")
    sl = [slice(None)] * len(m)
    sl[axis] = slice(0, layers)
    E[tuple(sl)] = E1
    return E


# ---- the cases shared by tests/test_homog_host.py and tests/test_gpu_homog.py

def inclusion(n, h, radius2=0.09):
    """ϕ < 0 outside a centred disc / ball of the unit-scaled box: the inclusion is the ersatz (soft) phase"""
    ax = [np.arange(nd) * hd for nd, hd in zip(n, h)]
    X = np.meshgrid(*ax, indexing="ij")
    c = [0.5 * (nd - 1) * hd for nd, hd in zip(n, h)]
    L = max((nd - 1) * hd for nd, hd in zip(n, h))
    r2 = sum(((x - ci) / L) ** 2 for x, ci in zip(X, c))
    return np.asfortranarray((radius2 - r2) * L)


def cases():
    """name → dict(n, hc, h, phi, E, E_in, E_out, nu, plane, level, dtype, both): `both` = run the Jacobi preconditioner as well"""
    rng = np.random.default_rng(23)
    out = {}

    def add(name, n, hc=None, E=None, contrast=1e-3, nu=0.3, plane="stress", level=0.0, dtype=np.float64, both=True, radius2=None):
        N = len(n)
        hc = tuple((nd - 1.0) / (max(n) - 1.0) for nd in n) if hc is None else hc
        h = tuple(x / (nd - 1) for x, nd in zip(hc, n))
        radius2 = (0.09 if N == 2 else 0.1) if radius2 is None else radius2
        out[name] = dict(n=n, hc=hc, h=h, phi=inclusion(n, h, radius2), E=E, E_in=1.0, E_out=contrast, nu=nu, plane=plane, level=level, dtype=dtype, both=both)

    add("5x5", (5, 5), contrast=0.1)                                   # one level, 16 nodes
    add("9x9", (9, 9), contrast=0.1, plane="strain")                   # 8 → 4
    add("13x9", (13, 9), contrast=0.1)                                 # 12,8 → 6,4 → 3,4: one axis coarsens alone, ω < 0.6
    add("11x11", (11, 11), contrast=0.1, level=0.02)                   # 10 → 5; a level other than zero
    add("24x24", (24, 24), contrast=0.1)                               # m = 23: one level of 529 nodes, the multi-launch coarsest
    add("17x33", (17, 33), hc=(1.0, 1.0), contrast=0.1)                # anisotropic h
    add("17x17_f32", (17, 17), contrast=0.1, dtype=np.float32)         # a float32 handle
    add("5x5x5", (5, 5, 5), contrast=0.1)
    add("9x9x9", (9, 9, 9), contrast=0.1)
    add("9x5x7", (9, 5, 7), contrast=0.1)
    add("8x8x8", (8, 8, 8), contrast=0.1)                              # m = 7: 343 nodes, one level
    add("12x10_given_E", (12, 10), E=np.asfortranarray(0.5 + rng.random((11, 9))))
    add("33x33_soft", (33, 33))                                        # a soft inclusion at contrast 1e-3
    add("17x17x17_soft", (17, 17, 17), both=False)
    return out


def build_case(cs, k0s=None, omegas=None):
    phi = cs["phi"].astype(cs["dtype"]).astype(np.float64)
    E = cs["E"] if cs["E"] is not None else cell_coefficients(phi, cs["h"], cs["level"], cs["E_in"], cs["E_out"])
    return Hierarchy(E, cs["h"], cs["nu"], cs["plane"], k0s, omegas)


_SOLVED = {}


def solved(name):
    """the restatement's results for a case, computed once: hier, the direct correctors, and per preconditioner (χ, iterations)"""
    if name not in _SOLVED:
        cs = cases()[name]
        hier = build_case(cs)
        res = dict(case=cs, hier=hier, direct=correctors(hier, "direct")[0])
        for pc in ("mg", "jacobi"):
            res[pc] = correctors(hier, "pcg", 1e-8, pc) if (pc == "mg" or cs["both"]) else None
        _SOLVED[name] = res
    return _SOLVED[name]


# the prototype table of DESIGN.md §7.23: a soft disc (radius 0.3) / ball (radius² 0.1) at contrast 1e-3
TABLE = [((33, 33), None), ((65, 65), None), ((49, 33), None), ((11, 11), None), ((9, 9, 9), None), ((17, 17, 17), None), ((17, 9, 13), (1.0, 0.6, 0.9))]


def prototype(n, hc=None, contrast=1e-3):
    N = len(n)
    hc = tuple((nd - 1.0) / (max(n) - 1.0) for nd in n) if hc is None else hc
    h = tuple(x / (nd - 1) for x, nd in zip(hc, n))
    E = cell_coefficients(inclusion(n, h, 0.09 if N == 2 else 0.1), h, 0.0, 1.0, contrast)
    return Hierarchy(E, h)


# ---- the first PCG iterate in long double: from x0 = 0, x₁ = α·M b, α = (b·Mb)/(Mb·A Mb)

def _apply_free_ld(op, x):
    return np.where(op.free, op.apply(np.where(op.free, x, LD(0))), LD(0))


def _transfer_ld(x, co, transpose):
    """P (transpose False: coarse → fine) or Pᵀ axis by axis, wrapped, in long double"""
    for d, c in enumerate(co):
        if not c:
            continue
        x = np.moveaxis(x, d, 0)
        if transpose:
            x = x[0::2] + LD(0.5) * (np.roll(x, 1, axis=0)[0::2] + np.roll(x, -1, axis=0)[0::2])
        else:
            f = np.zeros((2 * x.shape[0],) + x.shape[1:], dtype=LD)
            f[0::2] = x
            f[1::2] = LD(0.5) * (x + np.roll(x, -1, axis=0))
            x = f
        x = np.moveaxis(x, 0, d)
    return x


def _vcycle_ld(hier, r, lev=0):
    op = hier.ops[lev]
    D, om = op.D.astype(LD), LD(hier.omega(lev))
    coarsest = lev == hier.levels - 1
    x = np.where(op.free, om * r / D, LD(0))
    for _ in range((NCOARSE if coarsest else NPRE) - 1):
        x = np.where(op.free, x + om * (r - _apply_free_ld(op, x)) / D, LD(0))
    if coarsest:
        return x
    cop = hier.ops[lev + 1]
    _, scale, co = hier.P[lev]
    res = np.where(op.free, r - _apply_free_ld(op, x), LD(0))
    rc = np.stack([_transfer_ld(res[i], co, True) * LD(scale) for i in range(op.N)])
    xc = _vcycle_ld(hier, np.where(cop.free, rc, LD(0)), lev + 1)
    px = np.stack([_transfer_ld(xc[i], co, False) for i in range(op.N)])
    x = np.where(op.free, x + px, LD(0))
    for _ in range(NPOST):
        x = np.where(op.free, x + om * (r - _apply_free_ld(op, x)) / D, LD(0))
    return x


def first_iterate_ld(hier, f):
    op = hier.ops[0]
    b = np.where(op.free, np.asarray(f).astype(LD), LD(0))
    z = _vcycle_ld(hier, b)
    return (np.sum(b * z) / np.sum(z * _apply_free_ld(op, z))) * z


FIRST_RTOL, FIRST_RELRES = 0.97, 0.95
FIRST_ITERATE = ["5x5", "13x9", "24x24", "9x5x7", "8x8x8"]


def first_iterate_rhs(op):
    """name → f: load 0, and unit impulses (component 0) next to the pinned node and at the last node of every axis (the wrap)"""
    out = {"load0": op.load(0)}
    for name, j in (("next", (1,) + (0,) * (op.N - 1)), ("last", tuple(m - 1 for m in op.m))):
        f = np.zeros((op.N,) + op.m)
        f[(0,) + j] = 1.0
        out[name] = f
    for d in range(op.N):
        f = np.zeros((op.N,) + op.m)
        f[(d,) + tuple(op.m[e] - 1 if e == d else 0 for e in range(op.N))] = 1.0
        out[f"last{d}"] = f
    return out


def first_iterate_runs(hier):
    """[(name, f, x₁ of the restatement in float64, its relative residual)] for the right-hand sides whose relative residual after
    the restatement's first iteration is ≤ FIRST_RELRES (a solve at FIRST_RTOL then stops after exactly one iteration), and the
    names left out"""
    runs, left_out = [], []
    for name, f in first_iterate_rhs(hier.ops[0]).items():
        x, it, rel, ok = pcg(hier, f, None, FIRST_RTOL, 1, "mg")
        (runs if it == 1 and rel <= FIRST_RELRES else left_out).append((name, f, x, rel))
    return runs, left_out
