"""homogenize_conductivity restated in numpy and scipy.sparse (csrc/lsm_hcond.hip, include/lsm.h "homogenize_conductivity").

The torus has m = n − 1 nodes and cells per axis (node n − 1 is node 0); vectors are m-shaped.  The functions the device is compared
with bit for bit (Operator.apply, D, load, energy_cells, sensitivity; the cell array is _elliptic_ref.cell_coefficients) spell their
operation order out with np.roll; the hierarchy, the V-cycle and PCG are compared to rounding / by iteration counts.  Every sum
starts from +0.

  cells     the 2^N cells around node I, m = 0 … 2^N − 1: bit d of m set: cell I_d along d, clear: cell I_d − 1, wrapped
  edge      from I towards I ± e_d: k̄ = (Σ of the cells whose bit d is 1 (plus) or 0 (minus), m ascending)·2^−(N−1); w = k̄·ih2_d
  operator  (A u)_I = Σ_d [ w_−·(u_I − u_{I−e_d}) + w_+·(u_I − u_{I+e_d}) ], d ascending, minus before plus; D_I the sum of the w alike
  load      f^p_I = k̄_+(d = p)/h_p − k̄_−(d = p)/h_p
  g^p_{d,a} δ_dp + (χ^p[a + e_d] − χ^p[a])/h_d on the edge along d from corner a of a cell (bit d of a clear), δ = 1.0 or 0.0
  t^{pq}_C  (a_C·2^−(N−1))·(Σ_d Σ_a g^p_{d,a}·g^q_{d,a}), d ascending, within it a ascending
  K^H_pq    (Σ_C t^{pq}_C)/ncells
  sens.     cell_C = Σ_q Σ_{p≤q} (c·W_pq)·t^{pq}_C, c = 2 for p < q; s_I = (Σ of the cells around I, m ascending)·2^−N
  hierarchy _homog_ref's: axis d coarsens while m_d is even and > 4; coarse cell = mean of cells 2J, 2J+1; R = 2^−k·(½, 1, ½ per
            axis, wrapped); P = Rᵀ·2^k; node 0 pinned on every level; ω = 0.8; 2 + 2 sweeps, 16 on the coarsest level
"""
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from _elastic_ref import _bits
from _elliptic_ref import LD, NCOARSE, NPOST, NPRE, OMEGA, cell_coefficients
from _homog_ref import _transfer_ld, coarsen_cells, coarsen_shape, image, inclusion, laminate_cells, prolongation


class Operator:
    """one level of the torus: the cell coefficients a (shape m) and the mesh sizes h"""

    def __init__(self, a, h):
        self.a = np.asfortranarray(a, dtype=np.float64)
        self.N = N = self.a.ndim
        self.m = self.n = tuple(self.a.shape)
        self.h = tuple(float(x) for x in h)
        self.ih2 = tuple(1.0 / (x * x) for x in self.h)
        self.half = 2.0 ** -(N - 1)
        self.free = np.ones(self.m, dtype=bool)
        self.free[(0,) * N] = False
        self.kbar, self.w = [], []
        for d in range(N):
            kb = []
            for s in (0, 1):
                S = np.zeros(self.m)
                for m in range(1 << N):
                    if ((m >> d) & 1) == s:
                        S = S + self._cell(self.a, m)
                kb.append(S * self.half)
            self.kbar.append(kb)
            self.w.append([k * self.ih2[d] for k in kb])
        D = np.zeros(self.m)
        for d in range(N):
            D = D + self.w[d][0]
            D = D + self.w[d][1]
        self.D = D
        self._A = None

    def _cell(self, c, m):
        """cell m of every node: index I − 1 + bits(m), wrapped"""
        return np.roll(c, tuple(1 - b for b in _bits(m, self.N)), axis=tuple(range(self.N)))

    def _corner(self, v, b):
        """corner b of every cell: C + bits(b), wrapped"""
        return np.roll(v, tuple(-x for x in _bits(b, self.N)), axis=tuple(range(self.N)))

    def apply(self, u):
        """A u on all nodes, no pin, in the stated order (float64, or long double from the float64 coefficients)"""
        u = np.asarray(u)
        dt = LD if u.dtype == LD else np.float64
        u = u.astype(dt, copy=False)
        acc = np.zeros(self.m, dtype=dt)
        for d in range(self.N):
            acc = acc + self.w[d][0].astype(dt, copy=False) * (u - np.roll(u, 1, axis=d))
            acc = acc + self.w[d][1].astype(dt, copy=False) * (u - np.roll(u, -1, axis=d))
        return acc

    def apply_free(self, x):
        """the pinned operator: x is taken as zero at node 0, and so is the result"""
        zero = LD(0) if np.asarray(x).dtype == LD else 0.0
        return np.where(self.free, self.apply(np.where(self.free, x, zero)), zero)

    def load(self, p):
        return self.kbar[p][1] / self.h[p] - self.kbar[p][0] / self.h[p]

    def _grad(self, chi_p, p):
        """g^p[d][e]: the edges along d of every cell, their starting corners a (bit d clear) ascending"""
        out = []
        for d in range(self.N):
            row = []
            for a in range(1 << self.N):
                if (a >> d) & 1:
                    continue
                row.append((1.0 if d == p else 0.0) + (self._corner(chi_p, a | (1 << d)) - self._corner(chi_p, a)) / self.h[d])
            out.append(row)
        return out

    def _pair(self, gp, gq):
        s = np.zeros(self.m)
        for d in range(self.N):
            for e in range(len(gp[d])):
                s = s + gp[d][e] * gq[d][e]
        return (self.a * self.half) * s

    def energy_cells(self, chi, p, q):
        chi = np.asarray(chi, dtype=np.float64)
        return self._pair(self._grad(chi[p], p), self._grad(chi[q], q))

    def tensor(self, chi):
        """K^H from the cell integrands with math.fsum, mirrored"""
        N, nc = self.N, int(np.prod(self.m))
        K = np.zeros((N, N))
        for q in range(N):
            for p in range(q + 1):
                K[p, q] = K[q, p] = math.fsum(self.energy_cells(chi, p, q).reshape(-1)) / nc
        return K

    def sensitivity_cells(self, chi, W):
        chi = np.asarray(chi, dtype=np.float64)
        g = [self._grad(chi[p], p) for p in range(self.N)]
        acc = np.zeros(self.m)
        for q in range(self.N):
            for p in range(q + 1):
                c = 2.0 * W[p, q] if p < q else W[p, q]
                acc = acc + c * self._pair(g[p], g[q])
        return acc

    def sensitivity(self, chi, W):
        """the node field on the n = m + 1 nodes of the dense grid (node n − 1 is node 0)"""
        cell = self.sensitivity_cells(chi, np.asarray(W, dtype=np.float64))
        acc = np.zeros(self.m)
        for m in range(1 << self.N):
            acc = acc + self._cell(cell, m)
        return image(acc * 2.0 ** -self.N)

    def matrix(self):
        """the assembled periodic A (csr), node index axis 0 fastest"""
        if self._A is None:
            nn = int(np.prod(self.m))
            idx = np.arange(nn).reshape(self.m, order="F")
            i = idx.reshape(-1, order="F")
            rows, cols, vals = [], [], []
            for d in range(self.N):
                for s, shift in ((0, 1), (1, -1)):
                    j = np.roll(idx, shift, axis=d).reshape(-1, order="F")
                    w = self.w[d][s].reshape(-1, order="F")
                    rows += [i, i]
                    cols += [i, j]
                    vals += [w, -w]
            self._A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nn, nn))
        return self._A


class Hierarchy:
    def __init__(self, a, h):
        self.ops, self.P = [Operator(a, h)], []
        while True:
            f = self.ops[-1]
            cs = coarsen_shape(f.m)
            if cs is None:
                break
            _, co = cs
            hh = tuple(x * 2.0 if c else x for x, c in zip(f.h, co))
            self.ops.append(Operator(coarsen_cells(f.a, co), hh))
            self.P.append((prolongation(f.m, co), 2.0 ** -sum(co), co))

    @property
    def levels(self):
        return len(self.ops)

    def _smooth(self, op, x, r, sweeps):
        for _ in range(sweeps):
            if x is None:
                x = np.where(op.free, OMEGA * r / op.D, 0.0)
            else:
                x = np.where(op.free, x + OMEGA * (r - op.apply_free(x)) / op.D, 0.0)
        return x

    def vcycle(self, r, lev=0):
        op = self.ops[lev]
        r = np.where(op.free, r, 0.0)
        if lev == self.levels - 1:
            return self._smooth(op, None, r, NCOARSE)
        x = self._smooth(op, None, r, NPRE)
        P, scale, _ = self.P[lev]
        cop = self.ops[lev + 1]
        res = np.where(op.free, r - op.apply_free(x), 0.0)
        rc = (P.T @ res.reshape(-1, order="F") * scale).reshape(cop.m, order="F")
        xc = self.vcycle(np.where(cop.free, rc, 0.0), lev + 1)
        x = np.where(op.free, x + (P @ xc.reshape(-1, order="F")).reshape(op.m, order="F"), 0.0)
        return self._smooth(op, x, r, NPOST)

    def vcycle_matrix(self):
        """M as a dense matrix over the free nodes of level 0"""
        op = self.ops[0]
        idx = np.flatnonzero(op.free.reshape(-1, order="F"))
        out = np.zeros((idx.size, idx.size))
        for c, j in enumerate(idx):
            e = np.zeros(op.free.size)
            e[j] = 1.0
            out[:, c] = self.vcycle(e.reshape(op.m, order="F")).reshape(-1, order="F")[idx]
        return out


def pcg(hier, f, x0=None, rtol=1e-8, max_iters=500, precond="mg"):
    """PCG away from the pin until the recursive ‖r‖₂ ≤ rtol·‖f_free‖₂.  Returns (x, iterations, relres, converged)."""
    op = hier.ops[0]
    M = (lambda r: hier.vcycle(r, 0)) if precond == "mg" else (lambda r: np.where(op.free, r / op.D, 0.0))
    b = np.where(op.free, np.asarray(f, dtype=np.float64), 0.0)
    x = np.zeros_like(b) if x0 is None else np.where(op.free, np.asarray(x0, dtype=np.float64), 0.0)
    r = np.where(op.free, b - op.apply(x), 0.0)
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
    """the pinned sparse direct solve; the factorisation is kept on the operator for the N right-hand sides"""
    free = op.free.reshape(-1, order="F")
    if getattr(op, "_lu", None) is None:
        op._lu = spla.splu(op.matrix()[free][:, free].tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    x = np.zeros(free.size)
    x[free] = op._lu.solve(np.asarray(f, dtype=np.float64).reshape(-1, order="F")[free])
    return x.reshape(op.m, order="F")


def true_residual(op, f, x):
    """‖(f − A x)_free‖₂ with A x in the stated order, and ‖f_free‖₂"""
    r = np.where(op.free, f - op.apply(x), 0.0)
    return float(np.sqrt(np.sum(r * r))), float(np.sqrt(np.sum(np.where(op.free, f, 0.0) ** 2)))


def correctors(hier, how="direct", rtol=1e-8, precond="mg", max_iters=3000):
    """(χ of shape (N,)+m, iterations per corrector or None)"""
    op = hier.ops[0]
    if how == "direct":
        return np.stack([direct(op, op.load(k)) for k in range(op.N)]), None
    out, its = [], []
    for k in range(op.N):
        x, it, rel, ok = pcg(hier, op.load(k), None, rtol, max_iters, precond)
        assert ok, (k, it, rel)
        out.append(x)
        its.append(it)
    return np.stack(out), its


# ---- closed forms

def laminate_tensor(a1, a2, theta, N, axis=0):
    """layers normal to `axis`, phases a1 (volume fraction θ) and a2: the harmonic mean across the layers, the arithmetic mean along them"""
    K = np.eye(N) * (theta * a1 + (1 - theta) * a2)
    K[axis, axis] = 1.0 / (theta / a1 + (1 - theta) / a2)
    return K


# ---- the cases shared by tests/test_hcond_host.py and tests/test_gpu_hcond.py

def cases():
    """name → dict(n, hc, h, phi, a, a_in, a_out, level, dtype)"""
    rng = np.random.default_rng(29)
    out = {}

    def add(name, n, hc=None, a=None, contrast=0.1, level=0.0, dtype=np.float64):
        hc = tuple((nd - 1.0) / (max(n) - 1.0) for nd in n) if hc is None else hc
        h = tuple(x / (nd - 1) for x, nd in zip(hc, n))
        out[name] = dict(n=n, hc=hc, h=h, phi=inclusion(n, h, 0.09 if len(n) == 2 else 0.1), a=a, a_in=1.0, a_out=contrast, level=level, dtype=dtype)

    add("5x5", (5, 5))                                                 # one level, 16 nodes
    add("13x9", (13, 9))                                               # 12,8 → 6,4 → 3,4: one axis coarsens alone
    add("11x11_level", (11, 11), level=0.02)                           # 10 → 5; a level other than zero
    add("24x24", (24, 24))                                             # m = 23: one level of 529 nodes, the multi-launch coarsest
    add("17x17_f32", (17, 17), dtype=np.float32)                       # a float32 handle
    add("12x10_given_a", (12, 10), a=np.asfortranarray(0.5 + rng.random((11, 9))))
    add("33x33_soft", (33, 33), contrast=1e-3)                         # four levels, a soft inclusion
    add("9x5x7", (9, 5, 7))
    add("8x8x8", (8, 8, 8))                                            # m = 7: 343 nodes, one level
    add("17x17x17_soft", (17, 17, 17), contrast=1e-3)                  # three levels
    add("17x9x13_aniso_h", (17, 9, 13), hc=(1.0, 0.6, 0.9))            # h ∝ (1, 1.2, 1.2)
    return out


def build_case(cs):
    phi = cs["phi"].astype(cs["dtype"]).astype(np.float64)
    a = cs["a"] if cs["a"] is not None else cell_coefficients(phi, cs["h"], cs["level"], cs["a_in"], cs["a_out"])
    return Hierarchy(a, cs["h"])


_SOLVED = {}


def solved(name):
    """the restatement's results for a case, computed once: hier, the direct correctors, and per preconditioner (χ, iterations)"""
    if name not in _SOLVED:
        cs = cases()[name]
        hier = build_case(cs)
        res = dict(case=cs, hier=hier, direct=correctors(hier, "direct")[0])
        for pc in ("mg", "jacobi"):
            res[pc] = correctors(hier, "pcg", 1e-8, pc)
        _SOLVED[name] = res
    return _SOLVED[name]


# the prototype table of DESIGN.md §7.24: a soft disc (radius 0.3) / ball (radius² 0.1) at contrast 1e-3
TABLE = [((33, 33), None), ((65, 65), None), ((49, 33), None), ((11, 11), None), ((9, 9, 9), None), ((17, 17, 17), None), ((17, 9, 13), (1.0, 0.6, 0.9))]


def prototype(n, hc=None, contrast=1e-3):
    hc = tuple((nd - 1.0) / (max(n) - 1.0) for nd in n) if hc is None else hc
    h = tuple(x / (nd - 1) for x, nd in zip(hc, n))
    return Hierarchy(cell_coefficients(inclusion(n, h, 0.09 if len(n) == 2 else 0.1), h, 0.0, 1.0, contrast), h)


# ---- the first PCG iterate in long double: from x0 = 0, x₁ = α·M b, α = (b·Mb)/(Mb·A Mb)

def _vcycle_ld(hier, r, lev=0):
    op = hier.ops[lev]
    D, om = op.D.astype(LD), LD(OMEGA)
    coarsest = lev == hier.levels - 1
    x = np.where(op.free, om * r / D, LD(0))
    for _ in range((NCOARSE if coarsest else NPRE) - 1):
        x = np.where(op.free, x + om * (r - op.apply_free(x)) / D, LD(0))
    if coarsest:
        return x
    cop = hier.ops[lev + 1]
    _, scale, co = hier.P[lev]
    res = np.where(op.free, r - op.apply_free(x), LD(0))
    rc = np.where(cop.free, _transfer_ld(res, co, True) * LD(scale), LD(0))
    x = np.where(op.free, x + _transfer_ld(_vcycle_ld(hier, rc, lev + 1), co, False), LD(0))
    for _ in range(NPOST):
        x = np.where(op.free, x + om * (r - op.apply_free(x)) / D, LD(0))
    return x


def first_iterate_ld(hier, f):
    op = hier.ops[0]
    b = np.where(op.free, np.asarray(f).astype(LD), LD(0))
    z = _vcycle_ld(hier, b)
    return (np.sum(b * z) / np.sum(z * op.apply_free(z))) * z


FIRST_RTOL, FIRST_RELRES = 0.97, 0.95
FIRST_ITERATE = ["5x5", "13x9", "24x24", "9x5x7", "8x8x8"]


def first_iterate_rhs(op):
    """name → f: load 0, and unit impulses next to the pinned node, at the last node of all axes and at the last node of every axis (the wrap)"""
    out = {"load0": op.load(0)}
    for name, j in [("next", (1,) + (0,) * (op.N - 1)), ("last", tuple(m - 1 for m in op.m))] + [
            (f"last{d}", tuple(op.m[e] - 1 if e == d else 0 for e in range(op.N))) for d in range(op.N)]:
        f = np.zeros(op.m)
        f[j] = 1.0
        out[name] = f
    return out


def first_iterate_runs(hier):
    """[(name, f, x₁ of the restatement in float64, its relative residual)] for the right-hand sides whose relative residual after the
    restatement's first iteration is ≤ FIRST_RELRES (a solve at FIRST_RTOL then stops after exactly one iteration), and the names left out"""
    runs, left_out = [], []
    for name, f in first_iterate_rhs(hier.ops[0]).items():
        x, it, rel, ok = pcg(hier, f, None, FIRST_RTOL, 1, "mg")
        (runs if it == 1 and rel <= FIRST_RELRES else left_out).append((name, f, x, rel))
    return runs, left_out
