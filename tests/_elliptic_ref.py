"""elliptic_solve restated in numpy and scipy.sparse (csrc/lsm_elliptic.hip, include/lsm.h "elliptic_solve").

The problem: −∇·(a∇u) + c·u = f on the box of a dense 2-D or 3-D grid, unknowns at the nodes, natural (zero-flux) faces, a set of
fixed (Dirichlet) nodes.  Arrays are n-shaped (cells: n−1), axis 0 fastest (Fortran order).  Every function that the device is
compared with bit for bit (cell_coefficients, Operator.apply, Operator.energy) spells its operation order out; the assembled
matrix, the V-cycle and PCG are compared to rounding / by iteration counts; the first PCG iterate, which shows one V-cycle at
every node, to the rounding of a long-double restatement (first_iterate_ld).

  cell      ϕ̄ = (Σ corners, ascending linear index)·2^−N;  θ = min(max(½ − (ϕ̄ − level)/min(h), 0), 1);  a = a_out + (a_in − a_out)·θ
  edge      along d between I and I+e_d: S = Σ a over the existing cells that share it, ascending linear index; k = S·2^−(N−1);
            k̄ = S/(number of those cells); w = k·ih2_d, ih2_d = 1/(h_d·h_d)
  mass      m_I = Π_d (½ on a face of axis d, else 1)
  operator  (A u)_I = Σ_d [ w_−·(u_I − u_{I−e_d}) + w_+·(u_I − u_{I+e_d}) ] + (c_I·m_I)·u_I, accumulated from +0 in this order
            (d ascending, minus side before plus side, sides that do not exist skipped, the c term last)
  diagonal  D_I = Σ_d [ w_− + w_+ ] + c_I·m_I, same order
  energy    e_I = Σ_d ( Σ_± k̄·(g·g), g = (u_J − u_I)/h_d ) / (number of existing edges along d at I)
"""
import itertools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

OMEGA, NPRE, NPOST, NCOARSE = 0.8, 2, 2, 16


def _offsets(naxes):
    """{0,1}^naxes in ascending linear order (the first axis fastest)"""
    return [tuple(reversed(t)) for t in itertools.product((0, 1), repeat=naxes)]


def cell_coefficients(phi, h, level=0.0, a_in=1.0, a_out=1e-3):
    phi = np.asarray(phi, dtype=np.float64)
    N = phi.ndim
    s = None
    for off in _offsets(N):
        v = phi[tuple(slice(o, n - 1 + o) for o, n in zip(off, phi.shape))]
        s = v.copy() if s is None else s + v
    mean = s * 2.0 ** -N
    theta = np.minimum(np.maximum(0.5 - (mean - level) / min(h), 0.0), 1.0)
    return np.asfortranarray(a_out + (a_in - a_out) * theta)


def coarsen_shape(n):
    """(coarse shape, the axes that coarsen) or None when no axis does"""
    co = tuple(nd > 5 for nd in n)
    if not any(co):
        return None
    return tuple((nd + 1) // 2 if c else nd for nd, c in zip(n, co)), co


def coarsen_cells(a, co):
    """a coarse cell: the arithmetic mean of the fine cells {2J, 2J+1} per coarsened axis, summed in ascending linear index"""
    nc = tuple(((m + 2) // 2 - 1) if c else m for m, c in zip(a.shape, co))     # fine cells m = n − 1; coarse cells (n+1)//2 − 1
    axes = [d for d, c in enumerate(co) if c]
    s = None
    for off in _offsets(len(axes)):
        sl = [slice(0, m) for m in nc]
        for d, o in zip(axes, off):
            sl[d] = slice(o, o + 2 * nc[d] - 1, 2)
        v = a[tuple(sl)]
        s = v.copy() if s is None else s + v
    return np.asfortranarray(s * 2.0 ** -len(axes))


def _inject(x, co):
    return np.asfortranarray(x[tuple(slice(None, None, 2) if c else slice(None) for c in co)])


class Operator:
    """one level: the cell array `a` (shape n−1), c (scalar or n-shaped), the mesh sizes h, the fixed mask (bool, n-shaped) or None"""

    def __init__(self, a, h, c=0.0, fixed=None):
        self.a = np.asfortranarray(a, dtype=np.float64)
        self.N = self.a.ndim
        self.n = tuple(m + 1 for m in self.a.shape)
        self.h = tuple(float(x) for x in h)
        self.ih2 = tuple(1.0 / (x * x) for x in self.h)
        self.c = np.broadcast_to(np.asarray(c, dtype=np.float64), self.n)
        self.fixed = np.zeros(self.n, dtype=bool) if fixed is None else np.asarray(fixed, dtype=bool)
        self.free = ~self.fixed
        N = self.N
        self.k, self.kbar, self.w = [], [], []
        ones = np.ones_like(self.a)
        for d in range(N):
            pad = [(0, 0) if e == d else (1, 1) for e in range(N)]
            ap, op = np.pad(self.a, pad), np.pad(ones, pad)
            others = [e for e in range(N) if e != d]
            S = cnt = None
            for off in _offsets(N - 1):
                sl = [slice(None)] * N
                for e, o in zip(others, off):
                    sl[e] = slice(o, o + self.n[e])
                v, q = ap[tuple(sl)], op[tuple(sl)]
                S, cnt = (v.copy(), q.copy()) if S is None else (S + v, cnt + q)
            k = S * 2.0 ** -(N - 1)
            self.k.append(k)
            self.kbar.append(S / cnt)
            self.w.append(k * self.ih2[d])
        m = np.ones(self.n)
        for d in range(N):
            f = np.ones(self.n[d])
            f[0] = f[-1] = 0.5
            m = m * f.reshape([-1 if e == d else 1 for e in range(N)])
        self.m = m
        self.cm = self.c * self.m
        D = np.zeros(self.n)
        for d in range(N):
            lo, hi = self._sl(d, 1, None), self._sl(d, None, -1)
            D[lo] = D[lo] + self.w[d]
            D[hi] = D[hi] + self.w[d]
        self.D = D + self.cm
        self._A = None

    def _sl(self, d, a, b):
        return tuple(slice(a, b) if e == d else slice(None) for e in range(self.N))

    def apply(self, u):
        """A u on all nodes, no elimination: the operation order of the module docstring"""
        u = np.asarray(u, dtype=np.float64)
        acc = np.zeros(self.n)
        for d in range(self.N):
            lo, hi = self._sl(d, 1, None), self._sl(d, None, -1)
            acc[lo] = acc[lo] + self.w[d] * (u[lo] - u[hi])
            acc[hi] = acc[hi] + self.w[d] * (u[hi] - u[lo])
        return acc + self.cm * u

    def energy(self, u):
        u = np.asarray(u, dtype=np.float64)
        e = np.zeros(self.n)
        for d in range(self.N):
            lo, hi = self._sl(d, 1, None), self._sl(d, None, -1)
            s, cnt = np.zeros(self.n), np.zeros(self.n)
            g = (u[hi] - u[lo]) / self.h[d]
            s[lo] = s[lo] + self.kbar[d] * (g * g)
            cnt[lo] += 1
            g = (u[lo] - u[hi]) / self.h[d]
            s[hi] = s[hi] + self.kbar[d] * (g * g)
            cnt[hi] += 1
            e = e + s / cnt
        return e

    def matrix(self):
        """the assembled A (csr), node index axis 0 fastest"""
        if self._A is None:
            nn = int(np.prod(self.n))
            idx = np.arange(nn).reshape(self.n, order="F")
            A = sp.diags(self.cm.reshape(-1, order="F")).tocsr()
            for d in range(self.N):
                i = idx[self._sl(d, None, -1)].reshape(-1, order="F")
                j = idx[self._sl(d, 1, None)].reshape(-1, order="F")
                w = self.w[d].reshape(-1, order="F")
                ne = i.size
                G = sp.csr_matrix((np.concatenate([np.ones(ne), -np.ones(ne)]), (np.tile(np.arange(ne), 2), np.concatenate([i, j]))), shape=(ne, nn))
                A = A + G.T @ sp.diags(w) @ G
            self._A = A.tocsr()
        return self._A

    def apply_free(self, x):
        """the eliminated operator: x is zero on the fixed nodes, and so is the result"""
        return np.where(self.free, self.apply(np.where(self.free, x, 0.0)), 0.0)


def _p1(n):
    """1-D prolongation, n fine nodes from (n+1)//2 coarse ones: fine 2J ← J; fine 2J+1 ← ½(J, J+1), or J alone at the end"""
    nc = (n + 1) // 2
    P = sp.lil_matrix((n, nc))
    for i in range(n):
        J = i // 2
        if i % 2 == 0:
            P[i, J] = 1.0
        elif J + 1 < nc:
            P[i, J] = P[i, J + 1] = 0.5
        else:
            P[i, J] = 1.0
    return P.tocsr()


def prolongation(n, co):
    P = None
    for d in range(len(n)):
        Pd = _p1(n[d]) if co[d] else sp.identity(n[d], format="csr")
        P = Pd if P is None else sp.kron(Pd, P, format="csr")      # axis 0 fastest
    return P


class Hierarchy:
    """level 0 and its coarsenings: axis d coarsens while n_d > 5 to (n_d+1)//2 nodes (coarse J on fine 2J, h_d doubles); the same
    discretisation on every level with averaged cells, injected c and injected fixed mask"""

    def __init__(self, op):
        self.ops, self.P = [op], []
        while True:
            f = self.ops[-1]
            cs = coarsen_shape(f.n)
            if cs is None:
                break
            nc, co = cs
            h = tuple(x * 2.0 if c else x for x, c in zip(f.h, co))
            self.ops.append(Operator(coarsen_cells(f.a, co), h, _inject(f.c, co), _inject(f.fixed, co)))
            self.P.append((prolongation(f.n, co), 2.0 ** -sum(co)))

    @property
    def levels(self):
        return len(self.ops)

    def _smooth(self, op, x, r, sweeps):
        """damped Jacobi; x None: from zero, the first sweep is ω D⁻¹ r without an apply"""
        for _ in range(sweeps):
            if x is None:
                x = np.where(op.free, OMEGA * r / op.D, 0.0)
            else:
                x = np.where(op.free, x + OMEGA * (r - op.apply_free(x)) / op.D, 0.0)
        return x

    def vcycle(self, r, lev=0):
        """one V-cycle from zero for A x = r on the free nodes of level `lev` (r is zero on its fixed nodes)"""
        op = self.ops[lev]
        r = np.where(op.free, r, 0.0)
        if lev == self.levels - 1:
            return self._smooth(op, None, r, NCOARSE)
        x = self._smooth(op, None, r, NPRE)
        P, scale = self.P[lev]
        cop = self.ops[lev + 1]
        res = np.where(op.free, r - op.apply_free(x), 0.0)
        rc = (P.T @ res.reshape(-1, order="F") * scale).reshape(cop.n, order="F")
        xc = self.vcycle(np.where(cop.free, rc, 0.0), lev + 1)
        x = np.where(op.free, x + (P @ xc.reshape(-1, order="F")).reshape(op.n, order="F"), 0.0)
        return self._smooth(op, x, r, NPOST)


def rhs(op, f):
    return op.m * np.broadcast_to(np.asarray(f, dtype=np.float64), op.n)


def pcg(hier, f, u0, rtol=1e-8, max_iters=500, precond="mg"):
    """PCG on the free nodes from u0 (the fixed nodes of u0 hold g) until the recursive ‖r‖₂ ≤ rtol·‖b_free‖₂ (‖r₀‖₂ when b_free
    is zero).  Returns (u, iterations, relres, converged)."""
    op = hier.ops[0]
    M = (lambda r: hier.vcycle(r)) if precond == "mg" else (lambda r: np.where(op.free, r / op.D, 0.0))
    b = rhs(op, f)
    u = np.array(u0, dtype=np.float64, order="F")
    r = np.where(op.free, b - op.apply(u), 0.0)
    bb = float(np.sum(np.where(op.free, b, 0.0) ** 2))
    rr = float(np.sum(r * r))
    if bb == 0.0:
        bb = rr
    if rr <= rtol * rtol * bb:
        return u, 0, (np.sqrt(rr / bb) if bb > 0 else 0.0), True
    z = M(r)
    rho = float(np.sum(r * z))
    p = z
    for it in range(1, max_iters + 1):
        q = op.apply_free(p)
        alpha = rho / float(np.sum(p * q))
        u = u + alpha * p
        r = r - alpha * q
        rr = float(np.sum(r * r))
        if rr <= rtol * rtol * bb:
            return u, it, np.sqrt(rr / bb), True
        z = M(r)
        rho1 = float(np.sum(r * z))
        p = z + (rho1 / rho) * p
        rho = rho1
    return u, max_iters, np.sqrt(rr / bb), False


def direct(op, f, u0):
    """the solution by a sparse direct solve on the free nodes (the fixed nodes keep u0's values)"""
    A = op.matrix()
    free = op.free.reshape(-1, order="F")
    u = np.array(u0, dtype=np.float64, order="F").reshape(-1, order="F")
    u[free] = 0.0
    b = rhs(op, f).reshape(-1, order="F") - A @ u
    if free.any():
        u[free] = spla.spsolve(A[free][:, free].tocsc(), b[free])
    return u.reshape(op.n, order="F")


def true_residual(op, f, u):
    """‖(b − A u)_free‖₂ and ‖b_free‖₂"""
    b = rhs(op, f)
    r = np.where(op.free, b - op.apply(u), 0.0)
    return float(np.sqrt(np.sum(r * r))), float(np.sqrt(np.sum(np.where(op.free, b, 0.0) ** 2)))


def compliance(op, f, u):
    return float(np.prod(op.h)) * float(np.sum(rhs(op, f) * u))


# ---- the cases shared by tests/test_elliptic_host.py (the mg < jacobi condition, on the CPU) and tests/test_gpu_elliptic.py

def face_mask(n, d, side):
    m = np.zeros(n, dtype=bool)
    m[tuple(slice(None) if e != d else (0 if side == 0 else -1) for e in range(len(n)))] = True
    return m


def two_holes(n, h, shift=0.0):
    """a signed distance to a plate with two circular (spherical) holes: negative in the material"""
    x = np.meshgrid(*[np.arange(nd) * hd for nd, hd in zip(n, h)], indexing="ij", sparse=True)
    L = [(nd - 1) * hd for nd, hd in zip(n, h)]
    N = len(n)
    c1 = [0.3 * L[0] + shift, 0.35 * L[1]] + ([0.5 * L[2]] if N == 3 else [])
    c2 = [0.7 * L[0] + shift, 0.65 * L[1]] + ([0.4 * L[2]] if N == 3 else [])
    R = 0.17 * min(L)
    d1 = np.sqrt(sum((xi - ci) ** 2 for xi, ci in zip(x, c1))) - R
    d2 = np.sqrt(sum((xi - ci) ** 2 for xi, ci in zip(x, c2))) - R
    return np.asfortranarray(-np.minimum(d1, d2) + np.zeros(n))


def _patch(n, d, lo, hi):
    """a patch on the upper face of axis d: the middle third of the other axes"""
    m = face_mask(n, d, 1)
    for e in range(len(n)):
        if e != d:
            keep = np.zeros(n[e], dtype=bool)
            keep[int(lo * n[e]):max(int(hi * n[e]), int(lo * n[e]) + 1)] = True
            m &= keep.reshape([-1 if q == e else 1 for q in range(len(n))])
    return m


def cases():
    """name → dict(n, hc, h, phi | a, a_in, a_out, c, fixed, g, f, dtype): every shape and variant tests/test_gpu_elliptic.py runs"""
    rng = np.random.default_rng(7)
    out = {}

    def add(name, n, hc=None, contrast=1e-3, c=0.0, fixed=None, g=0.0, f=1.0, a=None, shift=0.0, dtype=np.float64):
        hc = tuple((nd - 1.0) / (max(n) - 1.0) for nd in n) if hc is None else hc      # the box is [0, hc]; h as CartesianGrid.meshsize
        h = tuple((x - 0.0) / (nd - 1) for x, nd in zip(hc, n))
        out[name] = dict(n=n, hc=hc, h=h, phi=two_holes(n, h, shift), a=a, a_in=1.0, a_out=contrast, c=c, fixed=fixed, g=g, f=f, dtype=dtype)

    n = (33, 33)
    add("33x33_face", n, fixed=face_mask(n, 0, 0))
    add("33x33_contrast1", n, contrast=1.0, fixed=face_mask(n, 0, 0), g=0.25)
    n = (64, 48)
    add("64x48_upper_patch", n, fixed=_patch(n, 0, 1 / 3, 2 / 3), shift=0.25)       # the interface runs through the boundary
    blob = np.zeros(n, dtype=bool)
    blob[20:25, 30:34] = True
    add("64x48_blob", n, fixed=blob, g=1.0, f=1.0, c=0.5)
    n = (65, 20)
    add("65x20_aniso_h", n, hc=(1.0, 0.6), fixed=face_mask(n, 1, 0))
    add("65x20_no_fixed", n, c=2.0, f=rng.standard_normal(n))
    n = (17, 17, 17)
    add("17c_face", n, fixed=face_mask(n, 2, 0))
    add("17c_f32", n, fixed=face_mask(n, 0, 1), g=0.5, dtype=np.float32)
    n = (24, 33, 10)
    add("24x33x10_patch", n, fixed=_patch(n, 0, 1 / 3, 2 / 3) | face_mask(n, 1, 0))
    add("24x33x10_aniso_given_a", n, hc=(1.0, 0.8, 0.7), c=1.0, a=np.asfortranarray(0.5 + rng.random(tuple(m - 1 for m in n))),
        f=rng.standard_normal(n))
    return out


def build_case(cs):
    """(Hierarchy, f, u0) of a case; an f32 case's ϕ and u0 are rounded to float32 first, as the handle stores them"""
    n, h = cs["n"], cs["h"]
    phi = cs["phi"].astype(cs["dtype"]).astype(np.float64)
    a = cs["a"] if cs["a"] is not None else cell_coefficients(phi, h, cs.get("level", 0.0), cs["a_in"], cs["a_out"])
    hier = Hierarchy(Operator(a, h, cs["c"], cs["fixed"]))
    u0 = np.zeros(n, order="F") if cs.get("u0") is None else np.array(cs["u0"], dtype=np.float64, order="F")
    if cs["fixed"] is not None:
        u0[cs["fixed"]] = cs["g"]
    u0 = u0.astype(cs["dtype"]).astype(np.float64)
    f = np.asfortranarray(np.broadcast_to(np.asarray(cs["f"], dtype=np.float64), n))
    return hier, f, u0


_SOLVED = {}


def solved(name):
    """the restatement's results for a case, computed once: hier, f, u0, the direct solve, and per preconditioner
    (u, iterations, relres, converged) at rtol 1e-8; an f32 case's u is rounded to float32 as the handle stores it (the fixed nodes
    hold float32 values already)"""
    if name not in _SOLVED:
        cs = cases()[name]
        hier, f, u0 = build_case(cs)
        res = dict(case=cs, hier=hier, f=f, u0=u0, direct=direct(hier.ops[0], f, u0))
        for pc in ("mg", "jacobi"):
            u, it, rel, ok = pcg(hier, f, u0, 1e-8, 2000, pc)
            res[pc] = (u.astype(cs["dtype"]).astype(np.float64), it, rel, ok)
        _SOLVED[name] = res
    return _SOLVED[name]


# ---- the first PCG iterate in long double: with u0 = 0 and zero Dirichlet values r₀ = b, so u₁ = α·M b, α = (b·Mb)/(Mb·A Mb) —
# a solve that stops after one iteration shows M b at every node (tests/test_gpu_elliptic_edges.py).  scipy.sparse has no long
# double: the operator is applied in the stated order from the float64 coefficients, P and Pᵀ axis by axis from _p1.

LD = np.longdouble


def _apply_free_ld(op, x):
    acc = np.zeros(op.n, dtype=LD)
    for d in range(op.N):
        lo, hi = op._sl(d, 1, None), op._sl(d, None, -1)
        w = op.w[d].astype(LD)
        acc[lo] = acc[lo] + w * (x[lo] - x[hi])
        acc[hi] = acc[hi] + w * (x[hi] - x[lo])
    return np.where(op.free, acc + op.cm.astype(LD) * x, LD(0))


def _transfer_ld(x, nf, co, transpose):
    """P x (coarse → fine, the fine shape nf) or Pᵀ x, one axis at a time"""
    for d in range(len(nf)):
        if co[d]:
            P = _p1(nf[d]).toarray().astype(LD)
            x = np.moveaxis(np.tensordot(P.T if transpose else P, x, axes=(1, d)), 0, d)
    return x


def _vcycle_ld(hier, r, lev=0):
    op = hier.ops[lev]
    D, om = op.D.astype(LD), LD(OMEGA)
    coarsest = lev == hier.levels - 1
    x = np.where(op.free, om * r / D, LD(0))
    for _ in range((NCOARSE if coarsest else NPRE) - 1):
        x = np.where(op.free, x + om * (r - _apply_free_ld(op, x)) / D, LD(0))
    if coarsest:
        return x
    cop = hier.ops[lev + 1]
    co = tuple(a != b for a, b in zip(op.n, cop.n))
    res = np.where(op.free, r - _apply_free_ld(op, x), LD(0))
    rc = np.where(cop.free, _transfer_ld(res, op.n, co, True) * LD(hier.P[lev][1]), LD(0))
    x = np.where(op.free, x + _transfer_ld(_vcycle_ld(hier, rc, lev + 1), op.n, co, False), LD(0))
    for _ in range(NPOST):
        x = np.where(op.free, x + om * (r - _apply_free_ld(op, x)) / D, LD(0))
    return x


def first_iterate_ld(hier, f, precond="mg"):
    """u₁ of PCG from u0 = 0 with zero Dirichlet values, every operation in np.longdouble (the coefficients are the float64 ones)"""
    op = hier.ops[0]
    b = np.where(op.free, rhs(op, f).astype(LD), LD(0))
    z = _vcycle_ld(hier, b) if precond == "mg" else np.where(op.free, b / op.D.astype(LD), LD(0))
    return (np.sum(b * z) / np.sum(z * _apply_free_ld(op, z))) * z


def first_iterate_rhs(op):
    """name → f: a standard normal field and the impulses f = e_j/m_j (so b = e_j: u₁ is a multiple of column j of M) at the upper
    corner n − 1 (the unpaired last node of every even axis), at n − 2 and at the odd interior node (n//2)|1; a fixed j is left out"""
    out = {"normal": np.asfortranarray(np.random.default_rng(13).standard_normal(op.n))}
    for name, j in (("corner", tuple(m - 1 for m in op.n)), ("corner-1", tuple(m - 2 for m in op.n)), ("odd", tuple((m // 2) | 1 for m in op.n))):
        if op.free[j]:
            f = np.zeros(op.n, order="F")
            f[j] = 1.0 / op.m[j]
            out[name] = f
    return out


# ---- the cases of tests/test_gpu_elliptic_edges.py: what tests/test_gpu_elliptic.py's ten shapes leave out

_EDGE_CASES = {}


def edge_cases():
    """name → the dict of cases() with the optional keys u0 (the guess, n-shaped; the fixed nodes take g), level, max_iters,
    solve ("both" | "mg"), direct (False: no sparse direct solve — 3-D fill — and the restatement's distance to its own solve at
    rtol/100 in its place), big (the two shapes beyond MG_MAXB workgroups: one mg solve, no comparison of u), devfield (c and f are
    given as device fields)"""
    if _EDGE_CASES:
        return _EDGE_CASES
    rng = np.random.default_rng(19)
    base = cases()
    out = _EDGE_CASES

    def add(name, n, hc=None, contrast=1e-3, c=0.0, fixed=None, g=0.0, f=1.0, dtype=np.float64, a_in=1.0, **extra):
        hc = tuple((nd - 1.0) / (max(n) - 1.0) for nd in n) if hc is None else hc
        h = tuple(x / (nd - 1) for x, nd in zip(hc, n))
        out[name] = dict(n=n, hc=hc, h=h, phi=two_holes(n, h), a=None, a_in=a_in, a_out=contrast, c=c, fixed=fixed, g=g, f=f, dtype=dtype, **extra)

    def free_guess(n, fixed):
        u0 = np.asfortranarray(rng.standard_normal(n))
        if fixed is not None:
            u0[fixed] = 0.0
        return u0

    # node-wise c, on every level
    n = (24, 33, 10)
    fixed = _patch(n, 0, 1 / 3, 2 / 3)
    add("24x33x10_cn", n, c=np.asfortranarray(rng.random(n)), f=rng.standard_normal(n), fixed=fixed, u0=free_guess(n, fixed))
    n = (6, 6, 6)
    add("6x6x6_cn_sparse", n, c=np.asfortranarray(rng.random(n) * (rng.random(n) > 0.5)), f=rng.standard_normal(n))
    n = (64, 48)
    blob = np.zeros(n, dtype=bool)
    blob[20:25, 30:34] = True
    c, f = np.asfortranarray(rng.random(n)), np.asfortranarray(rng.standard_normal(n))
    add("64x48_cn_devicefield", n, c=c, f=f, fixed=blob, g=1.0, devfield=True)
    add("64x48_cn_devicefield_f32", n, c=c.astype(np.float32).astype(np.float64), f=f.astype(np.float32).astype(np.float64), fixed=blob, g=1.0,
        dtype=np.float32, devfield=True)
    # one-level and minimal hierarchies (a device handle needs at least 4 nodes per dimension: 4x4 is the smallest grid there is)
    add("5x5_face", (5, 5), fixed=face_mask((5, 5), 0, 0))
    add("4x4_c", (4, 4), c=1.0, f=rng.standard_normal((4, 4)))
    add("5x5x5_laplace", (5, 5, 5), fixed=face_mask((5, 5, 5), 2, 1), g=1.0, f=0.0)
    add("4x5x4_cn", (4, 5, 4), c=np.asfortranarray(rng.random((4, 5, 4))), f=rng.standard_normal((4, 5, 4)))
    add("6x5_face", (6, 5), fixed=face_mask((6, 5), 0, 0))
    add("4x40_face", (4, 40), fixed=face_mask((4, 40), 1, 0))
    add("4x40_side", (4, 40), fixed=face_mask((4, 40), 0, 0))       # the first-iterate test's 4x40: the V-cycle is good enough on it
    # launch shapes: more than 256 workgroups (the reduction's second pass strides), more than MG_MAXB (a second grid-stride trip)
    add("300x230", (300, 230), fixed=face_mask((300, 230), 0, 0), max_iters=3000)
    add("45x41x37", (45, 41, 37), fixed=face_mask((45, 41, 37), 2, 0), direct=False)
    add("1000x530", (1000, 530), fixed=face_mask((1000, 530), 0, 0), big=True, solve="mg", direct=False)
    add("83x81x79", (83, 81, 79), fixed=face_mask((83, 81, 79), 2, 0), big=True, solve="mg", direct=False)
    # a guess that is not zero on the free nodes
    for name in ("33x33_face", "65x20_aniso_h", "17c_face", "17c_f32"):
        out[name + "_guess"] = dict(base[name], u0=free_guess(base[name]["n"], base[name]["fixed"]))
    # a level other than zero, and the stiff material outside
    n = (64, 48)
    add("64x48_level", n, fixed=face_mask(n, 0, 0), level=0.03, solve="mg")
    add("64x48_level_neg", n, fixed=face_mask(n, 0, 0), level=-0.02, a_in=1e-3, contrast=1.0, solve="mg")
    # a float32 handle in 2-D
    out["33x33_f32_2d"] = dict(base["33x33_face"], g=0.25, dtype=np.float32)
    return out


_EDGE = {}


def edge_case_names(big=None):
    """the names of the big cases (big=True), of the others (False) or of all"""
    return sorted(k for k, v in edge_cases().items() if big is None or bool(v.get("big")) == big)


def edge_solved(name):
    """solved() for an edge case: direct is None where the case has no direct solve, and then `tight` holds
    |u(rtol) − u(rtol/100)|∞ of the restatement per preconditioner (not for a big case); a preconditioner the case does not run is None"""
    if name not in _EDGE:
        cs = edge_cases()[name]
        hier, f, u0 = build_case(cs)
        want_direct = cs.get("direct", True)
        res = dict(case=cs, hier=hier, f=f, u0=u0, direct=direct(hier.ops[0], f, u0) if want_direct else None, tight={})
        mi = cs.get("max_iters", 2000)
        for pc in ("mg", "jacobi"):
            if pc == "jacobi" and cs.get("solve", "both") == "mg":
                res[pc] = None
                continue
            u, it, rel, ok = pcg(hier, f, u0, 1e-8, mi, pc)
            if not want_direct and not cs.get("big"):
                res["tight"][pc] = float(np.abs(u - pcg(hier, f, u0, 1e-10, mi, pc)[0]).max())
            res[pc] = (u.astype(cs["dtype"]).astype(np.float64), it, rel, ok)
        _EDGE[name] = res
    return _EDGE[name]


def any_solved(name):
    return solved(name) if name in cases() else edge_solved(name)


# the first-iterate test's shapes: the float64 cases of cases(), the smallest multi-level hierarchies (4x40_side stands for
# 4x40_face, whose V-cycle leaves 1.32 of the residual after one iteration for one impulse: tests/test_elliptic_host.py), c per
# node on four levels, and the one-level shapes, where M is the coarsest kernel alone; Jacobi, where u₁ = α·D⁻¹b, on two of them as
# the trivial control
FIRST_ITERATE = (sorted(k for k, v in cases().items() if v["dtype"] == np.float64)
                 + ["6x5_face", "4x40_side", "6x6x6_cn_sparse", "24x33x10_cn", "4x5x4_cn", "5x5x5_laplace", "5x5_face"])
FIRST_ITERATE_JACOBI = ["64x48_upper_patch", "6x6x6_cn_sparse"]
FIRST_ITERATE_PAIRS = [(k, "mg") for k in FIRST_ITERATE] + [(k, "jacobi") for k in FIRST_ITERATE_JACOBI]
