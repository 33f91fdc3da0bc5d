"""elasticity_solve restated in numpy and scipy.sparse (csrc/lsm_elastic.hip, include/lsm.h "elasticity_solve").

The problem: −∇·σ(u) = f on the box of a dense 2-D or 3-D grid, σ = E(x)·C₀(ν):ε(u), Q1 elements, the N displacement components
at the nodes, traction-free faces, a set of fixed displacement components (one byte per node, bit i = component i).  Vectors are
(N,)+n-shaped: component-major, nodes with axis 0 fastest.  The functions that the device is compared with bit for bit
(k0 to a few ulps; Operator.apply, Operator.energy, the cell array of _elliptic_ref.cell_coefficients) spell their operation
order out; the assembled matrix, the V-cycle and PCG are compared to rounding / by iteration counts and run on the assembled
matrix, which is what makes the cases quick.

  material  at E = 1: μ = 1/(2(1+ν)); λ = ν/((1+ν)(1−2ν)) in 3-D and for plane strain, λ = ν/(1−ν²) for plane stress
  K0        K0[(a,i),(b,j)] = (λ·G[a,b,i,j] + μ·G[a,b,j,i] + δᵢⱼ·μ·Σ_k G[a,b,k,k])/∏h,  G[a,b,i,j] = ∫_cell ∂ᵢN_a ∂ⱼN_b, a product
            over the axes of the 1-D factors mass (h/3, h/6), stiffness (±1/h) and mixed (±½: the sign of the differentiated corner);
            corner a has bit d set on the cell's upper side along d; row a·N + i
  operator  (A u)_{I,i} = Σ_C E_C·(Σ_b Σ_j K0[(a,i),(b,j)]·u_{b,j}): the cells C around I in ascending order (bit d of m set: cell
            index I_d, clear: I_d − 1), a = I's corner in C; the inner sum from +0, b ascending, j fastest; then ·E_C; the cell terms
            summed from +0.  A cell that does not exist has E = 0 and its missing nodes u = 0: it adds +0 or −0 to a sum that
            started from +0, which changes no bit.
  diagonal  D_{I,i} = Σ_C E_C·K0[(a,i),(a,i)]
  energy    e_I = (Σ_C E_C·q_C)/(number of existing cells around I), q_C = Σ_r u_r·(Σ_s K0[r,s]·u_s), both from +0 ascending
  rhs       b_{I,i} = m_I·f_{I,i}, m_I = ∏_d (½ on a face of axis d, else 1)
"""
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from _elliptic_ref import LD, _patch, _transfer_ld, cell_coefficients, coarsen_cells, coarsen_shape, face_mask, prolongation, two_holes

OMEGA, SAFE, NPRE, NPOST, NCOARSE = 0.6, 1.9, 2, 2, 16


def symbol_lambda(K, N):
    """λmax(D⁻¹A) on a uniform infinite grid from K0: the largest eigenvalue over the corner frequencies θ ∈ {0, π}^N of the symbol"""
    NC = 1 << N
    D = np.array([sum(K[a * N + i, a * N + i] for a in range(NC)) for i in range(N)])
    best = 0.0
    for th in range(NC):
        A = np.zeros((N, N))
        for a in range(NC):
            for b in range(NC):
                sg = -1.0 if bin((a ^ b) & th).count("1") & 1 else 1.0
                A += sg * K[a * N:(a + 1) * N, b * N:(b + 1) * N]
        best = max(best, float(np.linalg.eigvalsh(A / np.sqrt(np.outer(D, D))).max()))
    return best


def level_omega(K, N, omega=OMEGA):
    """the level's damping: ω, or SAFE/λ where ω·λ would pass SAFE (stretched cells: an axis that stopped coarsening)"""
    return min(omega, SAFE / symbol_lambda(K, N))


def symbol_lambda_power(K, N):
    """es_symbol_lambda (csrc/lsm_elastic.hip) operation for operation, in Python floats: D_i summed over the corners ascending from
    +0; per corner frequency the symbol A_ij accumulated from +0 over a, b ascending as (sg·K)/√(D_i·D_j); 500 power steps from
    (1, 0.9, 0.8), y_i from +0 with j ascending, ‖y‖² from +0 with i ascending, λ = ‖y‖.  Only +, ·, / and sqrt: on the device's own
    K0 it gives the value the host code computes, bit for bit."""
    NC = 1 << N
    K = [[float(v) for v in row] for row in np.asarray(K, dtype=np.float64)]
    D = [0.0] * N
    for i in range(N):
        for a in range(NC):
            D[i] = D[i] + K[a * N + i][a * N + i]
    best = 0.0
    for th in range(NC):
        A = [[0.0] * N for _ in range(N)]
        for a in range(NC):
            for b in range(NC):
                sg = -1.0 if bin((a ^ b) & th).count("1") & 1 else 1.0
                for i in range(N):
                    for j in range(N):
                        A[i][j] = A[i][j] + sg * K[a * N + i][b * N + j] / math.sqrt(D[i] * D[j])
        x, lam = [1.0, 0.9, 0.8][:N], 0.0
        for _ in range(500):
            y, nrm = [0.0] * N, 0.0
            for i in range(N):
                for j in range(N):
                    y[i] = y[i] + A[i][j] * x[j]
                nrm = nrm + y[i] * y[i]
            nrm = math.sqrt(nrm)
            if not nrm > 0.0:
                break
            lam = nrm
            for i in range(N):
                x[i] = y[i] / nrm
        best = max(best, lam)
    return best


def device_omegas(k0s, N):
    """the dampings the device uses on its levels: min(ω, SAFE/λ) with λ from the power iteration on each level's K0"""
    return [min(OMEGA, SAFE / symbol_lambda_power(K, N)) for K in k0s]


def material(nu, N, plane="stress"):
    mu = 1.0 / (2.0 * (1.0 + nu))
    if N == 2 and plane == "stress":
        lam = nu / (1.0 - nu * nu)
    else:
        lam = nu / ((1.0 + nu) * (1.0 - 2.0 * nu))
    return lam, mu


def k0(h, nu=0.3, plane="stress"):
    """the unit element matrix of a box cell with sides h, scaled by 1/∏h"""
    N = len(h)
    NC = 1 << N
    lam, mu = material(nu, N, plane)
    vol = 1.0
    for d in range(N):
        vol = vol * h[d]
    G = np.zeros((NC, NC, N, N))
    for a in range(NC):
        for b in range(NC):
            for i in range(N):
                for j in range(N):
                    g = 1.0
                    for d in range(N):
                        ad, bd = (a >> d) & 1, (b >> d) & 1
                        if i == j and d == i:
                            g = g * ((1.0 if ad == bd else -1.0) / h[d])
                        elif i != j and d == i:
                            g = g * (0.5 if ad else -0.5)
                        elif i != j and d == j:
                            g = g * (0.5 if bd else -0.5)
                        else:
                            g = g * (h[d] / 3.0 if ad == bd else h[d] / 6.0)
                    G[a, b, i, j] = g
    K = np.zeros((NC * N, NC * N))
    for a in range(NC):
        for b in range(NC):
            tr = 0.0
            for k in range(N):
                tr = tr + G[a, b, k, k]
            for i in range(N):
                for j in range(N):
                    v = lam * G[a, b, i, j] + mu * G[a, b, j, i]
                    if i == j:
                        v = v + mu * tr
                    K[a * N + i, b * N + j] = v / vol
    return K


def rigid_modes(h):
    """the N translations and N(N−1)/2 linearised rotations at the corners of a cell, as vectors of 2^N·N entries"""
    N = len(h)
    NC = 1 << N
    X = np.array([[((a >> d) & 1) * h[d] for d in range(N)] for a in range(NC)])
    out = []
    for i in range(N):
        v = np.zeros((NC, N))
        v[:, i] = 1.0
        out.append(v.reshape(-1))
    for i in range(N):
        for j in range(i + 1, N):
            v = np.zeros((NC, N))
            v[:, i], v[:, j] = -X[:, j], X[:, i]
            out.append(v.reshape(-1))
    return out


def _bits(m, N):
    return tuple((m >> d) & 1 for d in range(N))


class Operator:
    """one level: the cell moduli E (shape n−1), the mesh sizes h, the level's K0, the fixed bits (uint8, n-shaped) or None"""

    def __init__(self, E, h, K0, fixed=None):
        self.E = np.asfortranarray(E, dtype=np.float64)
        self.a = self.E                     # the name _elliptic_ref.coarsen_cells' callers use
        self.N = N = self.E.ndim
        self.n = tuple(m + 1 for m in self.E.shape)
        self.h = tuple(float(x) for x in h)
        self.K0 = np.array(K0, dtype=np.float64)
        self.bits = np.zeros(self.n, dtype=np.uint8) if fixed is None else np.asarray(fixed, dtype=np.uint8)
        self.fixed = np.stack([(self.bits >> i) & 1 != 0 for i in range(N)])
        self.free = ~self.fixed
        self.Epad = np.pad(self.E, 1)
        self.count = None
        for m in range(1 << N):
            v = np.pad(np.ones_like(self.E), 1)[self._cell(m)]
            self.count = v.copy() if self.count is None else self.count + v
        mass = np.ones(self.n)
        for d in range(N):
            f = np.ones(self.n[d])
            f[0] = f[-1] = 0.5
            mass = mass * f.reshape([-1 if e == d else 1 for e in range(N)])
        self.m = mass
        D = np.zeros((N,) + self.n)
        for m in range(1 << N):
            a = (~m) & ((1 << N) - 1)
            Ec = self.Epad[self._cell(m)]
            for i in range(N):
                D[i] = D[i] + Ec * self.K0[a * N + i, a * N + i]
        self.D = D
        self._A = None

    def _cell(self, m):
        """the slices of a 1-padded cell array that give cell m of every node"""
        return tuple(slice(b, b + nd) for b, nd in zip(_bits(m, self.N), self.n))

    def _node(self, m, b):
        """the slices of a 1-padded node array that give corner b of cell m of every node"""
        return tuple(slice(x + y, x + y + nd) for x, y, nd in zip(_bits(m, self.N), _bits(b, self.N), self.n))

    def apply(self, u):
        """A u on all components, no elimination: the operation order of the module docstring"""
        N, NC = self.N, 1 << self.N
        u = np.asarray(u)
        dt = LD if u.dtype == LD else np.float64           # a long-double u runs the same loops in long double (first_iterate_ld)
        u = u.astype(dt, copy=False)
        up = [np.pad(u[j], 1) for j in range(N)]
        acc = np.zeros((N,) + self.n, dtype=dt)
        for m in range(NC):
            a = (~m) & (NC - 1)
            Ec = self.Epad[self._cell(m)]
            inner = np.zeros((N,) + self.n, dtype=dt)
            for b in range(NC):
                sl = self._node(m, b)
                for j in range(N):
                    v = up[j][sl]
                    for i in range(N):
                        inner[i] = inner[i] + self.K0[a * N + i, b * N + j] * v
            for i in range(N):
                acc[i] = acc[i] + Ec * inner[i]
        return acc

    def energy(self, u):
        N, NC = self.N, 1 << self.N
        u = np.asarray(u, dtype=np.float64)
        cn = tuple(m - 1 for m in self.n)
        uc = [u[r % N][tuple(slice(o, o + c) for o, c in zip(_bits(r // N, N), cn))] for r in range(NC * N)]      # the cells' corner values
        q = np.zeros(cn)
        for r in range(NC * N):
            t = np.zeros(cn)
            for s in range(NC * N):
                t = t + self.K0[r, s] * uc[s]
            q = q + uc[r] * t
        w = np.pad(self.E * q, 1)
        acc = np.zeros(self.n)
        for m in range(NC):
            acc = acc + w[self._cell(m)]
        return acc / self.count

    def matrix(self):
        """the assembled A (csr) over component-major unknowns i·nn + id"""
        if self._A is None:
            N, NC = self.N, 1 << self.N
            nn = int(np.prod(self.n))
            idx = np.arange(nn).reshape(self.n, order="F")
            cn = tuple(m - 1 for m in self.n)
            corner = [idx[tuple(slice(o, o + c) for o, c in zip(_bits(b, N), cn))].reshape(-1, order="F") for b in range(NC)]
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
        nn = int(np.prod(self.n))
        return np.stack([x[i * nn:(i + 1) * nn].reshape(self.n, order="F") for i in range(self.N)])

    def apply_free(self, x):
        """the eliminated operator (by the assembled matrix): x is zero on the fixed components, and so is the result"""
        y = self.unflat(self.matrix() @ self.flat(np.where(self.free, x, 0.0)))
        return np.where(self.free, y, 0.0)


class Hierarchy:
    """level 0 and its coarsenings, _elliptic_ref.Hierarchy's per component: each level its own K0 (h doubles on the axes that
    coarsen), averaged cells, the bits of fine node 2J.  k0s: the levels' K0 (the device's, for the bitwise checks) or None;
    omegas: one damping per level in place of level_omega (the device's: device_omegas) or None"""

    def __init__(self, E, h, nu=0.3, plane="stress", fixed=None, k0s=None, fixed_omega=False, omegas=None):
        self.nu, self.plane, self.fixed_omega, self.omegas, self._om = nu, plane, fixed_omega, omegas, {}
        mk = (lambda l, hh: k0(hh, nu, plane)) if k0s is None else (lambda l, hh: k0s[l])
        self.ops, self.P = [Operator(E, h, mk(0, tuple(h)), fixed)], []
        while True:
            f = self.ops[-1]
            cs = coarsen_shape(f.n)
            if cs is None:
                break
            nc, co = cs
            hh = tuple(x * 2.0 if c else x for x, c in zip(f.h, co))
            bits = np.asfortranarray(f.bits[tuple(slice(None, None, 2) if c else slice(None) for c in co)])
            self.ops.append(Operator(coarsen_cells(f.E, co), hh, mk(len(self.ops), hh), bits))
            self.P.append((prolongation(f.n, co), 2.0 ** -sum(co)))
        assert omegas is None or len(omegas) == len(self.ops)

    @property
    def levels(self):
        return len(self.ops)

    def omega(self, lev, omega=OMEGA):
        """the damping of a level: the given one, else level_omega of its K0 (computed once)"""
        if self.omegas is not None:
            return self.omegas[lev]
        if self.fixed_omega:
            return omega
        if (lev, omega) not in self._om:
            self._om[lev, omega] = level_omega(self.ops[lev].K0, self.ops[lev].N, omega)
        return self._om[lev, omega]

    def _smooth(self, op, x, r, sweeps, omega):
        for _ in range(sweeps):
            if x is None:
                x = np.where(op.free, omega * r / op.D, 0.0)
            else:
                x = np.where(op.free, x + omega * (r - op.apply_free(x)) / op.D, 0.0)
        return x

    def vcycle(self, r, lev=0, omega=OMEGA):
        op = self.ops[lev]
        r = np.where(op.free, r, 0.0)
        om = self.omega(lev, omega)
        if lev == self.levels - 1:
            return self._smooth(op, None, r, NCOARSE, om)
        x = self._smooth(op, None, r, NPRE, om)
        P, scale = self.P[lev]
        cop = self.ops[lev + 1]
        res = np.where(op.free, r - op.apply_free(x), 0.0)
        rc = np.stack([(P.T @ res[i].reshape(-1, order="F") * scale).reshape(cop.n, order="F") for i in range(op.N)])
        xc = self.vcycle(np.where(cop.free, rc, 0.0), lev + 1, omega)
        px = np.stack([(P @ xc[i].reshape(-1, order="F")).reshape(op.n, order="F") for i in range(op.N)])
        x = np.where(op.free, x + px, 0.0)
        return self._smooth(op, x, r, NPOST, om)


def rhs(op, f):
    return op.m * np.asarray(f, dtype=np.float64)


def pcg(hier, f, u0, rtol=1e-8, max_iters=500, precond="mg", omega=OMEGA):
    """PCG on the free components from u0 (whose fixed components hold the prescribed values) until the recursive
    ‖r‖₂ ≤ rtol·‖b_free‖₂ (‖r₀‖₂ when b_free is zero).  Returns (u, iterations, relres, converged)."""
    op = hier.ops[0]
    M = (lambda r: hier.vcycle(r, 0, omega)) if precond == "mg" else (lambda r: np.where(op.free, r / op.D, 0.0))
    b = rhs(op, f)
    u = np.array(u0, dtype=np.float64)
    r = np.where(op.free, b - op.unflat(op.matrix() @ op.flat(u)), 0.0)
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
        if not np.isfinite(rr):
            break
        z = M(r)
        rho1 = float(np.sum(r * z))
        p = z + (rho1 / rho) * p
        rho = rho1
    return u, max_iters, np.sqrt(rr / bb), False


def direct(op, f, u0):
    """the solution by a sparse direct solve on the free components (the fixed ones keep u0's values)"""
    A = op.matrix()
    free = op.flat(op.free)
    u = op.flat(np.array(u0, dtype=np.float64))
    u[free] = 0.0
    b = op.flat(rhs(op, f)) - A @ u
    u[free] = spla.spsolve(A[free][:, free].tocsc(), b[free])
    return op.unflat(u)


def true_residual(op, f, u):
    """‖(b − A u)_free‖₂ with A u in the stated order, and ‖b_free‖₂"""
    b = rhs(op, f)
    r = np.where(op.free, b - op.apply(u), 0.0)
    return float(np.sqrt(np.sum(r * r))), float(np.sqrt(np.sum(np.where(op.free, b, 0.0) ** 2)))


def compliance(op, f, u):
    return float(np.prod(op.h)) * float(np.sum(rhs(op, f) * u))


def face_bits(n, d, side, bits):
    return face_mask(n, d, side).astype(np.uint8) * np.uint8(bits)


def traction(n, h, d, side, t):
    """f of a uniform traction t (an N-vector) on a face normal to d: 2t/h_d on the face's nodes"""
    f = np.zeros((len(n),) + tuple(n))
    m = face_mask(n, d, side)
    for i, ti in enumerate(t):
        f[i][m] = 2.0 * ti / h[d]
    return f


# ---- the cases shared by tests/test_elastic_host.py and tests/test_gpu_elastic.py

def cases():
    """name → dict(n, hc, h, phi, E (a cell array or None), E_in, E_out, nu, plane, bits, g, f, dtype)"""
    rng = np.random.default_rng(7)
    out = {}

    def add(name, n, bits, f, hc=None, contrast=1e-3, g=0.0, E=None, shift=0.0, plane="stress", nu=0.3, dtype=np.float64):
        N = len(n)
        hc = tuple((nd - 1.0) / (max(n) - 1.0) for nd in n) if hc is None else hc
        h = tuple(x / (nd - 1) for x, nd in zip(hc, n))
        f = f(h) if callable(f) else f
        f = np.array(np.broadcast_to(np.asarray(f, dtype=np.float64).reshape((N,) + (1,) * N) if np.ndim(f) == 1 else f, (N,) + tuple(n)))
        g = np.broadcast_to(np.asarray(g, dtype=np.float64), (N,)) if np.ndim(g) <= 1 else g
        out[name] = dict(n=n, hc=hc, h=h, phi=two_holes(n, h, shift), E=E, E_in=1.0, E_out=contrast, nu=nu, plane=plane,
                         bits=np.asfortranarray(bits.astype(np.uint8)), g=g, f=f, dtype=dtype)

    all2, all3 = 3, 7
    n = (33, 33)
    add("33x33_clamp", n, face_bits(n, 0, 0, all2), lambda h: traction(n, h, 0, 1, (0.0, -1.0)))
    add("33x33_contrast1_strain", n, face_bits(n, 0, 0, all2), (0.0, -1.0), contrast=1.0, g=(0.0, 0.25), plane="strain")
    n = (64, 48)
    add("64x48_upper_patch", n, _patch(n, 0, 1 / 3, 2 / 3).astype(np.uint8) * all2, (1.0, -1.0), shift=0.25)     # the interface runs through the boundary
    blob = np.zeros(n, dtype=np.uint8)
    blob[20:25, 30:34] = all2
    add("64x48_blob_roller", n, blob | face_bits(n, 1, 0, 2), (1.0, 0.5), g=(0.1, 0.0), plane="strain", nu=0.2)
    n = (65, 20)
    add("65x20_aniso_rollers", n, face_bits(n, 0, 0, 1) | face_bits(n, 1, 0, 2), rng.standard_normal((2,) + n), hc=(1.0, 0.6))
    n = (17, 17, 17)
    add("17c_clamp", n, face_bits(n, 2, 0, all3), lambda h: traction(n, h, 2, 1, (1.0, 0.0, 0.0)))
    add("17c_f32", n, face_bits(n, 0, 1, all3), (0.0, 0.0, -1.0), g=(0.0, 0.5, 0.0), dtype=np.float32)
    n = (24, 33, 10)
    add("24x33x10_patch", n, (_patch(n, 0, 1 / 3, 2 / 3) | face_mask(n, 1, 0)).astype(np.uint8) * all3, (0.0, 0.0, -1.0))
    add("24x33x10_aniso_given_E", n, face_bits(n, 0, 0, 1) | face_bits(n, 1, 0, 2) | face_bits(n, 2, 0, 4), rng.standard_normal((3,) + n),
        hc=(1.0, 1.2, 0.45), E=np.asfortranarray(0.5 + rng.random(tuple(m - 1 for m in n))))
    return out


def build_case(cs, k0s=None, omegas=None):
    """(Hierarchy, f, u0) of a case; an f32 case's ϕ and u0 are rounded to float32 first, as the handle stores them.  u0 is the
    case's guess (zero without one) with the prescribed values on the fixed components"""
    n, h, N = cs["n"], cs["h"], len(cs["n"])
    phi = cs["phi"].astype(cs["dtype"]).astype(np.float64)
    E = cs["E"] if cs["E"] is not None else cell_coefficients(phi, h, cs.get("level", 0.0), cs["E_in"], cs["E_out"])
    hier = Hierarchy(E, h, cs["nu"], cs["plane"], cs["bits"], k0s, omegas=omegas)
    u0 = np.zeros((N,) + tuple(n)) if cs.get("u0") is None else np.array(cs["u0"], dtype=np.float64)
    for i in range(N):
        u0[i][(cs["bits"] >> i) & 1 != 0] = cs["g"][i]
    u0 = u0.astype(cs["dtype"]).astype(np.float64)
    return hier, cs["f"], u0


_SOLVED = {}


def solved(name):
    """the restatement's results for a case, computed once: hier, f, u0, the direct solve, and per preconditioner
    (u, iterations, relres, converged) at rtol 1e-8; an f32 case's u is rounded to float32 as the handle stores it"""
    if name not in _SOLVED:
        cs = cases()[name]
        hier, f, u0 = build_case(cs)
        res = dict(case=cs, hier=hier, f=f, u0=u0, direct=direct(hier.ops[0], f, u0))
        for pc in ("mg", "jacobi"):
            u, it, rel, ok = pcg(hier, f, u0, 1e-8, 3000, pc)
            res[pc] = (u.astype(cs["dtype"]).astype(np.float64), it, rel, ok)
        _SOLVED[name] = res
    return _SOLVED[name]


# ---- the prototype problem of DESIGN.md §7.18's table: two ersatz holes, clamped on x = 0, a transverse load on the opposite face

def prototype(n, hc=None, contrast=1e-3, nu=0.3, plane="stress", fixed_omega=False):
    N = len(n)
    hc = tuple((nd - 1.0) / (max(n) - 1.0) for nd in n) if hc is None else hc
    h = tuple(x / (nd - 1) for x, nd in zip(hc, n))
    E = cell_coefficients(two_holes(n, h), h, 0.0, 1.0, contrast)
    hier = Hierarchy(E, h, nu, plane, face_bits(n, 0, 0, (1 << N) - 1), None, fixed_omega)
    t = [0.0] * N
    t[1] = -1.0
    return hier, traction(n, h, 0, 1, t), np.zeros((N,) + tuple(n))


TABLE = [((33, 33), None), ((65, 65), None), ((129, 129), None), ((129, 65), (2.0, 1.0)), ((129, 20), None), ((17, 17, 17), None), ((33, 33, 33), None),
         ((24, 33, 10), (1.0, 1.2, 0.45))]


# ---- the first PCG iterate in long double: with u0 = 0 and zero prescribed values r₀ = b, so u₁ = α·M b, α = (b·Mb)/(Mb·A Mb) — a
# solve that stops after one iteration shows M b at every node and component (tests/test_gpu_elastic_edges.py).  Operator.apply's
# loops run on long-double arrays from the float64 coefficients; P and Pᵀ go axis by axis, per component; ω is the float64 value.

def _apply_free_ld(op, x):
    return np.where(op.free, op.apply(np.where(op.free, x, LD(0))), LD(0))


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
    co = tuple(a != b for a, b in zip(op.n, cop.n))
    res = np.where(op.free, r - _apply_free_ld(op, x), LD(0))
    rc = np.stack([_transfer_ld(res[i], op.n, co, True) * LD(hier.P[lev][1]) for i in range(op.N)])
    xc = _vcycle_ld(hier, np.where(cop.free, rc, LD(0)), lev + 1)
    px = np.stack([_transfer_ld(xc[i], op.n, co, False) for i in range(op.N)])
    x = np.where(op.free, x + px, LD(0))
    for _ in range(NPOST):
        x = np.where(op.free, x + om * (r - _apply_free_ld(op, x)) / D, LD(0))
    return x


def first_iterate_ld(hier, f, precond="mg"):
    """u₁ of PCG from u0 = 0 with zero prescribed values, every operation in np.longdouble (the coefficients are the float64 ones)"""
    op = hier.ops[0]
    b = np.where(op.free, rhs(op, f).astype(LD), LD(0))
    z = _vcycle_ld(hier, b) if precond == "mg" else np.where(op.free, b / op.D.astype(LD), LD(0))
    return (np.sum(b * z) / np.sum(z * _apply_free_ld(op, z))) * z


def first_iterate_rhs(op):
    """name → f: a standard normal field and, for each component i that is free there, the impulses f = e_(i,j)/m_j (so b = e_(i,j):
    u₁ is a multiple of that column of M) at the upper corner n − 1 (the unpaired last node of every even axis), at n − 2 and at the
    odd interior node (n//2)|1"""
    out = {"normal": np.random.default_rng(13).standard_normal((op.N,) + op.n)}
    for name, j in (("corner", tuple(m - 1 for m in op.n)), ("corner-1", tuple(m - 2 for m in op.n)), ("odd", tuple((m // 2) | 1 for m in op.n))):
        for i in range(op.N):
            if op.free[(i,) + j]:
                f = np.zeros((op.N,) + op.n)
                f[(i,) + j] = 1.0 / op.m[j]
                out[f"{name}.{i}"] = f
    return out


FIRST_RTOL, FIRST_RELRES, FIRST_LEFT_OUT = 0.97, 0.95, 2


def first_iterate_runs(hier, precond):
    """[(name, f, u₁ of the restatement in float64, its relative residual)] for the right-hand sides of first_iterate_rhs that the
    device test uses: those whose relative residual after the restatement's first iteration is ≤ FIRST_RELRES, so that a solve at
    rtol = FIRST_RTOL stops after exactly one iteration with 2 % of margin; and the names of those left out"""
    op = hier.ops[0]
    runs, left_out = [], []
    for name, f in first_iterate_rhs(op).items():
        u, it, rel, ok = pcg(hier, f, np.zeros((op.N,) + op.n), FIRST_RTOL, 1, precond)
        if it == 1 and rel <= FIRST_RELRES:
            runs.append((name, f, u, rel))
        else:
            left_out.append((name, rel))
    return runs, left_out


# ---- the cases of tests/test_gpu_elastic_edges.py: what tests/test_gpu_elastic.py's nine shapes leave out

_EDGE_CASES = {}


def edge_cases():
    """name → the dict of cases() with the optional keys u0 (the guess, (N,)+n-shaped; the fixed components take g), level,
    solve ("both" | "mg"), direct (False: no sparse direct solve), big (the launch shapes: the prototype problem, one mg solve whose
    restatement the device test computes on the device's K0), devfield (f and u0 are given as device fields)"""
    if _EDGE_CASES:
        return _EDGE_CASES
    rng = np.random.default_rng(19)
    base = cases()
    out = _EDGE_CASES

    def add(name, n, bits, f=None, hc=None, E_in=1.0, E_out=1e-3, g=0.0, nu=0.3, plane="stress", dtype=np.float64, **extra):
        N = len(n)
        hc = tuple((nd - 1.0) / (max(n) - 1.0) for nd in n) if hc is None else hc
        h = tuple(x / (nd - 1) for x, nd in zip(hc, n))
        f = rng.standard_normal((N,) + tuple(n)) if f is None else f(h) if callable(f) else f
        f = np.array(np.broadcast_to(np.asarray(f, dtype=np.float64).reshape((N,) + (1,) * N) if np.ndim(f) == 1 else f, (N,) + tuple(n)))
        out[name] = dict(n=n, hc=hc, h=h, phi=two_holes(n, h), E=None, E_in=E_in, E_out=E_out, nu=nu, plane=plane,
                         bits=np.asfortranarray(bits.astype(np.uint8)), g=np.broadcast_to(np.asarray(g, dtype=np.float64), (N,)), f=f, dtype=dtype, **extra)

    def free_guess(cs):
        N = len(cs["n"])
        u0 = rng.standard_normal((N,) + tuple(cs["n"]))
        for i in range(N):
            u0[i][(cs["bits"] >> i) & 1 != 0] = 0.0
        return u0

    def rollers(n, side):
        b = np.zeros(n, dtype=np.uint8)
        for d in range(len(n)):
            b |= face_bits(n, d, side, 1 << d)
        return b

    all2, all3 = 3, 7
    # hierarchies of one level: M is the coarsest kernel alone (16 nodes in its 128 threads; 125 nodes with ω below 0.6)
    add("4x4_clamp", (4, 4), face_bits((4, 4), 0, 0, all2))
    add("5x5_rollers", (5, 5), rollers((5, 5), 0))
    add("4x5x4_clamp", (4, 5, 4), face_bits((4, 5, 4), 2, 0, all3))
    add("5x5x5_flat_clamp", (5, 5, 5), face_bits((5, 5, 5), 2, 0, all3), hc=(1.0, 1.0, 0.3))
    add("5x4x5_flat_rollers", (5, 4, 5), rollers((5, 4, 5), 0), hc=(1.0, 0.25, 1.0))
    # minimal hierarchies: a coarse axis of 3 nodes, an axis that never coarsens, four levels with a damping of their own each
    add("6x5_clamp", (6, 5), face_bits((6, 5), 0, 0, all2))
    add("4x40_side", (4, 40), face_bits((4, 40), 0, 0, all2))
    add("4x6x21_clamp", (4, 6, 21), face_bits((4, 6, 21), 2, 0, all3))
    # a lone partial bit on the unpaired last node of the even axis: injection keeps it or drops it by parity
    pin = face_bits((9, 12), 0, 0, 1)
    pin[4, 11] |= 2
    add("9x12_pin", (9, 12), pin)
    # fixed at the upper side of even axes only: no coarse level has a fixed component, the coarse operators are singular
    add("24x10_far_clamp", (24, 10), face_bits((24, 10), 0, 1, all2))
    add("6x6x6_far_clamp", (6, 6, 6), face_bits((6, 6, 6), 0, 1, all3))
    add("12x10x8_far_rollers", (12, 10, 8), rollers((12, 10, 8), 1))
    add("12x9_nu_neg", (12, 9), face_bits((12, 9), 0, 0, all2), nu=-0.5)
    # a float32 handle in 2-D
    out["33x33_f32_2d"] = dict(base["33x33_clamp"], g=np.array([0.0, 0.25]), dtype=np.float32)
    # a level other than zero, and the stiff material outside
    n = (64, 48)
    add("64x48_level", n, face_bits(n, 0, 0, all2), f=(0.0, -1.0), level=0.03, solve="mg")
    add("64x48_level_neg", n, face_bits(n, 0, 0, all2), f=(0.0, -1.0), level=-0.02, E_in=1e-3, E_out=1.0, solve="mg")
    # a guess that is not zero on the free components
    for name in ("33x33_clamp", "65x20_aniso_rollers", "17c_clamp", "17c_f32"):
        out[name + "_guess"] = dict(base[name], u0=free_guess(base[name]))
    # f and u0 as device fields
    out["64x48_devfield"] = dict(base["64x48_upper_patch"], f=rng.standard_normal((2,) + n), devfield=True)
    out["64x48_devfield"]["u0"] = free_guess(out["64x48_devfield"])
    # launch shapes (the prototype problem): more than 256 workgroups per node and more than MG_MAXB per unknown
    for n in ((300, 230), (45, 41, 37), (600, 500)):
        t = [0.0] * len(n)
        t[1] = -1.0
        add("x".join(map(str, n)), n, face_bits(n, 0, 0, (1 << len(n)) - 1), f=lambda h, n=n, t=t: traction(n, h, 0, 1, t), big=True, solve="mg", direct=False)
    return out


def edge_case_names(big=None):
    """the names of the big cases (big=True), of the others (False) or of all"""
    return sorted(k for k, v in edge_cases().items() if big is None or bool(v.get("big")) == big)


_EDGE = {}


def edge_solved(name):
    """solved() for an edge case; a preconditioner the case does not run is None, and a big case has neither (the device test solves
    its restatement on the device's K0) nor a direct solve"""
    if name not in _EDGE:
        cs = edge_cases()[name]
        hier, f, u0 = build_case(cs)
        res = dict(case=cs, hier=hier, f=f, u0=u0, direct=direct(hier.ops[0], f, u0) if cs.get("direct", True) else None)
        for pc in ("mg", "jacobi"):
            if cs.get("big") or (pc == "jacobi" and cs.get("solve", "both") == "mg"):
                res[pc] = None
                continue
            u, it, rel, ok = pcg(hier, f, u0, 1e-8, 3000, pc)
            res[pc] = (u.astype(cs["dtype"]).astype(np.float64), it, rel, ok)
        _EDGE[name] = res
    return _EDGE[name]


def any_solved(name):
    return solved(name) if name in cases() else edge_solved(name)


# the first-iterate test's shapes: the float64 cases of cases() with zero prescribed values, the one-level shapes, the minimal and
# stretched hierarchies, the lone pin, the coarse levels without a fixed component, a negative ν; Jacobi, where u₁ = α·D⁻¹b, on two of
# them as the trivial control.  (4x40 clamped on face (1, 0), 5x5x5 rollers at ν = 0.45 and plane strain at ν = 0.49 are out: one
# V-cycle leaves more than the whole residual for an impulse there; so is 64x48_upper_patch, the one float64 case of cases() with
# zero prescribed values that fails the condition: 1.92 for the normal right-hand side, tests/test_elastic_host.py.)
FIRST_ITERATE = (["33x33_clamp", "65x20_aniso_rollers", "17c_clamp", "24x33x10_patch", "24x33x10_aniso_given_E"]
                 + ["4x4_clamp", "5x5_rollers", "4x5x4_clamp", "5x5x5_flat_clamp", "5x4x5_flat_rollers", "6x5_clamp", "4x40_side", "4x6x21_clamp", "9x12_pin",
                    "24x10_far_clamp", "12x10x8_far_rollers", "12x9_nu_neg"])
FIRST_ITERATE_JACOBI = ["9x12_pin", "12x10x8_far_rollers"]
FIRST_ITERATE_PAIRS = [(k, "mg") for k in FIRST_ITERATE] + [(k, "jacobi") for k in FIRST_ITERATE_JACOBI]
