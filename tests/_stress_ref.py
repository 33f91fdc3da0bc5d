"""Stress recovery restated in numpy (csrc/lsm_elastic.hip, include/lsm.h "stress recovery"), over _elastic_ref.

Every function spells the header's operation order out, array-wide over the cells: the cell arrays and the node fields are what the
device is compared with bit for bit.  The aggregate, the adjoint load and the sensitivity differ from the device in the order of
the grand sum and in pow, so they are compared to rounding: every function runs in np.longdouble as well (dt=np.longdouble: the float64
coefficients c_j, λ, μ, E, K0 with long-double arithmetic), which is what bounds the float64 run's own error.

  gradient   d_ij = Σ_b (bit j of b ? u_{b,i} : −u_{b,i}), b ascending from +0;  G_ij = d_ij·c_j,  c_j = (1/h_j)·2^−(N−1)
  Voigt      2-D (00, 11, 01); 3-D (00, 11, 22, 12, 02, 01)
  strain     e_ii = G_ii; e_ij = G_ij + G_ji (i < j);  tr = G_00 + G_11 (+ G_22)
  unit       ŝ_ii = λ·tr + (2μ)·G_ii; τ̂_ij = μ·e_ij; 2-D: ŝ_zz = λ·tr (plane strain) or 0 (plane stress);  σ = E_C·(ŝ, τ̂)
  von Mises  v2 = 0.5·(((a−b)² + (b−c)²) + (c−a)²) + 3·Σ τ̂²;  s_C = E_C·sqrt(v2)
  node       (Σ over the existing cells around I, ascending, from +0)/(their number)
  aggregate  J′ = Σ_C pow(s_C/sref, p);  G_p = sref·(∏h·J′)^(1/p)
  load       g_{I,i} = Σ_C w_C·(Σ_j ±(c_j·Z_ij)), w_C = (p·((E_C/sref)·(E_C/sref)))·pow(r_C, p−2);  f = g/m_I
  sens       d_I = (scale·Σ_C (p·pow(r_C, p) − E_C·(Σ_r λ_r·(Σ_s K0[r,s]·u_s))))/(number of cells)
"""
import numpy as np

from _elastic_ref import _bits, direct, face_bits, material, pcg, traction

STRAIN, STRESS, VON_MISES = 0, 1, 2


def voigt(N):
    return [(0, 0), (1, 1), (0, 1)] if N == 2 else [(0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)]


class Stress:
    """the stress recovery of one level-0 _elastic_ref.Operator with the material (ν, plane)"""

    def __init__(self, op, nu, plane="stress"):
        self.op, self.N = op, op.N
        self.lam, self.mu = material(nu, op.N, plane)
        self.strain2d = op.N == 2 and plane == "strain"
        self.c = [(1.0 / op.h[j]) * (0.5 if op.N == 2 else 0.25) for j in range(op.N)]
        self.cn = tuple(m - 1 for m in op.n)

    # ---- per cell
    def corners(self, u, dt=np.float64):
        """uc[b][i]: component i at corner b of every cell"""
        N = self.N
        u = [np.asarray(u[i]).astype(dt) for i in range(N)]
        return [[u[i][tuple(slice(o, o + c) for o, c in zip(_bits(b, N), self.cn))] for i in range(N)] for b in range(1 << N)]

    def gradient(self, u, dt=np.float64):
        N = self.N
        uc = self.corners(u, dt)
        G = [[None] * N for _ in range(N)]
        for i in range(N):
            for j in range(N):
                d = np.zeros(self.cn, dtype=dt)
                for b in range(1 << N):
                    d = d + (uc[b][i] if (b >> j) & 1 else -uc[b][i])
                G[i][j] = d * dt(self.c[j])
        return G

    def unit(self, u, dt=np.float64):
        """(e: the M strains, sn: the three unit normal stresses, tau: the unit shears in Voigt order)"""
        N = self.N
        G = self.gradient(u, dt)
        tr = G[0][0] + G[1][1]
        if N > 2:
            tr = tr + G[2][2]
        lt, mu2 = dt(self.lam) * tr, dt(2.0 * self.mu)
        e = [G[i][i] for i in range(N)]
        sn = [lt + mu2 * G[i][i] for i in range(N)]
        if N == 2:
            sn.append(lt if self.strain2d else np.zeros(self.cn, dtype=dt))
        tau = []
        for i, j in voigt(N)[N:]:
            e.append(G[i][j] + G[j][i])
            tau.append(dt(self.mu) * e[-1])
        return e, sn, tau

    @staticmethod
    def v2(sn, tau, dt=np.float64):
        ab, bc, ca = sn[0] - sn[1], sn[1] - sn[2], sn[2] - sn[0]
        q = np.zeros(ab.shape, dtype=dt)
        for t in tau:
            q = q + t * t
        return dt(0.5) * ((ab * ab + bc * bc) + ca * ca) + dt(3.0) * q

    def cells(self, u, what, dt=np.float64):
        """the cell arrays: (M,)+cells for the strain and the stress, cells-shaped for von Mises"""
        e, sn, tau = self.unit(u, dt)
        E = self.op.E.astype(dt)
        if what == STRAIN:
            return np.stack(e)
        if what == STRESS:
            return np.stack([E * s for s in sn[:self.N]] + [E * t for t in tau])
        return E * np.sqrt(self.v2(sn, tau, dt))

    # ---- per node
    def node_mean(self, cell, scale=None):
        """(Σ over the existing cells, ascending, from +0)/(their number); with a scale (scale·Σ)/(number)"""
        op = self.op
        w = np.pad(cell, 1)
        acc = np.zeros(op.n, dtype=cell.dtype)
        for m in range(1 << self.N):
            acc = acc + w[op._cell(m)]
        if scale is not None:
            acc = cell.dtype.type(scale) * acc
        return acc / op.count.astype(cell.dtype)

    def nodes(self, u, what, dt=np.float64):
        c = self.cells(u, what, dt)
        return self.node_mean(c) if what == VON_MISES else np.stack([self.node_mean(x) for x in c])

    # ---- the aggregate
    def norm(self, u, p, sref, dt=np.float64):
        """(J′, smax)"""
        s = self.cells(u, VON_MISES, dt)
        return np.sum(np.power(s / dt(sref), dt(p))), np.max(s)

    def gp(self, J, sref, p):
        return float(sref) * (float(np.prod(self.op.h)) * float(J)) ** (1.0 / float(p))

    def load(self, u, p, sref, dt=np.float64):
        """f = g/m_I, (N,)+n"""
        N, op = self.N, self.op
        e, sn, tau = self.unit(u, dt)
        E = op.E.astype(dt)
        r = (E * np.sqrt(self.v2(sn, tau, dt))) / dt(sref)
        es = E / dt(sref)
        w = (dt(p) * (es * es)) * np.power(r, dt(p - 2.0))
        half = dt(0.5)
        m = [sn[0] - half * (sn[1] + sn[2]), sn[1] - half * (sn[0] + sn[2]), sn[2] - half * (sn[0] + sn[1])]
        sm = m[0] + m[1]
        if N > 2 or self.strain2d:
            sm = sm + m[2]
        ls, mu2, mu3 = dt(self.lam) * sm, dt(2.0 * self.mu), dt(3.0 * self.mu)
        Z = [[None] * N for _ in range(N)]
        for i in range(N):
            Z[i][i] = ls + mu2 * m[i]
        for k, (i, j) in enumerate(voigt(N)[N:]):
            Z[i][j] = Z[j][i] = mu3 * tau[k]
        g = np.zeros((N,) + op.n, dtype=dt)
        for mm in range(1 << N):
            for i in range(N):
                inner = np.zeros(self.cn, dtype=dt)
                for j in range(N):
                    t = dt(self.c[j]) * Z[i][j]
                    inner = inner + (-t if (mm >> j) & 1 else t)
                g[i] = g[i] + np.pad(w * inner, 1)[op._cell(mm)]
        return g / op.m.astype(dt)

    def sens_cells(self, u, lam, p, sref, dt=np.float64):
        """p·pow(r_C, p) − E_C·(Σ_r λ_r·(Σ_s K0[r,s]·u_s)): E_C·∂J′/∂E_C"""
        N, op = self.N, self.op
        R = (1 << N) * N
        s = self.cells(u, VON_MISES, dt)
        uc, lc = self.corners(u, dt), self.corners(lam, dt)
        K = op.K0.astype(dt)
        q = np.zeros(self.cn, dtype=dt)
        for a in range(R):
            t = np.zeros(self.cn, dtype=dt)
            for b in range(R):
                t = t + K[a, b] * uc[b // N][b % N]
            q = q + lc[a // N][a % N] * t
        return dt(p) * np.power(s / dt(sref), dt(p)) - op.E.astype(dt) * q

    def sensitivity(self, u, lam, p, sref, scale, dt=np.float64):
        return self.node_mean(self.sens_cells(u, lam, p, sref, dt), scale)

    def adjoint(self, u, p, sref):
        """the solution of A λ = g on the free components, zero on the fixed ones, by a sparse direct solve"""
        return direct(self.op, self.load(u, p, sref), np.zeros((self.N,) + self.op.n))

    def homogeneity(self, d):
        """Σ_I count_I·d_I, which vanishes with zero prescribed values"""
        return float(np.sum(self.op.count * d))


# ---- the cases of tests/test_gpu_stress.py, in the vocabulary of _elastic_ref.cases()

def _case(n, hc, phi, nu=0.3, plane="stress", E=None, E_out=1e-3, level=0.0, dtype=np.float64, f=None):
    N = len(n)
    h = tuple(x / (m - 1) for x, m in zip(hc, n))
    return dict(n=n, hc=hc, h=h, phi=np.asfortranarray(phi(n, h)), E=E, E_in=1.0, E_out=E_out, nu=nu, plane=plane, level=level,
                bits=np.asfortranarray(face_bits(n, 0, 0, (1 << N) - 1)), g=np.zeros(N), f=None if f is None else f(n, h), dtype=dtype)


def hole(n, h):
    """material (ϕ < 0) everywhere but in a ball of a quarter of the shortest side around the centre"""
    x = np.meshgrid(*[np.arange(m) * hd for m, hd in zip(n, h)], indexing="ij")
    c = [0.5 * (m - 1) * hd for m, hd in zip(n, h)]
    return 0.25 * min(2.0 * v for v in c) - np.sqrt(sum((xd - cd) ** 2 for xd, cd in zip(x, c)))


def _tip_load(n, h):
    t = [0.0] * len(n)
    t[1] = -1.0
    return traction(n, h, 0, 1, t)


def field_cases():
    """random displacements: every shape the issue names that a handle accepts (4 nodes per dimension at least: 4×4, 5×4 and 4×4×4
    stand for 3×3, 4×3 and 3×3×3), anisotropic h, both planes, ν = 0.3 and a negative one, moduli from ϕ and given, a level ≠ 0, one
    float32 handle; and the two launch shapes beyond 2048 workgroups of 256 threads"""
    rng = np.random.default_rng(23)
    given = lambda n: np.asfortranarray(0.05 + rng.random(tuple(m - 1 for m in n)))
    return {
        "4x4": _case((4, 4), (1.0, 1.0), hole),
        "5x4_strain_aniso_given_E_nu_neg": _case((5, 4), (1.0, 0.45), hole, nu=-0.4, plane="strain", E=given((5, 4))),
        "9x12_strain_level": _case((9, 12), (0.8, 1.0), hole, plane="strain", level=0.03),
        "9x12_f32": _case((9, 12), (0.8, 1.0), hole, dtype=np.float32),
        "4x4x4": _case((4, 4, 4), (1.0, 1.0, 1.0), hole),
        "5x4x6_aniso_given_E_nu_neg": _case((5, 4, 6), (1.0, 0.5, 1.3), hole, nu=-0.3, E=given((5, 4, 6))),
        "4x6x21_level": _case((4, 6, 21), (0.2, 0.3, 1.0), hole, level=-0.02),
        "1025x600": _case((1025, 600), (1024.0 / 599.0, 1.0), hole),
        "96x96x64": _case((96, 96, 64), (1.0, 1.0, 63.0 / 95.0), hole),
    }


AGGREGATE = ["9x12_strain_level", "9x12_f32", "5x4_strain_aniso_given_E_nu_neg", "5x4x6_aniso_given_E_nu_neg", "4x6x21_level"]


def solved_cases():
    """the four small solved problems: a cantilever with a hole at contrast 1e-3, clamped at x = 0 under a transverse tip traction"""
    return {
        "17x9_stress": _case((17, 9), (2.0, 1.0), hole, f=_tip_load),
        "17x9_strain": _case((17, 9), (2.0, 1.0), hole, plane="strain", f=_tip_load),
        "9x7x5": _case((9, 7, 5), (2.0, 1.5, 1.0), hole, f=_tip_load),
        "17x9_f32": _case((17, 9), (2.0, 1.0), hole, dtype=np.float32, f=_tip_load),
    }


def sensitivity_by(st, hier, f, u0, p, dtype, solver, rtol=1e-8):
    """(d, G_p, J′, sref, state iterations, adjoint iterations) of the restatement with solver = "direct" (float64 throughout, the
    reference) or a PCG preconditioner (u, λ and d rounded to the storage type, as the handle stores them: _elastic_ref.solved's
    convention); sref = smax of that u; scale = G_p/(p·J′)"""
    op = hier.ops[0]
    rnd = (lambda a: np.asarray(a, dtype=np.float64)) if solver == "direct" else (lambda a: np.asarray(a).astype(dtype).astype(np.float64))
    zero = np.zeros((op.N,) + op.n)
    if solver == "direct":
        u, it_u = rnd(direct(op, f, u0)), 0
    else:
        u, it_u, _, ok = pcg(hier, f, u0, rtol, 3000, solver)
        assert ok
        u = rnd(u)
    sref = float(st.norm(u, 2.0, 1.0)[1])
    J = float(st.norm(u, p, sref)[0])
    G = st.gp(J, sref, p)
    load = st.load(u, p, sref)
    if solver == "direct":
        lam, it_a = rnd(direct(op, load, zero)), 0
    else:
        lam, it_a, _, ok = pcg(hier, load, zero, rtol, 3000, solver)
        assert ok
        lam = rnd(lam)
    return rnd(st.sensitivity(u, lam, p, sref, G / (p * J))), G, J, sref, it_u, it_a
