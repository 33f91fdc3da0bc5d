"""Thermoelastic coupling restated in numpy (csrc/lsm_elastic.hip, include/lsm.h "thermoelastic coupling"), over
_elastic_ref.Operator and _stress_ref.Stress.

Every function spells the header's operation order out, array-wide over the cells; all of them are compared with the device bit for bit.

  β          3λ + 2μ in 3-D and for plane strain, 2λ + 2μ for plane stress
  unit       ab_C = α_C·β;  θ_C = (Σ_b T_b, b ascending from +0)·2^−N − t_ref;  t_C = ab_C·θ_C;  g_C = E_C·t_C
  load       b_{I,i} = Σ over the existing cells, ascending m, from +0, of ±(c_i·g_C), + where bit i of m is clear;  f = b/m_I
  stress     ŝ_ii − t_C for every normal unit stress (ŝ_zz of plane strain included, plane stress keeps 0); the shears unchanged
  source     q_I = (Σ_C E_C·(ab_C·tr_C(v)))/(number of cells),  tr_C(v) = G_00 + G_11 (+ G_22) of _stress_ref.Stress.gradient
  sens       z_C = E_C·(t_C·tr_C(v) − q_C), q_C = Σ_r u_r·(Σ_s K0[r,s]·v_s);  d_I = (Σ_C z_C)/(number of cells) − minus_I

A cell that does not exist enters a node's sum as +0 (the padding), which changes no bit of a sum that began at +0.

The coupled discrete problem, for the derivative checks: the state A(E) u = m·f + b_th(E, T) on the free components with the prescribed
values on the fixed ones, J′ = Σ (m·l)·u, the adjoint A v = m·l with zero on the fixed components.
"""
import numpy as np

import _elastic_ref as R
import _stress_ref as S
from _multiload_ref import mutual_cells

STRESS, VON_MISES = S.STRESS, S.VON_MISES


class Thermo:
    """the coupling on one _stress_ref.Stress: alpha a scalar or a cell array (shape n − 1), t_ref the stress-free temperature"""

    def __init__(self, st, alpha, t_ref=0.0, nu=None, plane=None):
        self.st, self.op, self.N, self.nu, self.plane = st, st.op, st.N, nu, plane      # nu, plane: with_cells' (coupling() sets them)
        plane_stress = st.N == 2 and not st.strain2d
        self.beta = (2.0 if plane_stress else 3.0) * st.lam + 2.0 * st.mu
        self.alpha = np.float64(alpha) if np.ndim(alpha) == 0 else np.asfortranarray(alpha, dtype=np.float64)
        self.t_ref = np.float64(t_ref)

    # ---- per cell
    def theta(self, T):
        N, cn = self.N, self.st.cn
        T = np.asarray(T, dtype=np.float64)
        s = np.zeros(cn)
        for b in range(1 << N):
            s = s + T[tuple(slice(o, o + c) for o, c in zip(R._bits(b, N), cn))]
        return s * 2.0 ** -N - self.t_ref

    def unit(self, T):
        """t_C = (α_C·β)·θ_C"""
        return (self.alpha * self.beta) * self.theta(T)

    def trace(self, v):
        G = self.st.gradient(v)
        tr = G[0][0] + G[1][1]
        if self.N > 2:
            tr = tr + G[2][2]
        return tr

    def stress_cells(self, u, T, what):
        """(M,)+cells for the stress, cells-shaped for von Mises"""
        N, st = self.N, self.st
        _, sn, tau = st.unit(u)
        t = self.unit(T)
        sn = [s - t for s in sn[:N]] + ([sn[2] - t if st.strain2d else sn[2]] if N == 2 else [])
        E = self.op.E
        if what == STRESS:
            return np.stack([E * s for s in sn[:N]] + [E * x for x in tau])
        if what == VON_MISES:
            return E * np.sqrt(st.v2(sn, tau))
        raise ValueError("the thermal stress is STRESS or VON_MISES: the total strain is the displacement's")

    def sens_cells(self, u, v, T):
        return self.op.E * (self.unit(T) * self.trace(v) - mutual_cells(self.op, u, v))

    # ---- per node
    def load(self, T):
        """f = b/m_I, (N,)+n"""
        N, op = self.N, self.op
        g = op.E * self.unit(T)
        b = np.zeros((N,) + op.n)
        for m in range(1 << N):
            for i in range(N):
                t = self.st.c[i] * g
                b[i] = b[i] + np.pad(-t if (m >> i) & 1 else t, 1)[op._cell(m)]
        return b / op.m

    def stress_nodes(self, u, T, what):
        c = self.stress_cells(u, T, what)
        return self.st.node_mean(c) if what == VON_MISES else np.stack([self.st.node_mean(x) for x in c])

    def source(self, v):
        return self.st.node_mean(self.op.E * ((self.alpha * self.beta) * self.trace(v)))

    def sensitivity(self, u, v, T, minus=None):
        d = self.st.node_mean(self.sens_cells(u, v, T))
        return d if minus is None else d - np.asarray(minus, dtype=np.float64)

    # ---- the coupled discrete problem
    def with_cells(self, E):
        """the same coupling on other cell moduli (the finite differences of the derivative checks)"""
        op = self.op
        return coupling(E, op.h, self.nu, self.plane, op.bits, self.alpha, self.t_ref, op.K0)

    def state(self, f, T, u0):
        """u of A u = m·f + b_th(T) on the free components by a direct solve; u0 holds the prescribed values"""
        return R.direct(self.op, np.asarray(f, dtype=np.float64) + self.load(T), u0)

    def adjoint(self, l):
        return R.direct(self.op, l, np.zeros((self.N,) + self.op.n))

    def objective(self, l, u):
        """J′ = Σ (m·l)·u"""
        return float(np.sum(R.rhs(self.op, l) * u))

    def free_expansion(self, theta, lc=None):
        """u_i = ε*·(x_i − lc_i) on the nodes, ε* = α·θ (3-D, plane stress) or (1+ν)·α·θ (plane strain): uniform α, E, θ"""
        op = self.op
        eps = float(self.alpha) * theta * ((1.0 + self.nu) if self.st.strain2d else 1.0)
        lc = (0.0,) * self.N if lc is None else lc
        x = np.meshgrid(*[np.arange(m) * hd for m, hd in zip(op.n, op.h)], indexing="ij")
        return np.stack([eps * (x[i] - lc[i]) for i in range(self.N)]), eps


def coupling(E, h, nu, plane, bits, alpha, t_ref=0.0, K0=None):
    """a Thermo from cell moduli: the closed-form K0 unless the device's is given"""
    K0 = R.k0(tuple(h), nu, plane) if K0 is None else K0
    return Thermo(S.Stress(R.Operator(E, h, K0, bits), nu, plane), alpha, t_ref, nu, plane)
