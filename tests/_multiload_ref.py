"""The multi-load fields of elasticity_solve restated in numpy (include/lsm.h "elasticity_solve": lsm_elastic_energy_many,
lsm_elastic_energy_mutual), on top of tests/_elastic_ref.py, whose Operator they take.

  mutual    m_I = (Σ_C E_C·q_C)/(number of existing cells around I), q_C = Σ_r u_r·(Σ_s K0[r,s]·v_s), both sums from +0 ascending:
            Operator.energy's loops with v in the inner sum, so that v = u gives its bits
  weighted  e_I = Σ_k w_k·e_{k,I}, k ascending from +0, e_k = Operator.energy(u_k) in float64
A batched solve has no restatement of its own: column k of it is the single solve of column k, bit for bit.
"""
import numpy as np

import _elastic_ref as R


def mutual_cells(op, u, v, K0=None):
    """q_C of every cell (shape n − 1): Σ_r u_r·(Σ_s K0[r,s]·v_s) over the cell's 2^N·N corner values, both from +0 ascending"""
    N, NC = op.N, 1 << op.N
    K0 = op.K0 if K0 is None else K0
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    cn = tuple(m - 1 for m in op.n)
    corner = lambda x, r: x[r % N][tuple(slice(o, o + c) for o, c in zip(R._bits(r // N, N), cn))]
    uc = [corner(u, r) for r in range(NC * N)]
    vc = [corner(v, r) for r in range(NC * N)]
    q = np.zeros(cn)
    for r in range(NC * N):
        t = np.zeros(cn)
        for s in range(NC * N):
            t = t + K0[r, s] * vc[s]
        q = q + uc[r] * t
    return q


def node_sum(op, w):
    """Σ over the existing cells around a node, ascending from +0, of the cell array w"""
    wp = np.pad(w, 1)
    acc = np.zeros(op.n)
    for m in range(1 << op.N):
        acc = acc + wp[op._cell(m)]
    return acc


def energy_mutual(op, u, v):
    return node_sum(op, op.E * mutual_cells(op, u, v)) / op.count


def energy_weighted(op, us, w):
    e = np.zeros(op.n)
    for uk, wk in zip(us, w):
        e = e + float(wk) * op.energy(uk)
    return e


def energy_mutual_abs(op, u, v):
    """Σ_C E_C·Σ|K0[r,s]|·|u_r|·|v_s| around a node, not divided by the count: the sum of the magnitudes of the terms of count·m"""
    return node_sum(op, op.E * mutual_cells(op, np.abs(u), np.abs(v), np.abs(op.K0)))
