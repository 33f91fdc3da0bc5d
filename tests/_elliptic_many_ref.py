"""The multi-source fields of elliptic_solve restated in numpy (include/lsm.h "elliptic_solve": lsm_elliptic_energy_many,
lsm_elliptic_energy_mutual), on top of tests/_elliptic_ref.py, whose Operator they take.

  mutual    m_I = Σ_d ( Σ_± k̄·(g_u·g_v), g_u = (u_J − u_I)/h_d, g_v = (v_J − v_I)/h_d ) / (number of existing edges along d at I):
            Operator.energy's statements with g·g replaced by g_u·g_v, so that v = u gives its bits; the a∇u·∇v part only (no c·u·v)
  weighted  e_I = Σ_k w_k·e_{k,I}, k ascending from +0, e_k = Operator.energy(u_k) in float64
A batched solve has no restatement of its own: column k of it is the single solve of column k, bit for bit.
"""
import numpy as np


def energy_mutual(op, u, v):
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    e = np.zeros(op.n)
    for d in range(op.N):
        lo, hi = op._sl(d, 1, None), op._sl(d, None, -1)
        s, cnt = np.zeros(op.n), np.zeros(op.n)
        gu, gv = (u[hi] - u[lo]) / op.h[d], (v[hi] - v[lo]) / op.h[d]
        s[lo] = s[lo] + op.kbar[d] * (gu * gv)
        cnt[lo] += 1
        gu, gv = (u[lo] - u[hi]) / op.h[d], (v[lo] - v[hi]) / op.h[d]
        s[hi] = s[hi] + op.kbar[d] * (gu * gv)
        cnt[hi] += 1
        e = e + s / cnt
    return e


def energy_weighted(op, us, w):
    e = np.zeros(op.n)
    for uk, wk in zip(us, w):
        e = e + float(wk) * op.energy(uk)
    return e


def energy_mutual_abs(op, u, v):
    """Σ_d (Σ_± k̄·|g_u|·|g_v|)/(existing edges): the sum of the magnitudes of the terms of m_I, each already divided by its count"""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    e = np.zeros(op.n)
    for d in range(op.N):
        lo, hi = op._sl(d, 1, None), op._sl(d, None, -1)
        s, cnt = np.zeros(op.n), np.zeros(op.n)
        t = op.kbar[d] * (np.abs((u[hi] - u[lo]) / op.h[d]) * np.abs((v[hi] - v[lo]) / op.h[d]))
        s[lo] = s[lo] + t
        cnt[lo] += 1
        s[hi] = s[hi] + t
        cnt[hi] += 1
        e = e + s / cnt
    return e
