"""The topological derivative of the compliance and the nucleation step restated in numpy (csrc/lsm_elastic.hip, csrc/lsm_nucleate.hip,
include/lsm.h "topological derivative" and "nucleation"), over _stress_ref and _elastic_ref.

Every function spells the header's operation order out, so the cell array, the node field, the centre list and the punched ϕ are
what the device is compared with bit for bit.

  constants  N = 2: g = (λ + 2μ)/((2μ)·(λ + μ)), a = g·(4μ), b = g·(λ − μ);  N = 3: g = (3·(λ + 2μ))/((4μ)·(9λ + 14μ)), a = g·(20μ), b = g·(3λ − 2μ)
  cell       w = Σ_i ŝ_ii·G_ii, then + τ̂_ij·e_ij in Voigt order (one accumulator from +0);  tr, trs the traces of G and ŝ over the N axes
             T_C = E_C·(a·w + b·(trs·tr))
  node       _stress_ref.Stress.node_mean
  candidate  t_I < threshold and ϕ_I ≤ level − clearance (false for NaN)
  centre     a candidate whose key (t_I, linear index I) is the smallest over the candidates of its box window |J_d − I_d| ≤ w_d,
             w_d = ceil(spacing/h_d); −0 and +0 are one value
  punch      B_d = floor(radius/h_d); d2 = Σ_d ((I_d − c_d)·h_d)², v = level + (radius − sqrt(d2)) over the clipped box; V = the largest v;
             ϕ_I := V_I where ϕ_I < V_I, rounded once; changed = the stored values whose bits differ
"""
import math

import numpy as np

import _stress_ref as S


def constants(lam, mu, N):
    if N == 2:
        g = (lam + 2.0 * mu) / ((2.0 * mu) * (lam + mu))
        return g * (4.0 * mu), g * (lam - mu)
    g = (3.0 * (lam + 2.0 * mu)) / ((4.0 * mu) * (9.0 * lam + 14.0 * mu))
    return g * (20.0 * mu), g * (3.0 * lam - 2.0 * mu)


def cells(st, u, dt=np.float64):
    """T_C of the displacement u on the _stress_ref.Stress st: an array of the cells' shape"""
    N = st.N
    a, b = constants(st.lam, st.mu, N)
    e, sn, tau = st.unit(u, dt)
    w = np.zeros(st.cn, dtype=dt)
    for i in range(N):
        w = w + sn[i] * e[i]
    for k in range(len(tau)):
        w = w + tau[k] * e[N + k]
    tr, trs = e[0] + e[1], sn[0] + sn[1]
    if N > 2:
        tr, trs = tr + e[2], trs + sn[2]
    return st.op.E.astype(dt) * (dt(a) * w + dt(b) * (trs * tr))


def work(st, u):
    """E_C·w, the strain energy density σ:ε of a cell (twice the stored energy)"""
    e, sn, tau = st.unit(u)
    w = np.zeros(st.cn)
    for i in range(st.N):
        w = w + sn[i] * e[i]
    for k in range(len(tau)):
        w = w + tau[k] * e[st.N + k]
    return st.op.E * w


def nodes(st, u):
    return st.node_mean(cells(st, u))


# ---- the search

def window(spacing, h):
    return tuple(int(math.ceil(float(spacing) / float(hd))) for hd in h)


def candidates(phi, t, threshold, level, clearance):
    phi, t = np.asarray(phi).astype(np.float64), np.asarray(t).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (t < float(threshold)) & (phi <= float(level) - float(clearance))


def centres(phi, t, threshold, level, clearance, w):
    """(linear indices ascending, axis 0 fastest; the values of t there as float64).  The keys are ranked once — a stable sort of the
    candidates' values (−0 folded into +0) taken in index order — and the ranks go through one sliding minimum per axis."""
    phi = np.asarray(phi)
    n = phi.shape
    cand = candidates(phi, t, threshold, level, clearance).ravel(order="F")
    tv = np.asarray(t).astype(np.float64).ravel(order="F")
    idx = np.flatnonzero(cand)
    none = np.iinfo(np.int64).max
    rank = np.full(cand.size, none, dtype=np.int64)
    rank[idx[np.argsort(tv[idx] + 0.0, kind="stable")]] = np.arange(idx.size)
    rank = rank.reshape(n, order="F")
    m = rank
    for d, wd in enumerate(w):
        wd = min(int(wd), n[d])
        pad = [(wd, wd) if e == d else (0, 0) for e in range(len(n))]
        p = np.pad(m, pad, constant_values=none)
        out = m
        for s in range(2 * wd + 1):
            out = np.minimum(out, p[tuple(slice(s, s + n[d]) if e == d else slice(None) for e in range(len(n)))])
        m = out
    keep = np.flatnonzero(((rank != none) & (m == rank)).ravel(order="F"))
    return keep.astype(np.int64), tv[keep]


def select(idx, val, max_holes=None):
    """sorted by (value, index), cut to the max_holes lowest"""
    order = np.lexsort((idx, val))
    if max_holes is not None:
        order = order[:int(max_holes)]
    return idx[order], val[order]


# ---- the punch

def punch(phi, centres_lin, h, level, radius):
    """(the punched ϕ in ϕ's dtype, the number of stored values whose bits changed) for a list of linear node indices"""
    phi = np.asarray(phi)
    n, N = phi.shape, phi.ndim
    B = [int(min(math.floor(float(radius) / float(hd)), m)) for hd, m in zip(h, n)]
    V = np.full(n, -np.inf)
    for c in np.asarray(centres_lin, dtype=np.int64).ravel():
        cI = np.unravel_index(int(c), n, order="F")
        lo = [max(0, int(ci) - b) for ci, b in zip(cI, B)]
        hi = [min(m - 1, int(ci) + b) for ci, b, m in zip(cI, B, n)]
        ax = np.meshgrid(*[np.arange(l, u + 1) for l, u in zip(lo, hi)], indexing="ij")
        d2 = np.zeros(ax[0].shape)
        for d in range(N):
            x = (ax[d] - int(cI[d])).astype(np.float64) * float(h[d])
            d2 = d2 + x * x
        v = float(level) + (float(radius) - np.sqrt(d2))
        box = tuple(slice(l, u + 1) for l, u in zip(lo, hi))
        V[box] = np.maximum(V[box], v)
    wide = phi.astype(np.float64)
    with np.errstate(invalid="ignore"):
        take = wide < V
    new = np.where(take, V, wide).astype(phi.dtype)
    new[~take] = phi[~take]
    bits = np.uint64 if phi.dtype == np.float64 else np.uint32
    changed = int((np.ascontiguousarray(new).view(bits) != np.ascontiguousarray(phi).view(bits)).sum())
    return new, changed


def nucleate(phi, t, h, *, threshold, radius, spacing=None, clearance=None, max_holes=None, level=0.0):
    """the whole step: (ϕ punched, centres' linear indices sorted by (value, index) and cut, their values, found, changed)"""
    spacing = 2.0 * radius if spacing is None else spacing
    clearance = radius if clearance is None else clearance
    idx, val = centres(phi, t, threshold, level, clearance, window(spacing, h))
    found = idx.size
    idx, val = select(idx, val, max_holes)
    new, changed = punch(phi, idx, h, level, radius)
    return new, idx, val, found, changed
