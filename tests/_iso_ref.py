"""numpy restatement of isosurface(ϕ, level) (csrc/lsm_iso.hip): marching simplices on the Freudenthal (Kuhn) subdivision of
every cell, giving an indexed, watertight, consistently oriented mesh of the zero set of the piecewise-linear interpolant
(DESIGN.md §7.11).  The device is tested against this file; tests/test_isosurface_host.py checks this file against facts that
do not come from it.  The rules:
  * inside(I) := ϕ[I] < level (ϕ == level and NaN are outside); float32 values widen exactly, all arithmetic is fp64;
  * cell C has corners C + m, m an N-bit mask (bit a = axis a); for every permutation π of the axes in lexicographic order one
    simplex with the corner chain m₀ = 0, m₁ = m₀ | 1<<π(0), …, m_N = 2^N − 1;
  * edge (I, d), d a non-empty mask, carries a vertex iff I + d is in the grid, inside(I) != inside(I + d) and an active cell
    contains the edge (dense: every cell; band: the cells whose 2^N corners are band nodes); vertices are numbered by
    ascending node (axis 0 fastest), then ascending d; position (lc + i·h) + t·h along the axes of d, t = (level − ϕ_a)/(ϕ_b − ϕ_a)
    with a = I, b = I + d;
  * active cells ascending, simplices in permutation order: k inside corners, 0 < k < N + 1, give one segment (2-D), one triangle
    (3-D, k = 1, 3) or the quad (ac, ad, bd, bc) as (ac, ad, bd), (ac, bd, bc) (3-D, k = 2; a < b inside, c < d outside by chain
    position); the last two vertices of an element are swapped when FLIP[sign pattern] xor (π odd), so that a triangle's
    (v1 − v0) × (v2 − v0), a segment's (Δy, −Δx), points from inside to outside."""
import itertools

import numpy as np

# sign patterns (bit j = chain corner j inside) whose canonical element is reversed on an even permutation
FLIP = {2: frozenset((2, 3, 6)), 3: frozenset((2, 5, 8, 10, 11, 14))}


def _parity_odd(p):
    return sum(p[i] > p[j] for i in range(len(p)) for j in range(i + 1, len(p))) % 2 == 1


def simplices(N):
    """[(corner chain m₀..m_N, π odd)] in lexicographic order of π"""
    out = []
    for p in itertools.permutations(range(N)):
        m = [0]
        for a in p:
            m.append(m[-1] | (1 << a))
        out.append((tuple(m), _parity_odd(p)))
    return out


def pattern_elements(N, s, odd):
    """the elements of a simplex with sign pattern s: tuples of edges (j, k), j < k chain positions"""
    ins = [j for j in range(N + 1) if s >> j & 1]
    outs = [j for j in range(N + 1) if not s >> j & 1]
    if not ins or not outs:
        return []
    E = lambda i, o: (min(i, o), max(i, o))
    if N == 2:
        els = [[E(i, o) for i in ins for o in outs]]
    elif len(ins) == 2:
        a, b = ins
        c, d = outs
        els = [[E(a, c), E(a, d), E(b, d)], [E(a, c), E(b, d), E(b, c)]]
    else:
        els = [[E(i, o) for i in ins for o in outs]]
    if (s in FLIP[N]) != odd:
        els = [e[:-2] + [e[-1], e[-2]] for e in els]
    return [tuple(e) for e in els]


def _shift(arr, m, n_out):
    """arr[I + m] for I over an index box of shape n_out"""
    return arr[tuple(slice((m >> a) & 1, ((m >> a) & 1) + n_out[a]) for a in range(arr.ndim))]


def active_cells(shape, mask=None):
    nc = tuple(k - 1 for k in shape)
    act = np.ones(nc, dtype=bool)
    if mask is not None:
        for m in range(1 << len(shape)):
            act &= _shift(np.asarray(mask, dtype=bool), m, nc)
    return act


def edge_masks(vals, level=0.0, mask=None):
    """per node: bit d − 1 set where edge (I, d) carries a vertex (uint8, shape of vals)"""
    v = np.asarray(vals)
    N, n = v.ndim, v.shape
    inside = v.astype(np.float64) < level
    act = active_cells(n, mask)
    cap = np.zeros(tuple(k + 1 for k in n), dtype=bool)        # cap[C + 1] = active(C), False outside the cell range
    cap[tuple(slice(1, k) for k in n)] = act
    em = np.zeros(n, dtype=np.uint8)
    for d in range(1, 1 << N):
        box = tuple(n[a] - ((d >> a) & 1) for a in range(N))   # the I with I + d in the grid
        chg = _shift(inside, 0, box) != _shift(inside, d, box)
        cover = np.zeros(box, dtype=bool)
        for mp in range(1 << N):
            if mp & d:
                continue
            # cell I − m': cap index I + 1 − m'
            cover |= cap[tuple(slice(1 - ((mp >> a) & 1), 1 - ((mp >> a) & 1) + box[a]) for a in range(N))]
        em[tuple(slice(0, b) for b in box)] |= ((chg & cover).astype(np.uint8) << (d - 1)).astype(np.uint8)
    return em


_POP = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def isosurface(vals, lc, hc, level=0.0, mask=None):
    """(vertices (nv, N) float64, elements (ne, N) int64) of the field `vals` (shape n, any float type) on [lc, hc]"""
    v = np.asarray(vals).astype(np.float64)
    N, n = v.ndim, v.shape
    assert N in (2, 3)
    lc = np.asarray(lc, dtype=np.float64)
    h = (np.asarray(hc, dtype=np.float64) - lc) / (np.array(n, dtype=np.float64) - 1.0)
    level = float(level)
    inside = v < level
    em = edge_masks(v, level, mask)
    emf = em.reshape(-1, order="F")
    vbase = np.concatenate([[0], np.cumsum(_POP[emf])])
    nv = int(vbase[-1])
    strides = np.cumprod((1,) + n[:-1]).astype(np.int64)
    lin = np.arange(emf.size, dtype=np.int64)
    idx = [(lin // strides[a]) % n[a] for a in range(N)]
    verts = np.zeros((nv, N), dtype=np.float64)
    vf = v.reshape(-1, order="F")
    with np.errstate(all="ignore"):
        for d in range(1, 1 << N):
            sel = np.nonzero(emf >> (d - 1) & 1)[0]
            if not sel.size:
                continue
            vid = vbase[sel] + _POP[emf[sel] & ((1 << (d - 1)) - 1)]
            pa = vf[sel]
            pb = vf[sel + sum(int(strides[a]) for a in range(N) if d >> a & 1)]
            t = (level - pa) / (pb - pa)
            for e in range(N):
                x = lc[e] + idx[e][sel].astype(np.float64) * h[e]
                verts[vid, e] = x + t * h[e] if d >> e & 1 else x
    # elements
    nc = tuple(k - 1 for k in n)
    act = active_cells(n, mask)
    cin = [_shift(inside, m, nc) for m in range(1 << N)]                      # inside flags of every cell's corners
    clin = np.zeros(nc, dtype=np.int64)                                       # node index of every cell's anchor
    for a in range(N):
        clin += np.arange(nc[a], dtype=np.int64).reshape([-1 if b == a else 1 for b in range(N)]) * strides[a]
    simp = simplices(N)
    pats = []
    cnt = np.zeros(nc + (len(simp),), dtype=np.int64)
    nel = np.array([len(pattern_elements(N, s, False)) for s in range(1 << (N + 1))], dtype=np.int64)
    for p, (chain, _) in enumerate(simp):
        s = np.zeros(nc, dtype=np.int64)
        for j, m in enumerate(chain):
            s |= cin[m].astype(np.int64) << j
        s[~act] = 0
        pats.append(s)
        cnt[..., p] = nel[s]
    # order: cells ascending (axis 0 fastest), then simplices
    order_cnt = np.stack([cnt[..., p].reshape(-1, order="F") for p in range(len(simp))], axis=1)
    off = np.concatenate([[0], np.cumsum(order_cnt.reshape(-1))])
    ne = int(off[-1])
    off = off[:-1].reshape(order_cnt.shape)
    elems = np.zeros((ne, N), dtype=np.int64)
    clf = clin.reshape(-1, order="F")
    for p, (chain, odd) in enumerate(simp):
        sf = pats[p].reshape(-1, order="F")
        for s in range(1, (1 << (N + 1)) - 1):
            cells = np.nonzero(sf == s)[0]
            if not cells.size:
                continue
            for t, el in enumerate(pattern_elements(N, s, odd)):
                for c, (j, k) in enumerate(el):
                    mj, d = chain[j], chain[k] ^ chain[j]
                    node = clf[cells] + sum(int(strides[a]) for a in range(N) if mj >> a & 1)
                    assert np.all(emf[node] >> (d - 1) & 1)
                    elems[off[cells, p] + t, c] = vbase[node] + _POP[emf[node] & ((1 << (d - 1)) - 1)]
    return verts, elems


def measure(verts, elems):
    """total length (2-D) or area (3-D)"""
    if not len(elems):
        return 0.0
    p = verts[elems]
    if verts.shape[1] == 2:
        return float(np.hypot(*(p[:, 1] - p[:, 0]).T).sum())
    return float(0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1).sum())


def enclosed(verts, elems):
    """signed enclosed area (2-D, shoelace) or volume (3-D, Σ v0·(v1 × v2)/6) of a closed mesh"""
    p = verts[elems]
    if verts.shape[1] == 2:
        return float(0.5 * (p[:, 0, 0] * p[:, 1, 1] - p[:, 1, 0] * p[:, 0, 1]).sum())
    return float((p[:, 0] * np.cross(p[:, 1], p[:, 2])).sum() / 6.0)
