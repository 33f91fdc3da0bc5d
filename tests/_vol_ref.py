"""numpy restatement of volume_mesh(ϕ, level) (csrc/lsm_vol.hip): the body-fitted simplicial mesh of {ϕ < level}, obtained by
splitting every simplex of the Freudenthal (Kuhn) subdivision that the level crosses — the first phase of
mmg2d_O3 / mmg3d_O3 -ls, without the remesher.  The device is tested against this file; tests/test_volume_mesh_host.py checks
this file against facts that do not come from it.  Dense fields, 2-D and 3-D.  The rules (those of tests/_iso_ref.py, and):
  * inside(I) := ϕ[I] < level (ϕ == level and NaN are outside); float32 values widen exactly, all arithmetic is fp64;
  * node I (ascending, axis 0 fastest) owns, in this order, itself if inside(I), at lc + i·h, and the cut vertices of its edges
    (I, d) by ascending direction mask d, exactly as isosurface defines them;
  * cells ascending, simplices in _iso_ref.simplices(N) order; with a < b < … the inside and c < d the outside corners by chain
    position and xy the cut vertex on the edge between chain corners x and y, a simplex gives
      all inside: itself;   none inside: nothing;
      2-D, k = 1: (a, ac, ad);                     2-D, k = 2: (a, b, bc), (a, bc, ac);
      3-D, k = 1: (a, ab', ac', ad') over the outside corners in chain order;
      3-D, k = 2: the prism u = (a, ac, ad), w = (b, bc, bd);      3-D, k = 3: the prism u = (a, b, c), w = (ad, bd, cd);
    a prism is cut as (u0, u1, u2, w2), (u0, u1, w1, w2), (u0, w0, w1, w2): the diagonal of a quad in a simplex face starts at
    the lower inside corner, so neighbours agree, and the interface quad is cut along ac–bd as isosurface cuts it;
  * the last two vertices of an element are swapped when SWAP[(sign pattern, sub-element)] xor (π odd): every signed volume
    det[v1 − v0, …] is >= 0, by a table and never a geometric test, so zero-volume elements are oriented too;
  * the interface elements are isosurface's, in its order and orientation, in this mesh's vertex numbering."""
import numpy as np

import _iso_ref as R

# (sign pattern, sub-element) whose canonical element has a negative signed volume on an even permutation; pattern bit j = chain
# corner j inside.  tests/test_volume_mesh_host.py derives this table again from random fields.
SWAP = {
    2: frozenset(((2, 0), (5, 0), (5, 1))),
    3: frozenset(((2, 0), (3, 1), (5, 0), (5, 2), (6, 1), (7, 1), (8, 0), (9, 1), (10, 0), (10, 2), (11, 0), (11, 2), (12, 1), (13, 1),
                  (14, 0), (14, 2))),
}
NO_SWAP = {2: frozenset(), 3: frozenset()}


def pattern_subelements(N, s):
    """the canonical sub-elements of a simplex with sign pattern s: tuples of vertices, a vertex being a chain position j (the
    node) or an edge (j, k), j < k (its cut vertex)"""
    ins = [j for j in range(N + 1) if s >> j & 1]
    outs = [j for j in range(N + 1) if not s >> j & 1]
    if not ins:
        return []
    if not outs:
        return [tuple(range(N + 1))]
    E = lambda i, o: (min(i, o), max(i, o))
    if N == 2:
        if len(ins) == 1:
            a, (c, d) = ins[0], outs
            return [(a, E(a, c), E(a, d))]
        (a, b), c = ins, outs[0]
        return [(a, b, E(b, c)), (a, E(b, c), E(a, c))]
    if len(ins) == 1:
        a = ins[0]
        return [(a,) + tuple(E(a, o) for o in outs)]
    if len(ins) == 2:
        (a, b), (c, d) = ins, outs
        u, w = (a, E(a, c), E(a, d)), (b, E(b, c), E(b, d))
    else:
        (a, b, c), d = ins, outs[0]
        u, w = (a, b, c), (E(a, d), E(b, d), E(c, d))
    return [(u[0], u[1], u[2], w[2]), (u[0], u[1], w[1], w[2]), (u[0], w[0], w[1], w[2])]


def pattern_elements(N, s, odd, swap=SWAP):
    """pattern_subelements with the orientation rule applied"""
    out = []
    for t, el in enumerate(pattern_subelements(N, s)):
        if ((s, t) in swap[N]) != odd:
            el = el[:-2] + (el[-1], el[-2])
        out.append(el)
    return out


def volume_mesh(vals, lc, hc, level=0.0, swap=SWAP, keys=False):
    """(vertices (nv, N) float64, elements (ne, N + 1) int64, interface (ni, N) int64) of the field `vals` (shape n, any float
    type) on [lc, hc]; keys = True appends an (ne, 3) array of (simplex, sign pattern, sub-element) per element"""
    v = np.asarray(vals).astype(np.float64)
    N, n = v.ndim, v.shape
    assert N in (2, 3)
    lc = np.asarray(lc, dtype=np.float64)
    h = (np.asarray(hc, dtype=np.float64) - lc) / (np.array(n, dtype=np.float64) - 1.0)
    level = float(level)
    inside = v < level
    insf = inside.reshape(-1, order="F").astype(np.int64)
    emf = R.edge_masks(v, level).reshape(-1, order="F")
    vbase = np.concatenate([[0], np.cumsum(insf + R._POP[emf])])
    nv = int(vbase[-1])
    strides = np.cumprod((1,) + n[:-1]).astype(np.int64)
    # vertices: the inside nodes, and isosurface's vertices (same order: ascending node, then ascending d) in the gaps
    iv, ie = R.isosurface(v, lc, hc, level)
    nodes = np.nonzero(insf)[0]
    node_id = vbase[nodes]
    is_cut = np.ones(nv, dtype=bool)
    is_cut[node_id] = False
    cut_id = np.nonzero(is_cut)[0]
    assert len(cut_id) == len(iv)
    verts = np.zeros((nv, N), dtype=np.float64)
    for e in range(N):
        verts[node_id, e] = lc[e] + ((nodes // strides[e]) % n[e]).astype(np.float64) * h[e]
    verts[cut_id] = iv
    interface = cut_id[ie] if len(ie) else np.zeros((0, N), dtype=np.int64)
    # elements
    nc = tuple(k - 1 for k in n)
    cin = [R._shift(inside, m, nc) for m in range(1 << N)]
    clin = np.zeros(nc, dtype=np.int64)
    for a in range(N):
        clin += np.arange(nc[a], dtype=np.int64).reshape([-1 if b == a else 1 for b in range(N)]) * strides[a]
    clf = clin.reshape(-1, order="F")
    simp = R.simplices(N)
    nel = np.array([len(pattern_subelements(N, s)) for s in range(1 << (N + 1))], dtype=np.int64)
    pats = []
    for chain, _ in simp:
        s = np.zeros(nc, dtype=np.int64)
        for j, m in enumerate(chain):
            s |= cin[m].astype(np.int64) << j
        pats.append(s.reshape(-1, order="F"))
    cnt = np.stack([nel[s] for s in pats], axis=1)                 # (cells, simplices): cells ascending, then simplices
    off = np.concatenate([[0], np.cumsum(cnt.reshape(-1))])
    ne = int(off[-1])
    off = off[:-1].reshape(cnt.shape)
    elems = np.zeros((ne, N + 1), dtype=np.int64)
    key = np.zeros((ne, 3), dtype=np.int64)
    for p, (chain, odd) in enumerate(simp):
        for s in range(1, 1 << (N + 1)):
            cells = np.nonzero(pats[p] == s)[0]
            if not cells.size:
                continue
            for t, el in enumerate(pattern_elements(N, s, odd, swap)):
                key[off[cells, p] + t] = (p, s, t)
                for c, vert in enumerate(el):
                    j, k = vert if isinstance(vert, tuple) else (vert, None)
                    node = clf[cells] + sum(int(strides[a]) for a in range(N) if chain[j] >> a & 1)
                    if k is None:
                        assert insf[node].all()
                        elems[off[cells, p] + t, c] = vbase[node]
                    else:
                        d = chain[k] ^ chain[j]
                        assert np.all(emf[node] >> (d - 1) & 1)
                        elems[off[cells, p] + t, c] = vbase[node] + insf[node] + R._POP[emf[node] & ((1 << (d - 1)) - 1)]
    return (verts, elems, interface, key) if keys else (verts, elems, interface)


def signed_volumes(verts, elems):
    """det[v1 − v0, …, vN − v0] / N! per element"""
    N = verts.shape[1]
    if not len(elems):
        return np.zeros(0)
    p = verts[elems]
    d = p[:, 1:] - p[:, :1]
    if N == 2:
        return 0.5 * (d[:, 0, 0] * d[:, 1, 1] - d[:, 0, 1] * d[:, 1, 0])
    return (d[:, 0] * np.cross(d[:, 1], d[:, 2])).sum(axis=1) / 6.0


def measure(verts, elems):
    """Σ signed element volumes (areas in 2-D)"""
    return float(signed_volumes(verts, elems).sum())
