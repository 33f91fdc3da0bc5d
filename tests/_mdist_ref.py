"""numpy restatement of mesh_distance (csrc/lsm_mdist.hip): the signed distance ϕ[I] = s(I)·min(d(I), c) from every grid node to a
closed, consistently oriented mesh (segments in 2-D, triangles in 3-D, oriented as InterfaceMesh documents), brute force: every
element against every node.  The device is tested against this file bit for bit; tests/test_mesh_distance_host.py
checks this file against facts that do not come from it.  Every expression below is written with the operation order the kernels
use (csrc is built with -ffp-contract=off: one rounding per operation, as numpy does).  The rules:
  * node I sits at x_a = lc_a + I_a·h_a, h = (hc − lc)/(n − 1);
  * d²(I) = min over the elements of the squared distance to the closest point of the element; the closest point by the region
    classification of Ericson (Real-Time Collision Detection §5.1.5: vertex a, vertex b, edge ab, vertex c, edge ac, edge bc,
    interior, in that priority) in 3-D, by the clamped projection on the segment in 2-D; a NaN (an element of zero size that
    reaches a division) never wins the minimum;
  * the sign is a crossing count along axis 0, independent of the closest feature.  A grid line (j[, k]) hits an element iff its
    (y[, z]) lies in the element's projection, counted half-open: 2-D, segment a→b: (a_y > y) != (b_y > y); 3-D: the projected
    triangle is made counter-clockwise (A2 < 0: vertices 1 and 2 swapped), every edge function is evaluated from the edge's
    vertex with the lower vertex number, (hi − lo) × (p − lo), and negated when the triangle traverses the edge from hi to lo —
    two triangles sharing an edge see the same magnitude — and the point is inside iff every edge function is > 0, or == 0 on an
    edge whose traversal has dz < 0, or dz == 0 and dy < 0 (the top-left rule).  Elements with A2 == 0 (3-D) or Δy == 0 (2-D)
    contribute nothing (they are counted: `skipped`);
  * a hit at ξ (the x of the intersection) adds −σ, σ the sign of the element's outward normal along axis 0, to the flip counter
    of the first node with x_i >= ξ: slot 0 when ξ lies left of the grid, slot n0 (part of no node's count) when right of it;
  * the winding count of node i is the sum of the slots 0..i of its line; s = −1 where it is non-zero, +1 elsewhere; a line whose
    n0 + 1 slots do not sum to zero is unbalanced (the mesh is open, or not consistently oriented, as seen from that line);
  * ϕ = s·sqrt(min(d², c²)): nodes farther than the cutoff carry ±sqrt(c·c)."""
import numpy as np


def axes(n, lc, hc):
    lc = np.asarray(lc, dtype=np.float64)
    h = (np.asarray(hc, dtype=np.float64) - lc) / (np.array(n, dtype=np.float64) - 1.0)
    return [lc[a] + np.arange(n[a]).astype(np.float64) * h[a] for a in range(len(n))], h


def _dot3(ux, uy, uz, vx, vy, vz):
    return (ux * vx + uy * vy) + uz * vz


def _tri_dist2(p, a, b, c):
    """squared distance of the points p = (px, py, pz) to the triangles (a, b, c); shapes broadcast"""
    px, py, pz = p
    ax, ay, az = a
    bx, by, bz = b
    cx, cy, cz = c
    abx, aby, abz = bx - ax, by - ay, bz - az
    acx, acy, acz = cx - ax, cy - ay, cz - az
    bcx, bcy, bcz = cx - bx, cy - by, cz - bz
    apx, apy, apz = px - ax, py - ay, pz - az
    d1 = _dot3(abx, aby, abz, apx, apy, apz)
    d2 = _dot3(acx, acy, acz, apx, apy, apz)
    bpx, bpy, bpz = px - bx, py - by, pz - bz
    d3 = _dot3(abx, aby, abz, bpx, bpy, bpz)
    d4 = _dot3(acx, acy, acz, bpx, bpy, bpz)
    cpx, cpy, cpz = px - cx, py - cy, pz - cz
    d5 = _dot3(abx, aby, abz, cpx, cpy, cpz)
    d6 = _dot3(acx, acy, acz, cpx, cpy, cpz)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    # interior
    den = (va + vb) + vc
    v, w = vb / den, vc / den
    r = [px - ((ax + v * abx) + w * acx), py - ((ay + v * aby) + w * acy), pz - ((az + v * abz) + w * acz)]

    def take(cond, q):
        for e in range(3):
            r[e] = np.where(cond, q[e], r[e])

    # lowest priority first: a later take overrides
    e43, e56 = d4 - d3, d5 - d6
    w = e43 / (e43 + e56)
    take((va <= 0) & (e43 >= 0) & (e56 >= 0), (px - (bx + w * bcx), py - (by + w * bcy), pz - (bz + w * bcz)))
    w = d2 / (d2 - d6)
    take((vb <= 0) & (d2 >= 0) & (d6 <= 0), (px - (ax + w * acx), py - (ay + w * acy), pz - (az + w * acz)))
    take((d6 >= 0) & (d5 <= d6), (cpx, cpy, cpz))
    v = d1 / (d1 - d3)
    take((vc <= 0) & (d1 >= 0) & (d3 <= 0), (px - (ax + v * abx), py - (ay + v * aby), pz - (az + v * abz)))
    take((d3 >= 0) & (d4 <= d3), (bpx, bpy, bpz))
    take((d1 <= 0) & (d2 <= 0), (apx, apy, apz))
    return (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]


def _seg_dist2(p, a, b):
    px, py = p
    ax, ay = a
    bx, by = b
    abx, aby = bx - ax, by - ay
    apx, apy = px - ax, py - ay
    t = abx * apx + aby * apy
    den = abx * abx + aby * aby
    u = t / den
    rx, ry = px - (ax + u * abx), py - (ay + u * aby)
    B = t >= den
    rx, ry = np.where(B, px - bx, rx), np.where(B, py - by, ry)
    A = t <= 0
    rx, ry = np.where(A, apx, rx), np.where(A, apy, ry)
    return rx * rx + ry * ry


def dist2(verts, elems, n, lc, hc, chunk=128, cull=True):
    """min over the elements of d² at every node: an array of shape n (inf without elements).  cull=False is the plain brute
    force, every element against every node.  cull=True gives the same bits in a fraction of the time: a pair (node, element) is
    skipped only when it cannot win — the node is farther from the element's bounding ball than from the nearest mesh vertex
    (which belongs to some element), with a relative margin of 1e-9 for the roundings; the pairs that remain go through the same
    expressions"""
    verts = np.asarray(verts, dtype=np.float64)
    elems = np.asarray(elems, dtype=np.int64)
    N = len(n)
    xs, _ = axes(n, lc, hc)
    P = [g.reshape(-1) for g in np.meshgrid(*xs, indexing="ij")]
    out = np.full(P[0].shape[0], np.inf)
    fn = _tri_dist2 if N == 3 else _seg_dist2
    with np.errstate(all="ignore"):
        if cull and len(elems):
            ub = np.full(P[0].shape[0], np.inf)
            used = verts[np.unique(elems)]
            for s in range(0, len(used), 4 * chunk):
                ub = np.minimum(ub, sum((P[d][:, None] - used[None, s:s + 4 * chunk, d]) ** 2 for d in range(N)).min(axis=1))
            reach = np.sqrt(ub)[:, None]
        for s in range(0, len(elems), chunk):
            pv = verts[elems[s:s + chunk]]                      # (E, N, N)
            if cull:
                cen = pv.mean(axis=1)
                rad = np.sqrt(((pv - cen[:, None, :]) ** 2).sum(axis=2)).max(axis=1)
                far = np.sqrt(sum((P[d][:, None] - cen[None, :, d]) ** 2 for d in range(N)))
                ni, ei = np.nonzero(far <= (reach + rad[None, :]) * (1 + 1e-9))
                d = fn([P[d][ni] for d in range(N)], *[[pv[ei, k, d] for d in range(N)] for k in range(N)])
                np.fmin.at(out, ni, d)                          # a NaN never wins
            else:
                V = [[pv[:, k, d].reshape(1, -1) for d in range(N)] for k in range(N)]
                out = np.fmin(out, np.fmin.reduce(fn([g.reshape(-1, 1) for g in P], *V), axis=1))
    return out.reshape(n)


def flips(verts, elems, n, lc, hc, chunk=256):
    """(flip counters of shape (n0 + 1, n1[, n2]) int64, elements skipped as degenerate in projection)"""
    verts = np.asarray(verts, dtype=np.float64)
    elems = np.asarray(elems, dtype=np.int64)
    N = len(n)
    xs, _ = axes(n, lc, hc)
    F = np.zeros((n[0] + 1,) + tuple(n[1:]), dtype=np.int64)
    skipped = 0
    with np.errstate(all="ignore"):
        for s in range(0, len(elems), chunk):
            g = elems[s:s + chunk]
            p = verts[g]                                   # (E, N, N)
            if N == 2:
                a, b = p[:, 0], p[:, 1]
                keep = a[:, 1] != b[:, 1]
                skipped += int((~keep).sum())
                a, b = a[keep], b[keep]
                y = xs[1].reshape(1, -1)
                ax, ay, bx, by = (c.reshape(-1, 1) for c in (a[:, 0], a[:, 1], b[:, 0], b[:, 1]))
                hit = (ay > y) != (by > y)
                xi = ax + ((y - ay) / (by - ay)) * (bx - ax)
                sigma = np.where(by > ay, 1, -1) + 0 * hit
                line = (np.arange(n[1]).reshape(1, -1) + 0 * hit,)
            else:
                A2 = (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 2] - p[:, 0, 2]) - (p[:, 1, 2] - p[:, 0, 2]) * (p[:, 2, 1] - p[:, 0, 1])
                keep = A2 != 0
                skipped += int((~keep).sum())
                g, p, A2 = g[keep], p[keep], A2[keep]
                swap = A2 < 0
                g = np.where(swap[:, None], g[:, [0, 2, 1]], g)
                p = np.where(swap[:, None, None], p[:, [0, 2, 1]], p)
                py, pz = xs[1].reshape(1, -1, 1), xs[2].reshape(1, 1, -1)
                E = []
                hit = True
                for i in range(3):
                    k = (i + 1) % 3
                    fwd = (g[:, i] < g[:, k]).reshape(-1, 1, 1)
                    cy, cz, ny, nz = (c.reshape(-1, 1, 1) for c in (p[:, i, 1], p[:, i, 2], p[:, k, 1], p[:, k, 2]))
                    loy, loz = np.where(fwd, cy, ny), np.where(fwd, cz, nz)
                    hiy, hiz = np.where(fwd, ny, cy), np.where(fwd, nz, cz)
                    Ec = (hiy - loy) * (pz - loz) - (hiz - loz) * (py - loy)
                    Ei = np.where(fwd, Ec, -Ec)
                    topleft = (nz < cz) | ((nz == cz) & (ny < cy))
                    hit = hit & ((Ei > 0) | ((Ei == 0) & topleft))
                    E.append(Ei)
                x0, x1, x2 = (p[:, i, 0].reshape(-1, 1, 1) for i in range(3))
                w0, w1, w2 = E[1], E[2], E[0]
                xi = ((w0 * x0 + w1 * x1) + w2 * x2) / ((w0 + w1) + w2)
                sigma = np.where(A2 > 0, 1, -1).reshape(-1, 1, 1) + 0 * hit
                line = (np.arange(n[1]).reshape(1, -1, 1) + 0 * hit, np.arange(n[2]).reshape(1, 1, -1) + 0 * hit)
            i0 = np.searchsorted(xs[0], xi[hit], side="left")      # the first node with x_i >= ξ; n0 when there is none
            np.add.at(F, (i0,) + tuple(ln[hit] for ln in line), -sigma[hit])
    return F, skipped


def winding(F):
    """(winding count of every node, total of every line)"""
    return np.cumsum(F[:-1], axis=0), F.sum(axis=0)


def mesh_distance(verts, elems, n, lc, hc, cutoff=np.inf, d2=None, F=None):
    """(ϕ of shape n float64, (nodes with d < c, unbalanced lines, elements skipped by the sign pass)); d2, F: dist2's and
    flips' results when the caller already has them"""
    d2 = dist2(verts, elems, n, lc, hc) if d2 is None else d2
    F, skipped = flips(verts, elems, n, lc, hc) if F is None else F
    W, tot = winding(F)
    c = np.float64(cutoff)
    c2 = c * c
    m = np.where(d2 < c2, d2, c2)
    phi = np.where(W != 0, -1.0, 1.0) * np.sqrt(m)
    return phi, (int((d2 < c2).sum()), int((tot != 0).sum()), int(skipped))
