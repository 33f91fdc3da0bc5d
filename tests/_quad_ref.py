"""TEST-ONLY restatement (numpy, Python loops: small grids only) of the cut-cell quadrature the device computes
(csrc/lsm_quad.hip): LevelSetMethods.quadrature (src/LevelSetMethods.jl:103-126, ext/ImplicitIntegrationExt.jl), built on
R. Saye, "High-order quadrature methods for implicitly defined surfaces and volumes in hyperrectangles", SIAM J. Sci.
Comput. 37(2), 2015, over the Bernstein patches of tests/_reinit_ref.py (ReinitRef.coeffs).

It is the contract the device is tested against node for node: same height direction, split rule, depth limits, root
iteration and fallback, and the same node order.  Per box, for a list of polynomials (Bernstein coefficients on the box):
  * drop every polynomial whose coefficient bound excludes 0; none left: the tensor rule (base levels, or a volume box
    whose top-level polynomial is negative there), else nothing;
  * 1-D: isolate the roots by Bernstein subdivision (at most ISO_DEPTH halvings), refine each, cut the interval;
  * height direction k = the first arg-max of |∂ψ/∂x_k| at the box centre, ψ the first polynomial left; every
    polynomial must be monotone along k (the bound of its k-difference excludes 0), else the box is halved along its
    first longest side, at most MAX_DEPTH times per level; a box at the limit gets the fallback (counted);
  * the base: the lower and upper k-faces of every polynomial, one dimension down, with no sign condition;
  * on the line through every base node: the roots (one per polynomial at most), then the q-point Gauss–Legendre rule
    on every piece (volume: where ψ < 0 at the piece's midpoint), or the root with weight w·|∇ψ|/|∂ψ/∂x_k| (surface).
Fallbacks: volume, the tensor rule keeping the nodes where ψ < 0; surface, one node per base node of the tensor rule
at the root on its line, if its end values differ in sign; base levels, the tensor rule."""
import itertools

import numpy as np

NONE, VOL, SURF = 0, 1, 2
MAX_DEPTH = 6       # halvings of a box per level (dimension >= 2)
ISO_DEPTH = 16      # halvings of an interval while isolating the roots of a 1-D polynomial
ROOT_ITERS = 64
EPS = float(np.finfo(float).eps)


def gauss01(q):
    x, w = np.polynomial.legendre.leggauss(q)
    return (x + 1.0) / 2.0, w / 2.0


def decas(b, t):
    """value and d/dt of a 1-D Bernstein polynomial at t (de Casteljau)"""
    b = [float(v) for v in b]
    n = len(b) - 1
    s = 1.0 - t
    for r in range(n, 1, -1):
        for i in range(r):
            b[i] = s * b[i] + t * b[i + 1]
    return s * b[0] + t * b[1], n * (b[1] - b[0])


def contract(c, keep, ts):
    """the 1-D polynomial along axis `keep` of c at local parameters ts[j] of the other axes (highest axis first)"""
    r = np.asarray(c, dtype=float)
    for j in range(r.ndim - 1, -1, -1):
        if j == keep:
            continue
        r = np.apply_along_axis(lambda f: decas(f, ts[j])[0], j, r)
    return r


def split(c, d):
    """de Casteljau halving along axis d: (left, right)"""
    b = np.moveaxis(np.array(c, dtype=float), d, 0).copy()
    n = b.shape[0] - 1
    L, R = [b[0].copy()], [b[n].copy()]
    for r in range(n, 0, -1):
        for i in range(r):
            b[i] = 0.5 * (b[i] + b[i + 1])
        L.append(b[0].copy())
        R.append(b[r - 1].copy())
    return np.moveaxis(np.array(L), 0, d), np.moveaxis(np.array(R[::-1]), 0, d)


def excludes0(c):
    return c.min() > 0.0 or c.max() < 0.0


def monotone(c, k):
    d = np.diff(c, axis=k)
    return d.min() > 0.0 or d.max() < 0.0


def root(b):
    """the crossing of the sign (v < 0) of b on [0, 1]: safeguarded Newton–bisection in Bernstein form"""
    s0 = b[0] < 0.0
    lo, hi, t = 0.0, 1.0, 0.5
    for _ in range(ROOT_ITERS):
        f, df = decas(b, t)
        if f == 0.0:
            return t
        if (f < 0.0) == s0:
            lo = t
        else:
            hi = t
        tn = t - f / df if df != 0.0 else -1.0
        if not (lo < tn < hi):
            tn = 0.5 * (lo + hi)
        if abs(tn - t) <= 4.0 * EPS:
            return tn
        t = tn
    return t


def isolate(b, out, t0=0.0, t1=1.0, depth=0):
    b = np.asarray(b, dtype=float)
    neg = b < 0.0
    if neg.all() or not neg.any():
        return
    d = np.diff(b)
    if d.min() > 0.0 or d.max() < 0.0 or depth == ISO_DEPTH:
        if (b[0] < 0.0) != (b[-1] < 0.0):
            out.append(t0 + root(b) * (t1 - t0))
        return
    bl, br = split(b, 0)
    tm = 0.5 * (t0 + t1)
    isolate(bl, out, t0, tm, depth + 1)
    isolate(br, out, tm, t1, depth + 1)


class QuadRef:
    def __init__(self, q):
        self.q = q
        self.gx, self.gw = gauss01(q)
        self.nfallback = 0

    # ---- helpers on a box [lo, hi]
    @staticmethod
    def _local(y, lo, hi, k):
        """local parameters of the base point y (coordinates of the axes != k) on the box, indexed by axis"""
        ts, m = [0.0] * len(lo), 0
        for j in range(len(lo)):
            if j == k:
                continue
            ts[j] = (y[m] - lo[j]) / (hi[j] - lo[j])
            m += 1
        return ts

    def _grad(self, c, ts, lo, hi):
        return [decas(contract(c, j, ts), ts[j])[1] / (hi[j] - lo[j]) for j in range(len(lo))]

    def _pieces(self, roots, y, wy, lo, hi, k, psi=None, ts=None):
        """Gauss–Legendre nodes on the pieces of the line cut at `roots`; psi: only the pieces where psi(midpoint) < 0"""
        out = []
        hk = hi[k] - lo[k]
        br = [0.0] + sorted(roots) + [1.0]
        for u, v in zip(br[:-1], br[1:]):
            if not v > u:
                continue
            if psi is not None and not decas(psi, 0.5 * (u + v))[0] < 0.0:
                continue
            for g, w in zip(self.gx, self.gw):
                x = np.insert(np.asarray(y, dtype=float), k, lo[k] + (u + (v - u) * g) * hk)
                out.append((x, wy * ((v - u) * w * hk)))
        return out

    def _surface_node(self, c, b, r, y, wy, lo, hi, k):
        ts = self._local(y, lo, hi, k)
        ts[k] = r
        g = self._grad(c, ts, lo, hi)
        g[k] = decas(b, r)[1] / (hi[k] - lo[k])
        x = np.insert(np.asarray(y, dtype=float), k, lo[k] + r * (hi[k] - lo[k]))
        return x, wy * (np.sqrt(sum(v * v for v in g)) / abs(g[k]))

    def _line(self, P, k, y, wy, lo, hi, mode):
        ts = self._local(y, lo, hi, k)
        lines = [contract(c, k, ts) for c in P]
        roots = [root(b) for b in lines if (b[0] < 0.0) != (b[-1] < 0.0)]
        if mode == SURF:
            return [self._surface_node(P[0], lines[0], r, y, wy, lo, hi, k) for r in roots]
        return self._pieces(roots, y, wy, lo, hi, k, psi=lines[0] if mode == VOL else None)

    def tensor(self, lo, hi):
        D = len(lo)
        if D == 1:
            return self._pieces([], [], 1.0, lo, hi, 0)
        out = []
        for y, wy in self.tensor(lo[:-1], hi[:-1]):
            out += self._pieces([], y, wy, lo, hi, D - 1)
        return out

    def _line1d(self, P, lo, hi, mode):
        roots = []
        for c in P:
            isolate(c, roots)
        if mode == SURF:
            return [(np.array([lo[0] + r * (hi[0] - lo[0])]), 1.0) for r in sorted(roots)]
        return self._pieces(roots, [], 1.0, lo, hi, 0, psi=P[0] if mode == VOL else None)

    def _fallback(self, psi, lo, hi, mode, k):
        D = len(lo)
        if mode == VOL:
            out = []
            for y, wy in self.tensor(lo[:-1], hi[:-1]):
                b = contract(psi, D - 1, self._local(y, lo, hi, D - 1))
                out += [n for n, g in zip(self._pieces([], y, wy, lo, hi, D - 1), self.gx) if decas(b, g)[0] < 0.0]
            return out
        if mode == SURF:
            out = []
            for y, wy in self.tensor(np.delete(lo, k), np.delete(hi, k)):
                b = contract(psi, k, self._local(y, lo, hi, k))
                if (b[0] < 0.0) != (b[-1] < 0.0):
                    out.append(self._surface_node(psi, b, root(b), y, wy, lo, hi, k))
            return out
        return self.tensor(lo, hi)

    def level(self, P, lo, hi, mode, depth=0):
        lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
        D = len(lo)
        top = P[0] if P else None
        P = [c for c in P if not excludes0(c)]
        if not P:
            if mode == NONE or (mode == VOL and top.max() < 0.0):
                return self.tensor(lo, hi)
            return []
        if D == 1:
            return self._line1d(P, lo, hi, mode)
        gc = self._grad(P[0], [0.5] * D, lo, hi)
        k, best = 0, abs(gc[0])
        for j in range(1, D):
            if abs(gc[j]) > best:
                k, best = j, abs(gc[j])
        if all(monotone(c, k) for c in P):
            base = []
            for c in P:
                base += [np.take(c, 0, axis=k), np.take(c, -1, axis=k)]
            out = []
            for y, wy in self.level(base, np.delete(lo, k), np.delete(hi, k), NONE):
                out += self._line(P, k, y, wy, lo, hi, mode)
            return out
        if depth == MAX_DEPTH:
            self.nfallback += 1
            return self._fallback(P[0], lo, hi, mode, k)
        j, best = 0, hi[0] - lo[0]
        for d in range(1, D):
            if hi[d] - lo[d] > best:
                j, best = d, hi[d] - lo[d]
        halves = [split(c, j) for c in P]
        mid = lo[j] + (hi[j] - lo[j]) * 0.5
        hl, lr = hi.copy(), lo.copy()
        hl[j] = lr[j] = mid
        return (self.level([h[0] for h in halves], lo, hl, mode, depth + 1) +
                self.level([h[1] for h in halves], lr, hi, mode, depth + 1))


def quadrature(ref, q, surface=False, cells=None):
    """The quadrature of a ReinitRef's interpolant: ({cut cell: (coords (m, N), weights (m,))}, [full cells], nfallback).
    Cells in ascending linear order (x fastest); `cells` restricts the sweep (a band's active cells)."""
    N = ref.N
    Q = QuadRef(q)
    if cells is None:
        cells = [tuple(I[::-1]) for I in itertools.product(*[range(k - 1) for k in ref.n[::-1]])]
    else:
        cells = sorted(cells, key=lambda I: tuple(I[::-1]))
    cut, full = {}, []
    for I in cells:
        c = ref.coeffs(I)
        m, M = float(c.min()), float(c.max())
        if (m * M > 0.0) if surface else (m > 0.0):
            continue
        if not surface and M < 0.0:
            full.append(I)
            continue
        lo = np.array([ref.lc[d] + I[d] * ref.h[d] for d in range(N)])
        hi = lo + ref.h                      # cell.hc = cell.lc + h (src/meshes.jl)
        nodes = Q.level([c], lo, hi, SURF if surface else VOL)
        if nodes:
            cut[I] = (np.array([x for x, _ in nodes]).reshape(-1, N), np.array([w for _, w in nodes]))
    return cut, full, Q.nfallback


def full_rule(q, N):
    """the tensor rule of a full cell on the unit cell: (coords (q^N, N), weights)"""
    nodes = QuadRef(q).tensor(np.zeros(N), np.ones(N))
    return np.array([x for x, _ in nodes]).reshape(-1, N), np.array([w for _, w in nodes])


def total(ref, q, surface=False, cells=None):
    cut, full, _ = quadrature(ref, q, surface, cells)
    s = sum(float(w.sum()) for _, w in cut.values())
    return s + len(full) * float(np.prod(ref.h))
