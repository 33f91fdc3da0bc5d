"""The march line of the 3-D WENO5 kernels as a ring of first differences (csrc/stage_kernel.h, LSM_ZD) against the ring of
values it replaces, as NumPy models of one thread's column.

The value ring holds ϕ(m-3 … m+3) and forms the line's five differences every plane.  The difference ring holds the six
intervals I(j) = ϕ(j+1) - ϕ(j), j = m-3 … m+2, in seven register slots — I(m+k) in slot (R + 3 + k) mod 7, R the rotation of the
7-fold unrolled loop — plus the last value loaded; a plane forms one new interval, nxt - last, over the slot no plane reads
any more, and takes its centre value from the LDS slot R, which was written four planes earlier.  The model below follows the
kernel's mechanics: the prologue's seven loads, the plane pointer that stops advancing at a clamped face (so the repeated
plane gives an interval of exactly 0), the slot indices, chunk seams, and a stencil direction that flips at arbitrary planes
(the flipped line reads the negated intervals in reverse).  Both rings must give the SAME five differences — the same
subtraction of the same two values, up to the sign of a zero — and therefore the same line value in the float64 model of
weno5_undivided_pq (tests/test_weno_forms_algebra.py).
"""
import numpy as np
import pytest

from test_gpu_weno_forms import _fields
from test_weno_forms_algebra import _fma, _r_new_f64

G = 3
RN = 2 * G + 1


def _weno5_model(e):
    """weno5_undivided_pq<PQ, X3 = true> in float64, from the smoothness model of test_weno_forms_algebra (the reciprocal exact)."""
    e = [float(x) for x in e]
    w = [e[k + 1] - e[k] for k in range(4)]
    A = [w[1] - w[0], w[2] - w[1], w[3] - w[2]]
    m = max(abs(x) for x in e)
    r = _r_new_f64(w, A, _fma(0.75e-6 * m, m, (13.0 / 16) * 1e-75))
    s = [x * x for x in r]
    N = s[1] * _fma(1.5, s[0] * (A[1] - A[2]), s[2] * (A[0] - A[1]))
    Dn = _fma(6.0, s[0] * s[2], s[1] * _fma(3.0, s[0], s[2]))
    return _fma(1.0 / Dn, N, _fma(0.5, w[1], _fma(3.0, e[2], w[2])))


class Column:
    """ϕ along the march axis with `ghost` planes on either side; mlo/mhi: the planes the march clamps at (a NeumannBC face
    clamps at the boundary plane and never reads its ghosts)."""

    def __init__(self, phi, ghost, clamp_lo, clamp_hi):
        self.n = len(phi)
        self.pad = np.concatenate([ghost[0], phi, ghost[1]])
        self.mlo = 0 if clamp_lo else -G
        self.mhi = self.n - 1 if clamp_hi else self.n + G - 1

    def clamp(self, p):
        return min(max(p, self.mlo), self.mhi)

    def at(self, p):                       # a load from plane p (already clamped)
        assert self.mlo <= p <= self.mhi
        return float(self.pad[p + G])


def _value_ring(col, m0, m1, flip):
    """Today's ring: values; returns per plane (c, e1..e5)."""
    out = []
    zl = [col.at(col.clamp(m0 - G + j)) for j in range(RN)]
    p = col.clamp(m0 + G)
    for m in range(m0, m1):
        R = (m - m0) % RN
        z = lambda k: zl[(R + G + k) % RN]
        ss = -1 if flip[m] else 1
        c = z(0)
        e = (z(-2 * ss) - z(-3 * ss), z(-ss) - z(-2 * ss), c - z(-ss), z(ss) - c, z(2 * ss) - z(ss))
        out.append((c, e))
        p = p + 1 if m + 1 + G <= col.mhi else p
        zl[R % RN] = col.at(p)
    return out


def _difference_ring(col, m0, m1, flip):
    """LSM_ZD: six intervals + the last value in registers, centre values in seven LDS slots."""
    out = []
    zl = [col.at(col.clamp(m0 - G + j)) for j in range(RN)]
    lds = [None] * RN
    for s in range(G + 1):
        lds[s] = zl[G + s]                                  # prologue: the centres of planes m0 … m0+G
    dz = [zl[j + 1] - zl[j] for j in range(2 * G)] + [None]
    last = zl[2 * G]
    p = col.clamp(m0 + G)
    for m in range(m0, m1):
        R = (m - m0) % RN
        I = lambda k: dz[(R + G + k) % RN]
        c = lds[R]
        if not flip[m]:
            e = (I(-3), I(-2), I(-1), I(0), I(1))
        else:
            e = (-I(2), -I(1), -I(0), -I(-1), -I(-2))
        assert all(x is not None for x in e) and c is not None
        out.append((c, e))
        p = p + 1 if m + 1 + G <= col.mhi else p
        nxt = col.at(p)
        dz[(R + 2 * G) % RN] = nxt - last                   # the entry of I(m-3) is the next iteration's free one
        last = nxt
        lds[(R + G + 1) % RN] = nxt                         # last read at iteration m-3
    return out


def _chunks(n, mc):
    return [(a, min(a + mc, n)) for a in range(0, n, mc)]


def _columns(nz):
    """Columns of the stress fields of test_gpu_weno_forms along the march axis, with ghost planes of another field."""
    shape = (6, 5, nz)
    fields = _fields(shape)
    rng = np.random.default_rng(5)
    for name, f in fields.items():
        for (i, j) in ((0, 0), (3, 2), (5, 4), (2, 1)):
            col = np.ascontiguousarray(f[i, j, :])
            scale = max(np.abs(col).max(), 1e-300)
            ghosts = (scale * rng.standard_normal(G), scale * rng.standard_normal(G))
            yield name, col, ghosts


@pytest.mark.parametrize("nz", [2, 5, 7, 8, 13, 15, 45])
def test_difference_ring_gives_the_value_rings_line_bitwise(nz):
    rng = np.random.default_rng(nz)
    lines = 0
    for name, phi, ghosts in _columns(nz):
        for clamp_lo, clamp_hi in ((True, True), (False, False), (True, False)):
            col = Column(phi, ghosts, clamp_lo, clamp_hi)
            flips = [np.zeros(nz, bool), np.ones(nz, bool), rng.random(nz) < 0.5, np.arange(nz) % 2 == 0]
            for flip in flips:
                for mc in (nz, 4, 16):
                    if mc > nz and mc != 4:
                        continue
                    for m0, m1 in _chunks(nz, mc):
                        a = _value_ring(col, m0, m1, flip)
                        b = _difference_ring(col, m0, m1, flip)
                        assert len(a) == len(b) == m1 - m0
                        for k, ((ca, ea), (cb, eb)) in enumerate(zip(a, b)):
                            m = m0 + k
                            assert ca == cb == phi[m], (name, m)
                            assert np.array_equal(np.array(ea), np.array(eb)), (name, m, ea, eb)
                            if clamp_lo and m <= 1:
                                assert ea[0] == 0.0 or flip[m]      # the repeated boundary plane: an interval of exactly 0
                            # the line value in the float64 model (every seventh line: the model's FMAs are exact rationals)
                            if lines % 7 == 0:
                                wa, wb = _weno5_model(ea), _weno5_model(eb)
                                assert wa == wb, (name, m, wa, wb)
                            lines += 1
    assert lines > 0


def test_clamped_face_intervals_are_exact_zeros():
    """NeumannBC on both faces of a column shorter than the ring: every interval that reaches past a face is +0."""
    phi = np.array([0.3, -0.7])
    col = Column(phi, (np.full(G, np.nan), np.full(G, np.nan)), True, True)       # the ghosts are never read
    (c0, e0), (c1, e1) = _difference_ring(col, 0, 2, np.zeros(2, bool))
    assert (c0, c1) == (0.3, -0.7)
    assert e0 == (0.0, 0.0, 0.0, -1.0, 0.0) and e1 == (0.0, 0.0, -1.0, 0.0, 0.0)
    assert not any(np.signbit(x) for x in e0 + e1 if x == 0.0)
