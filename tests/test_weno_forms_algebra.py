"""The shortened FAST forms of the WENO5 smoothness terms and weights (csrc/stage_math.h, weno5_undivided_pq) against the
forms they replace and against the reference's _weno5 (src/derivatives.jl:61-81): exact identities in rational
arithmetic, and float64 agreement on inputs chosen to cancel.

Notation of stage_math.h: undivided one-sided differences e1..e5, second differences w_k = e_{k+1} - e_k,
A_k = w_{k+1} - w_k, c = 3/13.
  old  r_k  = A_k² + c·B_k² + (12/13)ε,  B₁ = A₁ + 2w₂, B₂ = w₂ + w₃, B₃ = A₃ - 2w₃
  new  r_k' = A₁² + t₂(A₁ + w₂) + ε',  A₂² + t₂w₃ + ε',  A₃² + t₃(w₃ - A₃) + ε',  t_k = ¾w_k,  ε' = ¾ε
  old  correction = X/den,  X = c₁W₁(A₁-A₂) + c₃W₃(A₂-A₃),  den = 0.1W₁ + 0.6W₂ + 0.3W₃
  new  correction = N/(3Dn),  N = s₂(1.5 s₁(A₂-A₃) + s₃(A₁-A₂)),  Dn = 6s₁s₃ + s₂(3s₁ + s₃),  s_k = r_k'²
"""
import math
import random
from fractions import Fraction as Fr

import numpy as np
import pytest

C = Fr(3, 13)


def _diffs(e):
    w = [e[k + 1] - e[k] for k in range(4)]
    A = [w[k + 1] - w[k] for k in range(3)]
    return w, A


def _r_old(w, A, eps):
    """eps: the reference's ε (1e-6·m² + floor)."""
    B = [A[0] + 2 * w[1], w[1] + w[2], A[2] - 2 * w[2]]
    return [A[k] * A[k] + C * B[k] * B[k] + Fr(12, 13) * eps for k in range(3)]


def _r_new(w, A, eps):
    t2, t3 = Fr(3, 4) * w[1], Fr(3, 4) * w[2]
    e = Fr(3, 4) * eps
    return [A[0] * A[0] + t2 * (A[0] + w[1]) + e, A[1] * A[1] + t2 * w[2] + e, A[2] * A[2] + t3 * (w[2] - A[2]) + e]


def _corr_old(r, A):
    s = [x * x for x in r]
    W1, W2, W3 = s[1] * s[2], s[0] * s[2], s[0] * s[1]
    c1W1, c3W3 = Fr(1, 30) * W1, Fr(1, 20) * W3
    den = 3 * c1W1 + 6 * c3W3 + Fr(6, 10) * W2
    return (c1W1 * (A[0] - A[1]) + c3W3 * (A[1] - A[2])) / den


def _corr_new(r, A):
    s = [x * x for x in r]
    N = s[1] * (Fr(3, 2) * s[0] * (A[1] - A[2]) + s[2] * (A[0] - A[1]))
    Dn = 6 * s[0] * s[2] + s[1] * (3 * s[0] + s[2])
    return N / (3 * Dn)


def _reference_weno5(v, eps):
    """src/derivatives.jl:61-81 in exact arithmetic, ε given."""
    v1, v2, v3, v4, v5 = v
    d1 = Fr(1, 3) * v1 - Fr(7, 6) * v2 + Fr(11, 6) * v3
    d2 = -Fr(1, 6) * v2 + Fr(5, 6) * v3 + Fr(1, 3) * v4
    d3 = Fr(1, 3) * v3 + Fr(5, 6) * v4 - Fr(1, 6) * v5
    S1 = Fr(13, 12) * (v1 - 2 * v2 + v3) ** 2 + Fr(1, 4) * (v1 - 4 * v2 + 3 * v3) ** 2
    S2 = Fr(13, 12) * (v2 - 2 * v3 + v4) ** 2 + Fr(1, 4) * (v2 - v4) ** 2
    S3 = Fr(13, 12) * (v3 - 2 * v4 + v5) ** 2 + Fr(1, 4) * (3 * v3 - 4 * v4 + v5) ** 2
    a1, a2, a3 = Fr(1, 10) / (S1 + eps) ** 2, Fr(6, 10) / (S2 + eps) ** 2, Fr(3, 10) / (S3 + eps) ** 2
    return (a1 * d1 + a2 * d2 + a3 * d3) / (a1 + a2 + a3)


def _random_lines(n, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        out.append([Fr(rng.randint(-10 ** 6, 10 ** 6), rng.randint(1, 10 ** 4)) for _ in range(5)])
    # lines with zeros and equal second differences among them
    out += [[Fr(0)] * 5, [Fr(1), Fr(2), Fr(3), Fr(4), Fr(5)], [Fr(0), Fr(1), Fr(0), Fr(1), Fr(0)], [Fr(2), Fr(2), Fr(5), Fr(2), Fr(2)]]
    return out


LINES = _random_lines(200, 1)


def _eps(e):
    m = max(abs(x) for x in e)
    return Fr(1, 10 ** 6) * m * m + Fr(1, 10 ** 75)


def test_smoothness_terms_are_the_old_ones_over_sixteen_thirteenths():
    for e in LINES:
        w, A = _diffs(e)
        eps = _eps(e)
        old, new = _r_old(w, A, eps), _r_new(w, A, eps)
        for k in range(3):
            assert (1 + C) * new[k] == old[k], (e, k)
            assert new[k] > 0
        assert new[1] - Fr(3, 4) * eps >= Fr(3, 8) * (w[1] * w[1] + w[2] * w[2])   # positive definite


def test_weight_correction_is_the_old_one():
    for e in LINES:
        w, A = _diffs(e)
        eps = _eps(e)
        old, new = _r_old(w, A, eps), _r_new(w, A, eps)
        want = _corr_old(old, A)
        assert _corr_new(old, A) == want, e          # the weight form alone
        assert _corr_new(new, A) == want, e          # with the rescaled smoothness terms: only ratios enter


def test_new_form_is_the_reference_weno5_once_eps_is_matched():
    for e in LINES:
        w, A = _diffs(e)
        eps = _eps(e)
        dphi2 = e[2] + w[2] / 3 + w[1] / 6
        assert dphi2 + _corr_new(_r_new(w, A, eps), A) == _reference_weno5(e, eps), e


# ---------------------------------------------------------------------------------------------- float64

def _fma(a, b, c):
    """Correctly rounded a·b + c (the device's v_fma_f64), through exact rationals."""
    x = Fr(a) * Fr(b) + Fr(c)
    return float(x)


def _r_old_f64(w, A, eps):
    """stage_math.h before the change, operation for operation; eps = (12/13)·ε already."""
    B1 = _fma(2.0, w[1], A[0])
    B2 = w[1] + w[2]
    B3 = _fma(-2.0, w[2], A[2])
    c = 3.0 / 13
    return [_fma(A[0], A[0], _fma(c * B1, B1, eps)), _fma(A[1], A[1], _fma(c * B2, B2, eps)), _fma(A[2], A[2], _fma(c * B3, B3, eps))]


def _r_new_f64(w, A, eps34):
    """stage_math.h now, operation for operation; eps34 = ¾·ε."""
    t2, t3 = 0.75 * w[1], 0.75 * w[2]
    return [_fma(A[0], A[0], _fma(t2, A[0] + w[1], eps34)), _fma(A[1], A[1], _fma(t2, w[2], eps34)),
            _fma(A[2], A[2], _fma(t3, w[2] - A[2], eps34))]


def _adversarial():
    base = [
        (1.0, 0.5, -0.5, 0.25),            # w2 = -w3
        (0.3, 0.7, -0.7, 0.1),
        (2.0, 1.0, 0.3, -0.4),             # w1 = 2 w2: A1 + w2 = 0
        (-1.4, -0.7, 0.7, 0.2),            # both
        (0.0, 0.6, -0.1, 0.9), (0.4, 0.0, 0.3, -0.2), (0.4, 0.6, 0.0, -0.2), (0.4, 0.6, -0.1, 0.0),   # one w exactly 0
        (0.0, 0.0, 0.0, 0.0),
        (1.0 + 2.0 ** -30, 1.0, 1.0 - 2.0 ** -30, 1.0),     # nearly equal: A of rounding size
        (1.0 / 3, 2.0 / 3, -2.0 / 3 * (1 + 2.0 ** -52), 0.1),
    ]
    rng = np.random.default_rng(7)
    base += [tuple(rng.standard_normal(4)) for _ in range(40)]
    out = []
    for scale in (1.0, 1e-30, 1e30):
        out += [tuple(x * scale for x in b) for b in base]
    return out


def test_float64_smoothness_terms_agree_to_8_ulp():
    worst = 0.0
    for w in _adversarial():
        A = [w[1] - w[0], w[2] - w[1], w[3] - w[2]]
        m = max(abs(x) for x in w)                      # any positive ε of the right size does
        eps = 1e-6 * m * m
        old = _r_old_f64(w, A, (12.0 / 13) * eps)
        new = _r_new_f64(w, A, 0.75 * eps)
        for k in range(3):
            if old[k] == 0.0:
                assert new[k] == 0.0
                continue
            d = abs(Fr(16, 13) * Fr(new[k]) - Fr(old[k]))
            ulps = float(d / Fr(math.ulp(old[k])))
            worst = max(worst, ulps)
            assert ulps <= 8.0, (w, k, ulps)
    print(f"worst |16/13·r' - r| = {worst:.2f} ulp of r")


def test_float64_new_form_against_the_oracle_core(orc):
    """The new forms evaluated in float64 (undivided, h = 1) against the oracle's _weno5 — the FAST bar of a stage,
    1e-13·max|v|, holds with room for lines of any roughness."""
    rng = np.random.default_rng(11)
    worst = 0.0
    lines = [rng.standard_normal(5) * s for s in (1.0, 1e-30, 1e30) for _ in range(50)]
    lines += [np.array([1.0, -1.0, 1.0, -1.0, 1.0]), np.array([0.0, 0.0, 1.0, 0.0, 0.0]), np.array([1.0, 1.0, 1.0, 1.0, 1.0])]
    for e in lines:
        e = [float(x) for x in e]
        w = [e[k + 1] - e[k] for k in range(4)]
        A = [w[1] - w[0], w[2] - w[1], w[3] - w[2]]
        m = max(abs(x) for x in e)
        r = _r_new_f64(w, A, _fma(0.75e-6 * m, m, (13.0 / 16) * 1e-75))
        s = [x * x for x in r]
        N = s[1] * _fma(1.5, s[0] * (A[1] - A[2]), s[2] * (A[0] - A[1]))
        Dn = _fma(6.0, s[0] * s[2], s[1] * _fma(3.0, s[0], s[2]))
        got = _fma((1.0 / Dn) * (1.0 / 3), N, _fma(1.0 / 3, w[2], _fma(1.0 / 6, w[1], e[2])))
        want = orc.weno5_core(*e)
        err = abs(got - want) / m
        worst = max(worst, err)
        assert err <= 1e-13, (e, got, want)
    print(f"worst |new - oracle| / max|v| = {worst:.2e}")
