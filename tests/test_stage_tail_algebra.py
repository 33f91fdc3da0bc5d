"""The forms of the headline stage's tail (csrc/stage_math.h, csrc/stage_kernel.h) in float64, operation for operation,
against what they replace:

  * a WENO5 line returning THREE times its value, 3dϕ₂ + N/Dn with 3dϕ₂ = 3e₃ + w₃ + ½w₂, multiplied by a factor that
    carries the ⅓ (|u|/3h, and cdt·|u|/3h in the plain variants) — against the oracle's _weno5 times |u|/h;
  * the Eikonal term on the UNDIVIDED Godunov sum s = h²|∇ϕ|² (equal spacings, dx = h): one floor s' = max(s, 1e-300),
    √s' by one Goldschmidt step on a 2^-24 seed, S = c/√(c² + s'), |∇ϕ| - 1 = √s'/h - 1 in one FMA — against sqrt and
    c/√(c² + n2·dx²) with n2 = s/h².

The hardware seeds (v_rcp_f64, v_rsq_f64: 2^-24.4 / 2^-24.2 relative, tools/seedacc.hip) are modelled by the exact value
perturbed by ±2^-24, the worst the Newton / Goldschmidt steps have to absorb.
"""
import math
import os
from fractions import Fraction as Fr

import numpy as np
import pytest

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED_ERR = 2.0 ** -24


def _fma(a, b, c):
    """Correctly rounded a·b + c (v_fma_f64), through exact rationals; inf/nan operands go through float arithmetic."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    x = Fr(a) * Fr(b) + Fr(c)
    try:
        return float(x)
    except OverflowError:
        return math.copysign(math.inf, x)


def _rcp(x, sgn):
    """fast_rcp: seed + one Newton step."""
    r = (1.0 / x) * (1.0 + sgn * SEED_ERR)
    e = _fma(-x, r, 1.0)
    return _fma(r, e, r)


def _rsq_seed(x, sgn):
    return (1.0 / math.sqrt(x)) * (1.0 + sgn * SEED_ERR)


def _fast_rsqrt(x, sgn):
    r = _rsq_seed(x, sgn)
    e = _fma(-0.5 * x * r, r, 0.5)
    return _fma(r, e, r)


# ------------------------------------------------------------------------------------------------ WENO5, three-fold

def _weno5_x3(e, eps_floor, sgn):
    """weno5_undivided_pq<PQ, X3 = true>, operation for operation."""
    e1, e2, e3, e4, e5 = e
    w1, w2, w3, w4 = e2 - e1, e3 - e2, e4 - e3, e5 - e4
    A1, A2, A3 = w2 - w1, w3 - w2, w4 - w3
    m = max(abs(x) for x in e)
    eps = _fma(0.75e-6 * m, m, (13.0 / 16) * max(eps_floor, 1.0e-75))
    t2, t3 = 0.75 * w2, 0.75 * w3
    r1 = _fma(A1, A1, _fma(t2, A1 + w2, eps))
    r2 = _fma(A2, A2, _fma(t2, w3, eps))
    r3 = _fma(A3, A3, _fma(t3, w3 - A3, eps))
    s1, s2, s3 = r1 * r1, r2 * r2, r3 * r3
    N = s2 * _fma(1.5, s1 * (A2 - A3), s3 * (A1 - A2))
    Dn = _fma(6.0, s1 * s3, s2 * _fma(3.0, s1, s3))
    return _fma(_rcp(Dn, sgn), N, _fma(0.5, w2, _fma(3.0, e3, w3)))


def _lines():
    rng = np.random.default_rng(23)
    lines = [rng.standard_normal(5) * s for s in (1.0, 1e-30, 1e30) for _ in range(40)]
    # cancelling: w₂ = -w₃, 3e₃ + w₃ + ½w₂ = 0, equal differences, a single spike, a sawtooth, flat
    lines += [np.array(v, dtype=np.float64) for v in (
        (1.0, 0.5, 1.0, 0.5, 1.0), (0.3, 1.0, -0.5, 0.5, 2.0), (1.0, 1.0, 1.0, 1.0, 1.0), (0.0, 0.0, 1.0, 0.0, 0.0),
        (1.0, -1.0, 1.0, -1.0, 1.0), (0.0, 0.0, 0.0, 0.0, 0.0), (0.0, -0.0, 0.0, -0.0, 0.0),
        (1.0 + 2.0 ** -30, 1.0, 1.0 - 2.0 ** -30, 1.0, 1.0 + 2.0 ** -31))]
    return [[float(x) for x in e] for e in lines]


def test_threefold_weno5_times_folded_factor_against_the_oracle_core(orc):
    """|u|/h · _weno5(e) = (|u|/3h) · (3dϕ₂ + N/Dn) within the FAST bar of a stage (1e-13 of the line's largest value) and, on
    lines without cancellation, to a few ulp of the term."""
    z = np.load(os.path.join(G, "weno5_core.npz"))
    lines = _lines() + [[float(x) for x in row] for row in z["v"][:60]]
    u, h, cdt = 0.7, 0.125, 1.7e-3
    inv_h3 = (1.0 / h) / 3.0
    worst = 0.0
    for e in lines:
        m = max(abs(x) for x in e)
        want = (u / h) * orc.weno5_core(*e)
        for sgn in (-1.0, 1.0):
            w3 = _weno5_x3(e, 1e-99 * h * h, sgn)
            assert math.isfinite(w3)
            got = (u * inv_h3) * w3
            got_cdt = (cdt * inv_h3 * u) * w3                 # plain variants: cdt in the factor as well
            if m == 0.0:
                assert got == 0.0 and got_cdt == 0.0
                continue
            err = abs(got - want) / (m * u / h)
            worst = max(worst, err)
            assert err <= 1e-13, (e, got, want)
            assert abs(got_cdt - cdt * want) <= 1e-13 * cdt * m * u / h
    print(f"worst |3-fold form - oracle| / (max|v|·|u|/h) = {worst:.2e}")


def test_threefold_value_is_three_times_the_onefold_to_rounding():
    """Against the form it replaces (dϕ₂ + (rcp(Dn)/3)·N): the same N, Dn; a few ulp of three times the line's largest value."""
    for e in _lines():
        e1, e2, e3, e4, e5 = e
        w2, w3 = e3 - e2, e4 - e3
        x3 = _weno5_x3(e, 1e-101, 1.0)
        d3 = _fma(0.5, w2, _fma(3.0, e3, w3))
        d1 = _fma(1.0 / 3, w3, _fma(1.0 / 6, w2, e3))
        corr3 = x3 - d3
        one = d1 + corr3 / 3
        big = max(3 * max(abs(x) for x in e), 1e-300)           # the roundings happen at the size of 3e₃
        assert abs(x3 - 3 * one) <= 6 * np.spacing(big), (e, x3, 3 * one)


# ------------------------------------------------------------------------------------------------ Eikonal tail

def _tail_new(s, c, inv_h, sgn):
    """eikonal_tail_raw + the caller's FMA: returns (√s', S, |∇ϕ| - 1)."""
    sf = max(s, 1.0e-300)
    r = _rsq_seed(sf, sgn)
    g, hh = sf * r, 0.5 * r
    q = _fma(-g, hh, 0.5)
    root = _fma(g, q, g)
    S = c * _fast_rsqrt(_fma(c, c, sf), -sgn)
    return root, S, _fma(root, inv_h, -1.0)


S_VALUES = [0.0, 1e-300] + [10.0 ** k for k in range(-60, 61, 6)] + [2.0, 3.0, 0.1, 7.3e-11, 1.9e37]
C_VALUES = [0.0, -0.0, 1e-200, -1e-200, 5e-324, -5e-324, 1e-30, -1e-30, 0.3, -0.3, 1.0, 2.5e34, -2.5e34]


def test_goldschmidt_root_against_sqrt():
    worst = 0.0
    for s in S_VALUES:
        for sgn in (-1.0, 1.0):
            root, _, _ = _tail_new(s, 0.0, 8.0, sgn)
            want = math.sqrt(max(s, 1e-300))
            assert math.isfinite(root)
            rel = abs(root - want) / want
            worst = max(worst, rel)
            assert rel <= 1.5 * SEED_ERR ** 2 * 1.05 + 2 * 2.0 ** -53, (s, root, want)
    print(f"worst relative error of the Goldschmidt root = {worst:.2e}")


def test_tail_on_the_undivided_sum_against_the_divided_form():
    """S and S·(|∇ϕ| - 1) against c/√(c² + n2·dx²) and its product with √n2 - 1, n2 = s/h², dx = h, evaluated with sqrt
    and true divisions.  No NaN/Inf anywhere; S = 0 exactly at c = ±0; S to 1.5·seed² + 4 ulp; the term to that times |S|·(|∇ϕ| + 1)."""
    tolS = 1.5 * SEED_ERR ** 2 * 1.05 + 4 * 2.0 ** -53
    worst = 0.0
    for h in (0.125, 1.0 / 511, 3.0):
        inv_h = 1.0 / h
        for s in S_VALUES:
            for c in C_VALUES:
                for sgn in (-1.0, 1.0):
                    root, S, nm = _tail_new(s, c, inv_h, sgn)
                    assert math.isfinite(root) and math.isfinite(S) and math.isfinite(nm), (s, c)
                    if c == 0.0:
                        assert S == 0.0, (s, c, S)
                        continue
                    # reference in exact arithmetic up to the final square root
                    d2 = Fr(c) * Fr(c) + Fr(max(s, 1e-300))
                    wantS = c / math.sqrt(float(d2)) if float(d2) > 0 else math.copysign(1.0, c)
                    if float(d2) < 1e-290:
                        # c² underflows against the floor: |S| <= 1 is all either form can promise
                        assert abs(S) <= 1.0 + tolS
                        continue
                    assert abs(S - wantS) <= tolS * max(abs(wantS), 5e-324) + 5e-324, (s, c, S, wantS)
                    assert abs(S) <= 1.0 + tolS
                    if wantS == 0.0:                      # the smallest subnormal over a large gradient
                        continue
                    grad =math.sqrt(max(s, 1e-300)) * inv_h
                    want_term = wantS * (grad - 1.0)
                    got_term = S * nm
                    bound = 2 * tolS * abs(wantS) * (grad + 1.0) + 5e-324
                    worst = max(worst, abs(got_term - want_term) / (abs(wantS) * (grad + 1.0)))
                    assert abs(got_term - want_term) <= bound, (h, s, c, got_term, want_term)
    print(f"worst |term - reference| / (|S|·(|∇ϕ| + 1)) = {worst:.2e}")


def test_tail_agrees_with_the_form_it_replaces():
    """Operation for operation: the old tail (n2 = s·inv_h², fast_norm, d2 = n2·dx² + c² floored) and the new one, on the
    same seeds' worst cases — they may differ by the seeds' second-order terms and a few roundings, nothing else."""
    h = 0.125
    inv_h, inv_h2, dx2 = 1.0 / h, 1.0 / (h * h), h * h
    tol = 3 * SEED_ERR ** 2 * 1.05 + 8 * 2.0 ** -53
    for s in S_VALUES:
        for c in C_VALUES:
            n2 = s * inv_h2
            nrm = n2 * _fast_rsqrt(max(n2, 1e-300), 1.0)
            d2 = _fma(n2, dx2, c * c)
            S_old = c * _fast_rsqrt(max(d2, 1e-300), -1.0)
            old = S_old * (nrm - 1)
            _, S, nm = _tail_new(s, c, inv_h, 1.0)
            new = S * nm
            assert math.isfinite(old) and math.isfinite(new)
            assert abs(new - old) <= tol * abs(S_old) * (nrm + 1.0) + 1e-140, (s, c, new, old)
