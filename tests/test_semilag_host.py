"""SemiLagrangian's scheme through its numpy restatement (tests/_semilag_ref.py): is the scheme right?  Exact
shifts, polynomial reproduction, a revolution of an off-centre disk, the limiter and the periodic wrap.  The device is held to
this restatement bit for bit in tests/test_gpu_semilag.py."""
import math

import numpy as np
import pytest

import _semilag_ref as R

PER2 = (("periodic", "periodic"),) * 2
PER3 = (("periodic", "periodic"),) * 3


def _periodic_random(n, seed):
    u = np.random.default_rng(seed).uniform(-1, 1, n)
    for d in range(len(n)):   # equal end nodes: the period is n - 1
        s0 = [slice(None)] * len(n)
        s1 = [slice(None)] * len(n)
        s0[d], s1[d] = 0, -1
        u[tuple(s1)] = u[tuple(s0)]
    return u


@pytest.mark.parametrize("trace", [1, 2])
@pytest.mark.parametrize("limiter", [True, False])
@pytest.mark.parametrize("order", [1, 3, 5])
def test_exact_shift_2d(order, limiter, trace):
    n = (17, 33)
    u = _periodic_random(n, 1)
    got = R.step(u, ("const", (1.0, -2.0)), (0, 0), (1, 1), PER2, 0.0, 3 / 16, order, trace, limiter)
    i, j = np.meshgrid(np.arange(17), np.arange(33), indexing="ij")
    np.testing.assert_array_equal(got, u[(i - 3) % 16, (j + 12) % 32])


@pytest.mark.parametrize("order, limiter", [(1, True), (3, True), (3, False), (5, True), (5, False)])
def test_exact_shift_3d(order, limiter):
    n = (9, 9, 9)
    u = _periodic_random(n, 2)
    got = R.step(u, ("const", (1.0, -1.0, 2.0)), (0, 0, 0), (1, 1, 1), PER3, 0.0, 1 / 4, order, 2, limiter)
    i, j, k = np.meshgrid(*[np.arange(9)] * 3, indexing="ij")
    np.testing.assert_array_equal(got, u[(i - 2) % 8, (j + 2) % 8, (k - 4) % 8])


def _poly(deg):
    rng = np.random.default_rng(10 + deg)
    c = rng.uniform(-1, 1, (deg + 1, deg + 1))
    return lambda x, y: sum(c[a, b] * x ** a * y ** b for a in range(deg + 1) for b in range(deg + 1))


def _poly_error(order, deg):
    n, lc = (12, 9), (0.0, 0.0)
    hc = (0.1 * 11, 0.13 * 8)
    h = R.meshsize(lc, hc, n)
    X, Y = np.meshgrid(*[lc[d] + np.arange(n[d]) * h[d] for d in range(2)], indexing="ij")
    f = _poly(deg)
    u = f(X, Y)
    got = R.step(u, ("const", (0.037, -0.021)), lc, hc, (("neumann", "neumann"),) * 2, 0.0, 1.0, order, 2, False)
    inner = (slice(3, -3), slice(3, -3))
    return float(np.abs(got - f(X - 0.037, Y + 0.021))[inner].max()), float(np.abs(u).max())


def test_order_3_reproduces_a_cubic_and_order_1_does_not():
    """the bound is the rounding of 16 products with weights below 1.3 (found: 6.7e-16 at max|ϕ| = 2.6)"""
    err, scale = _poly_error(3, 3)
    assert err <= 1e-13 * scale
    err1, _ = _poly_error(1, 3)
    assert err1 > 1e-3


def test_order_5_reproduces_a_quintic():
    err, scale = _poly_error(5, 5)
    assert err <= 1e-13 * scale
    assert _poly_error(3, 5)[0] > 1e-7


def _revolution(m, order):
    """one revolution of the off-centre disk at m² with Δt = 4h; the largest error within 3h of the interface"""
    n, lc, hc = (m, m), (-1.0, -1.0), (1.0, 1.0)
    h = R.meshsize(lc, hc, n)
    X, Y = np.meshgrid(*[lc[d] + np.arange(m) * h[d] for d in range(2)], indexing="ij")
    u0 = np.hypot(X - 0.4, Y) - 0.3
    u, tc, tf, dt, steps = u0, 0.0, 2 * math.pi, 4 * h[0], 0
    bcs = (("neumann", "neumann"),) * 2
    while tc <= tf - np.spacing(tc):
        s = min(dt, tf - tc)
        u = R.step(u, ("rotation", 1.0, 0.0, 0.0), lc, hc, bcs, tc, s, order, 2, True)
        tc += s
        steps += 1
    near = np.abs(u0) <= 3 * h[0]
    return float(np.abs(u - u0)[near].max()), steps, int((u < 0).sum()) - int((u0 < 0).sum())


def test_rotation_of_an_off_centre_disk():
    e3, steps, dcount = _revolution(65, 3)
    assert steps == 51
    assert e3 <= 1.0e-2           # found: 7.08e-3
    assert dcount == 0            # the cubic keeps the count of ϕ < 0 nodes
    e1, _, dcount1 = _revolution(65, 1)
    assert e3 < e1 / 3            # found: linear 2.65e-2
    assert dcount1 < 0            # the linear interpolant diffuses the convex disk away: found −31 of 289 nodes
    f3, steps, _ = _revolution(129, 3)
    assert steps == 101
    assert f3 <= 2.4e-3           # found: 1.70e-3
    assert f3 <= e3 / 3           # second order: the midpoint trace dominates


@pytest.mark.parametrize("order", [3, 5])
def test_limiter_keeps_a_step_function_in_range(order):
    n = (40, 30)
    i, j = np.meshgrid(np.arange(40), np.arange(30), indexing="ij")
    u = np.where((i > 12) & (i < 27) & (j > 8) & (j < 20), 1.0, -1.0)
    args = (u, ("const", (0.43, -0.31)), (0, 0), (39 * 0.1, 29 * 0.1), PER2, 0.0, 1.0, order, 2)
    lim = R.step(*args, True)
    raw = R.step(*args, False)
    assert lim.min() >= -1.0 and lim.max() <= 1.0
    assert raw.min() < -1.0 - 1e-3 and raw.max() > 1.0 + 1e-3


def test_periodic_wrap_of_more_than_two_periods():
    n = (17,)
    x = np.arange(17) / 16
    u = np.sin(2 * np.pi * x) + 0.3 * np.cos(6 * np.pi * x)
    u[-1] = u[0]
    bcs = (("periodic", "periodic"),)
    far = R.step(u, ("const", (1.0,)), (0,), (1,), bcs, 0.0, (2 * 16 + 3.3) / 16, 3, 2, True)
    near = R.step(u, ("const", (1.0,)), (0,), (1,), bcs, 0.0, 3.3 / 16, 3, 2, True)
    assert np.abs(far - near).max() <= 1e-13
    assert np.abs(near - u).max() > 0.1


def test_non_finite_velocity_gives_nan_and_an_in_range_cell():
    xi = np.array([np.nan, np.inf, -np.inf, -0.5, 3.2, 7.0, 1e300, -1e300])
    j, th = R.cell(xi, 8)
    assert j.min() >= 0 and j.max() <= 6
    assert j[0] == 0 and np.isnan(th[0])
    w = R.wrap(xi, 8, True)
    assert np.isnan(w[:3]).all()
    jw, _ = R.cell(w, 8)
    assert jw.min() >= 0 and jw.max() <= 6
    c = R.wrap(xi, 8, False)
    np.testing.assert_array_equal(c[1:], [7.0, 0.0, 0.0, 3.2, 7.0, 7.0, 0.0])


def test_the_library_names_the_integrator_and_its_entry_point():
    import lsm_amd as lsm
    assert lsm.show(lsm.SemiLagrangian()) == "SemiLagrangian (backward characteristics, Lagrange interpolation)\n  └─ cfl: 4.0"
    integ = lsm.SemiLagrangian(2.5, order=5, trace=1, limiter=False)
    assert (integ.cfl, integ.order, integ.trace, integ.limiter) == (2.5, 5, 1, False)
    assert "lsm_advance_semilag" in lsm._lib.EXPORTS
    assert "SemiLagrangian" in lsm.__all__
