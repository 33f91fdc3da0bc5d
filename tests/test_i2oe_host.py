"""SemiImplicitI2OE on the host: the numpy restatement (tests/_i2oe_ref.py) against the reference's own tests
(test/test-semi-implicit.jl) and its documented step count, hand-built 1-D systems for every supported boundary
condition, the integrator's `show`, and the validation the host layer does before any device call."""
import math
import types

import numpy as np
import pytest

import _i2oe_ref as R


@pytest.fixture(scope="module")
def lsm():
    import lsm_amd
    return lsm_amd


PER1 = (("periodic", "periodic"),)


# ----------------------------------------------------------------------------- test/test-semi-implicit.jl, restated
def test_ref_periodic_transport_1d():
    """:5-27"""
    lc, hc, n = (0.0,), (1.0,), (201,)
    x = R.node_coords(lc, hc, n)[0]
    f = lambda x: np.sin(2 * np.pi * x) + 0.15 * np.cos(6 * np.pi * x)
    u, _ = R.integrate(f(x), lc, hc, PER1, lambda t: (np.ones(n),), 3.0, 0.35)
    assert np.abs(u - f(np.mod(x - 0.35, 1.0))).max() < 0.12


def test_ref_periodic_transport_2d():
    """:29-52"""
    lc, hc, n = (0.0, 0.0), (1.0, 1.0), (121, 111)
    x, y = np.meshgrid(*R.node_coords(lc, hc, n), indexing="ij")
    f = lambda x, y: np.sin(2 * np.pi * x) + 0.4 * np.cos(2 * np.pi * y)
    u, _ = R.integrate(f(x, y), lc, hc, PER1 * 2, lambda t: (np.full(n, 0.75), np.full(n, -0.35)), 2.5, 0.2)
    assert np.abs(u - f(np.mod(x - 0.75 * 0.2, 1.0), np.mod(y + 0.35 * 0.2, 1.0))).max() < 0.2


def test_ref_linear_extrapolation_keeps_a_constant():
    """:54-66"""
    lc, hc, n = (0.0,), (1.0,), (121,)
    x = R.node_coords(lc, hc, n)[0]
    u, _ = R.integrate(np.full(n, 0.7), lc, hc, (("linear", "linear"),), lambda t: (np.sin(2 * np.pi * x),), 4.0, 0.6)
    assert np.abs(u - 0.7).max() < 1.0e-12


def test_ref_invalid_setup_on_the_restatement():
    """:68-92 (the size check; the term count is the host layer's, below)"""
    with pytest.raises(ValueError, match="at least 3 grid nodes"):
        R.integrate(np.zeros(2), (0.0,), (1.0,), (("neumann", "neumann"),), lambda t: (np.ones(2),), 2.0, 0.1)
    with pytest.raises(ValueError, match="not supported by SemiImplicitI2OE"):
        R.relation("symmetry", 0, 5, -1)


def test_ref_larger_steps_than_forward_euler_1d():
    """:94-136"""
    lc, hc, n = (0.0,), (1.0,), (401,)
    x = R.node_coords(lc, hc, n)[0]
    f = lambda x: np.sin(2 * np.pi * x) + 0.2 * np.cos(4 * np.pi * x)
    semi, _ = R.integrate(f(x), lc, hc, PER1, lambda t: (np.ones(n),), 2.0, 0.5)
    with np.errstate(all="ignore"):
        expl = R.upwind_fe_periodic(f(x), lc, hc, (1.0,), 2.0, 0.5)
    ref = f(np.mod(x - 0.5, 1.0))
    assert np.abs(semi - ref).max() < 0.2
    assert not np.all(np.isfinite(expl)) or np.abs(expl - ref).max() > 0.5


def test_ref_outperforms_forward_euler_2d():
    """:138-174"""
    lc, hc, n = (0.0, 0.0), (1.0, 1.0), (121, 121)
    x, y = np.meshgrid(*R.node_coords(lc, hc, n), indexing="ij")
    f = lambda x, y: np.sin(2 * np.pi * x) + 0.25 * np.cos(4 * np.pi * y)
    semi, _ = R.integrate(f(x, y), lc, hc, PER1 * 2, lambda t: (np.full(n, 0.9), np.full(n, -0.55)), 4.0, 0.25)
    with np.errstate(all="ignore"):
        expl = R.upwind_fe_periodic(f(x, y), lc, hc, (0.9, -0.55), 4.0, 0.25)
    ref = f(np.mod(x - 0.9 * 0.25, 1.0), np.mod(y + 0.55 * 0.25, 1.0))
    err_semi = np.abs(semi - ref).max()
    err_expl = np.abs(expl - ref).max()
    assert err_semi < 0.05
    assert err_expl > 3 * err_semi


# ----------------------------------------------------------------------------- docs/src/time-integrators.md:92-115
def dumbbell(lc, hc, n):
    x, y = np.meshgrid(*R.node_coords(lc, hc, n), indexing="ij")
    disk = lambda c: np.hypot(x - c[0], y - c[1]) - 0.25
    bar = np.maximum(np.abs(x) - 0.5, np.abs(y) - 0.1)
    return np.minimum(np.minimum(disk((-0.5, 0.0)), disk((0.5, 0.0))), bar), x, y


def test_dumbbell_revolution_takes_198_steps():
    lc, hc, n = (-1.0, -1.0), (1.0, 1.0), (64, 64)
    u0, x, y = dumbbell(lc, hc, n)
    times = []
    u, steps = R.integrate(u0, lc, hc, (("neumann", "neumann"),) * 2, lambda t: (-y, x), 2.0, 2 * math.pi,
                           posthook=times.append)
    assert steps == 198
    assert times[-1] == 2 * math.pi
    assert np.abs(u - u0)[np.abs(u0) < 0.1].max() < 0.2   # the shape came back, smeared by the first-order scheme


# ----------------------------------------------------------------------------- hand-built 1-D systems (5 nodes)
def _dense(M):
    return M.toarray() if hasattr(M, "toarray") else np.asarray(M)


@pytest.mark.parametrize("bc", ["periodic", "neumann", "linear"])
def test_five_node_system(bc):
    """v = 1 everywhere, h = 1/4, Δt = h: fac = Δt/(2h) = 1/2 (face measure 1 in 1-D).  Every node has inflow through its
    lower face and outflow through its upper one."""
    h, dt, f = 0.25, 0.25, 0.5
    u = np.array([0.3, -1.0, 2.0, 0.5, 4.0])
    M, rhs = R.assemble(u, (np.ones(5),), [h], ((bc, bc),), dt)
    A = np.zeros((5, 5))
    b = u.copy()
    for p in range(1, 5):
        A[p, p], A[p, p - 1] = 1 + f, -f
    for p in range(4):
        b[p] += f * (u[p] - u[p + 1])
    if bc == "periodic":        # lower neighbour of node 0 is node n-2 = 3, upper of node 4 is node 1
        A[0, 0], A[0, 3] = 1 + f, -f
        b[4] += f * (u[4] - u[1])
    elif bc == "neumann":       # the inflow entry lands on the diagonal and cancels the diagonal increment
        A[0, 0] = 1.0
        b[4] += f * (u[4] - u[4])
    else:                       # ghost = 2u_0 - u_1: diagonal 1 - f, +f towards the inward neighbour
        A[0, 0], A[0, 1] = 1 - f, f
        b[4] += f * (u[4] - (2 * u[4] - u[3]))
    np.testing.assert_allclose(_dense(M), A, rtol=0, atol=1e-15)
    np.testing.assert_allclose(rhs, b, rtol=0, atol=1e-15)


def test_linear_extrapolation_inflow_row_loses_its_diagonal():
    """Local cfl 2 through a LinearExtrapolationBC face: diag = 1 - cfl/2 = 0; beyond it the diagonal is negative."""
    for dt, want in ((0.5, 0.0), (1.0, -1.0)):
        M, _ = R.assemble(np.zeros(5), (np.ones(5),), [0.25], (("linear", "linear"),), dt)
        assert _dense(M)[0, 0] == want


# ----------------------------------------------------------------------------- the public API
def test_show(lsm):
    assert lsm.show(lsm.SemiImplicitI2OE()) == "SemiImplicitI2OE (semi-implicit advection, Mikula et al.)\n  └─ cfl: 2.0"
    assert lsm.show(lsm.SemiImplicitI2OE(cfl=3.0, rtol=1e-10, max_iters=7)) == \
        "SemiImplicitI2OE (semi-implicit advection, Mikula et al.)\n  └─ cfl: 3.0"
    s = lsm.SemiImplicitI2OE()
    assert (s.cfl, s.rtol, s.max_iters) == (2.0, 1e-13, 500)


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before validation")


def _fake_equation(lsm, terms, n, bc, band=False, world=1):
    grid = lsm.CartesianGrid(tuple(0.0 for _ in n), tuple(1.0 for _ in n), n)
    eq = types.SimpleNamespace(terms=terms, mesh_=grid, bcs=lsm.api._normalize_bc(bc, len(n)), band=band,
                               comm=object() if world > 1 else None, world=world, t=0.0, integrator=lsm.SemiImplicitI2OE(),
                               backend=_NoDevice(), state=_NoDevice())
    eq.current_time = lambda: eq.t
    return eq


@pytest.mark.parametrize("case, msg", [
    ("band", "SemiImplicitI2OE requires a full-grid MeshField"),
    ("two_terms", "SemiImplicitI2OE requires exactly one AdvectionTerm"),
    ("curvature", "SemiImplicitI2OE requires exactly one AdvectionTerm"),
    ("small", "SemiImplicitI2OE requires at least 3 grid nodes along each dimension"),
    ("symmetry", "boundary condition SymmetryBC() is not supported by SemiImplicitI2OE"),
    ("quadratic", r"boundary condition ExtrapolationBC\{2\}\(\) is not supported by SemiImplicitI2OE"),
    ("mixed", "boundary condition SymmetryBC() is not supported by SemiImplicitI2OE"),
    ("slab", "SemiImplicitI2OE runs on a single device"),
])
def test_validation_before_any_device_call(lsm, case, msg):
    adv = lsm.AdvectionTerm((1.0,), lsm.Upwind())
    kw = dict(terms=(adv,), n=(41,), bc=lsm.PeriodicBC())
    if case == "band":
        kw["band"] = True
    elif case == "two_terms":
        kw["terms"] = (adv, lsm.CurvatureTerm(-0.1))
    elif case == "curvature":
        kw["terms"] = (lsm.CurvatureTerm(-0.1),)
    elif case == "small":
        kw.update(n=(2,), bc=lsm.NeumannBC())
    elif case == "symmetry":
        kw["bc"] = lsm.SymmetryBC()
    elif case == "quadratic":
        kw["bc"] = lsm.ExtrapolationBC(2)
    elif case == "mixed":
        kw.update(terms=(lsm.AdvectionTerm((1.0, 0.0)),), n=(9, 9), bc=(lsm.NeumannBC(), (lsm.LinearExtrapolationBC(), lsm.SymmetryBC())))
    elif case == "slab":
        kw["world"] = 2
    eq = _fake_equation(lsm, **kw)
    with pytest.raises(ValueError, match=msg.replace("(", r"\(").replace(")", r"\)") if case != "quadratic" else msg):
        lsm.integrate_(eq, 0.1)
    assert eq.t == 0.0
