"""SemiImplicitI2OE on the device (lsm_advance_i2oe) against the numpy restatement of the reference (tests/_i2oe_ref.py):
single steps over dimensions, boundary conditions, velocity kinds, CFL numbers and both arithmetic modes; the reference's
six testsets; the documented dumbbell revolution; hooks; Float32 storage; a large 3-D step checked by its residual; and
the failure report of a solve that runs out of iterations."""
import math

import numpy as np
import pytest

import _i2oe_ref as R

pytestmark = pytest.mark.gpu

BCS = {"P": "periodic", "N": "neumann", "L": "linear"}


@pytest.fixture(scope="module")
def lsm():
    import lsm_amd
    return lsm_amd


def _bc_obj(lsm, c):
    return {"P": lsm.PeriodicBC, "N": lsm.NeumannBC, "L": lsm.LinearExtrapolationBC}[c]()


def _velocity(lsm, kind, lc, hc, n, t0):
    """(velocity spec for AdvectionTerm, host velocity(t) -> tuple of node arrays)"""
    N = len(n)
    X = np.meshgrid(*R.node_coords(lc, hc, n), indexing="ij")
    if kind == "const":
        c = (0.8, -0.45, 0.3)[:N]
        return c, lambda t: tuple(np.full(n, v) for v in c)
    if kind == "rotation":
        w, c = 1.3, (0.1, -0.2)
        return lsm.RigidRotation(w, c), lambda t: (-(w * (X[1] - c[1])), w * (X[0] - c[0])) + ((np.zeros(n),) if N == 3 else ())
    if kind == "separable":
        rng = np.random.default_rng(7)
        tabs = [[rng.uniform(-1, 1, n[d]) for d in range(N)] for _ in range(N)]
        T = 1.7
        spec = lsm.SeparableCoefficient(tabs, time=("cos", T))

        def host(t):
            out = []
            for c in range(N):
                p = tabs[c][0].reshape([-1] + [1] * (N - 1))
                for d in range(1, N):
                    shp = [1] * N
                    shp[d] = -1
                    p = p * tabs[c][d].reshape(shp)
                out.append(np.broadcast_to(p * math.cos(math.pi * t / T), n).copy())
            return tuple(out)
        return spec, host
    f = lambda X, t: tuple(np.sin(2.1 * X[(d + 1) % N] + 0.3 * d) * (1 + 0.5 * t) + 0.2 for d in range(N))
    if kind == "field":
        vals = np.stack([np.broadcast_to(v, n) for v in f(X, t0)])
        return lsm.MeshField(vals, lsm.CartesianGrid(lc, hc, n)), lambda t: f(X, t0)
    return (lambda xs, t: f(xs, t)), lambda t: tuple(np.broadcast_to(v, n) for v in f(X, t))   # host callable


def _one_step(lsm, n, bcs, vkind, cfl, mode, t0=0.25, dtype=np.float64):
    N = len(n)
    lc, hc = tuple(-0.5 - 0.1 * d for d in range(N)), tuple(1.0 + 0.2 * d for d in range(N))
    X = np.meshgrid(*R.node_coords(lc, hc, n), indexing="ij")
    u0 = np.sin(3 * X[0] + 0.5) + (np.cos(2 * X[1]) if N > 1 else 0) + (X[2] ** 2 if N > 2 else 0)
    spec, host = _velocity(lsm, vkind, lc, hc, n, t0)
    h = R.meshsize(lc, hc, n)
    dt = 0.999 * cfl * R.advection_cfl(host(t0), h)
    grid = lsm.CartesianGrid(lc, hc, n)
    bc = tuple((_bc_obj(lsm, a), _bc_obj(lsm, b)) for a, b in bcs)
    eq = lsm.LevelSetEquation(terms=lsm.AdvectionTerm(spec, lsm.Upwind()), ic=lsm.MeshField(u0.astype(dtype), grid), bc=bc,
                              integrator=lsm.SemiImplicitI2OE(cfl=cfl), mode=mode, t=t0)
    lsm.integrate_(eq, t0 + dt, dt)
    ref = R.step(u0, host(t0), h, tuple((BCS[a], BCS[b]) for a, b in bcs), dt)
    return eq, eq.current_state().values(), ref


CASES = [
    ((41,), ("PP",), "const", 0.5), ((41,), ("NN",), "const", 2.0), ((41,), ("LL",), "const", 4.0),
    ((41,), ("NL",), "field", 2.0), ((41,), ("LN",), "callable", 4.0), ((41,), ("PP",), "separable", 2.0),
    ((33, 29), ("PP", "PP"), "rotation", 2.0), ((33, 29), ("NN", "NN"), "rotation", 4.0), ((33, 29), ("LL", "LL"), "rotation", 0.5),
    ((33, 29), ("PP", "LL"), "separable", 2.0), ((33, 29), ("NN", "PP"), "field", 4.0), ((33, 29), ("LN", "NL"), "callable", 2.0),
    ((33, 29), ("LL", "NN"), "const", 4.0),
    # 66 563 nodes, 261 workgroups: the last workgroup's sum over the partials takes a second trip, the grid-stride loop one
    ((259, 257), ("PP", "LL"), "rotation", 2.0),
    ((17, 15, 13), ("PP", "NN", "LL"), "separable", 2.0), ((17, 15, 13), ("LL", "LL", "LL"), "field", 4.0),
    ((17, 15, 13), ("NN", "NN", "NN"), "rotation", 2.0), ((17, 15, 13), ("PP", "PP", "PP"), "const", 0.5),
    ((17, 15, 13), ("NL", "PP", "LN"), "callable", 4.0),
]


@pytest.mark.parametrize("mode", ["fast", "strict"])
@pytest.mark.parametrize("n, bcs, vkind, cfl", CASES, ids=lambda x: str(x).replace(" ", ""))
def test_one_step_against_the_restatement(lsm, n, bcs, vkind, cfl, mode):
    eq, dev, ref = _one_step(lsm, n, bcs, vkind, cfl, mode)
    assert np.abs(dev - ref).max() <= 1e-10 * np.abs(ref).max()
    assert eq.i2oe_last[1] <= 1e-13


@pytest.mark.parametrize("cfl", [2.0, 4.0])
def test_linear_extrapolation_inflow_zero_or_negative_diagonal(lsm, cfl):
    """v = 1 enters through the LinearExtrapolationBC face of node 0 at local cfl 2 (diagonal 0) and 4 (diagonal -1)."""
    n = (41,)
    lc, hc = (0.0,), (1.0,)
    x = R.node_coords(lc, hc, n)[0]
    u0 = np.cos(4 * x) + x
    h = R.meshsize(lc, hc, n)
    dt = cfl * h[0]
    M, _ = R.assemble(u0, (np.ones(n),), h, (("linear", "linear"),), dt)
    assert M.toarray()[0, 0] <= 1e-12
    eq = lsm.LevelSetEquation(terms=lsm.AdvectionTerm((1.0,), lsm.Upwind()), ic=lsm.MeshField(u0, lsm.CartesianGrid(lc, hc, n)),
                              bc=lsm.LinearExtrapolationBC(), integrator=lsm.SemiImplicitI2OE(cfl=100.0))
    lsm.integrate_(eq, dt, dt)
    ref = R.step(u0, (np.ones(n),), h, (("linear", "linear"),), dt)
    assert np.abs(eq.current_state().values() - ref).max() <= 1e-10 * np.abs(ref).max()


# ----------------------------------------------------------------------------- test/test-semi-implicit.jl on the device
def _periodic_case(lsm, n, vel, f, cfl, tf):
    N = len(n)
    lc, hc = (0.0,) * N, (1.0,) * N
    X = np.meshgrid(*R.node_coords(lc, hc, n), indexing="ij")
    grid = lsm.CartesianGrid(lc, hc, n)
    u0 = f(*X)
    eq = lsm.LevelSetEquation(terms=lsm.AdvectionTerm(lsm.MeshField(np.stack([np.full(n, v) for v in vel]), grid), lsm.Upwind()),
                              ic=lsm.MeshField(u0, grid), bc=lsm.PeriodicBC(), integrator=lsm.SemiImplicitI2OE(cfl=cfl))
    lsm.integrate_(eq, tf)
    dev = eq.current_state().values()
    ref, _ = R.integrate(u0, lc, hc, (("periodic", "periodic"),) * N, lambda t: tuple(np.full(n, v) for v in vel), cfl, tf)
    assert np.abs(dev - ref).max() <= 1e-8 * np.abs(ref).max()
    exact = f(*[np.mod(X[d] - vel[d] * tf, 1.0) for d in range(N)])
    return dev, exact, grid, u0


def _fe(lsm, grid, u0, vel, cfl, tf):
    eq = lsm.LevelSetEquation(terms=lsm.AdvectionTerm(tuple(vel), lsm.Upwind()), ic=lsm.MeshField(u0, grid), bc=lsm.PeriodicBC(),
                              integrator=lsm.ForwardEuler(cfl=cfl), mode="strict")
    lsm.integrate_(eq, tf)
    return eq.current_state().values()


def test_ref_periodic_transport_1d(lsm):
    dev, exact, *_ = _periodic_case(lsm, (201,), (1.0,), lambda x: np.sin(2 * np.pi * x) + 0.15 * np.cos(6 * np.pi * x), 3.0, 0.35)
    assert np.abs(dev - exact).max() < 0.12


def test_ref_periodic_transport_2d(lsm):
    dev, exact, *_ = _periodic_case(lsm, (121, 111), (0.75, -0.35), lambda x, y: np.sin(2 * np.pi * x) + 0.4 * np.cos(2 * np.pi * y), 2.5, 0.2)
    assert np.abs(dev - exact).max() < 0.2


def test_ref_linear_extrapolation_keeps_a_constant(lsm):
    grid = lsm.CartesianGrid((0.0,), (1.0,), (121,))
    eq = lsm.LevelSetEquation(terms=lsm.AdvectionTerm(lambda x, t: np.sin(2 * np.pi * x[0]), lsm.Upwind()),
                              ic=lsm.MeshField(lambda x: 0.7, grid), bc=lsm.LinearExtrapolationBC(), integrator=lsm.SemiImplicitI2OE(cfl=4.0))
    lsm.integrate_(eq, 0.6)
    assert np.abs(eq.current_state().values() - 0.7).max() < 1.0e-12


def test_ref_invalid_setup(lsm):
    grid = lsm.CartesianGrid((0.0,), (1.0,), (41,))
    eq = lsm.LevelSetEquation(terms=(lsm.AdvectionTerm(lambda x, t: 1.0 + 0 * x[0], lsm.Upwind()), lsm.CurvatureTerm(-0.1)),
                              ic=lsm.MeshField(lambda x: x[0], grid), bc=lsm.PeriodicBC(), integrator=lsm.SemiImplicitI2OE())
    with pytest.raises(ValueError, match="exactly one AdvectionTerm"):
        lsm.integrate_(eq, 0.1)
    # a 2-node grid: the device handle itself needs 4 nodes per dimension (lsm_create), so the equation is refused
    # when it is built, before integrate! could refuse it (the host layer's own check: test_i2oe_host.py)
    small = lsm.CartesianGrid((0.0,), (1.0,), (2,))
    with pytest.raises((ValueError, lsm.LsmError), match="at least"):
        eq = lsm.LevelSetEquation(terms=(lsm.AdvectionTerm(lambda x, t: 1.0 + 0 * x[0], lsm.Upwind()),),
                                  ic=lsm.MeshField(lambda x: x[0], small), bc=lsm.NeumannBC(), integrator=lsm.SemiImplicitI2OE())
        lsm.integrate_(eq, 0.1)


def test_ref_larger_steps_than_forward_euler_1d(lsm):
    f = lambda x: np.sin(2 * np.pi * x) + 0.2 * np.cos(4 * np.pi * x)
    dev, exact, grid, u0 = _periodic_case(lsm, (401,), (1.0,), f, 2.0, 0.5)
    with np.errstate(all="ignore"):
        expl = _fe(lsm, grid, u0, (1.0,), 2.0, 0.5)
        assert np.abs(dev - exact).max() < 0.2
        assert not np.all(np.isfinite(expl)) or np.abs(expl - exact).max() > 0.5


def test_ref_outperforms_forward_euler_2d(lsm):
    f = lambda x, y: np.sin(2 * np.pi * x) + 0.25 * np.cos(4 * np.pi * y)
    dev, exact, grid, u0 = _periodic_case(lsm, (121, 121), (0.9, -0.55), f, 4.0, 0.25)
    expl = _fe(lsm, grid, u0, (0.9, -0.55), 4.0, 0.25)
    err_semi = np.abs(dev - exact).max()
    assert err_semi < 0.05
    assert np.abs(expl - exact).max() > 3 * err_semi


# ----------------------------------------------------------------------------- docs/src/time-integrators.md:92-115
def test_dumbbell_revolution(lsm, orc):
    from test_i2oe_host import dumbbell
    lc, hc, n = (-1.0, -1.0), (1.0, 1.0), (64, 64)
    u0, x, y = dumbbell(lc, hc, n)
    grid = lsm.CartesianGrid(lc, hc, n)
    eq = lsm.LevelSetEquation(terms=lsm.AdvectionTerm(lsm.RigidRotation()), ic=lsm.MeshField(u0, grid), bc=lsm.NeumannBC(),
                              integrator=lsm.SemiImplicitI2OE())
    steps = []
    lsm.integrate_(eq, 2 * math.pi, posthook=lambda e: steps.append(e.current_time()))
    assert len(steps) == 198 and eq.current_time() == 2 * math.pi
    ref, nref = R.integrate(u0, lc, hc, (("neumann", "neumann"),) * 2, lambda t: (-y, x), 2.0, 2 * math.pi)
    assert nref == 198
    og = orc.Grid(lc, hc, n)
    a_dev, a_ref = orc.volume(og, np.asfortranarray(eq.current_state().values())), orc.volume(og, np.asfortranarray(ref))
    assert abs(a_dev - a_ref) <= 1e-8 * abs(a_ref)


def test_time_dependent_callable_with_hooks(lsm):
    lc, hc, n = (0.0, 0.0), (1.0, 1.0), (40, 36)
    X = np.meshgrid(*R.node_coords(lc, hc, n), indexing="ij")
    u0 = np.sin(2 * np.pi * X[0]) * np.cos(np.pi * X[1])
    vel = lambda xs, t: (np.cos(t) * np.sin(np.pi * xs[1]) + 0 * xs[0], -np.sin(2 * t) * np.cos(np.pi * xs[0]) + 0 * xs[1])
    grid = lsm.CartesianGrid(lc, hc, n)
    eq = lsm.LevelSetEquation(terms=lsm.AdvectionTerm(vel), ic=lsm.MeshField(u0, grid), bc=lsm.NeumannBC(), integrator=lsm.SemiImplicitI2OE())
    pre, post = [], []
    lsm.integrate_(eq, 0.4, prehook=lambda e: pre.append(e.current_time()), posthook=lambda e: post.append(e.current_time()))
    rpre, rpost = [], []
    ref, steps = R.integrate(u0, lc, hc, (("neumann", "neumann"),) * 2, lambda t: vel(X, t), 2.0, 0.4, prehook=rpre.append, posthook=rpost.append)
    assert len(pre) == len(post) == steps > 1
    np.testing.assert_allclose(pre, rpre, rtol=1e-12)
    np.testing.assert_allclose(post, rpost, rtol=1e-12)
    assert np.abs(eq.current_state().values() - ref).max() <= 1e-8 * np.abs(ref).max()


def test_float32_storage(lsm):
    out = {}
    for dt in (np.float64, np.float32):
        _, dev, ref = _one_step(lsm, (33, 29), ("PP", "LL"), "rotation", 2.0, "fast", dtype=dt)
        out[dt] = dev
    assert out[np.float32].dtype == np.float32
    assert np.abs(out[np.float32].astype(np.float64) - out[np.float64]).max() <= 1e-6 * np.abs(out[np.float64]).max()


def test_vortex_160_residual(lsm):
    """A 160³ step of the vortex (vortex_deformation) at cfl 2: the device result satisfies the reference's system,
    checked matrix-free on the host (no direct solve at this size)."""
    n = (160, 160, 160)
    lc, hc = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    grid = lsm.CartesianGrid(lc, hc, n)
    X = np.meshgrid(*R.node_coords(lc, hc, n), indexing="ij", sparse=True)
    u0 = np.sqrt((X[0] - 0.35) ** 2 + (X[1] - 0.35) ** 2 + (X[2] - 0.35) ** 2) - 0.15
    coeff = lsm.vortex_deformation(grid)
    t0 = 0.3
    eq = lsm.LevelSetEquation(terms=lsm.AdvectionTerm(coeff), ic=lsm.MeshField(u0, grid), bc=lsm.NeumannBC(),
                              integrator=lsm.SemiImplicitI2OE(), t=t0)
    h = R.meshsize(lc, hc, n)
    g = math.cos(math.pi * t0 / 3.0)
    vel = []
    for c in range(3):
        T = coeff.tables[c]
        vel.append(((T[0][:, None, None] * T[1][None, :, None]) * T[2][None, None, :]) * g)
    dt = 2.0 * R.advection_cfl(vel, h)
    lsm.integrate_(eq, t0 + dt, dt)
    res, b = R.residual_norms(eq.current_state().values(), u0, vel, h, (("neumann", "neumann"),) * 3, dt)
    assert res <= 1e-12 * b, (res, b, eq.i2oe_last)


def test_not_converged_is_reported(lsm):
    lc, hc, n = (0.0, 0.0), (1.0, 1.0), (48, 48)
    X = np.meshgrid(*R.node_coords(lc, hc, n), indexing="ij")
    u0 = np.hypot(X[0] - 0.4, X[1] - 0.5) - 0.2
    grid = lsm.CartesianGrid(lc, hc, n)
    eq = lsm.LevelSetEquation(terms=lsm.AdvectionTerm(lsm.RigidRotation(1.0, (0.5, 0.5))), ic=lsm.MeshField(u0, grid), bc=lsm.PeriodicBC(),
                              integrator=lsm.SemiImplicitI2OE(max_iters=1))
    with pytest.raises(lsm.LsmNotConvergedError, match="1 iterations, relative residual"):
        lsm.integrate_(eq, 0.5)
    assert eq.current_time() == 0.0
    np.testing.assert_array_equal(eq.current_state().values(), u0)
    assert lsm._lib.ERR_NOT_CONVERGED == -5
