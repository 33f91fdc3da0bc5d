"""SemiLagrangian on the device (lsm_advance_semilag) against the numpy restatement of DESIGN.md §7.30 (tests/_semilag_ref.py),
bit for bit: single steps over dimensions, launch shapes, boundary kinds, velocity kinds, orders, traces, the limiter,
displacements, Float32 storage and both arithmetic modes; the staged and the direct kernel against each other; non-finite
velocities; the exact shift; ten steps through integrate_ with a hook; every refusal; and one step at 96³.

Not reachable from here, so not tested: fewer than 2 nodes in a dimension and an axis periodic on one face only (lsm_create
refuses both before a handle exists), and a handle with a communicator (it is a slab handle, which is tested)."""
import math

import numpy as np
import pytest

import _semilag_ref as R

pytestmark = pytest.mark.gpu

BC_NAMES = {"P": "periodic", "N": "neumann", "L": "linear", "S": "symmetry", "E": ("extrapolation", 2)}


@pytest.fixture(scope="module")
def lsm():
    import lsm_amd
    return lsm_amd


def _bc_obj(lsm, c):
    return {"P": lsm.PeriodicBC(), "N": lsm.NeumannBC(), "L": lsm.LinearExtrapolationBC(), "S": lsm.SymmetryBC(), "E": lsm.ExtrapolationBC(2)}[c]


def _coords(lc, hc, n):
    h = R.meshsize(lc, hc, n)
    return np.meshgrid(*[lc[d] + np.arange(n[d]) * h[d] for d in range(len(n))], indexing="ij")


def _velocity(lsm, kind, lc, hc, n):
    """(spec for AdvectionTerm, spec for the restatement)"""
    N = len(n)
    X = _coords(lc, hc, n)
    if kind == "rotation" and N == 1:
        kind = "field"
    if kind == "const":
        c = (0.8, -0.45, 0.3)[:N]
        return c, ("const", c)
    if kind == "rotation":
        return lsm.RigidRotation(1.3, (0.1, -0.2)), ("rotation", 1.3, 0.1, -0.2)
    if kind == "separable":
        rng = np.random.default_rng(7)
        tabs = [[rng.uniform(-1, 1, n[d]) for d in range(N)] for _ in range(N)]
        return lsm.SeparableCoefficient(tabs, time=("cos", 1.7)), ("separable", tabs, R.cos_factor(1.7))
    vals = np.stack([np.broadcast_to(np.sin(2.1 * X[(d + 1) % N] + 0.3 * d) * 1.2 + 0.2 + 0.1 * np.cos(3 * X[d]), n) for d in range(N)])
    return lsm.MeshField(vals, lsm.CartesianGrid(lc, hc, n)), ("field", tuple(vals))


def _initial(lc, hc, n, dtype):
    X = _coords(lc, hc, n)
    N = len(n)
    u = np.sin(3 * X[0] + 0.5) + (np.cos(2 * X[1]) if N > 1 else 0) + (X[2] ** 2 if N > 2 else 0)
    u = u + 0.05 * np.random.default_rng(3).uniform(-1, 1, n)
    return np.asfortranarray(u.astype(dtype))


def _equation(lsm, n, bcs, vkind, dtype=np.float64, mode="fast", tuning=None, integrator=None):
    N = len(n)
    lc, hc = tuple(-0.5 - 0.1 * d for d in range(N)), tuple(1.0 + 0.2 * d for d in range(N))
    spec, rvel = _velocity(lsm, vkind, lc, hc, n)
    u0 = _initial(lc, hc, n, dtype)
    bc = tuple((_bc_obj(lsm, a), _bc_obj(lsm, b)) for a, b in bcs)
    eq = lsm.LevelSetEquation(terms=lsm.AdvectionTerm(spec, lsm.Upwind()), ic=lsm.MeshField(u0, lsm.CartesianGrid(lc, hc, n)), bc=bc,
                              integrator=integrator or lsm.SemiLagrangian(), mode=mode, tuning=tuning)
    return eq, u0, rvel, lc, hc, tuple((BC_NAMES[a], BC_NAMES[b]) for a, b in bcs)


def _dt_for(rvel, n, lc, hc, t, cells):
    """Δt that moves the fastest node `cells` cells along its fastest dimension"""
    h = R.meshsize(lc, hc, n)
    u = R.vel_node(rvel, n, lc, h, t)
    return cells / max(float(np.abs(u[d]).max()) / h[d] for d in range(len(n)))


def _device_step(lsm, eq, tc, dt, order, trace, limiter):
    out = eq.backend.alloc()
    out.fill_(-7.0)
    stats = eq.backend.advance_semilag(lsm.api._terms_c(eq.terms), eq.state.buf, out, tc, dt, order, trace, limiter)
    return eq.backend.download(out), stats


SHAPES = [
    ((9,), ("PP",)), ((9,), ("NL",)), ((9,), ("SE",)),
    ((13, 10), ("PP", "PP")), ((13, 10), ("NN", "LL")), ((13, 10), ("SL", "EN")), ((13, 10), ("PP", "SS")),
    ((9, 7, 6), ("PP", "PP", "PP")), ((9, 7, 6), ("NN", "LL", "SS")), ((9, 7, 6), ("EL", "PP", "NS")),
    ((130, 12), ("PP", "NL")), ((130, 12), ("LS", "PP")),                  # several workgroups along x
    ((70, 9, 9), ("NN", "PP", "EE")), ((70, 9, 9), ("PP", "SL", "NN")),
    ((9, 9, 11), ("LL", "NN", "PP")), ((9, 9, 11), ("SS", "EE", "LN")),    # three workgroups along the slowest axis
]
VKINDS = ["const", "rotation", "separable", "field"]


def _pruned():
    """every shape twice; the other factors cycle with different periods, so every value of every factor meets every shape class"""
    cases = []
    for p in range(2):
        for k, (n, bcs) in enumerate(SHAPES):
            q = k + 5 * p
            disp = [0.5, 4.0, max(n) + 2.5][(q // 2 + p) % 3]
            cases.append((n, bcs, VKINDS[(q + p) % 4], [1, 3, 5][q % 3], 1 + (q // 3 + p) % 2, q % 5 != 0, disp))
    return cases


def _id(x):
    return str(x).replace(" ", "").replace("'", "")


@pytest.mark.parametrize("n, bcs, vkind, order, trace, limiter, cells", _pruned(), ids=_id)
def test_one_step_equals_the_restatement(lsm, n, bcs, vkind, order, trace, limiter, cells):
    eq, u0, rvel, lc, hc, rbcs = _equation(lsm, n, bcs, vkind)
    tc = 0.25
    dt = _dt_for(rvel, n, lc, hc, tc, cells)
    ref = R.step(u0, rvel, lc, hc, rbcs, tc, dt, order, trace, limiter)
    assert eq.backend.get_tuning("LSM_SEMILAG_STAGE") == 0   # the direct kernel is the default; the staged one first
    eq.backend.set_tuning("LSM_SEMILAG_STAGE", 1)
    dev, stats = _device_step(lsm, eq, tc, dt, order, trace, limiter)
    np.testing.assert_array_equal(dev, ref)
    _, disp = R.trace(rvel, n, lc, hc, rbcs, tc, dt, trace)
    assert stats[0] + stats[1] > 0 and stats[2] == math.ceil(disp)
    # the direct kernel: the same bits
    eq.backend.set_tuning("LSM_SEMILAG_STAGE", 0)
    direct, dstats = _device_step(lsm, eq, tc, dt, order, trace, limiter)
    np.testing.assert_array_equal(direct, ref)
    wgs = -(-n[0] // 256) if len(n) == 1 else -(-n[0] // 64) * -(-n[1] // 4) * (n[2] if len(n) == 3 else 1)   # 64 × 4 nodes of one plane
    assert dstats[0] == 0 and dstats[1] == wgs and dstats[2] == stats[2]


STORAGE_CASES = [
    ((9,), ("NL",), "field", 3, 2, True, 4.0), ((13, 10), ("PP", "SS"), "separable", 5, 2, False, 0.5),
    ((13, 10), ("SL", "EN"), "rotation", 3, 1, True, 4.0), ((9, 7, 6), ("NN", "LL", "SS"), "field", 3, 2, True, 4.0),
    ((70, 9, 9), ("PP", "SL", "NN"), "separable", 1, 2, True, 72.5), ((9, 9, 11), ("SS", "EE", "LN"), "const", 5, 1, False, 0.5),
]


@pytest.mark.parametrize("n, bcs, vkind, order, trace, limiter, cells", STORAGE_CASES, ids=_id)
def test_float32_storage_widens_computes_in_fp64_and_rounds_once(lsm, n, bcs, vkind, order, trace, limiter, cells):
    eq, u0, rvel, lc, hc, rbcs = _equation(lsm, n, bcs, vkind, dtype=np.float32)
    dt = _dt_for(rvel, n, lc, hc, 0.25, cells)
    ref = R.step(u0, rvel, lc, hc, rbcs, 0.25, dt, order, trace, limiter, storage=np.float32)
    dev, _ = _device_step(lsm, eq, 0.25, dt, order, trace, limiter)
    assert dev.dtype == np.float32
    np.testing.assert_array_equal(dev, ref)


@pytest.mark.parametrize("n, bcs, vkind, order, trace, limiter, cells", STORAGE_CASES, ids=_id)
def test_strict_and_fast_handles_give_the_same_bits(lsm, n, bcs, vkind, order, trace, limiter, cells):
    eq, u0, rvel, lc, hc, rbcs = _equation(lsm, n, bcs, vkind, mode="strict")
    dt = _dt_for(rvel, n, lc, hc, 0.25, cells)
    ref = R.step(u0, rvel, lc, hc, rbcs, 0.25, dt, order, trace, limiter)
    dev, _ = _device_step(lsm, eq, 0.25, dt, order, trace, limiter)
    np.testing.assert_array_equal(dev, ref)


# ----------------------------------------------------------------------------- the two paths
@pytest.mark.parametrize("n, bcs, order", [((130, 12), ("NN", "LL"), 3), ((70, 9, 9), ("NN", "SS", "LL"), 5), ((40, 20, 11), ("LL", "NN", "EE"), 3),
                                           ((600,), ("NN",), 5)], ids=_id)
def test_direct_and_staged_kernels_agree_where_every_box_fits(lsm, n, bcs, order):
    outs = {}
    for stage in (0, 2):
        eq, u0, rvel, lc, hc, rbcs = _equation(lsm, n, bcs, "field", tuning={"LSM_SEMILAG_STAGE": stage})
        dt = _dt_for(rvel, n, lc, hc, 0.0, 2.0)
        outs[stage], stats = _device_step(lsm, eq, 0.0, dt, order, 2, True)
        assert (stats[0] == 0) == (stage == 0) and (stats[1] == 0) == (stage == 2)
    np.testing.assert_array_equal(outs[0], outs[2])
    np.testing.assert_array_equal(outs[2], R.step(u0, rvel, lc, hc, rbcs, 0.0, dt, order, 2, True))


def _shear(lsm, tuning=None):
    """rows 0..31 of a 400 × 64 grid stand still, rows 32..63 move up to 300 cells along x: the workgroups of the upper tiles
    cannot stage their departure boxes (32 rows × 300 cells and the halo are more than the LDS budget), the lower ones can"""
    n, lc, hc = (400, 64), (0.0, 0.0), (399 * 0.01, 63 * 0.02)
    ramp = np.concatenate([np.zeros(32), np.linspace(0.0, 1.0, 32)])
    tabs = [[np.ones(400), ramp], [np.zeros(400), np.zeros(64)]]
    X = _coords(lc, hc, n)
    u0 = np.asfortranarray(np.sin(5 * X[0]) * np.cos(3 * X[1]) + 0.1 * np.random.default_rng(5).uniform(-1, 1, n))
    eq = lsm.LevelSetEquation(terms=lsm.AdvectionTerm(lsm.SeparableCoefficient(tabs, time=("cos", 2.0)), lsm.Upwind()),
                              ic=lsm.MeshField(u0, lsm.CartesianGrid(lc, hc, n)), bc=(lsm.PeriodicBC(), lsm.NeumannBC()),
                              integrator=lsm.SemiLagrangian(), tuning=tuning)
    rvel = ("separable", tabs, R.cos_factor(2.0))
    rbcs = (("periodic", "periodic"), ("neumann", "neumann"))
    dt = 300 * 0.01 / math.cos(math.pi * 0.05 / 2.0)
    return eq, u0, rvel, lc, hc, rbcs, dt


def test_a_shear_takes_both_paths_in_one_launch(lsm):
    """at setting 1: at the default setting, 0, no workgroup stages"""
    eq, u0, rvel, lc, hc, rbcs, dt = _shear(lsm, tuning={"LSM_SEMILAG_STAGE": 1})
    dev, stats = _device_step(lsm, eq, 0.0, dt, 3, 1, True)
    assert stats[0] > 0 and stats[1] > 0, stats
    np.testing.assert_array_equal(dev, R.step(u0, rvel, lc, hc, rbcs, 0.0, dt, 3, 1, True))


def test_forced_staging_refuses_a_box_that_does_not_fit(lsm):
    eq, u0, rvel, lc, hc, rbcs, dt = _shear(lsm, tuning={"LSM_SEMILAG_STAGE": 2})
    out = eq.backend.alloc()
    out.fill_(-7.0)
    before = eq.state.values()
    with pytest.raises(lsm.LsmError, match="do not fit"):
        eq.backend.advance_semilag(lsm.api._terms_c(eq.terms), eq.state.buf, out, 0.0, dt, 3, 1, True)
    assert bool((out == -7.0).all())
    np.testing.assert_array_equal(eq.state.values(), before)
    with pytest.raises(lsm.LsmError):
        eq.backend.set_tuning("LSM_SEMILAG_STAGE", 3)


# ----------------------------------------------------------------------------- non-finite velocities
@pytest.mark.parametrize("trace", [1, 2])
@pytest.mark.parametrize("bcs", [("NN", "LL"), ("PP", "NN")], ids=_id)
def test_non_finite_velocity_nodes(lsm, bcs, trace):
    """the cell index is formed from values in range only and clamped as an integer (sl_cell): a NaN departure point reads cell 0
    and gives NaN, an infinite one reads the boundary on a clamped axis and gives NaN on a periodic one"""
    n = (13, 10)
    eq, u0, rvel, lc, hc, rbcs = _equation(lsm, n, bcs, "field")
    vals = np.array(rvel[1])
    vals[0][4, 5] = np.nan
    vals[0][9, 2] = np.inf
    eq.terms[0].coeff.set_values(vals)
    rvel = ("field", tuple(vals))
    dt = 0.03
    ref = R.step(u0, rvel, lc, hc, rbcs, 0.0, dt, 3, trace, True)
    for stage in (1, 0):
        eq.backend.set_tuning("LSM_SEMILAG_STAGE", stage)
        dev, stats = _device_step(lsm, eq, 0.0, dt, 3, trace, True)
        np.testing.assert_array_equal(dev, ref)
        if trace == 1:
            assert stats[2] == 2 ** 63 - 1   # the infinite node's displacement saturates the counter
    bad = np.isnan(ref)
    assert np.isfinite(ref[~bad]).all()
    if trace == 1:
        want = np.zeros(n, dtype=bool)
        want[4, 5] = True
        want[9, 2] = bcs[0] == "PP"
        np.testing.assert_array_equal(bad, want)
    else:
        assert bad[4, 5] and 1 <= bad.sum() <= 24   # the nodes whose midpoint lies in a cell that touches a bad node


# ----------------------------------------------------------------------------- through integrate_
@pytest.mark.parametrize("trace", [1, 2])
@pytest.mark.parametrize("limiter", [True, False])
@pytest.mark.parametrize("order", [1, 3, 5])
def test_exact_shift_2d(lsm, order, limiter, trace):
    n = (17, 33)
    u = np.random.default_rng(1).uniform(-1, 1, n)
    u[-1, :] = u[0, :]
    u[:, -1] = u[:, 0]
    eq = lsm.LevelSetEquation(terms=lsm.AdvectionTerm((1.0, -2.0)), ic=lsm.MeshField(np.asfortranarray(u), lsm.CartesianGrid((0, 0), (1, 1), n)),
                              bc=lsm.PeriodicBC(), integrator=lsm.SemiLagrangian(cfl=1e9, order=order, trace=trace, limiter=limiter))
    lsm.integrate_(eq, 3 / 16, 3 / 16)
    i, j = np.meshgrid(np.arange(17), np.arange(33), indexing="ij")
    np.testing.assert_array_equal(eq.current_state().values(), u[(i - 3) % 16, (j + 12) % 32])
    assert eq.semilag_last[2] == 12


@pytest.mark.parametrize("trace", [1, 2])
@pytest.mark.parametrize("limiter", [True, False])
@pytest.mark.parametrize("order", [1, 3, 5])
def test_exact_shift_3d(lsm, order, limiter, trace):
    n = (9, 9, 9)
    u = np.random.default_rng(2).uniform(-1, 1, n)
    u[-1] = u[0]
    u[:, -1] = u[:, 0]
    u[:, :, -1] = u[:, :, 0]
    eq = lsm.LevelSetEquation(terms=lsm.AdvectionTerm((1.0, -1.0, 2.0)), ic=lsm.MeshField(np.asfortranarray(u), lsm.CartesianGrid((0, 0, 0), (1, 1, 1), n)),
                              bc=lsm.PeriodicBC(), integrator=lsm.SemiLagrangian(cfl=1e9, order=order, trace=trace, limiter=limiter))
    lsm.integrate_(eq, 1 / 4, 1 / 4)
    i, j, k = np.meshgrid(*[np.arange(9)] * 3, indexing="ij")
    np.testing.assert_array_equal(eq.current_state().values(), u[(i - 2) % 8, (j + 2) % 8, (k - 4) % 8])


def test_ten_steps_with_a_hook_that_rewrites_the_velocity(lsm):
    n, lc, hc = (21, 18), (-0.5, -0.6), (1.0, 1.2)
    X = _coords(lc, hc, n)
    vel = lambda t: np.stack([np.sin(2 * X[1] + t) + 0.3, np.cos(3 * X[0] - 2 * t) * 0.8])
    u0 = _initial(lc, hc, n, np.float64)
    grid = lsm.CartesianGrid(lc, hc, n)
    seen = []

    def update(coeff, field, t):
        seen.append(t)
        coeff.set_values(vel(t))
    eq = lsm.LevelSetEquation(terms=lsm.AdvectionTerm(lsm.MeshField(vel(0.0), grid), lsm.Upwind(), update), ic=lsm.MeshField(u0, grid),
                              bc=(lsm.NeumannBC(), lsm.LinearExtrapolationBC()), integrator=lsm.SemiLagrangian(cfl=1e9))
    dt, tf = 0.07, 0.7 - 1e-3
    posts = []
    lsm.integrate_(eq, tf, dt, posthook=lambda ls: posts.append((ls.t, ls.state.ghosts_dirty)))
    u, tc, steps = u0, 0.0, 0
    rbcs = (("neumann", "neumann"), ("linear", "linear"))
    times = []
    while tc <= tf - np.spacing(tc):
        times.append(tc)
        s = min(dt, tf - tc)
        u = R.step(u, ("field", tuple(vel(tc))), lc, hc, rbcs, tc, s)
        tc += s
        steps += 1
    assert steps == 10 and len(posts) == 10 and seen == times
    assert all(d for _, d in posts) and eq.state.ghosts_dirty
    assert eq.t == tf and eq.current_time() == tf
    np.testing.assert_array_equal(eq.current_state().values(), u)
    # the ghost state is handled: measures and reinitialize! run as usual
    v = lsm.volume(eq)
    assert np.isfinite(v) and v > 0
    lsm.reinitialize_(eq)
    assert np.isfinite(eq.current_state().values()).all()


# ----------------------------------------------------------------------------- refusals
def test_the_c_abi_refuses_bad_arguments_and_writes_nothing(lsm):
    L = lsm._lib
    eq, u0, rvel, lc, hc, rbcs = _equation(lsm, (13, 10), ("NN", "LL"), "field")
    b = eq.backend
    out = b.alloc()
    out.fill_(-7.0)
    phi = b.clone(eq.state.buf)
    adv = lsm.api._terms_c(eq.terms)
    nm = lsm.api._terms_c(eq.terms)
    nm[0].kind = L.TERM_NORMAL_MOTION
    P, O = b.ptr(eq.state.buf), b.ptr(out)
    call = b.lib.lsm_advance_semilag
    bad = [
        (adv, P, P, 0.0, 0.01, 3, 2), (adv, None, O, 0.0, 0.01, 3, 2), (adv, P, None, 0.0, 0.01, 3, 2), (None, P, O, 0.0, 0.01, 3, 2),
        (nm, P, O, 0.0, 0.01, 3, 2), (adv, P, O, 0.0, 0.01, 2, 2), (adv, P, O, 0.0, 0.01, 7, 2), (adv, P, O, 0.0, 0.01, 3, 0),
        (adv, P, O, 0.0, 0.01, 3, 3), (adv, P, O, 0.0, -0.01, 3, 2), (adv, P, O, 0.0, float("nan"), 3, 2), (adv, P, O, 0.0, float("inf"), 3, 2),
    ]
    for term, p, o, tc, dt, order, trace in bad:
        assert call(b.h, term, p, o, tc, dt, order, trace, 1, None) == L.ERR_INVALID, (order, trace, dt)
    assert call(None, adv, P, O, 0.0, 0.01, 3, 2, 1, None) == L.ERR_INVALID
    assert bool((out == -7.0).all()) and bool((eq.state.buf == phi).all())   # ghosts included: nothing ran
    np.testing.assert_array_equal(eq.state.values(), u0)
    # a slab handle
    from lsm_amd.backend import HipBackend
    grid = lsm.CartesianGrid(lc, hc, (13, 10))
    sb = HipBackend(grid._c(), lsm.api._bc_c(eq.bcs, 2, (False, True)), slab=(0, 6))
    a, c = sb.alloc(), sb.alloc()
    const = (L.LsmTerm * 1)()
    const[0].kind = L.TERM_ADVECTION
    const[0].coeff.kind = L.COEFF_CONST
    assert call(sb.h, const, sb.ptr(a), sb.ptr(c), 0.0, 0.01, 3, 2, 1, None) == L.ERR_INVALID
    assert b"slab" in sb.lib.lsm_last_error(sb.h)


def test_the_python_layer_refuses_before_any_step(lsm):
    grid = lsm.CartesianGrid((0.0, 0.0), (1.0, 1.0), (21, 17))
    ic = lsm.MeshField(lambda x: np.hypot(x[0] - 0.5, x[1] - 0.5) - 0.25, grid)
    adv = lambda: lsm.AdvectionTerm((1.0, 0.5), lsm.Upwind())

    def refused(match, **kw):
        kw.setdefault("terms", adv())
        kw.setdefault("integrator", lsm.SemiLagrangian())
        kw.setdefault("ic", ic)
        eq = lsm.LevelSetEquation(bc=lsm.NeumannBC(), **kw)
        before = eq.current_state().values()
        with pytest.raises(ValueError, match=match):
            lsm.integrate_(eq, 0.1)
        np.testing.assert_array_equal(eq.current_state().values(), before)
        assert eq.t == 0
        return eq
    refused("exactly one AdvectionTerm", terms=(adv(), lsm.CurvatureTerm(-0.1)))
    refused("exactly one AdvectionTerm", terms=lsm.NormalMotionTerm(1.0))
    refused("full-grid", ic=lsm.NarrowBandMeshField(ic, nlayers=4))
    for order in (0, 2, 4, 7, 3.5, True):
        refused("order must be", integrator=lsm.SemiLagrangian(order=order))
    for trace in (0, 3, True):
        refused("trace must be", integrator=lsm.SemiLagrangian(trace=trace))
    # a slab decomposition: the equation says it has peers
    eq = lsm.LevelSetEquation(terms=adv(), ic=ic, bc=lsm.NeumannBC(), integrator=lsm.SemiLagrangian())
    eq.comm, eq.world = object(), 2
    with pytest.raises(ValueError, match="single device"):
        lsm.api._validate_semilag(eq)
    eq.comm, eq.world = None, 1
    lsm.integrate_(eq, 0.05)
    assert eq.t == 0.05 and eq.semilag_last[0] + eq.semilag_last[1] > 0
    # without the counters: the same bits, nothing to read back
    quiet = lsm.LevelSetEquation(terms=adv(), ic=ic, bc=lsm.NeumannBC(), integrator=lsm.SemiLagrangian(stats=False))
    lsm.integrate_(quiet, 0.05)
    assert quiet.t == 0.05 and quiet.semilag_last is None and quiet.state.ghosts_dirty
    np.testing.assert_array_equal(quiet.current_state().values(), eq.current_state().values())


# ----------------------------------------------------------------------------- a large launch
def test_one_step_at_96_cubed(lsm):
    """many workgroups on every axis: the default path (the direct kernel, 2 × 24 × 96 workgroups), then the staged one (3 × 12 × 24
    tiles); the restatement takes about two seconds here"""
    n = (96, 96, 96)
    eq, u0, rvel, lc, hc, rbcs = _equation(lsm, n, ("NN", "PP", "LL"), "separable")
    dt = _dt_for(rvel, n, lc, hc, 0.25, 4.0)
    ref = R.step(u0, rvel, lc, hc, rbcs, 0.25, dt, 3, 2, True)
    dev, stats = _device_step(lsm, eq, 0.25, dt, 3, 2, True)
    assert stats[:2] == (0, 2 * 24 * 96)
    np.testing.assert_array_equal(dev, ref)
    eq.backend.set_tuning("LSM_SEMILAG_STAGE", 1)
    dev, stats = _device_step(lsm, eq, 0.25, dt, 3, 2, True)
    assert stats[0] + stats[1] == 3 * 12 * 24
    np.testing.assert_array_equal(dev, ref)
