"""The auxiliary kernels of csrc/lsm_aux.hip that every user script calls — measure_kernel, the band_lines_* kernels,
geometry_kernel, signed_normals_kernel, eikonal_sign_kernel, extrema_kernel — against the CPU oracle and the exact sums of
tests/_measure_ref.py: float32 storage, stretched cells, periodic / Neumann / linear / per-face mixed boundary conditions,
vanishing gradients, grids above the launch caps (the grid-stride loops take a second trip), NaN entries, and the measures
of slab-decomposed equations.

The reference is never a device run.  float32 storage: the device widens exactly and computes in fp64, so the oracle gets
the float32-rounded values widened to fp64 and the fp64 tolerances hold unchanged.  One thing the oracle's dense ϕ[I] does
not model: a float32 field keeps its ghost layers in float32 too (tests/test_gpu_f32.py: "what the device holds"), so a
ghost behind a weighted extrapolation face (LinearExtrapolationBC, ExtrapolationBC(2)) is the oracle's value rounded once
more.  There the reference reads the oracle's ghost fill rounded to float32 (`_held`): _measure_ref.geometry_padded, which
tests/test_geometry.py checks against the oracle, and _measure_ref.perimeter.  Copy faces (periodic, Neumann, symmetry) are
exact and compare with the oracle directly.

Tolerances (the project's own: tests/test_geometry.py, test_velocity_extension.py, test_gpu_api.py, test_gpu_narrowband.py):
gradient, eikonal_sign, frozen mask: bit for bit; normal: 4e-16 absolute; curvature: 1e-13·max|κ_ref| (pow(q, 1.5) of the
device's libm against the host's); measures: 1e-12 relative; extension: STRICT bit for bit, FAST 1e-12·max(1, |F|)."""
import functools
import math
import threading

import numpy as np
import pytest

import _measure_ref as mref

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
EPS = 2.220446049250313e-16
LC, HC = (-1.0, -0.7, -0.4), (1.1, 0.9, 0.85)          # hc - lc = 2.1, 1.6, 1.25: every axis has its own cell size


@pytest.fixture(scope="module")
def lsm():
    import lsm_amd
    return lsm_amd


def _bc(lsm, name, nd):
    """(host-API boundary conditions, the oracle's spec of the same)."""
    N, Lin, P, S, E2 = lsm.NeumannBC(), lsm.LinearExtrapolationBC(), lsm.PeriodicBC(), lsm.SymmetryBC(), lsm.ExtrapolationBC(2)
    if name != "mixed":
        return {"periodic": P, "neumann": N, "linear": Lin}[name], name
    return {1: (((N, Lin),), (("neumann", "linear"),)),
            2: (((Lin, N), (E2, S)), (("linear", "neumann"), (("extrapolation", 2), "symmetry"))),
            3: (((N, Lin), P, (S, E2)), (("neumann", "linear"), "periodic", ("symmetry", ("extrapolation", 2))))}[nd]


def _copy_faces(bcname):
    return bcname in ("periodic", "neumann")


def _grid(orc, shape, lc=LC, hc=HC):
    nd = len(shape)
    return orc.Grid(lc[:nd], hc[:nd], shape)


def _stored(vals, dtype):
    """The values a field of this storage type holds, widened to fp64."""
    return np.asfortranarray(np.asarray(vals).astype(dtype).astype(F64))


def _equation(lsm, og, vals, lbc, dtype=F64, mode="fast", band=False, **kw):
    lg = lsm.CartesianGrid(og.lc, og.hc, og.n)
    ic = lsm.MeshField(np.asfortranarray(vals), lg, dtype=dtype)
    if band:
        ic = lsm.NarrowBandMeshField(ic, nlayers=3)
    return lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=ic, bc=lbc, mode=mode, **kw)


def _held(orc, og, obc, p, dtype):
    """The field as the device holds it after its ghost fill, with ONE ghost layer (edges and corners included): the
    oracle's fill of the padded layout, rounded to the storage type."""
    lay = orc.layout(og)
    full = orc.fill_ghosts_padded(og, obc, lay, orc.to_padded(lay, og.ndim, p))
    g = orc.GHOST - 1
    return _stored(full[(slice(g, -g),) * og.ndim], dtype)


def _tilted(og):
    """A tilted plane plus small sinusoids: smooth, crosses zero, |∇ϕ| >= 0.5 at every node under every BC used here."""
    X = np.meshgrid(*og.coords(), indexing="ij")
    a = (1.6, 1.3, -1.4)
    phi = sum(a[d] * (x - 0.5 * (og.lc[d] + og.hc[d]) - 0.03 * (d + 1)) for d, x in enumerate(X))
    phi = phi + 0.05 * np.sin(3.0 * X[0] + 1.0) + 0.04 * np.cos(2.5 * X[-1] - 0.3)
    return np.asfortranarray(phi)


def _geometry_refs(orc, og, obc, bcname, p, dtype):
    """(κ, ∇ϕ, n) of the stored field p: the oracle; for float32 storage behind weighted faces the restatement on `_held`."""
    if dtype == F64 or _copy_faces(bcname):
        return tuple(orc.geometry(og, obc, p, w) for w in ("curvature", "gradient", "normal"))
    held, h = _held(orc, og, obc, p, dtype), og.meshsize()
    return tuple(mref.geometry_padded(held, h, w) for w in ("curvature", "gradient", "normal"))


def _check_geometry(lsm, st, refs, scales=(1.0,)):
    wk, wg, wn = refs
    for s in scales:
        got = lsm.curvature_field(st, scale=s).values()
        assert np.abs(got - s * wk).max() <= 1e-13 * np.abs(s * wk).max(), ("curvature", s)
        for d, f in enumerate(lsm.gradient_field(st, scale=s)):
            assert np.array_equal(f.values(), s * wg[d]), ("gradient", s, d)
        for d, f in enumerate(lsm.normal_field(st, scale=s)):
            assert np.abs(f.values() - s * wn[d]).max() <= 4e-16, ("normal", s, d)


# ------------------------------------------------------------------------------------------------- a. geometry matrix

@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("bcname", ["periodic", "neumann", "linear", "mixed"])
@pytest.mark.parametrize("shape", [(67,), (45, 37), (23, 19, 21), (9, 7, 5)], ids=str)
def test_geometry_matrix(lsm, orc, shape, bcname, dtype):
    """curvature / gradient / normal at every node, scale 1 and -2, on stretched cells; in 2-D and 3-D also the seed form
    of curvature_field: band, fill and the frozen mask."""
    nd = len(shape)
    og = _grid(orc, shape)
    lbc, ospec = _bc(lsm, bcname, nd)
    obc = orc.make_bc(ospec, nd)
    p = _stored(_tilted(og), dtype)
    refs = _geometry_refs(orc, og, obc, bcname, p, dtype)
    gn = np.sqrt(sum(g * g for g in refs[1]))
    assert gn.min() >= 0.5 and np.abs(refs[0]).max() <= 100.0, (gn.min(), np.abs(refs[0]).max())   # the κ bound means something
    st = _equation(lsm, og, p, lbc, dtype).current_state()
    _check_geometry(lsm, st, refs, scales=(1.0, -2.0))
    if nd == 1:
        return
    band = 1.5 * min(og.meshsize())
    on = np.abs(p) <= band
    assert on.sum() >= 8 and (~on).sum() >= 8
    fz = lsm.SideField(st.backend, st.mesh)
    got = lsm.curvature_field(st, scale=-2.0, band=band, fill=-7.0, frozen_out=fz).values()
    assert np.array_equal(fz.values(), on.astype(F64))
    assert np.array_equal(got[~on], np.full((~on).sum(), -7.0))
    assert np.abs(got[on] + 2.0 * refs[0][on]).max() <= 1e-13 * np.abs(2.0 * refs[0][on]).max()


# ------------------------------------------------------------------------------------------------- b. vanishing gradient

@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(67,), (45, 37), (9, 7, 5)], ids=str)
def test_constant_field_has_zero_curvature_and_the_oracles_nan_normal(lsm, orc, shape, dtype):
    nd = len(shape)
    og = _grid(orc, shape)
    p = _stored(np.full(shape, 0.3), dtype)
    st = _equation(lsm, og, p, lsm.LinearExtrapolationBC(), dtype).current_state()
    assert np.array_equal(lsm.curvature_field(st).values(), np.zeros(shape))          # src/levelsetops.jl:201
    want = orc.geometry(og, orc.make_bc("linear", nd), p, "normal")                     # 0/0 at every node
    assert all(np.isnan(w).all() for w in want)
    for d, f in enumerate(lsm.normal_field(st)):
        assert np.array_equal(f.values(), want[d], equal_nan=True)
    for f in lsm.gradient_field(st):
        assert np.array_equal(f.values(), np.zeros(shape))


@pytest.mark.parametrize("shape", [(67,), (45, 37), (9, 7, 5)], ids=str)
def test_curvature_on_both_sides_of_the_small_gradient_switch(lsm, orc, shape):
    """ϕ = ε·x₁ with ε² just below and just above eps(Float64): κ = 0 by the switch below it, the full formula above it."""
    nd = len(shape)
    og = _grid(orc, shape)
    obc = orc.make_bc("linear", nd)
    x = np.meshgrid(*og.coords(), indexing="ij")[0]
    for side, factor in (("below", 1.0 - 1e-6), ("above", 1.0 + 1e-6)):
        p = np.asfortranarray(math.sqrt(EPS) * factor * x)
        g = orc.geometry(og, obc, p, "gradient")
        nrmsq = sum(gd * gd for gd in g)
        assert (nrmsq < EPS).all() if side == "below" else (nrmsq > EPS).all(), side
        want = orc.geometry(og, obc, p, "curvature")
        st = _equation(lsm, og, p, lsm.LinearExtrapolationBC()).current_state()
        got = lsm.curvature_field(st).values()
        if side == "below":
            assert np.array_equal(want, np.zeros(shape)) and np.array_equal(got, want)
        else:
            assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), side


# ------------------------------------------------------------------------------------------------- c. launch caps

CAP_SHAPES = {2: (1450, 1449), 3: (131, 127, 127)}     # 2 101 050 and 2 112 899 nodes: above 8192·256, twice 4096·256


@functools.lru_cache(maxsize=None)
def _cap_case(nd):
    """Built once per module: the grid, the field in both storage types and the oracle's results for it."""
    from oracle import oracle as orc
    og = _grid(orc, CAP_SHAPES[nd])
    obc = orc.make_bc("neumann", nd)
    out = {"grid": og}
    for dtype in (F64, F32):
        p = _stored(_tilted(og), dtype)
        out[dtype] = (p, tuple(orc.geometry(og, obc, p, w) for w in ("curvature", "gradient", "normal")), orc.eikonal_sign(og, p))
    return out


def _check_cap_shape(lsm, orc, nd):
    case = _cap_case(nd)
    og = case["grid"]
    assert np.prod(og.n) > 8192 * 256
    for dtype in (F64, F32):
        p, refs, sign = case[dtype]
        st = _equation(lsm, og, p, lsm.NeumannBC(), dtype, mode="strict").current_state()
        _check_geometry(lsm, st, refs)
        s0 = lsm.SideField(st.backend, st.mesh)
        st.backend.eikonal_sign(st.buf, s0.buf)
        assert np.array_equal(s0.values(), sign)
    return case


def test_launch_caps_2d(lsm, orc):
    """(1450, 1449): every strided loop of the geometry and sign kernels takes a second trip."""
    _check_cap_shape(lsm, orc, 2)


def test_launch_caps_3d(lsm, orc):
    """(131, 127, 127); also extend_along_normals_ (band rule, three STRICT sweeps) through signed_normals_kernel."""
    case = _check_cap_shape(lsm, orc, 3)
    og = case["grid"]
    p = case[F64][0]
    X = np.meshgrid(*og.coords(), indexing="ij", sparse=True)
    F = np.asfortranarray(np.broadcast_to(np.sin(2 * X[0]) * np.cos(3 * X[1]) + X[2], og.shape).copy())
    want = F.copy(order="F")
    orc.extend_along_normals(og, orc.make_bc("neumann", 3), want, p, nb_iters=3, cfl=0.45)
    st = _equation(lsm, og, p, lsm.NeumannBC(), mode="strict").current_state()
    Fd = st.copy()
    Fd.copy_(lsm.MeshField(F, st.mesh))
    lsm.extend_along_normals_(Fd, st, nb_iters=3, cfl=0.45)
    assert np.array_equal(Fd.values(), want)


# ------------------------------------------------------------------------------------------------- d. extrema and range

@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(300,), (70, 65), (30, 20, 10)], ids=str)
def test_extrema_positions_and_nan_entries(lsm, orc, shape, dtype):
    og = _grid(orc, shape)
    base = _stored(np.random.default_rng(7).uniform(-1.0, 1.0, shape), dtype)
    fast = _equation(lsm, og, base, lsm.NeumannBC(), dtype)
    strict = _equation(lsm, og, base, lsm.NeumannBC(), dtype, mode="strict")
    st = fast.current_state()
    N = base.size
    for k in (0, N - 1, 63, 64, 255, 256):
        for v in (-5.0, 5.0):
            a = base.copy(order="F")
            a.reshape(-1, order="F")[k] = v                   # linear index in storage order (first index fastest)
            a = np.asfortranarray(a)
            st.copy_(lsm.MeshField(a, st.mesh, dtype=dtype))
            assert st.extrema() == (float(a.min()), float(a.max())), (k, v)
    a = base.copy(order="F")
    a.reshape(-1, order="F")[[0, 5, 63, 64, N // 2, N - 1]] = np.nan
    a = np.asfortranarray(a)
    a.reshape(-1, order="F")[[1, N - 2]] = (-3.0, 4.0)        # the extrema of the finite entries sit next to NaN entries
    a = np.asfortranarray(a)
    st.copy_(lsm.MeshField(a, st.mesh, dtype=dtype))
    assert st.extrema() == (-3.0, 4.0) == (float(np.nanmin(a)), float(np.nanmax(a)))
    assert st.backend.check_range(st.buf) == (True, 4.0)
    nan = np.full(shape, np.nan, order="F")
    for eq in (fast, strict):
        eq.current_state().copy_(lsm.MeshField(nan, st.mesh, dtype=dtype))
    assert strict.backend.check_range(strict.current_state().buf) == (True, 0.0)
    assert fast.backend.check_range(st.buf)[1] == 0.0


# ------------------------------------------------------------------------------------------------- e. dense measures

MEASURE_SHAPES = {1: (101,), 2: (64, 50), 3: (30, 26, 22)}
MLC, MHC = (-1.0, -0.8, -0.6), (1.3, 0.9, 0.7)


def _measure_fields(og):
    """name -> field.  `cut`: a body cut by two faces, so that the delta's support reaches the boundary nodes and the
    centred gradient reads BC ghosts; `edge`: nodes at ϕ = ±dmin exactly (the closed ends of the supports)."""
    nd, h = og.ndim, og.meshsize()
    dmin = min(h)
    X = np.meshgrid(*og.coords(), indexing="ij")
    L = [og.hc[d] - og.lc[d] for d in range(nd)]
    c = [0.5 * (og.lc[d] + og.hc[d]) + 0.013 * (d + 1) for d in range(nd)]
    body = np.sqrt(sum((x - c[d]) ** 2 for d, x in enumerate(X))) - 0.3 * min(L)
    if nd == 1:
        cut = np.minimum(X[0] - (og.lc[0] + 0.3 * h[0]), (og.hc[0] - 0.4 * h[0]) - X[0])
    else:
        cc = [og.lc[0] + 0.1 * L[0], og.lc[1] + 0.15 * L[1]] + c[2:]
        cut = np.sqrt(sum((x - cc[d]) ** 2 for d, x in enumerate(X))) - 0.3 * min(L)
    near = np.argwhere(np.abs(body) < 1.5 * dmin)
    edge = body.copy()
    edge[tuple(near[0])], edge[tuple(near[-1])] = dmin, -dmin
    nan = body.copy()
    nan[tuple(near[len(near) // 2])] = np.nan
    fields = {"body": body, "cut": cut, "edge": edge, "inside": -1.0 - 0.1 * X[0], "outside": 1.0 + 0.1 * X[0], "nan": nan}
    return {k: np.asfortranarray(v) for k, v in fields.items()}


def _measure_refs(orc, og, obc, p, dtype):
    h = og.meshsize()
    inner = (slice(1, -1),) * og.ndim
    held = _held(orc, og, obc, p, dtype)
    assert np.array_equal(held[inner], p, equal_nan=True)
    return mref.volume(p, h), mref.perimeter(held, h)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("bcname", ["periodic", "neumann", "linear"])
@pytest.mark.parametrize("nd", [1, 2, 3])
def test_dense_measures(lsm, orc, nd, bcname, dtype):
    """volume(eq) / perimeter(eq) of every field of _measure_fields against the exact sums of _measure_ref on what the device
    holds (1e-12; the empty, full and NaN sets exactly), then a scalar write on the boundary before the next perimeter."""
    og = _grid(orc, MEASURE_SHAPES[nd], MLC, MHC)
    lbc, ospec = _bc(lsm, bcname, nd)
    obc = orc.make_bc(ospec, nd)
    h = og.meshsize()
    fields = {k: _stored(v, dtype) for k, v in _measure_fields(og).items()}
    eq = _equation(lsm, og, fields["body"], lbc, dtype)
    st = eq.current_state()
    for name, p in fields.items():
        st.copy_(lsm.MeshField(p, st.mesh, dtype=dtype))
        vol, per = lsm.volume(eq), lsm.perimeter(eq)
        rv, rp = _measure_refs(orc, og, obc, p, dtype)
        if name == "nan":
            assert math.isnan(vol) and math.isnan(per) and math.isnan(rv) and math.isnan(rp)
        elif name == "inside":
            assert vol == pytest.approx(p.size * float(np.prod(h)), rel=1e-12) and vol == pytest.approx(rv, rel=1e-12)
            assert per == 0.0 and rp == 0.0
        elif name == "outside":
            assert vol == 0.0 and per == 0.0 and rv == 0.0 and rp == 0.0
        else:
            assert rv > 0 and rp > 0
            assert vol == pytest.approx(rv, rel=1e-12), name
            assert per == pytest.approx(rp, rel=1e-12), name
    # where the oracle's dense ϕ[I] is what the device holds: its own pairwise sums, and the exact sum over ϕ[I] node by node
    if dtype == F64 or _copy_faces(bcname):
        p = fields["cut"]
        st.copy_(lsm.MeshField(p, st.mesh, dtype=dtype))
        assert lsm.volume(eq) == pytest.approx(orc.volume(og, p), rel=1e-12)
        assert lsm.perimeter(eq) == pytest.approx(orc.perimeter(og, p, obc), rel=1e-12)
        assert lsm.perimeter(eq) == pytest.approx(mref.perimeter(lambda I: orc.get(og, obc, p, I), h, n=tuple(og.n)), rel=1e-12)
    # stale ghosts: ϕ[I] = v on a boundary node inside the delta's support and on its neighbour (the periodic image of the
    # opposite face's ghost); the ghost layers must follow
    p = fields["cut"].copy(order="F")
    st.copy_(lsm.MeshField(p, st.mesh, dtype=dtype))
    before = lsm.perimeter(eq)
    J = tuple(int(i) for i in np.unravel_index(np.argmin(np.abs(p[0])), p[0].shape)) if nd > 1 else ()
    assert abs(p[(0,) + J]) < min(h)
    for I, v in (((0,) + J, 0.25 * min(h)), ((1,) + J, -0.125 * min(h))):
        st[I] = v
        assert st.ghosts_dirty
        p[I] = float(dtype(v))
    after = lsm.perimeter(eq)
    rp = _measure_refs(orc, og, obc, p, dtype)[1]
    assert after == pytest.approx(rp, rel=1e-12) and abs(after - before) > 1e-6 * rp


# ------------------------------------------------------------------------------------------------- f. slab measures

@pytest.mark.parametrize("bcname", ["neumann", "periodic"])
@pytest.mark.parametrize("world", [2, 3])
def test_slab_measures_equal_the_single_device_values(lsm, world, bcname):
    """volume(eq) / perimeter(eq) of a LocalGroup slab equation (sum over ranks): a sphere whose surface
    crosses every slab interface, so the centred gradient of the perimeter needs the neighbours' planes; before any step
    and after one integrate_.  Ranks = threads, as in test_gpu_api.py."""
    grid = lsm.CartesianGrid((0, 0, 0), (1, 1, 1), (24, 20, 41))
    ic = lsm.MeshField(lambda x: np.sqrt((x[0] - 0.5) ** 2 + (x[1] - 0.48) ** 2 + (x[2] - 0.5) ** 2) - 0.35, grid)
    h = min(grid.meshsize())
    for k in {1: (), 2: (21,), 3: (14, 28)}[world]:                 # the interface planes carry delta-support nodes
        assert (np.abs(ic.vals[:, :, k - 1:k + 1]) < h).any()
    bc, _ = _bc(lsm, bcname, 3)
    mk = lambda **kw: lsm.LevelSetEquation(terms=(lsm.AdvectionTerm(lsm.vortex_deformation(grid), lsm.WENO5()),
                                                  lsm.EikonalReinitializationTerm()), ic=ic, bc=bc, integrator=lsm.RK3(), **kw)

    def measures(eq):
        out = [(lsm.volume(eq), lsm.perimeter(eq))]
        lsm.integrate_(eq, 0.01)
        out.append((lsm.volume(eq), lsm.perimeter(eq)))
        return out

    want = measures(mk())
    assert want[0] != want[1] and all(v > 0 and p > 0 for v, p in want)
    g = lsm.LocalGroup(world)
    got, errs = [None] * world, []

    def run(r):
        try:
            eq = mk(comm=g.rank(r))
            assert eq.lib_comm
            got[r] = measures(eq)
        except BaseException:   # noqa: BLE001 - reported by the main thread
            import traceback
            errs.append((r, traceback.format_exc()))
            g.abort()

    ts = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not errs, errs
    assert not any(t.is_alive() for t in ts)
    for r in range(world):
        assert got[r] == got[0], r                                   # identical on all ranks
        for (v, p), (wv, wp) in zip(got[r], want):
            assert v == pytest.approx(wv, rel=1e-12) and p == pytest.approx(wp, rel=1e-12), (r, v, wv, p, wp)


# ------------------------------------------------------------------------------------------------- g. band measures

def _band_fields(og):
    """Level-set functions per dimension: (150, 60): lines of three 64-node steps with several gaps and clipped tails;
    (70, 24, 22): a hollow channel between two plates that reach the faces of the second dimension, with a wavy wall —
    lines without a band node lie inside the plates as well as in the channel; (120,): an interval and its complement."""
    nd = og.ndim
    X = np.meshgrid(*og.coords(), indexing="ij")
    L = [og.hc[d] - og.lc[d] for d in range(nd)]
    mid = [0.5 * (og.lc[d] + og.hc[d]) for d in range(nd)]
    if nd == 1:
        f = np.abs(X[0] - (mid[0] + 0.01)) - 0.27 * L[0]
        return [f, -f]
    if nd == 2:
        disc = lambda cx, cy, r: np.hypot(X[0] - (og.lc[0] + cx * L[0]), X[1] - (og.lc[1] + cy * L[1])) - r * L[1]
        return [np.minimum(np.minimum(disc(0.2, 0.5, 0.3), disc(0.55, 0.45, 0.28)), disc(0.97, 0.6, 0.35)),
                X[1] - mid[1] + 0.1 * L[1] * np.sin(7.0 * X[0])]
    hy = og.meshsize()[1]
    wall = (5.3 + 1.2 * np.sin(2 * np.pi * (X[0] - og.lc[0]) / L[0]) * np.cos(np.pi * (X[2] - og.lc[2]) / L[2])) * hy
    return [wall - np.abs(X[1] - (mid[1] + 0.2 * hy))]


@pytest.mark.parametrize("shape,dtype", [((120,), F64), ((150, 60), F64), ((150, 60), F32), ((70, 24, 22), F64)],
                         ids=["1d", "2d", "2d-f32", "3d"])
def test_band_measures(lsm, orc, shape, dtype):
    """volume / perimeter of a NarrowBandMeshField (nlayers = 3) on stretched cells: the literal restatement of the
    reference's scanline count (1e-12) and the dense device value (the reference's ≈, rtol √eps)."""
    nd = len(shape)
    og = _grid(orc, shape)
    h = og.meshsize()
    for vals in _band_fields(og):
        p = _stored(vals, dtype)
        dense = _equation(lsm, og, p, lsm.LinearExtrapolationBC(), dtype)
        band = _equation(lsm, og, p, lsm.LinearExtrapolationBC(), dtype, band=True)
        st = band.current_state()
        m, v = st.active_mask(), st.values().astype(F64)
        assert np.array_equal(v[m], p[m]) and 0 < m.sum() < m.size
        if nd == 3:      # lines along the first dimension without a band node, on both sides of the interface, and cut lines
            free = ~m.any(axis=0)
            assert (free & (p[0] < 0)).sum() >= 4 and (free & (p[0] > 0)).sum() >= 4
            assert (m.any(axis=0) & ~m.all(axis=0)).sum() >= 20
        ref = mref._band_volume_ref({tuple(int(i) for i in I): float(v[tuple(I)]) for I in np.argwhere(m)}, tuple(shape), h, min(h))
        vb = lsm.volume(band)
        assert vb == pytest.approx(ref, rel=1e-12)
        assert vb == pytest.approx(lsm.volume(dense), rel=1e-7)
        assert vb == pytest.approx(mref.volume(p, h), rel=1e-7)
        assert lsm.perimeter(band) == pytest.approx(lsm.perimeter(dense), rel=1e-7)


# ------------------------------------------------------------------------------------------------- h. extension

def _extension_case(orc, nd):
    shape = {2: (41, 33), 3: (21, 19, 17)}[nd]
    og = _grid(orc, shape)
    X = np.meshgrid(*og.coords(), indexing="ij")
    c = [0.5 * (og.lc[d] + og.hc[d]) + 0.02 * (d + 1) for d in range(nd)]
    phi = np.sqrt(sum((x - c[d]) ** 2 for d, x in enumerate(X))) - 0.3 * min(og.hc[d] - og.lc[d] for d in range(nd))
    F = np.sin(2 * X[0]) * np.cos(3 * X[1]) + (X[2] if nd == 3 else 0.0)
    return og, np.asfortranarray(phi), np.asfortranarray(F)


EXTENSION_CASES = [(nd, bc, mode, F64) for nd, bc in ((2, "neumann"), (3, "periodic"), (2, "linear"), (3, "linear")) for mode in ("strict", "fast")]
EXTENSION_CASES += [(2, "neumann", "strict", F32), (3, "periodic", "strict", F32)]


@pytest.mark.parametrize("nd,bcname,mode,dtype", EXTENSION_CASES, ids=lambda v: v.__name__ if isinstance(v, type) else str(v))
def test_extension_with_the_frozen_mask_of_curvature_field(lsm, orc, nd, bcname, mode, dtype):
    """The reference's cycle (test/test-velocityextension.jl:118-131): curvature_field(..., band=1.5Δ, frozen_out=) writes
    the mask, extend_along_normals_ takes that SideField.  float32 storage (STRICT only): F is rounded to float32 after
    every sweep (the stage-by-stage rounding of tests/test_gpu_f32.py), so the oracle runs one sweep at a time; on copy
    faces, where the ghosts of F are float32 values already."""
    og, phi, F = _extension_case(orc, nd)
    lbc, ospec = _bc(lsm, bcname, nd)
    obc = orc.make_bc(ospec, nd)
    p, F0 = _stored(phi, dtype), _stored(F, dtype)
    iters = 8
    frozen = np.abs(p) <= 1.5 * min(og.meshsize())
    assert 8 <= frozen.sum() < frozen.size // 2
    want = F0.copy(order="F")
    if dtype == F64:
        orc.extend_along_normals(og, obc, want, p, nb_iters=iters, frozen=frozen, cfl=0.45)
    else:
        for _ in range(iters):
            orc.extend_along_normals(og, obc, want, p, nb_iters=1, frozen=frozen, cfl=0.45)
            want = _stored(want, dtype)
    assert np.abs(want - F0).max() > 1e-3 and np.array_equal(want[frozen], F0[frozen])
    st = _equation(lsm, og, p, lbc, dtype, mode=mode).current_state()
    fz = lsm.SideField(st.backend, st.mesh)
    lsm.curvature_field(st, scale=-1.0, band=1.5 * min(og.meshsize()), fill=0.0, frozen_out=fz)
    assert np.array_equal(fz.values(), frozen.astype(F64))
    Fd = st.copy()
    Fd.copy_(lsm.MeshField(F0, st.mesh, dtype=dtype))
    assert lsm.extend_along_normals_(Fd, st, nb_iters=0, frozen=fz, cfl=0.45) is Fd
    assert np.array_equal(Fd.values().astype(F64), F0)                                   # no sweep: F bit for bit
    lsm.extend_along_normals_(Fd, st, nb_iters=iters, frozen=fz, cfl=0.45)
    got = Fd.values().astype(F64)
    if mode == "strict":
        assert np.array_equal(got, want), np.abs(got - want).max()
    else:
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
