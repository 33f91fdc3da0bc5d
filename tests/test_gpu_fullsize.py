"""Parity at BASELINE.json's FULL sizes through size-independent properties — analytic identities of the
scheme itself, which need no reference run.  (The oracle needs minutes per 512³ step on ONE thread; it is
OpenMP-parallel behind `oracle.set_threads`, and tests/test_gpu_stage_geometry.py compares the 512³ headline
step and the stage kernels' large-grid launch shapes with it directly.)  Here:

  * a linear field is differentiated exactly by every scheme: one RK3 step of advection with a
    constant velocity gives ϕ - Δt u·∇ϕ to rounding, Eikonal/NormalMotion see |∇ϕ| exactly,
    curvature sees κ = 0;
  * an exact signed-distance plane is a fixed point of the Eikonal term;
  * an exactly constant field is a fixed point of every term (ε floor of the WENO weights,
    zero-gradient guards) — no NaN;
  * the CFL Δt of the vortex-deformation field equals the value reduced on the host from the
    separable tables at the arg-max node set (bitwise);
  * slab composition: updating 512³ in three plane ranges equals one full launch (bitwise).
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lsm():
    import lsm_amd
    return lsm_amd


def _interior_err(out, want, pad=4):
    sl = tuple(slice(pad, -pad) for _ in range(out.ndim))
    return np.abs(out[sl] - want[sl]).max()


def test_512_cubed_linear_field_advection_is_exact(lsm):
    n = 512
    grid = lsm.CartesianGrid((0, 0, 0), (1, 1, 1), (n, n, n))
    a = (0.7, -0.4, 0.25)
    u = (0.3, 0.9, -0.6)
    ic = lsm.LazyMeshField(lambda x: a[0] * x[0] + a[1] * x[1] + a[2] * x[2] - 0.2, grid)
    eq = lsm.LevelSetEquation(terms=(lsm.AdvectionTerm(u, lsm.WENO5()),), ic=ic, bc=lsm.LinearExtrapolationBC(), integrator=lsm.RK3())
    dt = 0.5 * eq.compute_cfl(0.0)
    h = grid.meshsize(0)
    assert dt == 0.5 * (1 / (abs(u[0]) / h + abs(u[1]) / h + abs(u[2]) / h))   # src/levelsetterms.jl:90-96
    eq._advance(0.0, dt)
    out = eq.current_state().values()
    want = ic.local_values(None) - dt * (u[0] * a[0] + u[1] * a[1] + u[2] * a[2])
    assert np.abs(out - want).max() <= 1e-13      # linear extrapolation keeps the field linear in the ghosts too
    del out, want


def test_1024_cubed_whole_grid_on_one_device(lsm):
    """BASELINE config 4's grid (1024³, 8 GiB per array: byte offsets beyond 2³², 1.1·10⁹ padded elements) as ONE slab:
    the headline equation's CFL is the analytic one, and a linear field advected by a constant velocity through the fused
    WENO5 + RK3 step stays linear — checked plane range by plane range on the host."""
    import torch
    if torch.cuda.mem_get_info()[0] < 48 * 2 ** 30:
        pytest.skip("needs 48 GiB of free device memory")
    n = 1024
    grid = lsm.CartesianGrid((0, 0, 0), (1, 1, 1), (n, n, n))
    a = (0.7, -0.4, 0.25)
    u = (0.3, 0.9, -0.6)
    ic = lsm.LazyMeshField(lambda x: a[0] * x[0] + a[1] * x[1] + a[2] * x[2] - 0.2, grid)
    eq = lsm.LevelSetEquation(terms=(lsm.AdvectionTerm(u, lsm.WENO5()),), ic=ic, bc=lsm.LinearExtrapolationBC(), integrator=lsm.RK3())
    del ic
    dt = 0.5 * eq.compute_cfl(0.0)
    h = grid.meshsize(0)
    assert dt == 0.5 * (1 / (abs(u[0]) / h + abs(u[1]) / h + abs(u[2]) / h))
    eq._advance(0.0, dt)
    out = eq.current_state().values()
    x = grid.coords()
    shift = dt * (u[0] * a[0] + u[1] * a[1] + u[2] * a[2])
    worst = 0.0
    for k0 in range(0, n, 64):
        want = (a[0] * x[0])[:, None, None] + (a[1] * x[1])[None, :, None] + (a[2] * x[2][k0:k0 + 64])[None, None, :] - 0.2 - shift
        worst = max(worst, float(np.abs(out[:, :, k0:k0 + 64] - want).max()))
    assert worst <= 2e-13
    del out


def test_512_cubed_sdf_plane_is_eikonal_fixed_point_and_constant_field_is_inert(lsm):
    n = 512
    grid = lsm.CartesianGrid((0, 0, 0), (1, 1, 1), (n, n, n))
    nx = (2 / 3, -1 / 3, 2 / 3)     # unit normal
    ic = lsm.LazyMeshField(lambda x: nx[0] * (x[0] - 0.5) + nx[1] * (x[1] - 0.5) + nx[2] * (x[2] - 0.5), grid)
    eq = lsm.LevelSetEquation(terms=(lsm.EikonalReinitializationTerm(),), ic=ic, bc=lsm.LinearExtrapolationBC(), integrator=lsm.RK3())
    dt = 0.5 * eq.compute_cfl(0.0)
    assert dt == 0.5 * grid.meshsize(0)            # src/levelsetterms.jl:250
    eq._advance(0.0, dt)
    out = eq.current_state().values()
    assert np.abs(out - ic.local_values(None)).max() <= 1e-14
    del out
    flat = lsm.LazyMeshField(lambda x: 0.25 + 0.0 * x[0], grid)
    eq2 = lsm.LevelSetEquation(terms=(lsm.AdvectionTerm(lsm.vortex_deformation(grid), lsm.WENO5()), lsm.EikonalReinitializationTerm(),
                                      lsm.NormalMotionTerm(0.3), lsm.CurvatureTerm(-0.1)), ic=flat, bc=lsm.NeumannBC(),
                               integrator=lsm.RK3())
    eq2._advance(0.0, 1.0e-3)
    lo, hi = eq2.current_state().extrema()
    # |∇ϕ| = 0: advection, curvature contribute 0; Eikonal S·(0-1) = -ϕ/|ϕ| and NormalMotion 0 -> uniform shift, no NaN
    assert lo == hi and not math.isnan(lo)


def test_512_cubed_vortex_cfl_matches_host_reduction(lsm):
    n = 512
    grid = lsm.CartesianGrid((0, 0, 0), (1, 1, 1), (n, n, n))
    vel = lsm.vortex_deformation(grid)
    ic = lsm.LazyMeshField(lambda x: np.sqrt((x[0] - 0.35) ** 2 + (x[1] - 0.35) ** 2 + (x[2] - 0.35) ** 2) - 0.15, grid)
    eq = lsm.LevelSetEquation(terms=(lsm.AdvectionTerm(vel, lsm.WENO5()),), ic=ic, bc=lsm.NeumannBC(), integrator=lsm.RK3())
    t = 0.37
    got = eq.compute_cfl(t)
    g = math.cos(math.pi * t / 3.0)
    h = grid.meshsize(0)
    # host: the same ((T1*T2)*T3)*g products, |u|/h sums and max, plane by plane (numpy is IEEE: identical bits)
    best = 0.0
    T = vel.tables
    for k in range(n):
        s = 0.0
        for c in range(3):
            p = (T[c][0][:, None] * T[c][1][None, :]) * T[c][2][k]
            s = (np.abs(p * g) / h) if c == 0 else s + np.abs(p * g) / h
        best = max(best, float(s.max()))
    assert got == 1 / best


def test_512_cubed_plane_ranges_compose(lsm):
    n = 512
    grid = lsm.CartesianGrid((0, 0, 0), (1, 1, 1), (n, n, n))
    ic = lsm.LazyMeshField(lambda x: np.sqrt((x[0] - 0.35) ** 2 + (x[1] - 0.35) ** 2 + (x[2] - 0.35) ** 2) - 0.15, grid)
    eq = lsm.LevelSetEquation(terms=(lsm.AdvectionTerm(lsm.vortex_deformation(grid), lsm.WENO5()), lsm.EikonalReinitializationTerm()),
                              ic=ic, bc=lsm.NeumannBC(), integrator=lsm.RK3())
    from lsm_amd.api import _terms_c
    b = eq.backend
    b.fill_ghosts(eq.state.buf)
    full, part = b.alloc(), b.alloc()
    arr = _terms_c(eq.terms)
    b.stage(arr, 2, eq.state.buf, None, full, None, 0, 1e-3, 0.0, 0.1)
    for m0, m1 in ((0, 4), (n - 4, n), (4, n - 4)):
        b.stage_planes(arr, 2, eq.state.buf, None, part, None, 0, 1e-3, 0.0, 0.1, m0, m1)
    import torch
    assert torch.equal(full, part)


def test_2048_squared_zalesak_rotation_step_is_symmetric_under_point_reflection(lsm):
    """Config 2 size.  Rigid rotation about the origin commutes with the point reflection x -> -x;
    on a grid symmetric about the origin one RK3 step of a point-symmetric field stays point-symmetric
    (the scheme's upwind stencils mirror exactly): bitwise in STRICT mode."""
    n = 2048
    grid = lsm.CartesianGrid((-1.5, -1.5), (1.5, 1.5), (n, n))
    f = lambda x: np.minimum(np.hypot(x[0] + 0.75, x[1]) - 0.5, np.hypot(x[0] - 0.75, x[1]) - 0.5)
    ic = lsm.MeshField(f, grid)
    assert np.abs(ic.vals - ic.vals[::-1, ::-1]).max() <= 1e-14    # node coordinates mirror to an ulp
    eq = lsm.LevelSetEquation(terms=(lsm.AdvectionTerm(lsm.RigidRotation(), lsm.WENO5()),), ic=ic, bc=lsm.NeumannBC(),
                              integrator=lsm.RK3())
    for _ in range(3):
        eq._advance(0.0, 0.5 * eq.compute_cfl(0.0))
    out = eq.current_state().values()
    assert np.abs(out - out[::-1, ::-1]).max() <= 1e-12
    assert np.abs(out - ic.vals).max() > 1e-4                       # it did move


def test_stage_refuses_planes_of_two_gib_and_accepts_just_below(lsm):
    """The stage kernel addresses a padded plane (the whole array in 1-D) through a 2 GiB buffer descriptor: lsm_stage
    must refuse larger planes loudly, and a plane just below the limit must still be updated correctly at its far end."""
    import ctypes as C
    from lsm_amd import _lib as L
    from lsm_amd.backend import HipBackend
    import torch

    def backend(n):
        g = L.LsmGrid()
        g.ndim, g.n[0], g.n[1], g.n[2] = 1, n, 1, 1
        g.lc[0], g.hc[0] = 0.0, 1.0
        bc = L.BcArray()
        for d in range(3):
            for s in range(2):
                bc[d][s].kind, bc[d][s].degree = L.BC_EXTRAPOLATION, 0
        return HipBackend(g, bc, mode="fast")

    term = (L.LsmTerm * 1)()
    term[0].kind, term[0].scheme = L.TERM_ADVECTION, L.SCHEME_UPWIND
    term[0].coeff.kind = L.COEFF_CONST
    term[0].coeff.value[0] = 1.0
    big = backend((1 << 28) + 8)                      # (n + 6)·8 bytes >= 2 GiB
    psi, out = big.alloc(), big.alloc()
    with pytest.raises(lsm.LsmError, match="smaller than 2 GiB"):
        big.stage(term, 1, psi, None, out, None, L.BASE_PSI, 1e-3, 0.0, 0.0)
    del psi, out, big
    torch.cuda.empty_cache()
    n = (1 << 28) - 64                                # just below: 2 GiB - 464 bytes
    b = backend(n)
    psi, out = b.alloc(), b.alloc()
    h = 1.0 / (n - 1)
    org = int(b.lay.origin)
    psi[org:org + n] = torch.arange(n, dtype=torch.float64, device=psi.device) * h      # ψ = x: D⁻ψ = 1
    b.fill_ghosts(psi)
    cdt = 0.25 * h
    b.stage(term, 1, psi, None, out, None, L.BASE_PSI, cdt, 0.0, 0.0)
    tail = out[org + n - 1000:org + n].cpu().numpy()
    want = (np.arange(n - 1000, n) * h) - cdt * 1.0
    assert np.abs(tail - want).max() <= 1e-12


def _symmetric_sphere(n, r0, dtype=np.float64):
    """ϕ = ‖x‖ − r0 on [-1, 1]^3 sampled at coordinates c_i = (2i − (n−1))/(n−1): c_{n−1−i} = −c_i EXACTLY, so the array is
    bit-for-bit invariant under the reflections of the axes and under permutations of them."""
    c = (2.0 * np.arange(n) - (n - 1)) / (n - 1)
    assert np.array_equal(c[::-1], -c)
    c2 = c * c
    out = np.empty((n, n, n), dtype=dtype, order="F")
    for k in range(n):                                  # plane by plane: no 2 x n^3 float64 temporaries
        out[:, :, k] = (np.sqrt((c2[:, None] + c2[None, :]) + c2[k]) - r0).astype(dtype)
    return out


def test_512_cubed_config3_sphere_octant_symmetry_and_radial_speed(lsm):
    """BASELINE config 3 at full size: 512³ sphere under NormalMotionTerm(0.1) + CurvatureTerm(-0.1), ExtrapolationBC(2), one
    RK3 step (Δt from the curvature CFL, src/levelsetterms.jl:123-127).  Size-independent properties of the scheme:
      * the scheme is equivariant under the reflections of the axes up to the association of its three-term second differences
        ((ϕ₊ − 2ϕ₀) + ϕ₋ becomes (ϕ₋ − 2ϕ₀) + ϕ₊, src/derivatives.jl:129-175): the result of an exactly symmetric field is
        symmetric in all eight octants to a few ulp in STRICT mode (the reference's operation order) — nothing of the
        tiling, the march direction or the wave-uniform sign paths may show through — and to FAST's tolerance in FAST mode;
      * a sphere ϕ = r − R moves with radial speed v + 2b/r (κ = 2/r, |∇ϕ| = 1): (ϕ⁰ − ϕ¹)/Δt equals it near the interface to
        O(h²) — in STRICT and in FAST mode, which agree to FAST's stated tolerance."""
    n, R, v, b = 512, 0.5, 0.1, -0.1
    grid = lsm.CartesianGrid((-1, -1, -1), (1, 1, 1), (n, n, n))
    phi0 = _symmetric_sphere(n, R)
    h = grid.meshsize(0)
    res = {}
    for mode in ("strict", "fast"):
        eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(v), lsm.CurvatureTerm(b)), ic=lsm.MeshField(phi0, grid), bc=lsm.ExtrapolationBC(2),
                                  integrator=lsm.RK3(), mode=mode)
        dt = 0.5 * eq.compute_cfl(0.0)
        sv = (abs(v) / h + abs(v) / h) + abs(v) / h                                   # src/levelsetterms.jl:172-178, summed left to right
        assert dt == 0.5 * min(h * h / (2 * abs(b)), 1 / sv)                          # :123-127
        eq._advance(0.0, dt)
        res[mode] = eq.current_state().values()
        del eq
    out = res["strict"]
    assert all(np.array_equal(phi0, np.flip(phi0, axis=ax)) for ax in range(3))
    for mode, tol in (("strict", 1e-15), ("fast", 3e-13)):
        for ax in range(3):
            d = np.abs(res[mode] - np.flip(res[mode], axis=ax)).max()
            assert d <= tol * np.abs(out).max(), (mode, ax, d)
    r = phi0 + R
    near = np.abs(phi0) < 2 * h
    assert near.sum() > 100000
    for mode, o in res.items():
        speed = (phi0[near] - o[near]) / dt                 # ϕ¹ = ϕ⁰ − Δt (v + bκ)|∇ϕ|
        err = np.abs(speed - (v + 2 * b / r[near])).max()
        assert err <= 60 * h * h, (mode, err, h * h)          # second-order ENO / centred differences on a smooth field
    assert np.abs(res["fast"] - out).max() <= 3e-13 * np.abs(out).max()


def test_768_cubed_config5_float32_band_is_symmetric_and_matches_the_dense_run(lsm):
    """BASELINE config 5 at full size on one device: 768³, float32 storage, sphere r = 0.5, rigid rotation about z (WENO5) +
    CurvatureTerm(-0.01), RK3, NeumannBC, narrow band nlayers = 3.  Properties that do not need an oracle run:
      * the band built from the exactly symmetric field is invariant under the reflections of the three axes and under x <-> y
        (cut cells and L1 dilations commute with them; the tile decomposition — 32 x 8 x 8 bricks — must not show through),
        at the start and after a step + update_band!;
      * one RK3 step on the band against the same step on the dense field: the band's edge nodes read extrapolated values
        (src/meshfield.jl:481-511) and every stage carries their influence one stencil further in, so nothing is bitwise;
        nodes whose own stencil lies inside the band agree to 1e-6, every band node within 1.5 h of the interface to 1e-5
        (config 5's stated tolerance is 1e-4).  Both bounds are TOLERANCES, not pins: an nlayers = 3 band is about seven nodes
        thick and an RK3 step carries the edge's extrapolated values three stencils (9 nodes) inward, so NO node of this band is
        free of them — "deep" only means one stencil further from the edge; a first version that asked those nodes to agree with
        the dense run to an ulp failed for that reason, not for a defect."""
    import torch
    n = 768
    grid = lsm.CartesianGrid((-1, -1, -1), (1, 1, 1), (n, n, n))
    phi0 = _symmetric_sphere(n, 0.5, np.float32)
    terms = lambda: (lsm.AdvectionTerm(lsm.RigidRotation(), lsm.WENO5()), lsm.CurvatureTerm(-0.01))
    band = lsm.LevelSetEquation(terms=terms(), ic=lsm.NarrowBandMeshField(lsm.MeshField(phi0, grid, dtype=np.float32), nlayers=3),
                                bc=lsm.NeumannBC(), integrator=lsm.RK3())

    def symmetric(m):
        return all(np.array_equal(m, np.flip(m, axis=ax)) for ax in range(3)) and np.array_equal(m, m.transpose(1, 0, 2))

    m0 = band.current_state().active_mask()
    assert 3.0e6 < m0.sum() < 4.5e6 and symmetric(m0)
    dt = 0.5 * band.compute_cfl(0.0)
    band._advance(0.0, dt)
    vb = band.current_state().values()                    # before update_band!: the band is still m0
    band.update_band()
    m1 = band.current_state().active_mask()
    assert symmetric(m1)
    del band
    torch.cuda.empty_cache()
    dense = lsm.LevelSetEquation(terms=terms(), ic=lsm.MeshField(phi0, grid, dtype=np.float32), bc=lsm.NeumannBC(), integrator=lsm.RK3())
    assert 0.5 * dense.compute_cfl(0.0) <= dt               # the dense minimum runs over more nodes (the grid's corners): the band's Δt is taken for both
    dense._advance(0.0, dt)
    vd = dense.current_state().values()
    del dense
    # nodes whose whole stencil (3 along each axis, the 3^3 box) lies in the band: erode the mask accordingly — on two slabs of
    # planes (the equator, where the band's normal lies in the plane, and the polar cap, where it is the march axis): the
    # whole-array rolls of a 768³ mask cost minutes
    h = grid.meshsize(0)
    n_deep = n_near = 0
    d_deep = d_near = 0.0
    for z0, z1 in ((340, 428), (556, 600)):
        sl = (slice(None), slice(None), slice(z0 - 3, z1 + 3))
        mm = m0[sl]
        deep = mm.copy()
        for ax in range(3):
            for k in (1, 2, 3):
                deep &= np.roll(mm, k, axis=ax) & np.roll(mm, -k, axis=ax)
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    deep &= np.roll(mm, (dx, dy, dz), axis=(0, 1, 2))
        deep[:, :, :3] = False                        # the rolls wrapped around inside the slab there
        deep[:, :, -3:] = False
        b64, d64 = vb[sl].astype(np.float64), vd[sl].astype(np.float64)
        near = mm & (np.abs(phi0[sl]) < 1.5 * h)
        n_deep += int(deep.sum()); n_near += int(near.sum())
        d_deep = max(d_deep, float(np.abs(b64[deep] - d64[deep]).max()))
        d_near = max(d_near, float(np.abs(b64[near] - d64[near]).max()))
    assert n_deep > 1.0e5 and n_near > 3.0e4 and d_deep <= 1e-6 and d_near <= 1e-5, (n_deep, n_near, d_deep, d_near)


def test_768_cubed_config5_band_reinitialize_is_symmetric_and_a_distance(lsm):
    """`reinitialize!` at config 5's size (768³, float32 storage, nlayers = 3: 3.7 M band nodes, the workload of
    `bench.py --config 5r`), from a field that is NOT a distance function (x² + y² + z² − ¼, |∇ϕ| = 1 on the interface only):
      * every band node ends at sign(ϕ)·distance to the sphere r = ½ — to 1e-6 with the solver's tolerances at 1e-9 (their default
        is √eps of the storage type: 3.5e-4 for float32, src/sdf.jl:66-67), where the input was off by more than 1e-4;
      * the reflections of the three axes and x <-> y map the result onto itself to the last bit of its float32 values but for
        ties: the exact nearest sample of two mirror nodes are mirror samples, the solves start from them — 1e-7;
      * nothing was left unconverged or without a sample, and the band itself is untouched."""
    import warnings
    n = 768
    grid = lsm.CartesianGrid((-1, -1, -1), (1, 1, 1), (n, n, n))
    ax = np.linspace(-1.0, 1.0, n)
    ax = 0.5 * (ax - ax[::-1])                           # exactly antisymmetric coordinates
    r2 = (ax ** 2)[:, None, None] + (ax ** 2)[None, :, None] + (ax ** 2)[None, None, :]
    phi0 = np.asfortranarray((r2 - 0.25).astype(np.float32))
    del r2
    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.NarrowBandMeshField(lsm.MeshField(phi0, grid, dtype=np.float32), nlayers=3),
                              bc=lsm.NeumannBC())
    st = eq.current_state()
    m0 = st.active_mask()
    assert 3.0e6 < m0.sum() < 4.5e6
    with warnings.catch_warnings():
        warnings.simplefilter("error")                   # a non-converged node or a node without samples warns
        lsm.reinitialize_(st, xtol=1e-9, ftol=1e-9)
    assert np.array_equal(st.active_mask(), m0)
    v = st.values()
    idx = np.nonzero(m0)
    got = v[idx].astype(np.float64)
    exact = np.sqrt(ax[idx[0]] ** 2 + ax[idx[1]] ** 2 + ax[idx[2]] ** 2) - 0.5
    assert np.abs(phi0[idx] - exact).max() > 1e-4        # the input was not a distance function
    assert np.abs(got - exact).max() < 1e-6
    for mirror in (v[::-1, :, :], v[:, ::-1, :], v[:, :, ::-1], v.transpose(1, 0, 2)):
        assert np.abs(mirror[idx].astype(np.float64) - got).max() < 1e-7
