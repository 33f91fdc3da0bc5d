"""Device NarrowBandMeshField (next row) against (a) a literal dict-based
restatement of the reference's band algorithms (tests/_nb_ref.py: update_band!, nearest-band-node
ring, affine extrapolation — bit for bit) and (b) the reference's own band tests restated
(test/test-narrow-band.jl:8-54,151-176,259-292, test/test-levelsetequation.jl:144-222)."""
import math

import numpy as np
import pytest

from _measure_ref import _band_volume_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lsm():
    import lsm_amd
    return lsm_amd


def _eq(lsm, phi, nlayers, bc=None, terms=None, integrator=None, mode="fast"):
    nb = lsm.NarrowBandMeshField(phi, nlayers=nlayers)
    return lsm.LevelSetEquation(terms=terms or (lsm.NormalMotionTerm(0.0),), ic=nb, bc=bc or lsm.ExtrapolationBC(2),
                                integrator=integrator, mode=mode)


def _circle(lsm, n=(40, 36), r=0.5, c=(0.1, -0.05)):
    grid = lsm.CartesianGrid((-1.0,) * len(n), (1.0,) * len(n), n)
    f = lambda x: np.sqrt(sum((xi - c[i % len(c)]) ** 2 for i, xi in enumerate(x))) - r
    return grid, lsm.MeshField(f, grid)


@pytest.mark.parametrize("shape,nlayers", [((40, 36), 2), ((40, 36), 3), ((33, 47), 5), ((18, 16, 14), 3), ((45,), 3)])
def test_band_set_and_values_match_reference_algorithm_bitwise(lsm, shape, nlayers):
    from _nb_ref import NBRef
    grid, phi = _circle(lsm, shape)
    eq = _eq(lsm, phi, nlayers)
    st = eq.current_state()
    ref = NBRef(phi.vals, nlayers)
    assert np.array_equal(st.active_mask(), ref.mask())
    assert st.active_count() == len(ref.d)
    got = st.values()
    m = ref.mask()
    assert np.array_equal(got[m], ref.dense()[m])


@pytest.mark.parametrize("shape,nlayers", [((40, 36), 3), ((18, 16, 14), 2)])
def test_update_band_after_motion_matches_reference_algorithm_bitwise(lsm, shape, nlayers):
    """Shift the stored band values (the interface moves), rebuild: new band set, kept values and the
    affine-extrapolated values of newly active nodes must equal the dict-based restatement."""
    from _nb_ref import NBRef
    grid, phi = _circle(lsm, shape)
    eq = _eq(lsm, phi, nlayers)
    st = eq.current_state()
    ref = NBRef(phi.vals, nlayers)
    h = min(grid.meshsize())
    for shift in (-0.9 * h, 1.7 * h):
        st.buf += shift                      # band and scratch entries alike; only band entries matter
        ref.d = {I: v + shift for I, v in ref.d.items()}
        st.rebuild(from_dense=False)
        ref.update_band()
        m = ref.mask()
        assert np.array_equal(st.active_mask(), m)
        assert np.array_equal(st.values()[m], ref.dense()[m])


@pytest.mark.parametrize("shape", [(40, 36), (18, 16, 14)])
def test_band_halo_extrapolation_matches_reference_bitwise(lsm, shape):
    """Every non-band node within Chebyshev distance 3 of the band receives _extrapolate_to_ghost."""
    from _nb_ref import NBRef
    grid, phi = _circle(lsm, shape)
    eq = _eq(lsm, phi, 3)
    st = eq.current_state()
    ref = NBRef(phi.vals, 3)
    st.prepare(st.buf)
    dense = st.backend.download(st.buf)
    halo = st.backend.mask_to_host(st.halo)
    band = ref.mask()
    targets = np.argwhere(halo & ~band)
    assert len(targets) > 50
    for I in targets:
        I = tuple(int(i) for i in I)
        assert dense[I] == ref.extrapolate(I), I


def test_construction(lsm):
    """test/test-narrow-band.jl:8-32"""
    grid = lsm.CartesianGrid((-2.0, -2.0), (2.0, 2.0), (100, 100))
    phi = lsm.MeshField(lambda x: np.sqrt(x[0] ** 2 + x[1] ** 2) - 0.5, grid)
    st = _eq(lsm, phi, 5).current_state()
    n_active = st.active_count()
    assert 0 < n_active < 100 * 100
    m = st.active_mask()
    assert np.array_equal(st.values()[m], phi.vals[m])            # inherited unchanged
    h = min(grid.meshsize())
    assert np.abs(phi.vals[m]).max() <= 5 * math.sqrt(2) * h + h
    assert _eq(lsm, phi, 10).current_state().active_count() > n_active
    st_f = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), bc=lsm.ExtrapolationBC(2),
                                ic=lsm.NarrowBandMeshField(lambda x: np.sqrt(x[0] ** 2 + x[1] ** 2) - 0.5, grid, nlayers=5)).current_state()
    assert np.array_equal(st_f.active_mask(), m)


def test_extrapolation_outside_band_is_affine_exact(lsm):
    """test/test-narrow-band.jl:34-54 (LinearExtrapolationBC composes exactly past the grid edge)"""
    grid = lsm.CartesianGrid((-2.0, -2.0), (2.0, 2.0), (100, 100))
    f = lambda x: 3 * x[0] - 2 * x[1] + 1.0
    phi = lsm.MeshField(f, grid)
    st = _eq(lsm, phi, 4, bc=lsm.LinearExtrapolationBC()).current_state()
    idx = np.argwhere(st.active_mask())
    imin, imax = idx.min(axis=0), idx.max(axis=0)
    h = grid.meshsize()
    node = lambda I: (grid.lc[0] + I[0] * h[0], grid.lc[1] + I[1] * h[1])
    k = 5
    for a in range(k + 1):
        for b in range(k + 1):
            for I in ((int(imax[0]) + a, int(imax[1]) + b), (int(imin[0]) - a, int(imin[1]) - b)):
                assert st[I] == pytest.approx(f(node(I)), abs=1e-10), I


def test_band_update_is_idempotent_and_value_preserving(lsm):
    """test/test-narrow-band.jl:151-176"""
    grid = lsm.CartesianGrid((-1.0, -1.0), (1.0, 1.0), (50, 50))
    phi = lsm.MeshField(lambda x: np.sqrt(x[0] ** 2 + x[1] ** 2) - 0.5, grid)
    st = _eq(lsm, phi, 5).current_state()
    m0, v0 = st.active_mask(), st.values()
    st.rebuild(from_dense=False)
    assert st.active_count() > 0
    assert np.array_equal(st.active_mask(), m0)
    assert np.array_equal(st.values()[m0], v0[m0])
    assert np.abs(st.values()[m0] - phi.vals[m0]).max() < 1.0e-5


def test_far_index_raises_and_periodic_is_rejected(lsm):
    """test/test-narrow-band.jl:259-260,286-292"""
    grid = lsm.CartesianGrid((-2.0, -2.0), (2.0, 2.0), (100, 100))
    phi = lsm.MeshField(lambda x: np.sqrt(x[0] ** 2 + x[1] ** 2) - 0.5, grid)
    st = _eq(lsm, phi, 3).current_state()
    with pytest.raises(ValueError, match="more than 6 nodes from the band"):
        st[(2, 2)]
    with pytest.raises(ValueError, match="PeriodicBC is not supported"):
        lsm.NarrowBandMeshField(lsm.MeshField(phi.vals, grid, bc=lsm.PeriodicBC()))
    with pytest.raises(lsm.LsmError, match="PeriodicBC is not supported"):
        lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.NarrowBandMeshField(phi), bc=lsm.PeriodicBC())


def _nb_full_error(nb_state, full_vals, nlayers, h):
    """max |nb - full| over active nodes within half the band width of the interface
    (test/test-levelsetequation.jl:14-20)"""
    g = nlayers * h
    m = nb_state.active_mask()
    v = nb_state.values()
    near = m & (np.abs(np.nan_to_num(v, nan=1e9)) < g / 2)
    return np.abs(v[near] - full_vals[near]).max()


def test_integrate_advection_matches_full_grid(lsm):
    """test/test-levelsetequation.jl:144-154 without the reinitialize! hooks (with them: further down)"""
    grid = lsm.CartesianGrid((-2.0, -2.0), (2.0, 2.0), (60, 60))
    phi = lsm.MeshField(lambda x: np.sqrt(x[0] ** 2 + x[1] ** 2) - 0.5, grid)
    terms = lambda: (lsm.AdvectionTerm((1.0, 0.0)),)
    nb = _eq(lsm, phi, 5, terms=terms())
    full = lsm.LevelSetEquation(terms=terms(), ic=phi, bc=lsm.ExtrapolationBC(2))
    lsm.integrate_(full, 0.1)
    lsm.integrate_(nb, 0.1)
    assert nb.current_state().active_count() > 0
    assert _nb_full_error(nb.current_state(), full.current_state().values(), 5, min(grid.meshsize())) < 1.0e-3
    # the band followed the interface: exact solution is the translated circle
    st = nb.current_state()
    m = st.active_mask()
    X, Y = np.meshgrid(*grid.coords(), indexing="ij")
    exact = np.sqrt((X - 0.1) ** 2 + Y ** 2) - 0.5
    near = m & (np.abs(exact) < 1.5 * min(grid.meshsize()))
    assert np.abs(st.values()[near] - exact[near]).max() < 0.01


def test_integrate_full_rotation_and_curvature_match_full_grid(lsm):
    """test/test-levelsetequation.jl:194-222 (rotation) and :171-192-style curvature flow, 3-D included"""
    grid = lsm.CartesianGrid((-2.0, -2.0), (2.0, 2.0), (40, 40))
    phi = lsm.MeshField(lambda x: np.sqrt((x[0] - 0.8) ** 2 + x[1] ** 2) - 0.5, grid)
    terms = lambda: (lsm.AdvectionTerm(lsm.RigidRotation()),)
    # WITHOUT any reinitialisation (the reference's own runs, with reinitialize! after every step, are restated
    # further down): the band-edge extrapolation error accumulates over the ~250 steps (measured: 0.071 /
    # 0.014 / 0.008 for nlayers 3 / 5 / 7), so the 0.02 bar is met with nlayers = 5, and by nlayers = 3 over a
    # quarter turn.
    for nl, tf in ((5, 2 * math.pi), (3, math.pi / 2)):
        nb = _eq(lsm, phi, nl, terms=terms())
        full = lsm.LevelSetEquation(terms=terms(), ic=phi, bc=lsm.ExtrapolationBC(2))
        lsm.integrate_(full, tf)
        lsm.integrate_(nb, tf)
        assert nb.current_state().active_count() > 0
        assert _nb_full_error(nb.current_state(), full.current_state().values(), nl, min(grid.meshsize())) < 0.02
    g3 = lsm.CartesianGrid((-1, -1, -1), (1, 1, 1), (40, 40, 40))
    p3 = lsm.MeshField(lambda x: np.sqrt(x[0] ** 2 + x[1] ** 2 + x[2] ** 2) - 0.6, g3)
    t3 = lambda: (lsm.NormalMotionTerm(0.3), lsm.CurvatureTerm(-0.05))
    nb3 = _eq(lsm, p3, 3, terms=t3(), integrator=lsm.RK3())
    full3 = lsm.LevelSetEquation(terms=t3(), ic=p3, bc=lsm.ExtrapolationBC(2), integrator=lsm.RK3())
    lsm.integrate_(full3, 0.05)
    lsm.integrate_(nb3, 0.05)
    frac = nb3.current_state().active_count() / 40 ** 3
    assert 0.02 < frac < 0.5
    assert _nb_full_error(nb3.current_state(), full3.current_state().values(), 3, min(g3.meshsize())) < 0.01


@pytest.mark.parametrize("shape,bcspec", [
    ((30, 26), [("extrapolation", 5), ("symmetry", ("extrapolation", 2))]),
    ((26, 30), [("symmetry", "neumann"), ("extrapolation", 4)]),
    ((14, 12, 16), [("extrapolation", 3), ("symmetry", "linear"), ("extrapolation", 2)]),
])
def test_band_stage_reads_reference_values_at_the_grid_boundary(shape, bcspec):
    """A band that runs into the grid boundary: every position a band node's stencil reads — in the grid
    (stored or extrapolated from the nearest band node) or outside it (resolved by _getindexbc over those
    values, src/meshfield.jl:248-260,475-511) — must hold the reference's value, and a stage over the band
    must equal the reference stage evaluated on those values.  Through the C ABI, strict mode."""
    import itertools
    import _hip as hip
    from _nb_ref import NBRef
    from lsm_amd import _lib as L
    from oracle import oracle as orc
    nd = len(shape)
    c = hip.Case(shape, bcspec, mode="strict")
    ax = [np.linspace(-1.0, 1.0, n) for n in shape]
    X = np.meshgrid(*ax, indexing="ij")
    ctr = (-0.85, -0.7, 0.75)
    phi = np.asfortranarray(np.sqrt(sum((X[d] - ctr[d]) ** 2 for d in range(nd))) - 0.62)
    ref = NBRef(phi, 3)
    band = ref.mask()
    assert band[0].any() and band[:, 0].any()          # the band touches the low faces

    be = c.be
    vals = c.to_dev(c.pad(phi, fill=False))
    mask, halo, sa, sb = (be.alloc_mask() for _ in range(4))
    MC = 8
    tiles = be.alloc_tiles(MC)
    hlist, hcount = be.alloc_halo_list(64)             # deliberately too short: exercises the regrow path
    be.band_update(vals, mask, True, 3, sa, sb, halo, tiles, MC, hlist, hcount)
    want_n, missed = be.band_status(hcount)
    assert want_n > 64 and not missed
    hlist, hcount = be.alloc_halo_list(want_n)
    be.band_halo(vals, mask, halo, tiles, MC, hlist, hcount)
    assert be.band_status(hcount) == (want_n, False)
    assert np.array_equal(be.mask_to_host(mask), band)

    # the reference's view of the field: stored values on the band, the affine extrapolant elsewhere
    D = np.zeros(shape, order="F")
    known = np.zeros(shape, dtype=bool)
    for I in np.ndindex(*shape):
        try:
            D[I] = ref.get(I)
            known[I] = True
        except ValueError:
            pass
    psi = c.pad(D)                                     # + _getindexbc ghosts (oracle, bitwise-checked elsewhere)
    kpad = c.pad(known.astype(np.float64)) != 0        # crude: which padded entries derive from known nodes only

    be.band_fill_list(vals, mask, hlist, hcount)
    be.fill_ghosts(vals, 7)
    got = c.to_host(vals)
    G = 3
    offs = set()
    for d in range(nd):
        for k in range(-3, 4):
            offs.add(tuple(k if e == d else 0 for e in range(nd)))
    offs |= set(itertools.product((-1, 0, 1), repeat=nd))
    nread = 0
    for I in np.argwhere(band):
        for o in offs:
            J = tuple(int(I[d]) + o[d] + G for d in range(nd))
            assert got[J] == psi[J], (tuple(I), o, got[J], psi[J])
            nread += 1
    assert nread > 1000

    specs = [("adv", ("const", (0.7, -0.4, 0.3)[:nd]), "weno5"), ("nm", ("const", (0.5,))), ("curv", ("const", (-0.05,)))]
    for sub in ([specs[0]], [specs[1]], specs[1:], [specs[0], specs[2]]):
        ot, arr = c.terms(sub)
        cdt = 2.0e-3
        want = np.full_like(psi, np.nan)
        orc.stage_padded(c.grid, c.bc, c.olay, ot, psi, None, want, None, L.BASE_PSI, cdt, 0.0, 0.1)
        out = c.to_dev(np.zeros_like(psi))
        be.stage_band(arr, len(sub), vals, None, out, None, L.BASE_PSI, cdt, 0.0, 0.1, mask, tiles, MC)
        g, w = c.interior(c.to_host(out)), c.interior(want)
        if any(s[0] == "curv" for s in sub):
            assert np.abs(g[band] - w[band]).max() <= 1e-13 * np.abs(w[band]).max()
        else:
            assert np.array_equal(g[band], w[band])
        assert np.all(g[~band] == 0.0)                 # only band nodes are stored


@pytest.mark.parametrize("env", ["LSM_BAND_BYTES", "LSM_BAND_NO_LISTS"])
def test_fallback_band_paths_give_the_same_band_and_values(lsm, monkeypatch, env):
    """The A/B switches select the generic paths (byte-mask kernels in 3-D; launches over every tile instead of the
    compact lists).  Both must step a 3-D band to bitwise the same state as the default path."""
    grid = lsm.CartesianGrid((-1, -1, -1), (1, 1, 1), (40, 36, 44))
    phi = lsm.MeshField(lambda x: np.sqrt((x[0] - 0.1) ** 2 + x[1] ** 2 + (x[2] + 0.05) ** 2) - 0.55, grid)
    mk = lambda **kw: lsm.LevelSetEquation(terms=(lsm.AdvectionTerm(lsm.RigidRotation(), lsm.WENO5()), lsm.CurvatureTerm(-0.02)),
                                           ic=lsm.NarrowBandMeshField(phi, nlayers=3), bc=lsm.ExtrapolationBC(2), integrator=lsm.RK3(), **kw)
    ref = mk()
    lsm.integrate_(ref, 0.03)
    alt = mk(tuning={env: 1})       # lsm_set_tuning right after lsm_create: the band is built on that path too
    assert alt.backend.get_tuning(env) == 1 and ref.backend.get_tuning(env) == 0
    lsm.integrate_(alt, 0.03)
    a, b = ref.current_state(), alt.current_state()
    m = a.active_mask()
    assert m.sum() > 1000 and np.array_equal(m, b.active_mask())
    assert np.array_equal(a.values()[m], b.values()[m])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("case", ["rot_weno_curv", "const_upwind", "nm", "weno_nm", "eik", "weno_eik", "nm_curv"])
def test_brick_stage_equals_the_tiled_band_stage_bitwise(lsm, monkeypatch, case, dtype):
    """The band stage with one lane per band node (csrc/stage_brick.h, the default for the plain FAST cases) against the tiled
    march over the same pieces (LSM_BAND_BRICKS=0): the same node_update on the same values, so every band value must agree
    bitwise after several RK3 steps — on a band that runs into the faces of a grid that is no multiple of the 32 x 8 x 16 brick."""
    grid = lsm.CartesianGrid((-1, -1, -1), (1, 1, 1), (70, 37, 45))
    phi = lsm.MeshField(lambda x: np.sqrt((x[0] - 0.3) ** 2 + (x[1] + 0.2) ** 2 + (x[2] - 0.25) ** 2) - 0.8, grid, dtype=np.dtype(dtype))
    terms = {
        "rot_weno_curv": (lsm.AdvectionTerm(lsm.RigidRotation(), lsm.WENO5()), lsm.CurvatureTerm(-0.02)),
        "const_upwind": (lsm.AdvectionTerm((0.6, -0.8, 0.3), lsm.Upwind()),),
        "nm": (lsm.NormalMotionTerm(0.7),),
        "weno_nm": (lsm.AdvectionTerm((-0.5, 0.4, 0.9), lsm.WENO5()), lsm.NormalMotionTerm(-0.3)),
        "eik": (lsm.EikonalReinitializationTerm(),),
        "weno_eik": (lsm.AdvectionTerm(lsm.RigidRotation(), lsm.WENO5()), lsm.EikonalReinitializationTerm()),
        "nm_curv": (lsm.NormalMotionTerm(0.4), lsm.CurvatureTerm(-0.03)),
    }[case]
    mk = lambda **kw: lsm.LevelSetEquation(terms=terms, ic=lsm.NarrowBandMeshField(phi, nlayers=3), bc=lsm.ExtrapolationBC(2),
                                           integrator=lsm.RK3(), **kw)
    out = []
    for bricks in (1, 0):
        eq = mk(tuning={"LSM_BAND_BRICKS": bricks})
        lsm.integrate_(eq, 0.02)
        st = eq.current_state()
        out.append((st.active_mask(), st.values()))
    (ma, va), (mb, vb) = out
    assert ma.sum() > 5000 and np.array_equal(ma, mb)
    assert ma[0].any() or ma[:, 0].any() or ma[:, :, -1].any()          # the band reaches a face
    assert np.array_equal(va[ma], vb[mb])


# ---- the reference's band integration tests with their reinitialize! hooks (test/test-levelsetequation.jl:144-222)

def _reinit(lsm):
    return lambda eq: lsm.reinitialize_(eq)


def test_reference_band_tests_with_reinitialize_hooks(lsm):
    bc = lsm.ExtrapolationBC(2)
    # :144-154 advection matches full grid (nlayers 5; both runs reinitialised every step)
    grid = lsm.CartesianGrid((-2.0, -2.0), (2.0, 2.0), (60, 60))
    phi = lsm.MeshField(lambda x: np.sqrt(x[0] ** 2 + x[1] ** 2) - 0.5, grid)
    t = lambda: (lsm.AdvectionTerm((1.0, 0.0)),)
    nb = lsm.LevelSetEquation(terms=t(), ic=lsm.NarrowBandMeshField(phi, nlayers=5), bc=bc)
    full = lsm.LevelSetEquation(terms=t(), ic=phi, bc=bc)
    lsm.integrate_(full, 0.1, prehook=_reinit(lsm))
    lsm.integrate_(nb, 0.1, posthook=_reinit(lsm))
    assert _nb_full_error(nb.current_state(), full.current_state().values(), 5, min(grid.meshsize())) < 1.0e-3
    # :156-172 advection with reinitialisation, default nlayers = 3, against the exact translated circle
    nb = lsm.LevelSetEquation(terms=t(), ic=lsm.NarrowBandMeshField(phi), bc=bc)
    lsm.integrate_(nb, 0.1, posthook=_reinit(lsm))
    st = nb.current_state()
    m, v = st.active_mask(), st.values()
    X, Y = np.meshgrid(*grid.coords(), indexing="ij")
    exact = np.sqrt((X - 0.1) ** 2 + Y ** 2) - 0.5
    near = m & (np.abs(np.nan_to_num(v, nan=1e9)) < 1.5 * min(grid.meshsize()))
    assert m.sum() > 0 and np.abs(v[near] - exact[near]).max() < 0.01


def test_reference_band_full_and_star_rotation_with_reinitialize(lsm):
    bc = lsm.ExtrapolationBC(2)
    rot = lambda: (lsm.AdvectionTerm(lsm.RigidRotation()),)
    # :194-205 full rotation, nlayers = 3, reinitialize! after every step
    grid = lsm.CartesianGrid((-2.0, -2.0), (2.0, 2.0), (40, 40))
    phi = lsm.MeshField(lambda x: np.sqrt((x[0] - 0.8) ** 2 + x[1] ** 2) - 0.5, grid)
    nb = lsm.LevelSetEquation(terms=rot(), ic=lsm.NarrowBandMeshField(phi), bc=bc)
    full = lsm.LevelSetEquation(terms=rot(), ic=phi, bc=bc)
    lsm.integrate_(full, 2 * math.pi)
    lsm.integrate_(nb, 2 * math.pi, posthook=_reinit(lsm))
    assert nb.current_state().active_count() > 0
    assert _nb_full_error(nb.current_state(), full.current_state().values(), 3, min(grid.meshsize())) < 0.02
    # :207-222 star rotation over half a turn
    g2 = lsm.CartesianGrid((-1.0, -1.0), (1.0, 1.0), (40, 40))
    star = lsm.MeshField(lambda x: np.sqrt(x[0] ** 2 + x[1] ** 2) - (0.5 + 0.1 * np.cos(5 * (np.arctan2(x[1], x[0]) - math.pi / 2))), g2)
    nb = lsm.LevelSetEquation(terms=rot(), ic=lsm.NarrowBandMeshField(star), bc=bc)
    full = lsm.LevelSetEquation(terms=rot(), ic=star, bc=bc)
    lsm.integrate_(full, math.pi)
    lsm.integrate_(nb, math.pi, posthook=_reinit(lsm))
    assert nb.current_state().active_count() > 0
    assert _nb_full_error(nb.current_state(), full.current_state().values(), 3, min(g2.meshsize())) < 0.05


def test_reference_band_spiral_curvature_flow_with_reinitialize(lsm):
    """:174-192 — a spiral whose arms are closer than the band is wide stresses the band rebuild."""
    grid = lsm.CartesianGrid((-1.0, -1.0), (1.0, 1.0), (50, 50))
    r0, th0, al = 0.5, -math.pi / 3, math.pi / 100
    R = np.array([[math.cos(al), -math.sin(al)], [math.sin(al), math.cos(al)]])
    M = R @ np.array([[1 / 0.06 ** 2, 0.0], [0.0, 1 / (4 * math.pi ** 2)]]) @ R.T

    def spiral(x):
        r, th = np.sqrt(x[0] ** 2 + x[1] ** 2), np.arctan2(x[1], x[0])
        best = None
        for i in range(5):
            v0, v1 = r - r0, th + (2 * i - 4) * math.pi - th0
            q = np.sqrt(M[0, 0] * v0 * v0 + 2 * M[0, 1] * v0 * v1 + M[1, 1] * v1 * v1) - 1
            best = q if best is None else np.minimum(best, q)
        return best
    phi = lsm.MeshField(spiral, grid)
    bc = lsm.ExtrapolationBC(2)
    nb = lsm.LevelSetEquation(terms=(lsm.CurvatureTerm(-0.1),), ic=lsm.NarrowBandMeshField(phi), bc=bc)
    full = lsm.LevelSetEquation(terms=(lsm.CurvatureTerm(-0.1),), ic=phi, bc=bc)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # the reference warns on non-converged nodes too
        lsm.integrate_(full, 0.1, prehook=_reinit(lsm))
        lsm.integrate_(nb, 0.1, posthook=_reinit(lsm))
    assert _nb_full_error(nb.current_state(), full.current_state().values(), 3, min(grid.meshsize())) < 0.05


def test_field_without_interface(lsm):
    """No cut cell: the band is empty, stepping and reinitialize! are no-ops; a dense field keeps its values and warns."""
    import warnings
    for n in ((30, 26), (20, 18, 16)):
        grid = lsm.CartesianGrid((-1.0,) * len(n), (1.0,) * len(n), n)
        phi = lsm.MeshField(lambda x: 1.0 + 0 * x[0], grid)
        eq = lsm.LevelSetEquation(terms=(lsm.AdvectionTerm((1.0,) * len(n)),), ic=lsm.NarrowBandMeshField(phi), bc=lsm.ExtrapolationBC(2))
        assert eq.current_state().active_count() == 0
        lsm.integrate_(eq, 0.05)
        lsm.reinitialize_(eq)
        assert eq.current_time() == 0.05 and eq.current_state().active_count() == 0
        dense = lsm.LevelSetEquation(terms=(lsm.AdvectionTerm((1.0,) * len(n)),), ic=phi, bc=lsm.ExtrapolationBC(2))
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            lsm.reinitialize_(dense)
        assert any("no interface sample" in str(x.message) for x in w)
        assert np.array_equal(dense.current_state().values(), phi.vals)



def test_reference_band_volume_and_perimeter(lsm, orc):
    """test/test-narrow-band.jl:207-241: the band-only measures reproduce the full-grid ones (compact, two components,
    clipped by the boundary, slab spanning the domain; 3-D sphere; empty band), and equal the literal restatement of
    the reference's scanline count."""
    grid = lsm.CartesianGrid((-1.0, -1.0), (1.0, 1.0), (100, 100))
    cases = (lambda x: np.hypot(x[0], x[1]) - 0.5,
             lambda x: np.minimum(np.hypot(x[0] - 0.4, x[1]) - 0.25, np.hypot(x[0] + 0.4, x[1]) - 0.2),
             lambda x: np.hypot(x[0] - 0.7, x[1]) - 0.6,
             lambda x: x[1] + 0 * x[0])
    for f in cases:
        phi = lsm.MeshField(f, grid)
        dense = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=phi, bc=lsm.LinearExtrapolationBC())
        band = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.NarrowBandMeshField(phi, nlayers=3), bc=lsm.LinearExtrapolationBC())
        vb, vd = lsm.volume(band), lsm.volume(dense)
        assert vb == pytest.approx(vd, rel=1e-7)                      # the reference's ≈ (rtol √eps)
        m = band.current_state().active_mask()
        vals = band.current_state().values()
        ref = _band_volume_ref({tuple(int(i) for i in I): float(vals[tuple(I)]) for I in np.argwhere(m)}, grid.n, grid.meshsize(), min(grid.meshsize()))
        assert vb == pytest.approx(ref, rel=1e-12)
    phi = lsm.MeshField(cases[0], grid)
    dense = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=phi, bc=lsm.LinearExtrapolationBC())
    band = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.NarrowBandMeshField(phi, nlayers=3), bc=lsm.LinearExtrapolationBC())
    assert lsm.perimeter(band) == pytest.approx(lsm.perimeter(dense), rel=1e-7)
    assert lsm.perimeter(band) == pytest.approx(2 * np.pi * 0.5, rel=1e-2)
    g3 = lsm.CartesianGrid((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (40, 40, 40))
    p3 = lsm.MeshField(lambda x: np.sqrt(x[0] ** 2 + x[1] ** 2 + x[2] ** 2) - 0.5, g3)
    d3 = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=p3, bc=lsm.LinearExtrapolationBC())
    b3 = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.NarrowBandMeshField(p3, nlayers=3), bc=lsm.LinearExtrapolationBC())
    assert lsm.volume(b3) == pytest.approx(lsm.volume(d3), rel=1e-7)
    m = b3.current_state().active_mask()
    vals = b3.current_state().values()
    ref = _band_volume_ref({tuple(int(i) for i in I): float(vals[tuple(I)]) for I in np.argwhere(m)}, g3.n, g3.meshsize(), min(g3.meshsize()))
    assert lsm.volume(b3) == pytest.approx(ref, rel=1e-12)
    assert lsm.perimeter(b3) == pytest.approx(lsm.perimeter(d3), rel=1e-7)
    # an empty band (no interface captured) measures zero
    flat = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.NarrowBandMeshField(lsm.MeshField(lambda x: 1.0 + 0 * x[0], grid), nlayers=3),
                                bc=lsm.LinearExtrapolationBC())
    assert flat.current_state().active_count() == 0 and lsm.volume(flat) == 0.0


def test_active_cellindices(lsm):
    """src/meshfield.jl:364-369: a cell is active when all its corners are band nodes."""
    grid = lsm.CartesianGrid((-1.0, -1.0), (1.0, 1.0), (31, 29))
    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.NarrowBandMeshField(lsm.MeshField(lambda x: np.hypot(x[0], x[1]) - 0.5, grid), nlayers=2),
                              bc=lsm.NeumannBC())
    st = eq.current_state()
    nodes = set(st.active_nodeindices())
    want = {I for I in nodes if I[0] < 30 and I[1] < 28 and all((I[0] + a, I[1] + b) in nodes for a in (0, 1) for b in (0, 1))}
    assert set(st.active_cellindices()) == want and len(want) > 50


@pytest.mark.parametrize("shape,integ,dtype,hooked", [((40, 36, 44), "rk3", "float32", False), ((40, 36, 44), "rk2", "float64", False),
                                                    ((40, 36, 44), "fe", "float64", False), ((48, 40), "rk3", "float64", False),
                                                    ((30, 28, 26), "rk3", "float64", True), ((48, 40), "rk2", "float32", True)])
def test_library_band_step_equals_the_stage_by_stage_sequence_bitwise(lsm, monkeypatch, shape, integ, dtype, hooked):
    """lsm_advance_band_fe/rk2/rk3 (what `_advance!` of a band field ccalls, include/lsm.h) against the same step driven stage
    by stage through lsm_band_prepare + lsm_stage_band: band sets and band values bit for bit over several steps with
    update_band! between them — with and without an update hook (a speed field refreshed from the stage input at the stage
    time, src/timestepping.jl:174,185,196)."""
    dt = np.dtype(dtype)
    N = len(shape)
    grid = lsm.CartesianGrid((-1.0,) * N, (1.0,) * N, shape)
    phi = lsm.MeshField(lambda x: np.sqrt(sum((xi - 0.07 * (i + 1)) ** 2 for i, xi in enumerate(x))) - 0.55, grid, dtype=dt)
    I = {"rk3": lsm.RK3, "rk2": lsm.RK2, "fe": lsm.ForwardEuler}[integ]
    calls = []

    def terms():
        adv = lsm.AdvectionTerm(lsm.RigidRotation(), lsm.WENO5())
        if not hooked:
            return (adv, lsm.CurvatureTerm(-0.02))
        speed = lsm.MeshField(np.zeros(shape), grid)

        def upd(coeff, field, t):            # v = 0.3 + t: depends on the stage time only, so both drivers see the same field
            calls.append(t)
            coeff.set_values(np.full(shape, 0.3 + t))
        return (adv, lsm.NormalMotionTerm(speed, update_func=upd))

    def run(py):
        monkeypatch.setenv("LSM_BAND_PY", "1" if py else "0")
        calls.clear()
        eq = lsm.LevelSetEquation(terms=terms(), ic=lsm.NarrowBandMeshField(phi, nlayers=3), bc=lsm.ExtrapolationBC(2), integrator=I())
        lsm.integrate_(eq, 0.05)
        st = eq.current_state()
        return st.active_mask(), st.values(), list(calls)

    m0, v0, c0 = run(True)
    m1, v1, c1 = run(False)
    assert m0.sum() > 500 and np.array_equal(m0, m1)
    assert v0.dtype == dt and np.array_equal(v0[m0], v1[m1])
    assert c0 == c1 and (len(c0) > 0) == hooked


@pytest.mark.parametrize("dtype,nlayers", [("float64", 3), ("float32", 3), ("float64", 2)])
def test_bit_row_update_equals_the_byte_mask_update_bitwise(lsm, monkeypatch, dtype, nlayers):
    """update_band! through the bit-row kernels (band_bits / band_grow_bits: every node read once, mask updated in place, new
    nodes extrapolated by the grow kernel) against the byte-mask kernels (LSM_BAND_BITS=0): band sets, band values, halo masks
    and the values every stage input gets on the halo, bit for bit, over several RK3 steps of config 5's equation.
    The band keeps clear of the faces, but its work tiles do not: it occupies tiles 1 and 2 of the 4 along the last axis, so
    their neighbours 0 and 3 lie on faces and the halo is searched by band_search3_kernel on both sides — none of the 6628
    (6324 for nlayers = 2) list entries carries the 0x40 that band_halo_bits_kernel sets (printed below).  That kernel is
    compared with the restatement in tests/test_gpu_band_update.py."""
    dt = np.dtype(dtype)
    n = (192, 64, 64)
    grid = lsm.CartesianGrid((-3, -1, -1), (3, 1, 1), n)
    phi = lsm.MeshField(lambda x: np.sqrt((x[0] - 0.03) ** 2 + (x[1] + 0.02) ** 2 + x[2] ** 2) - 0.3, grid, dtype=dt)

    def run(bits):
        eq = lsm.LevelSetEquation(terms=(lsm.AdvectionTerm(lsm.RigidRotation(2.0, (0.4, 0.0)), lsm.WENO5()), lsm.CurvatureTerm(-0.01)),
                                  ic=lsm.NarrowBandMeshField(phi, nlayers=nlayers), bc=lsm.NeumannBC(), integrator=lsm.RK3(),
                                  tuning={"LSM_BAND_BITS": 1 if bits else 0})
        masks = []
        tc = 0.0
        for _ in range(8):
            step = 0.5 * eq.compute_cfl(tc)
            eq._advance(tc, step)
            eq.update_band()
            tc += step
            masks.append(eq.state.active_mask().copy())
        st = eq.state
        assert st.backend.lib.lsm_band_status is not None
        halo = st.backend.mask_to_host(st.halo)
        vals = st.values()
        st.prepare(st.buf)                      # what a stage input looks like: band halo by extrapolation
        prepared = st.backend.download(st.buf)
        n = int(st._hcount.item())
        flags = (st._hlist[:2 * n].cpu().numpy()[1::2] >> 56) & 0xff      # BandEntry::d[3] of the list's entries
        print(f"bits={bits}: {int(((flags & 0x40) != 0).sum())} of {n} halo list entries carry 0x40 (written by band_halo_bits_kernel)")
        return masks, vals, halo, prepared, n

    m0, v0, h0, p0, c0 = run(False)
    m1, v1, h1, p1, c1 = run(True)
    assert m0[-1].sum() > 3000 and not np.array_equal(m0[0], m0[-1])      # the band moved
    for a, b in zip(m0, m1):
        assert np.array_equal(a, b)
    m = m0[-1]
    assert np.array_equal(v0[m], v1[m])
    assert np.array_equal(h0, h1) and h0.sum() > m.sum() and c0 == c1 == int(h0.sum() - m.sum())
    assert np.array_equal(p0[h0], p1[h1])


def test_band_buffers_rewritten_in_place_need_the_handles_state_rebuilt(lsm):
    """include/lsm.h, lsm_band_invalidate: what the handle remembers about a band — compact tile lists, the halo list's length as the host
    last read it, a prefetched Δt — is keyed by the ADDRESSES of the caller's buffers.  copy!(dst, src) (src/meshfield.jl:282-292) rewrites
    dst's buffers in place with ANOTHER band: the host layer rebuilds that state (lsm_band_retile + lsm_band_status, as julia/ROCMeshField.jl's
    copy! does), after which dst steps exactly as src does — bit for bit, Δt included.  And the bare lsm_band_invalidate is enough for
    correctness: the kernels then run over all tiles and take the list's length from the device."""
    grid = lsm.CartesianGrid((-1, -1, -1), (1, 1, 1), (72, 40, 48))
    big = lsm.MeshField(lambda x: np.sqrt(x[0] ** 2 + x[1] ** 2 + x[2] ** 2) - 0.6, grid)
    small = lsm.MeshField(lambda x: np.sqrt((x[0] - 0.2) ** 2 + (x[1] + 0.1) ** 2 + x[2] ** 2) - 0.3, grid)
    terms = lambda: (lsm.AdvectionTerm(lsm.RigidRotation(), lsm.WENO5()), lsm.CurvatureTerm(-0.02))
    mk = lambda phi: lsm.LevelSetEquation(terms=terms(), ic=lsm.NarrowBandMeshField(phi, nlayers=3), bc=lsm.NeumannBC(), integrator=lsm.RK3())

    def steps(eq, n=3):
        tc, dts = 0.0, []
        for _ in range(n):
            dt = 0.5 * eq.compute_cfl(tc)
            eq._advance(tc, dt)
            eq.update_band()
            tc += dt
            dts.append(dt)
        st = eq.current_state()
        return dts, st.active_mask(), st.values()

    want_dts, want_m, want_v = steps(mk(small))
    for how in ("copy!", "invalidate"):
        eq, src = mk(big), mk(small)
        steps(eq, 2)                                     # the handle holds lists, a halo count and a prefetched Δt of the BIG band
        a, b = eq.state, src.state
        if how == "copy!":
            a.copy_(b)
        else:                                            # the same rewrite by hand, and only the bare invalidation
            eq.backend.copy_(a.buf, b.buf)
            a.mask.copy_(b.mask); a.halo.copy_(b.halo); a.tiles.copy_(b.tiles)
            nl = min(a._hlist.numel(), b._hlist.numel())     # (the big band's list is the longer one: the small band's entries fit)
            assert 2 * int(b._hcount.item()) <= nl
            a._hlist[:nl].copy_(b._hlist[:nl])
            a._hcount.copy_(b._hcount)
            from lsm_amd import _lib as L
            L.check(eq.backend.h, eq.backend.lib.lsm_band_invalidate(eq.backend.h), "lsm_band_invalidate")
            a.ghosts_dirty = True
        dts, m, v = steps(eq)
        assert dts == want_dts, (how, dts, want_dts)
        assert np.array_equal(m, want_m) and np.array_equal(v[m], want_v[want_m]), how


def test_tuning_switches_live_on_the_handle(lsm):
    """include/lsm.h, "tuning switches": every handle starts from the environment's values (read once per process), lsm_set_tuning
    changes one handle's, unknown names and the create-time switch are refused."""
    from lsm_amd import _lib as L
    grid = lsm.CartesianGrid((-1, -1), (1, 1), (40, 36))
    ic = lsm.MeshField(lambda x: np.hypot(x[0], x[1]) - 0.5, grid)
    mk = lambda **kw: lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.3),), ic=ic, bc=lsm.NeumannBC(), **kw)
    a, b = mk(), mk(tuning={"LSM_STAGE_GENERIC": 1, "LSM_XREDIRECT": 0})
    assert a.backend.get_tuning("LSM_STAGE_GENERIC") == 0 and b.backend.get_tuning("LSM_STAGE_GENERIC") == 1
    assert a.backend.get_tuning("LSM_XREDIRECT") == 1 and b.backend.get_tuning("LSM_XREDIRECT") == 0
    assert a.backend.get_tuning("LSM_STAGE_TAIL") == 16 and a.backend.get_tuning("LSM_COMM_TIMEOUT_MS") > 0
    a.backend.set_tuning("LSM_STAGE_TAIL", 0)
    assert a.backend.get_tuning("LSM_STAGE_TAIL") == 0 and b.backend.get_tuning("LSM_STAGE_TAIL") == 16
    with pytest.raises(L.LsmError, match="no such switch"):
        a.backend.set_tuning("LSM_STAGE_YFAST", 1)                  # an experiment that lost: its switch went with its code
    with pytest.raises(L.LsmError, match="fixed when the handle is created"):
        a.backend.set_tuning("LSM_LAYOUT_ALIGN", 0)
    lsm.integrate_(a, 0.05)
    lsm.integrate_(b, 0.05)                                        # general kernels, materialised ghosts: the same equation
    va, vb = a.current_state().values(), b.current_state().values()
    assert np.abs(va - vb).max() <= 1e-13 * np.abs(va).max()
