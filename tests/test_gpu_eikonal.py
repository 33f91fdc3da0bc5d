"""eikonal_ on the device (csrc/lsm_eikonal.hip, lsm_eikonal through the Python API) against the restatement's Jacobi fixed point
(tests/_eikonal_ref.py) — the rounding bound is tol = 16·Σ(n_d − 1)·eps·max T, the measured difference 0 in every case, so the
same bits are asked for —, signs and zeros exactly: a grid inside one tile, partial tiles on
every axis, a front crossing many tiles (list rebuilds), two fronts meeting in a shock, a random speed, an interface cut by a
face of the grid, anisotropic spacing everywhere, both seedings; cutoffs; float32 storage; determinism; non-convergence; the
refusals; the round trip mesh → mesh_distance → eikonal; scratch reuse.  The tile shapes are 8×8×8 and 32×8."""
import numpy as np
import pytest

import _eikonal_ref as R
from test_eikonal_host import mesh_seeded_case, solved, widths

pytestmark = pytest.mark.gpu

INF = float("inf")
PASSES = 8      # Jacobi passes per visit of a tile (EK_PASSES)


def _lsm():
    import lsm_amd
    return lsm_amd


def _field(lsm, vals, lc, hc, dtype=None, bc=None):
    mf = lsm.MeshField(vals, lsm.CartesianGrid(lc, hc, vals.shape), dtype=dtype)
    return lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=mf, bc=bc or lsm.NeumannBC()).current_state()


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _close(got, want, n, tmax, what=""):
    """ϕ against the restatement's, signs and zeros exactly; prints the difference in eps·max T and the nodes that differ.  The
    order-independence argument bounds the difference by tol = 16·Σ(n_d − 1)·eps·max T (R.tol); the measured difference is 0 in
    every case of this file, so the same bits are asked for."""
    assert got.shape == want.shape and got.dtype == want.dtype
    diff = np.abs(got - want)
    print(f"{what}: max difference {diff.max() / (R.EPS * tmax):.3g} eps·max T (tol {R.tol(n, tmax) / (R.EPS * tmax):.0f}), "
          f"{int((diff != 0).sum())} of {got.size} nodes differ")
    assert np.array_equal(np.signbit(got), np.signbit(want))
    assert np.array_equal(got == 0, want == 0)
    assert diff.max() <= R.tol(n, tmax)
    assert np.array_equal(got, want)


CASES = [(name, s) for name in R.FIXTURES for s in (0, 1)]


@pytest.mark.parametrize("name,seeding", CASES, ids=[f"{n}-{('crossing', 'width')[s]}" for n, s in CASES])
def test_device_matches_restatement(name, seeding):
    lsm = _lsm()
    phi0, n, lc, hc, h, speed = R.fixture(name)
    T, frozen, passes, _ = solved(name, seeding)
    want = np.copysign(T, phi0)
    phi = _field(lsm, phi0, lc, hc)
    assert np.array_equal(R.meshsize(n, lc, hc), np.array(phi.mesh.meshsize()))
    stats = phi.backend.eikonal(phi.buf, speed, 0.0 if seeding == 0 else widths(h)[1], INF, 0)
    print(f"{name}: stats {stats}, {passes} Jacobi passes in the restatement")
    _close(phi.values(), want, n, float(T.max()), name)
    ntile = int(np.prod([-(-k // e) for k, e in zip(n, (8, 8, 8) if len(n) == 3 else (32, 8))]))
    assert stats[0] == int(frozen.sum()) and stats[3] == 0
    assert stats[1] >= -(-passes // PASSES) and stats[1] <= stats[2] <= stats[1] * ntile
    if name == "one_tile":
        assert stats[1] == stats[2]
    if name.startswith("nine_tiles"):
        assert stats[1] >= 8                    # the front crosses the tiles one launch after the other


def test_api_in_place_on_fields_and_equations():
    lsm = _lsm()
    phi0, n, lc, hc, h, _ = R.fixture("partial_tiles")
    T = solved("partial_tiles", 0)[0]
    phi = _field(lsm, phi0, lc, hc)
    phi.ghosts_dirty = False
    assert lsm.eikonal_(phi) is phi and phi.ghosts_dirty
    _close(phi.values(), np.copysign(T, phi0), n, float(T.max()), "field")
    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(phi0, lsm.CartesianGrid(lc, hc, n)), bc=lsm.NeumannBC())
    lsm.eikonal_(eq, width=None, cutoff=None, max_iters=None)
    assert np.array_equal(_bits(eq.current_state().values()), _bits(phi.values()))
    host = lsm.eikonal(lsm.MeshField(phi0, lsm.CartesianGrid(lc, hc, n)))
    assert isinstance(host, lsm.MeshField) and np.array_equal(_bits(np.asarray(host.vals)), _bits(phi.values()))
    # a uniform speed F: distance / F; a scalar, an array and a MeshField are the same speed
    F = 2.5
    outs = []
    for sp in (F, np.full(n, F), lsm.MeshField(np.full(n, F), lsm.CartesianGrid(lc, hc, n))):
        f = _field(lsm, phi0, lc, hc)
        lsm.eikonal_(f, speed=sp)
        outs.append(f.values())
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])) and np.array_equal(_bits(outs[0]), _bits(outs[2]))
    assert np.abs(outs[0] - phi.values() / F).max() <= R.tol(n, float(T.max()))


def test_width_beyond_the_grid_freezes_everything():
    """zero iterations, ϕ comes back bit for bit, −0.0 included"""
    lsm = _lsm()
    phi0, n, lc, hc, h, _ = R.fixture("partial_tiles")
    phi0 = np.array(phi0, order="F")
    phi0[3, 4, 5] = -0.0
    phi0[4, 4, 5] = 0.0
    for dtype in (np.float64, np.float32):
        phi = _field(lsm, phi0.astype(dtype), lc, hc, dtype=dtype)
        before = phi.values()
        stats = phi.backend.eikonal(phi.buf, None, 100.0, INF, 0)
        assert stats == (phi0.size, 0, 0, 0)
        assert np.array_equal(_bits(phi.values()), _bits(before)) and np.signbit(phi.values()[3, 4, 5]) and not np.signbit(phi.values()[4, 4, 5])


@pytest.mark.parametrize("name", ("partial_tiles", "two_circles", "nine_tiles_2d", "two_spheres_speed"))
def test_cutoff(name):
    """values <= c equal the ones without a cutoff (within tol of the restatement's), the rest are ±c"""
    lsm = _lsm()
    phi0, n, lc, hc, h, speed = R.fixture(name)
    for seeding in (0, 1):
        T = solved(name, seeding)[0]
        for c in (3 * float(h.max()), 0.5 * float(h.min())):
            want = R.eikonal(phi0, h, speed, None, c, T=T)
            phi = _field(lsm, phi0, lc, hc)
            lsm.eikonal_(phi, speed=speed, width=widths(h)[seeding], cutoff=c)
            got = phi.values()
            _close(got, want, n, float(T.max()), f"{name} c = {c:.3g}")
            far = T > c + R.tol(n, float(T.max()))
            assert far.any() and (np.abs(got[far]) == c).all() and np.abs(got).max() <= c
            again = _field(lsm, phi0, lc, hc)
            stats = again.backend.eikonal(again.buf, speed, 0.0 if seeding == 0 else widths(h)[1], c, 0)
            assert abs(stats[3] - int((T > c).sum())) <= int((np.abs(T - c) <= R.tol(n, float(T.max()))).sum())


def test_float32_storage_rounds_the_fp64_result_once():
    """relative to the device's own fp64 run on the same (float32-representable) input"""
    lsm = _lsm()
    for name in ("partial_tiles", "two_circles"):
        phi0, n, lc, hc, h, _ = R.fixture(name)
        p32 = phi0.astype(np.float32)
        for kw in ({}, {"width": 1.5 * float(h.max())}, {"cutoff": 3 * float(h.max())}):
            a = _field(lsm, p32.astype(np.float64), lc, hc)
            b = _field(lsm, p32, lc, hc, dtype=np.float32)
            lsm.eikonal_(a, **kw)
            lsm.eikonal_(b, **kw)
            got = b.values()
            assert got.dtype == np.float32
            assert np.array_equal(_bits(got), _bits(a.values().astype(np.float32)))


def test_determinism():
    """two calls on the same input: the concurrent tiles may read each other's layers at different moments, the fixed point is
    the same"""
    lsm = _lsm()
    for name in ("nine_tiles_3d", "two_spheres_speed", "two_circles"):
        phi0, n, lc, hc, h, speed = R.fixture(name)
        outs = []
        for _ in range(2):
            phi = _field(lsm, phi0, lc, hc)
            lsm.eikonal_(phi, speed=speed)
            outs.append(phi.values())
        d = np.abs(outs[0] - outs[1])
        print(f"{name}: {int((d != 0).sum())} nodes differ between two calls, max {d.max() / (R.EPS * np.abs(outs[0]).max()):.3g} eps·max T")
        assert np.array_equal(_bits(outs[0]), _bits(outs[1]))


def test_non_convergence_leaves_phi_untouched():
    lsm = _lsm()
    phi0, n, lc, hc, h, _ = R.fixture("nine_tiles_2d")
    assert solved("nine_tiles_2d", 0)[2] > PASSES      # one launch moves the front PASSES nodes at the most: one is not enough
    for dtype in (np.float64, np.float32):
        phi = _field(lsm, phi0.astype(dtype), lc, hc, dtype=dtype)
        before = phi.values()
        with pytest.raises(RuntimeError, match="did not empty within max_iters"):
            lsm.eikonal_(phi, max_iters=1)
        with pytest.raises(lsm.LsmNotConvergedError):
            lsm.eikonal_(phi, max_iters=2)
        assert np.array_equal(_bits(phi.values()), _bits(before))
    lsm.eikonal_(phi)                                   # the handle stays usable
    assert not np.array_equal(phi.values(), before)


def test_refusals_leave_phi_unchanged():
    lsm = _lsm()
    phi0, n, lc, hc, h, _ = R.fixture("one_tile")
    grid = lsm.CartesianGrid(lc, hc, n)
    phi = _field(lsm, phi0, lc, hc)
    before = phi.values()
    with pytest.raises(TypeError, match="device field"):
        lsm.eikonal_(phi0)
    with pytest.raises(TypeError, match="host MeshField"):
        lsm.eikonal(phi)
    bad = np.array(phi0, order="F")
    bad[2, 3, 1] = np.nan
    nanphi = _field(lsm, bad, lc, hc)
    with pytest.raises(ValueError, match="eikonal_: phi must be finite"):
        lsm.eikonal_(nanphi)
    assert np.array_equal(_bits(nanphi.values()), _bits(bad))
    same_sign = _field(lsm, np.abs(phi0) + 0.1, lc, hc)
    with pytest.raises(ValueError, match="eikonal_: phi has no interface"):
        lsm.eikonal_(same_sign)
    assert np.array_equal(same_sign.values(), np.abs(phi0) + 0.1)
    speed = np.ones(n)
    speed[1, 1, 1] = 0.0
    for sp in (speed, 0.0, -1.0, INF, np.where(speed == 0, np.nan, speed)):
        with pytest.raises(ValueError, match="eikonal_: the speed must be finite and positive"):
            lsm.eikonal_(phi, speed=sp)
    with pytest.raises(ValueError, match="the speed has shape"):
        lsm.eikonal_(phi, speed=np.ones((3, 3, 3)))
    for kw in ({"width": 0.0}, {"width": -1.0}, {"width": INF}, {"cutoff": 0.0}, {"cutoff": -2.0}, {"cutoff": float("nan")}):
        with pytest.raises(ValueError, match="must be positive"):
            lsm.eikonal_(phi, **kw)
    for width, cutoff in ((-1.0, INF), (INF, INF), (0.0, 0.0), (0.0, float("nan"))):
        with pytest.raises(lsm.LsmError, match="lsm_eikonal: (width|cutoff) must be"):
            phi.backend.eikonal(phi.buf, None, width, cutoff, 0)
    per = _field(lsm, phi0, lc, hc, bc=(lsm.NeumannBC(), lsm.PeriodicBC(), lsm.NeumannBC()))
    with pytest.raises(ValueError, match="PeriodicBC"):
        lsm.eikonal_(per)
    with pytest.raises(lsm.LsmError, match="periodic dimension"):
        per.backend.eikonal(per.buf, None, 0.0, INF, 0)
    assert np.array_equal(_bits(per.values()), _bits(phi0))
    one = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(lambda x: x[0] - 0.4, lsm.CartesianGrid((0.0,), (1.0,), (17,))),
                               bc=lsm.NeumannBC())
    with pytest.raises(ValueError, match="1 dimensional"):
        lsm.eikonal_(one)
    with pytest.raises(lsm.LsmError, match="1-dimensional"):
        one.backend.eikonal(one.current_state().buf, None, 0.0, INF, 0)
    fine = lsm.CartesianGrid(lc, hc, (17, 18, 16))
    band = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), bc=lsm.NeumannBC(),
                                ic=lsm.NarrowBandMeshField(lsm.MeshField(lambda x: np.sqrt(x[0] ** 2 + x[1] ** 2 + x[2] ** 2) - 0.5, fine), nlayers=2))
    with pytest.raises(ValueError, match="NarrowBandMeshField"):
        lsm.eikonal_(band)
    g = lsm.LocalGroup(1)
    slab = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(phi0, grid), bc=lsm.NeumannBC(), comm=g.rank(0))
    with pytest.raises(ValueError, match="slab"):
        lsm.eikonal_(slab)
    with pytest.raises(lsm.LsmError, match="slab"):
        slab.backend.eikonal(slab.current_state().buf, None, 0.0, INF, 0)
    assert np.array_equal(_bits(slab.current_state().values()), _bits(phi0))
    assert np.array_equal(_bits(phi.values()), _bits(before))
    lsm.eikonal_(phi)                                   # and the handle still works
    assert not np.array_equal(phi.values(), before)


def test_round_trip_from_a_mesh():
    """mesh_distance(…, cutoff = 3h, far="eikonal"): exact where plain mesh_distance is below the width, first order beyond"""
    lsm = _lsm()
    v, e, n, lc, hc, h, c, width, exact, bound, want = mesh_seeded_case()
    grid = lsm.CartesianGrid(lc, hc, n)
    near = lsm.mesh_distance((v, e), grid, cutoff=c)
    again = lsm.mesh_distance((v, e), grid, cutoff=c, far=None)
    assert np.array_equal(_bits(np.asarray(near.vals)), _bits(np.asarray(again.vals)))
    full = np.asarray(lsm.mesh_distance((v, e), grid, cutoff=c, far="eikonal").vals)
    err = float(np.abs(full - exact).max())
    print(f"max |ϕ − (|x| − r)| = {err / h.max():.3f} h_max (bound {bound / h.max():.2f} h_max)")
    assert err <= bound
    inside = np.abs(np.asarray(near.vals)) <= width
    assert inside.any() and not inside.all()
    assert np.array_equal(_bits(full[inside]), _bits(np.asarray(near.vals)[inside]))
    _close(full, want, n, float(np.abs(want).max()), "mesh-seeded")
    assert np.abs(full).max() > c
    with pytest.raises(ValueError, match="far must be"):
        lsm.mesh_distance((v, e), grid, cutoff=c, far="sweep")
    with pytest.raises(ValueError, match="larger than one cell diagonal"):
        lsm.mesh_distance((v, e), grid, cutoff=0.5 * float(h.min()), far="eikonal")


def test_scratch_reuse_and_statistics():
    """a handle's second call reuses its scratch (with and without a speed, with another seeding); handles of a smaller, then a
    larger grid each get their own"""
    lsm = _lsm()
    for name in ("one_tile", "two_spheres_speed", "nine_tiles_3d"):
        phi0, n, lc, hc, h, speed = R.fixture(name)
        phi = _field(lsm, phi0, lc, hc)
        keep = phi.backend.clone(phi.buf)
        first = phi.backend.eikonal(phi.buf, speed, 0.0, INF, 0)
        out = phi.values()
        phi.backend.copy_(phi.buf, keep)
        assert phi.backend.eikonal(phi.buf, None, 1.5 * float(h.max()), 2 * float(h.max()), 0)[3] > 0
        phi.backend.copy_(phi.buf, keep)
        second = phi.backend.eikonal(phi.buf, speed, 0.0, INF, 0)
        assert first[0] == second[0] and first[3] == second[3] == 0 and second[1] > 0 and second[2] >= second[1]
        assert np.array_equal(_bits(phi.values()), _bits(out))
        # a distance is a fixed point of its own width seeding: nothing moves
        if speed is None:
            assert phi.backend.eikonal(phi.buf, None, 100.0, INF, 0) == (phi0.size, 0, 0, 0) and np.array_equal(_bits(phi.values()), _bits(out))
