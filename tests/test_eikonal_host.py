"""The restatement of eikonal_ (tests/_eikonal_ref.py) pinned on the host: the three solvers (Jacobi, Gauss–Seidel sweeps, heap fast
marching) reach the same fixed point within tol = 16·Σ(n_d − 1)·eps·max T on every fixture the device tests use, the fixed point
has no residual, it converges to the distance of a sphere, a cutoff only clamps, a uniform speed only scales, and the seeding's
edge cases; the fixtures of tests/test_gpu_eikonal_edges.py (checkerboards and their census of G's branches, plane fronts, 300
and 336 tiles, seed fields) and what holds of them on the restatement.  No device."""
import functools

import numpy as np
import pytest

import _eikonal_ref as R
import _iso_ref as I
import _mdist_ref as M

INF = float("inf")


def widths(h):
    return (None, 1.5 * float(h.max()))


@functools.lru_cache(maxsize=None)
def solved(name, seeding):
    """(T, frozen, passes) of the Jacobi solver, computed once, read-only; seeding 0: crossing seed, 1: width = 1.5·h_max"""
    phi, n, lc, hc, h, speed = R.fixture(name)
    slow = None if speed is None else 1.0 / speed
    T0, frozen = R.seed(phi, h, slow, widths(h)[seeding])
    T, passes = R.solve_jacobi(T0, frozen, h, slow)
    for a in (T, frozen, T0):
        a.setflags(write=False)
    return T, frozen, passes, T0


def test_scalar_and_vector_update_agree_bit_for_bit():
    rng = np.random.default_rng(3)
    for N, h in ((2, (0.3, 0.2)), (3, (0.3, 0.2, 0.25)), (3, (0.002, 0.002, 0.0021))):
        a = rng.random((N, 4000)) * 3 * max(h)
        a[rng.random((N, 4000)) < 0.15] = INF
        a[:, :50] = a[0, :50]                         # ties
        a[:, 50:60] = INF
        s = 0.25 + 3 * rng.random(4000)
        v = R.G_vec(a, s, np.array(h))
        w = np.array([R.G([float(x) for x in a[:, i]], float(s[i]), list(h)) for i in range(4000)])
        assert np.array_equal(v, w)
        fin = np.isfinite(v)
        assert (v[fin] > a.min(axis=0)[fin]).all() and not fin[50:60].any()


@pytest.mark.parametrize("name", list(R.FIXTURES))
@pytest.mark.parametrize("seeding", (0, 1), ids=("crossing", "width"))
def test_the_three_solvers_agree(name, seeding):
    phi, n, lc, hc, h, speed = R.fixture(name)
    slow = None if speed is None else 1.0 / speed
    T, frozen, passes, T0 = solved(name, seeding)
    assert np.isfinite(T).all() and (T >= 0).all() and 0 < frozen.sum() < T.size
    assert np.array_equal(T[frozen], T0[frozen])
    tmax = float(T.max())
    tol = R.tol(n, tmax)
    Ts, _ = R.solve_sweep(T0, frozen, h, slow)
    Tf = R.solve_fmm(T0, frozen, h, slow)
    spread = max(float(np.abs(Ts - T).max()), float(np.abs(Tf - T).max()), float(np.abs(Tf - Ts).max()))
    print(f"{name}/{seeding}: spread {spread / (R.EPS * tmax):.3g} eps·max T (tol {tol / (R.EPS * tmax):.0f}), {passes} Jacobi passes")
    assert spread <= tol
    res = R.residual(T, frozen, h, slow)
    print(f"residual {res / (R.EPS * tmax):.3g} eps·max T")
    assert res <= 16 * R.EPS * tmax


@pytest.mark.parametrize("N", (2, 3))
@pytest.mark.parametrize("seeding", (0, 1), ids=("crossing", "width"))
def test_accuracy_on_a_sphere(N, seeding):
    """max |T − ||x − c| − r|| <= h_max, and smaller at twice the resolution"""
    errs = []
    for n1 in (17, 33) if N == 3 else (33, 65):
        n = (n1, n1 - 2, n1 - 1)[:N]
        lc, hc = (-1.0, -1.1, -0.9)[:N], (1.0, 1.2, 1.1)[:N]
        balls = [((0.05, -0.02, 0.03)[:N], 0.5)]
        phi = R.spheres(n, lc, hc, balls)
        h = R.meshsize(n, lc, hc)
        T0, frozen = R.seed(phi, h, None, widths(h)[seeding])
        T, _ = R.solve_jacobi(T0, frozen, h)
        errs.append(float(np.abs(T - np.abs(phi)).max()))
        print(f"n = {n}: max error {errs[-1] / h.max():.3f} h_max")
        assert errs[-1] <= h.max()
    assert errs[1] < errs[0]


@pytest.mark.parametrize("name", ("partial_tiles", "two_circles"))
def test_a_cutoff_only_clamps(name):
    """a solve that prunes at the cutoff (the tile schedule's rule: a change to a value >= c wakes nobody), then min(T, c): the
    values <= c are the ones of the solve without a cutoff, the rest are ±c"""
    phi, n, lc, hc, h, speed = R.fixture(name)
    slow = None if speed is None else 1.0 / speed
    T, frozen, _, T0 = solved(name, 0)
    full = np.copysign(T, phi)
    for c in (3 * float(h.max()), 0.5 * float(h.min())):
        Tc, launches, visits = R.solve_tiles(T0, frozen, h, slow, cutoff=c)
        assert visits < R.solve_tiles(T0, frozen, h, slow)[2]          # the front was not followed beyond c
        out = R.eikonal(phi, h, speed, None, c, T=Tc)
        near = T <= c
        assert near.any() and not near.all()
        assert np.array_equal(out[near], full[near]) and (np.abs(out[~near]) == c).all()
        assert np.array_equal(np.signbit(out), np.signbit(phi))


def test_uniform_speed_gives_distance_over_speed():
    phi, n, lc, hc, h, _ = R.fixture("partial_tiles")
    T = solved("partial_tiles", 0)[0]
    for F in (2.0, 0.3):
        T0, frozen = R.seed(phi, h, 1.0 / F, None)
        TF, _ = R.solve_jacobi(T0, frozen, h, 1.0 / F)
        assert float(np.abs(TF - T / F).max()) <= R.tol(n, max(T.max(), TF.max()))


def test_seeding_edge_cases():
    h = np.array([0.5, 0.25])
    # ϕ = 0 on a node; ϕ_J = 0 next to ϕ_I != 0: σ = h_d, whole
    phi = np.asfortranarray(np.array([[-1.0, -0.5, 0.0, 0.5, 1.0]] * 4).T)       # (5, 4): zero along the line i = 2
    T0, frozen = R.seed(phi, h)
    assert (T0[2] == 0).all() and frozen[2].all()
    assert frozen[1].all() and frozen[3].all() and not frozen[0].any() and not frozen[4].any()
    assert np.array_equal(T0[1], np.full(4, 1.0 / np.sqrt(1.0 / (0.5 * 0.5))))
    T, _ = R.solve_jacobi(T0, frozen, h)
    assert np.array_equal(T[:, 0], [1.0, 0.5, 0.0, 0.5, 1.0])
    assert np.array_equal(np.signbit(R.eikonal(np.where(phi == 0, -0.0, phi), h)), np.signbit(np.where(phi == 0, -0.0, phi)))
    # the width seeding keeps |ϕ| there and freezes what is within w
    T0, frozen = R.seed(phi * 0.7, h, None, 0.4)
    assert frozen[1:4].all() and not frozen[0].any() and np.array_equal(T0[1], np.full(4, 0.35))
    # an interface leaving the grid through a face: the crossing next to the face is seeded from the neighbours that exist
    phi = np.asfortranarray(np.fromfunction(lambda i, j: (i * 0.5 - 1.6) + 0 * j, (5, 4)))
    T0, frozen = R.seed(phi, h)
    assert frozen[3].all() and frozen[4].all() and not frozen[:3].any()
    assert np.allclose(T0[3], 0.1) and np.allclose(T0[4], 0.4)
    # a sliver of one sign, one node thick: crossings on both sides, the nearer one wins per axis
    phi = np.asfortranarray(np.array([[1.0, 0.75, -0.05, 0.2, 1.0]] * 4).T)
    T0, frozen = R.seed(phi, h)
    assert frozen[1:4].all() and not frozen[0].any() and not frozen[4].any()
    sig = min(0.5 * (0.05 / (0.05 + 0.75)), 0.5 * (0.05 / (0.05 + 0.2)))
    assert sig == 0.5 * (0.05 / (0.05 + 0.75)) and T0[2, 0] == 1.0 / np.sqrt(1.0 / (sig * sig))
    # the refusals
    for bad in (np.full((5, 4), 1.0), np.where(np.arange(20).reshape(5, 4) == 7, np.nan, phi)):
        with pytest.raises(ValueError):
            R.seed(bad, h)
    for s in (0.0, -1.0, INF, np.nan):
        with pytest.raises(ValueError):
            R.seed(phi, h, s)


def test_the_shifted_form_is_what_keeps_the_solvers_together():
    """the un-shifted textbook quadratic gives the same numbers to rounding, with a larger spread between visiting orders"""
    phi, n, lc, hc, h, speed = R.fixture("tiny_h")
    slow = 1.0 / speed
    T, frozen, _, T0 = solved("tiny_h", 0)
    Tt, _ = R.solve_sweep(T0, frozen, h, slow, update=R.G_textbook)
    assert float(np.abs(Tt - T).max()) <= 1e-9 * float(T.max())


@functools.lru_cache(maxsize=None)
def mesh_seeded_case():
    """(vertices, elements, n, lc, hc, h, cutoff, width, |x| − r, the bound on the error, the restatement's result) of
    mesh_distance(sphere mesh, grid, cutoff = 3h, far="eikonal") on a 21×19×17 grid"""
    n, lc, hc = (21, 19, 17), (-1.0, -1.1, -0.9), (1.0, 1.2, 1.1)
    h = R.meshsize(n, lc, hc)
    exact = R.spheres(n, lc, hc, [((0.05, -0.02, 0.03), 0.55)])
    v, e = I.isosurface(exact, lc, hc)
    c = 3 * float(h.max())
    width = c - float(np.sqrt((h * h).sum()))
    near, stats = M.mesh_distance(v, e, n, lc, hc, c)
    assert stats[1] == 0
    want = R.eikonal(near, h, None, width)
    for a in (exact, near, want):
        a.setflags(write=False)
    return v, e, n, lc, hc, h, c, width, exact, 1.5 * float(h.max()), want


def test_mesh_seeded_far_field_is_within_the_bound():
    """the round trip the device test runs, on the restatements: exact distances within the width, first order beyond"""
    v, e, n, lc, hc, h, c, width, exact, bound, want = mesh_seeded_case()
    err = float(np.abs(want - exact).max())
    print(f"mesh-seeded: max error {err / h.max():.3f} h_max")
    assert 0 < width < c and err <= bound
    assert np.array_equal(np.signbit(want), np.signbit(exact))


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_the_tile_schedule_reaches_the_same_fixed_point(name):
    """the device's activation rule, run one tile after the other with the halo read before the launch or as the earlier tiles left
    it: both end, at the Jacobi fixed point; with a cutoff the values <= c are the ones without it"""
    phi, n, lc, hc, h, speed = R.fixture(name)
    slow = None if speed is None else 1.0 / speed
    for seeding in (0, 1):
        T, frozen, passes, T0 = solved(name, seeding)
        tmax = float(T.max())
        for snapshot in (True, False):
            Tt, launches, visits = R.solve_tiles(T0, frozen, h, slow, snapshot=snapshot)
            d = float(np.abs(Tt - T).max())
            print(f"{name}/{seeding}/{'before' if snapshot else 'during'}: {launches} launches, {visits} visits, difference {d / (R.EPS * tmax):.3g} eps·max T")
            assert d <= R.tol(n, tmax) and launches >= -(-passes // 8)
        for c in (3 * float(h.max()), 0.5 * float(h.min())):
            Tc = R.solve_tiles(T0, frozen, h, slow, cutoff=c)[0]
            near = T <= c
            assert float(np.abs(Tc[near] - T[near]).max()) <= R.tol(n, tmax) and (Tc[~near] > c).all()


# ---- the fixtures of tests/test_gpu_eikonal_edges.py: checkerboards, plane fronts, many tiles, seeds

@functools.lru_cache(maxsize=None)
def checkerboard_case(name, f32=False):
    """a checkerboard with ϕ > 0, solved once, read-only: (phi, n, lc, hc, h, speed, w, T, T0, frozen, (free, g, stage, ties of
    the two smallest, ties of the two largest), (launches, visits) of the tile schedule); ϕ < 0 is the same T with the other sign"""
    phi, n, lc, hc, h, speed, w = R.checkerboard(name, 1.0, f32)
    T0, frozen = R.seed(phi, h, 1.0 / speed, w)
    T, _ = R.solve_jacobi(T0, frozen, h, 1.0 / speed)
    census = R.checkerboard_census(phi, h, speed, w)
    tiles = R.solve_tiles(T0, frozen, h, 1.0 / speed)
    assert np.array_equal(tiles[0], T)
    for a in (phi, speed, T, T0, frozen) + census[:3]:
        a.setflags(write=False)
    return phi, n, lc, hc, h, speed, w, T, T0, frozen, census, tiles[1:]


@functools.lru_cache(maxsize=None)
def plane_case(name, axis, end):
    """(phi, n, lc, hc, h, T, frozen, (launches, visits)) of a plane front (R.plane), the crossing seed, s ≡ 1"""
    phi, n, lc, hc, h = R.plane(name, axis, end)
    T0, frozen = R.seed(phi, h)
    T, launches, visits = R.solve_tiles(T0, frozen, h)
    for a in (phi, T, frozen):
        a.setflags(write=False)
    return phi, n, lc, hc, h, T, frozen, (launches, visits)


@functools.lru_cache(maxsize=None)
def solved_f32(name, seeding):
    """solved() of the fixture rounded to float32: (phi as float32, T, frozen, passes, T0)"""
    phi, n, lc, hc, h, speed = R.fixture(name)
    p32 = phi.astype(np.float32)
    slow = None if speed is None else 1.0 / speed
    T0, frozen = R.seed(p32.astype(np.float64), h, slow, widths(h)[seeding])
    T, passes = R.solve_jacobi(T0, frozen, h, slow)
    for a in (p32, T, frozen, T0):
        a.setflags(write=False)
    return p32, T, frozen, passes, T0


# the launches and visits of the tile schedule on the checkerboards: every tile once, and once more because every face woke a
# neighbour (one tile: its only pass changes something, nobody is woken)
CB_STATS = {"cb_336_tiles": (2, 672), "cb_300_tiles": (2, 600), "cb_one_tile": (1, 1), "cb_4x4x4": (1, 1), "cb_4x4": (1, 1), "cb_2x2x2": (1, 1),
            "cb_2x2": (1, 1)}


@pytest.mark.parametrize("f32", (False, True), ids=("fp64", "f32-rounded"))
@pytest.mark.parametrize("name", list(R.CHECKERBOARDS))
def test_checkerboard_construction_and_census(name, f32):
    """frozen is exactly the even nodes, nothing is crossing-adjacent, every free node is the scalar G of its neighbour minima
    after one pass with either halo order, and the branches of G are all there: at least 100 nodes of every stage the dimension
    has and 500 of each tie on the two large grids (the small ones have 2 to 105 free nodes: every stage at least once from
    7×6×5 on, and every stage over the 2- and 4-node grids together)"""
    phi, n, lc, hc, h, speed, w, T, T0, frozen, (free, g, stage, tie_small, tie_large), stats = checkerboard_case(name, f32)
    N = len(n)
    even = np.indices(n).sum(axis=0) % 2 == 0
    assert np.array_equal(frozen, even) and np.array_equal(free, ~even)
    with pytest.raises(ValueError, match="no interface"):         # no node is crossing-adjacent or zero: the width alone freezes
        R.seed(phi, h, 1.0 / speed, None)
    assert (phi > 0).all() and (phi[free] == R.CB_FREE).all() and (phi[even] <= 0.99 * w * (1 + 1e-7)).all()
    assert np.array_equal(T[even], phi[even]) and np.array_equal(T[free], g[free])
    assert np.array_equal(np.abs(R.eikonal(-phi, h, speed, w)), T) and (R.eikonal(-phi, h, speed, w) < 0).all()
    T0n, frozen_n = R.seed(-phi, h, 1.0 / speed, w)
    assert np.array_equal(T0n, T0) and np.array_equal(frozen_n, frozen)
    for snapshot in (True, False):
        Tt, launches, visits = R.solve_tiles(T0, frozen, h, 1.0 / speed, snapshot=snapshot)
        assert np.array_equal(Tt, T) and (launches, visits) == stats == CB_STATS[name]
    counts = np.bincount(stage[free], minlength=4)
    print(f"{name}: {int(free.sum())} free nodes, stages 1/2/3: {counts[1]}/{counts[2]}/{counts[3]}, ties of the two smallest {tie_small}, of the two largest {tie_large}")
    assert counts[0] == 0 and counts[1:N + 1].sum() == free.sum()
    if name in ("cb_336_tiles", "cb_300_tiles"):
        assert (counts[1:N + 1] >= 100).all() and tie_small >= 500 and tie_large >= 500
        assert len(set(float(x) for x in h)) == N
    elif name == "cb_one_tile":
        assert (counts[1:N + 1] >= 1).all()
    # the cutoff below every free result: no change is live, so the first launch wakes nobody
    c = 0.5 * float(T[free].min())
    for snapshot in (True, False):
        Tc, launches, visits = R.solve_tiles(T0, frozen, h, 1.0 / speed, cutoff=c, snapshot=snapshot)
        assert np.array_equal(Tc, T) and (launches, visits) == (1, R.ntiles(n))
    assert (np.abs(R.eikonal(phi, h, speed, w, c))[free] == c).all()


def test_g_stage_names_the_branch():
    h = [0.3, 0.02, 0.11]
    assert R.G_stage([0.1, 0.5, 0.9], 1.0, h) == 1 and R.G([0.1, 0.5, 0.9], 1.0, h) == 0.1 + 1.0 * 0.3      # 0.4 <= 0.5
    assert R.G_stage([0.1, 0.3, 0.9], 1.0, h) == 2                                                         # 0.4 > 0.3, τ2 <= s·h1
    assert R.G_stage([0.1, 0.1, 0.1], 1.0, h) == 3
    assert R.G_stage([0.1, INF, INF], 1.0, h) == 1 and R.G_stage([INF, INF, INF], 1.0, h) == 0
    assert R.G_stage([0.1, 0.3], 1.0, h[:2]) == 2 and R.G_stage([0.1, 0.5], 1.0, h[:2]) == 1
    rng = np.random.default_rng(5)
    for _ in range(500):
        a = [float(x) for x in rng.random(3)]
        s = 0.25 + 3 * float(rng.random())
        g, k = R.G(a, s, h), R.G_stage(a, s, h)
        srt = sorted(a)
        assert g > srt[k - 1] and (k == 3 or g <= srt[k])             # causality: exactly the k smallest lie below G


PLANES = [("many_tiles_3d", d, e) for d in (2, 1, 0) for e in (0, 1)] + [("many_tiles_2d", 1, 0), ("many_tiles_2d", 1, 1)]


@pytest.mark.parametrize("name,axis,end", PLANES, ids=[f"{n}-axis{d}-{('up', 'down')[e]}" for n, d, e in PLANES])
def test_plane_fronts_do_not_depend_on_the_schedule(name, axis, end):
    """R.plane: the same bits as Jacobi and the same launches and visits with either halo order — the front crosses one layer of
    tiles per launch (8 passes are one tile edge along the axes used; along axis 0 of the 32×8 tiles they are not, and there the
    counts do depend on the order: that plane is left out)"""
    phi, n, lc, hc, h, T, frozen, stats = plane_case(name, axis, end)
    T0 = R.seed(phi, h)[0]
    Tj, passes = R.solve_jacobi(T0, frozen, h)
    assert np.array_equal(T, Tj) and passes == n[axis] - 2
    assert (np.signbit(phi) == (end == 1)).all() and int(frozen.sum()) == 2 * T.size // n[axis]
    Td, launches, visits = R.solve_tiles(T0, frozen, h, snapshot=False)
    print(f"{name} axis {axis} end {end}: {stats[0]} launches, {stats[1]} visits, {passes} Jacobi passes")
    assert np.array_equal(Td, Tj) and (launches, visits) == stats
    assert stats[0] >= -(-n[axis] // R.TILES[len(n)][axis]) and R.unsatisfied(T, frozen, h) == 0


LARGE_CASES = [(name, s) for name in R.LARGE for s in (0, 1)]


@pytest.mark.parametrize("name,seeding", LARGE_CASES, ids=[f"{n}-{('crossing', 'width')[s]}" for n, s in LARGE_CASES])
def test_many_tiles_what_holds_when_the_schedule_shows(name, seeding):
    """300 and 336 tiles: the tile schedule with either halo order is within tol of Jacobi, no free node is left with G < T, the
    residual is within the bar of test_the_three_solvers_agree — and the bits are not Jacobi's (many_tiles_3d), which is why the
    device tests of these fixtures do not ask for them"""
    phi, n, lc, hc, h, speed = R.fixture(name)
    slow = None if speed is None else 1.0 / speed
    T, frozen, passes, T0 = solved(name, seeding)
    tmax = float(T.max())
    assert np.isfinite(T).all() and R.ntiles(n) >= 300
    assert R.unsatisfied(T, frozen, h, slow) == 0 and R.residual(T, frozen, h, slow) <= 16 * R.EPS * tmax
    outs = []
    for snapshot in (True, False):
        Tt, launches, visits = R.solve_tiles(T0, frozen, h, slow, snapshot=snapshot)
        d = np.abs(Tt - T)
        res = R.residual(Tt, frozen, h, slow)
        print(f"{name}/{seeding}/{'before' if snapshot else 'during'}: {launches} launches, {visits} visits, {passes} Jacobi passes, "
              f"{int((d != 0).sum())} nodes differ from Jacobi by at most {d.max() / (R.EPS * tmax):.3g} eps·max T "
              f"(tol {R.tol(n, tmax) / (R.EPS * tmax):.0f}), residual {res / (R.EPS * tmax):.3g} eps·max T")
        assert d.max() <= R.tol(n, tmax)
        assert np.array_equal(Tt[frozen], T0[frozen])
        assert R.unsatisfied(Tt, frozen, h, slow) == 0
        assert res <= 16 * R.EPS * tmax
        assert -(-passes // 8) <= launches <= visits <= launches * R.ntiles(n)
        if name == "many_tiles_3d":
            assert (d != 0).any()
        outs.append(Tt)
    print(f"{int((outs[0] != outs[1]).sum())} nodes differ between the two halo orders")


def test_unsatisfied_notices_a_node_that_was_not_updated():
    """one free node left above G of its neighbours — by one ulp, or at +inf as a tile that was never woken leaves it — counts;
    one below it does not (T never rises: such a node is what the strict rule leaves alone)"""
    phi, n, lc, hc, h, speed = R.fixture("two_spheres_speed")
    T, frozen, _, _ = solved("two_spheres_speed", 0)
    free = np.argwhere(~frozen)
    for at in (free[0], free[len(free) // 2], free[-1]):
        I = tuple(int(i) for i in at)
        for value, count in ((np.nextafter(T[I], INF), 1), (INF, 1), (np.nextafter(T[I], 0.0), 0)):
            Tp = np.array(T, order="F")
            Tp[I] = value
            downstream = R.unsatisfied(Tp, frozen, h, 1.0 / speed, where=np.arange(T.size).reshape(n, order="F") != np.ravel_multi_index(I, n, order="F"))
            assert R.unsatisfied(Tp, frozen, h, 1.0 / speed) - downstream == count


def test_seed_fields_on_the_restatement():
    """the fields tests/test_gpu_eikonal_edges.py seeds the device with: what each is there for holds on the restatement"""
    F = R.seed_fields()
    seeds = {k: R.seed(phi, R.meshsize(phi.shape, lc, hc)) for k, (phi, lc, hc, _) in F.items()}
    T0, frozen = seeds["zero_line"]
    assert (T0[2] == 0).all() and frozen[1:4].all() and not frozen[0].any() and not frozen[4].any() and (T0[1] == 0.5).all()
    phi = F["negative_zero_line"][0]
    assert np.signbit(phi[2]).all() and np.array_equal(seeds["negative_zero_line"][0], T0)
    assert np.array_equal(np.signbit(R.eikonal(phi, np.array([0.5, 0.25]))), np.signbit(phi))
    phi = F["one_zero_node"][0]
    T0, frozen = seeds["one_zero_node"]
    assert int((phi == 0).sum()) == 1 and phi[2, 1] == 0 and T0[2, 1] == 0
    # towards the zero σ = h_d, whole: alone along axis 0 at (1, 1); at (2, 0) beside a crossing a quarter of h_0 away along axis 0
    assert T0[1, 1] == 1.0 / np.sqrt(1.0 / (0.5 * 0.5)) and T0[2, 0] == 1.0 / np.sqrt(1.0 / (0.125 * 0.125) + 1.0 / (0.25 * 0.25))
    T0, frozen = seeds["sliver"]
    assert frozen[1:4].all() and not frozen[0].any() and not frozen[4].any()
    T0, frozen = seeds["leaves_through_a_face"]
    assert frozen[3:].all() and not frozen[:3].any()
    T0, frozen = seeds["zero_plane"]
    assert (T0[2] == 0).all() and frozen[1:4].all() and not frozen[0].any() and not frozen[4].any()
    T0, frozen = seeds["face_node_one_axis"]
    assert frozen[:, :, 4:].all() and not frozen[:, :, :4].any()
    assert np.allclose(T0[:, :, 5], 0.075) and np.allclose(T0[:, :, 4], 0.05)
    for k in ("corner_4x4", "corner_4x4x4", "corner_2x2", "corner_2x2x2"):
        phi = F[k][0]
        assert int((phi < 0).sum()) == 1 and int(seeds[k][1].sum()) == phi.ndim + 1 and (phi != 0).all()
    # the distances are fixed points of their own width seeding up to the first-order error; the rest are not asked for it
    for k, (phi, lc, hc, dist) in F.items():
        h = R.meshsize(phi.shape, lc, hc)
        assert len(set(float(x) for x in h)) == phi.ndim
        if dist:
            T0, frozen = R.seed(phi, h, None, 1.5 * float(h.max()))
            assert frozen.sum() >= seeds[k][1].sum() and np.array_equal(T0[frozen], np.abs(phi)[frozen])


def test_one_launch_is_not_enough_for_the_long_grid():
    """what the device test of max_iters = 1 relies on"""
    phi, n, lc, hc, h, _ = R.fixture("nine_tiles_2d")
    T, frozen, passes, T0 = solved("nine_tiles_2d", 0)
    assert passes > 8 and R.solve_tiles(T0, frozen, h)[1] > 2
    with pytest.raises(RuntimeError):
        R.solve_tiles(T0, frozen, h, max_iters=2)
