"""The restatement of eikonal_ (tests/_eikonal_ref.py) pinned on the host: the three solvers (Jacobi, Gauss–Seidel sweeps, heap fast
marching) reach the same fixed point within tol = 16·Σ(n_d − 1)·eps·max T on every fixture the device tests use, the fixed point
has no residual, it converges to the distance of a sphere, a cutoff only clamps, a uniform speed only scales, and the seeding's
edge cases.  No device."""
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


def test_one_launch_is_not_enough_for_the_long_grid():
    """what the device test of max_iters = 1 relies on"""
    phi, n, lc, hc, h, _ = R.fixture("nine_tiles_2d")
    T, frozen, passes, T0 = solved("nine_tiles_2d", 0)
    assert passes > 8 and R.solve_tiles(T0, frozen, h)[1] > 2
    with pytest.raises(RuntimeError):
        R.solve_tiles(T0, frozen, h, max_iters=2)
