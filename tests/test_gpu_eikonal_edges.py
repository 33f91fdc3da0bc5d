"""eikonal_ on the device (csrc/lsm_eikonal.hip) where tests/test_gpu_eikonal.py does not reach:
  A. checkerboards — every free node has only frozen neighbours, so the result is G of chosen inputs after one pass whatever the
     schedule: the update (ties between axes of different h, strong anisotropy, every stage entered and not entered) and the
     launch bookkeeping (two compaction workgroups, three different tile counts, last tiles 1, 2 and 3 nodes thick) bit for bit
     against the restatement at 336 and 300 tiles, with the statistics exact; plane fronts, whose launches and visits do not
     depend on the schedule either and which reach the next layer of tiles through one face flag and one stride alone;
  B. two spheres over 336 tiles and two circles over 300, where the schedule shows in the last bits: what must hold then —
     signs, seeds, tol, no free node with G < T, the residual, the statistics' bounds — and what is only printed;
  C. the seeding's edge cases on one tile, where the bits of the restatement are owed.
A device handle has at least 4 nodes per dimension (lsm_create), so the 2-node grids lsm_eikonal's own check allows are refused
before it: the smallest grids here are 4×4 and 4×4×4; the restatement runs 2×2 and 2×2×2 (tests/test_eikonal_host.py)."""
import numpy as np
import pytest

import _eikonal_ref as R
from test_eikonal_host import CB_STATS, PLANES, checkerboard_case, plane_case, solved, solved_f32, widths

pytestmark = pytest.mark.gpu

INF = float("inf")
PASSES = 8      # Jacobi passes per visit of a tile (EK_PASSES)


def _lsm():
    import lsm_amd
    return lsm_amd


def _field(lsm, vals, lc, hc, dtype=None):
    mf = lsm.MeshField(vals, lsm.CartesianGrid(lc, hc, vals.shape), dtype=dtype)
    return lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=mf, bc=lsm.NeumannBC()).current_state()


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _run(phi0, lc, hc, h, speed=None, width=None, cutoff=INF, f32=False):
    """(ϕ after lsm_eikonal, stats) on a handle of ϕ0's grid; f32: a float32 handle (ϕ0 is then float32-representable)"""
    lsm = _lsm()
    phi = _field(lsm, phi0.astype(np.float32) if f32 else phi0, lc, hc, dtype=np.float32 if f32 else None)
    assert np.array_equal(h, np.array(phi.mesh.meshsize()))
    stats = phi.backend.eikonal(phi.buf, speed, 0.0 if width is None else width, cutoff, 0)
    got = phi.values()
    assert got.dtype == (np.float32 if f32 else np.float64) and got.shape == phi0.shape
    return got, stats


def _same_bits(got, want):
    want = want.astype(got.dtype)
    assert np.array_equal(_bits(got), _bits(want)), f"{int((_bits(got) != _bits(want)).sum())} of {got.size} nodes differ"


# ---- A. checkerboards and plane fronts

DEVICE_CB = [k for k in R.CHECKERBOARDS if min(R.CHECKERBOARDS[k][0]) >= 4]
CB_CASES = [(name, sign, f32) for name in DEVICE_CB for sign in (1.0, -1.0) for f32 in ((False, True) if name in ("cb_336_tiles", "cb_300_tiles") else (False,))]


@pytest.mark.parametrize("name,sign,f32", CB_CASES, ids=[f"{n}-{'pos' if s > 0 else 'neg'}-{'f32' if f else 'fp64'}" for n, s, f in CB_CASES])
def test_checkerboard(name, sign, f32):
    """ϕ equals the restatement's bit for bit (float32: its fp64 result rounded once), every free node is the scalar G of its
    neighbour minima, the sign is kept, and the statistics are the tile schedule's: 2 launches and 2·tiles visits where there is
    more than one tile, 1 and 1 on one tile"""
    phi, n, lc, hc, h, speed, w, T, T0, frozen, (free, g, stage, _, _), tiles = checkerboard_case(name, f32)
    got, stats = _run(sign * phi, lc, hc, h, speed, w, f32=f32)
    print(f"{name}: stats {stats}, {R.ntiles(n)} tiles")
    assert (np.signbit(got) == (sign < 0)).all()
    _same_bits(got, np.copysign(T, sign))
    assert np.array_equal(np.abs(got)[free], g[free].astype(got.dtype))
    assert stats == (int(frozen.sum()), tiles[0], tiles[1], 0) and tiles == CB_STATS[name]


@pytest.mark.parametrize("name", DEVICE_CB)
def test_checkerboard_cutoff_below_every_free_result(name):
    """c = half the smallest free result: no change is live, one launch over every tile wakes nobody, every free node (and every
    frozen one above c) comes back as ±c and is counted"""
    phi, n, lc, hc, h, speed, w, T, T0, frozen, (free, g, stage, _, _), tiles = checkerboard_case(name)
    c = 0.5 * float(T[free].min())
    launches, visits = R.solve_tiles(T0, frozen, h, 1.0 / speed, cutoff=c)[1:]
    for sign in (1.0, -1.0):
        got, stats = _run(sign * phi, lc, hc, h, speed, w, cutoff=c)
        print(f"{name}: c = {c:.3g}, stats {stats}")
        _same_bits(got, R.eikonal(sign * phi, h, speed, w, c, T=T))
        assert (got[free] == sign * c).all()
        assert stats == (int(frozen.sum()), launches, visits, int((T > c).sum())) and stats[3] >= int(free.sum())
        assert (launches, visits) == (1, R.ntiles(n))


def test_two_node_grids_do_not_reach_the_kernels():
    """lsm_eikonal's own minimum is two nodes per dimension, a handle's is four: 2×2 and 2×2×2 are refused when the handle is made"""
    lsm = _lsm()
    for name in ("cb_2x2", "cb_2x2x2"):
        phi, n, lc, hc, h, speed, w = R.checkerboard(name)
        with pytest.raises(lsm.LsmError, match="at least 4 nodes per dimension"):
            _field(lsm, phi, lc, hc)


@pytest.mark.parametrize("name,axis,end", PLANES, ids=[f"{n}-axis{d}-{('up', 'down')[e]}" for n, d, e in PLANES])
def test_plane_front(name, axis, end):
    """a front moving along one axis, up or down: the restatement's bits, −0.0 kept, and exactly its launches and visits — a
    layer of tiles that its neighbour's face flag did not reach is woken from the side one launch later, and both counts show it"""
    phi, n, lc, hc, h, T, frozen, tiles = plane_case(name, axis, end)
    got, stats = _run(phi, lc, hc, h)
    print(f"{name} axis {axis} end {end}: stats {stats}, the restatement's launches and visits {tiles}")
    _same_bits(got, np.copysign(T, phi))
    assert stats == (int(frozen.sum()), tiles[0], tiles[1], 0)


# ---- B. many tiles: what must hold when the schedule shows

def _invariants(got, stats, phi0, n, h, slow, T, T0, frozen, passes, what):
    """1–7 of DESIGN.md §7.15 "at size" for one call without a cutoff on an fp64 handle; prints the figures first"""
    tmax = float(T.max())
    mine = np.abs(got)
    d = np.abs(mine - T)
    res = R.residual(mine, frozen, h, slow) if np.isfinite(mine).all() else INF
    unsat = R.unsatisfied(mine, frozen, h, slow)
    print(f"{what}: stats {stats}; {int((d != 0).sum())} of {got.size} nodes differ from Jacobi, max {d.max() / (R.EPS * tmax):.3g} eps·max T "
          f"(tol {R.tol(n, tmax) / (R.EPS * tmax):.0f}); {unsat} free nodes with G < T; residual {res / (R.EPS * tmax):.3g} eps·max T; "
          f"{passes} Jacobi passes in the restatement")
    assert np.array_equal(np.signbit(got), np.signbit(phi0)) and np.array_equal(got == 0, phi0 == 0)       # 1
    assert np.array_equal(mine[frozen], T0[frozen])                                                       # 2
    assert d.max() <= R.tol(n, tmax)                                                                      # 3
    assert unsat == 0                                                                                     # 4
    assert res <= 16 * R.EPS * tmax                                                                       # 5
    assert stats[0] == int(frozen.sum()) and stats[3] == 0                                                # 6
    assert -(-passes // PASSES) <= stats[1] <= stats[2] <= stats[1] * R.ntiles(n)                         # 7


LARGE_CASES = [(name, s) for name in R.LARGE for s in (0, 1)]
LARGE_IDS = [f"{n}-{('crossing', 'width')[s]}" for n, s in LARGE_CASES]


@pytest.mark.parametrize("name,seeding", LARGE_CASES, ids=LARGE_IDS)
def test_many_tiles(name, seeding):
    """two calls, each held to the invariants; the bits of Jacobi and of the other call are printed, not asked for"""
    phi0, n, lc, hc, h, speed = R.fixture(name)
    slow = None if speed is None else 1.0 / speed
    T, frozen, passes, T0 = solved(name, seeding)
    outs = []
    for call in (1, 2):
        got, stats = _run(phi0, lc, hc, h, speed, widths(h)[seeding])
        _invariants(got, stats, phi0, n, h, slow, T, T0, frozen, passes, f"{name}/{('crossing', 'width')[seeding]} call {call}")
        outs.append(got)
    print(f"{name}/{('crossing', 'width')[seeding]}: {int((outs[0] != outs[1]).sum())} nodes differ between the two calls")


@pytest.mark.parametrize("seeding", (0, 1), ids=("crossing", "width"))
def test_many_tiles_float32(seeding):
    """a float32 handle on the float32-rounded input: every node lies between float32(T_j − tol) and float32(T_j + tol), T_j the
    fp64 Jacobi result of the same input; no node is left out"""
    name = "many_tiles_3d_speed"
    _, n, lc, hc, h, speed = R.fixture(name)
    p32, T, frozen, passes, T0 = solved_f32(name, seeding)
    tol = R.tol(n, float(T.max()))
    got, stats = _run(p32.astype(np.float64), lc, hc, h, speed, widths(h)[seeding], f32=True)
    mine = np.abs(got)
    print(f"{name} float32: stats {stats}, {int((mine != T.astype(np.float32)).sum())} nodes are not the rounded Jacobi value")
    assert np.array_equal(np.signbit(got), np.signbit(p32)) and np.array_equal(got == 0, p32 == 0)
    assert ((T - tol).astype(np.float32) <= mine).all() and (mine <= (T + tol).astype(np.float32)).all()
    assert np.array_equal(mine[frozen], T0[frozen].astype(np.float32))
    assert stats[0] == int(frozen.sum()) and stats[3] == 0
    assert -(-passes // PASSES) <= stats[1] <= stats[2] <= stats[1] * R.ntiles(n)


@pytest.mark.parametrize("name,seeding", LARGE_CASES, ids=LARGE_IDS)
def test_many_tiles_cutoff(name, seeding):
    """c = 3·h_max: the values <= c are within tol of the ones without a cutoff, the rest are ±c, and no free node with T <= c
    is left with G < T"""
    phi0, n, lc, hc, h, speed = R.fixture(name)
    slow = None if speed is None else 1.0 / speed
    T, frozen, passes, T0 = solved(name, seeding)
    tmax = float(T.max())
    tol = R.tol(n, tmax)
    c = 3 * float(h.max())
    want = R.eikonal(phi0, h, speed, None, c, T=T)
    got, stats = _run(phi0, lc, hc, h, speed, widths(h)[seeding], cutoff=c)
    d = np.abs(got - want)
    unsat = R.unsatisfied(np.abs(got), frozen, h, slow, where=T <= c)
    print(f"{name} c = {c:.3g}: stats {stats}; {int((d != 0).sum())} nodes differ, max {d.max() / (R.EPS * tmax):.3g} eps·max T; {unsat} free nodes "
          f"with T <= c and G < T; without a cutoff the restatement's Jacobi needs {passes} passes")
    assert np.array_equal(np.signbit(got), np.signbit(want)) and np.array_equal(got == 0, want == 0)
    assert d.max() <= tol
    far = T > c + tol
    assert far.any() and (np.abs(got[far]) == c).all() and np.abs(got).max() <= c
    assert unsat == 0
    assert stats[0] == int(frozen.sum())
    assert abs(stats[3] - int((T > c).sum())) <= int((np.abs(T - c) <= tol).sum())
    assert 1 <= stats[1] <= stats[2] <= stats[1] * R.ntiles(n)


# ---- C. seeds on one tile

SEEDS = R.seed_fields()
SEED_CASES = [(k, f32) for k in SEEDS if min(SEEDS[k][0].shape) >= 4 for f32 in (False, True)]


@pytest.mark.parametrize("name,f32", SEED_CASES, ids=[f"{k}-{'f32' if f else 'fp64'}" for k, f in SEED_CASES])
def test_seeds_on_one_tile(name, f32):
    """the grid lies inside one tile: one workgroup's Jacobi passes, so the restatement's bits (float32 storage: of the rounded
    input, rounded once), the sign bit of −0.0 included, and its count of frozen nodes; both seedings where the field is a distance"""
    phi0, lc, hc, dist = SEEDS[name]
    n = phi0.shape
    h = R.meshsize(n, lc, hc)
    if f32:
        phi0 = phi0.astype(np.float32).astype(np.float64)
    assert R.ntiles(n) == 1
    for width in (None, 1.5 * float(h.max())) if dist else (None,):
        T0, frozen = R.seed(phi0, h, None, width)
        T, launches, visits = R.solve_tiles(T0, frozen, h)         # one tile: the Jacobi passes themselves, eight to a visit
        got, stats = _run(phi0, lc, hc, h, None, width, f32=f32)
        print(f"{name} width {width}: stats {stats}")
        _same_bits(got, np.copysign(T, phi0))
        assert np.array_equal(T, R.solve_jacobi(T0, frozen, h)[0])
        assert stats == (int(frozen.sum()), launches, visits, 0) and launches == visits
