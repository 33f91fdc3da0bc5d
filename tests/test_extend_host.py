"""The restatement of extend_from_interface_ (tests/_extend_ref.py) pinned on the host: the nodes in key order, global Jacobi waves
and the device's tile schedule with both halo orders give the same bits on every fixture the device tests use and leave no entry
unset; a first-order distance (copysign(T_jacobi, ϕ0)) has no orphan under either seeding; the maximum principle holds exactly;
constants come back; source="interface" reproduces a tangentially linear function on a plane front; the error against x/|x| on a
circle and a sphere falls with the mesh size; the orphan and cutoff counts on a planted ϕ and on eikonal_'s plateau.  No device."""
import itertools

import numpy as np
import pytest

import _eikonal_ref as R
import _extend_ref as X

INF = float("inf")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


CASES = [(name, s, src) for name in R.FIXTURES for s, src in ((0, "nodes"), (1, "nodes"), (0, "interface"))]


@pytest.mark.parametrize("name,seeding,source", CASES, ids=[f"{n}-{('crossing', 'width')[s]}-{src}" for n, s, src in CASES])
def test_key_order_and_tile_schedules_give_the_same_bits(name, seeding, source):
    phi, n, lc, hc, h = X.distance(name, seeding)
    F = X.fields(n, lc, hc, 3)
    P = X.prepare(phi, h, F, width=X.widths(h)[seeding], source=source)
    assert P.stats["orphans"] == 0 and P.stats["filled"] == 0 and 0 < P.stats["frozen"] < phi.size
    key = X.solve_key_order(P)
    waves, passes = X.solve_waves(P)
    snap, l1, v1 = X.solve_tiles(P, snapshot=True)
    seq, l2, v2 = X.solve_tiles(P, snapshot=False)
    print(f"{name}/{seeding}/{source}: {passes} waves; tiles: {l1} launches, {v1} visits (snapshot), {l2}, {v2} (sequential)")
    for out in (key, waves, snap, seq):
        assert not any(np.isnan(w).any() for w in out)
    assert _same(key, waves) and _same(key, snap) and _same(key, seq)
    nt = R.ntiles(n)
    for l, v in ((l1, v1), (l2, v2)):
        assert 1 <= l <= v <= l * nt
    # the maximum principle, exactly; the frozen nodes keep their seeds
    for w0, w in zip(P.W, key):
        seeds = w0[P.frozen]
        assert w.min() >= seeds.min() and w.max() <= seeds.max()
        assert np.array_equal(_bits(w[P.fixed]), _bits(w0[P.fixed]))


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_a_first_order_distance_has_no_orphan(name):
    """a condition: every free node of the Jacobi fixed point holds G > its smallest neighbour, and the extension's frozen set
    contains the solve's, whichever of the two seedings either used"""
    for s_solve, s_ext in itertools.product((0, 1), repeat=2):
        phi, n, lc, hc, h = X.distance(name, s_solve)
        P = X.prepare(phi, h, X.fields(n, lc, hc, 1), width=X.widths(h)[s_ext])
        assert P.stats["orphans"] == 0, (name, s_solve, s_ext, P.stats)
        assert P.stats["frozen"] == int(X.frozen_nodes(phi, h, "rule", X.widths(h)[s_ext]).sum())


@pytest.mark.parametrize("name", ("partial_tiles", "two_circles", "tiny_h"))
@pytest.mark.parametrize("rule", ("rule", "inside", "outside", "mask"))
def test_constants_come_back(name, rule):
    phi, n, lc, hc, h = X.distance(name)
    mask = np.abs(phi) <= 2.0 * h.max() if rule == "mask" else None
    for const in (0.7, -3.25e-7, 0.0, -0.0):
        F = np.full(n, const, order="F")
        F[~X.frozen_nodes(phi, h, rule, None, mask)] = np.nan          # the input at the free nodes is never read
        (out,), stats = X.extend(phi, h, [F], rule=rule, mask=mask)
        assert np.abs(out - const).max() <= 4 * R.EPS * abs(const)
        assert stats["orphans"] == 0


PLANES = [((29, 23), 0), ((29, 23), 1), ((12, 11, 13), 0), ((12, 11, 13), 1), ((12, 11, 13), 2)]


@pytest.mark.parametrize("n,axis", PLANES, ids=[f"{len(n)}d-axis{d}" for n, d in PLANES])
def test_interface_source_on_a_plane_front(n, axis):
    N = len(n)
    lc, hc = (-1.0, -1.1, -0.9)[:N], (1.0, 1.2, 1.1)[:N]
    x0 = lc[axis] + 0.4137 * (hc[axis] - lc[axis])
    phi, h = X.plane_front(n, lc, hc, axis, x0)
    Xs = R.nodes(n, lc, hc)
    want = sum((0.3 + 0.5 * d) * Xs[d] for d in range(N) if d != axis) + 0.25
    adjacent, _ = X.crossings(phi, h)
    F = np.where(adjacent, want, np.nan)
    (out,), stats = X.extend(phi, h, [np.asfortranarray(F)], source="interface")
    err = float(np.abs(out - want).max())
    print(f"plane front {n} axis {axis}: max error {err / (R.EPS * np.abs(want).max()):.3g} eps·max|F|, stats {stats}")
    assert stats["orphans"] == 0 and stats["frozen"] == int(adjacent.sum())
    assert err <= 4 * R.EPS * float(np.abs(want).max())


def _radial_error(n, N):
    lc, hc = (-1.0,) * N, (1.0,) * N
    phi0 = R.spheres(n, lc, hc, [((0.0,) * N, 0.5)])
    h = R.meshsize(n, lc, hc)
    T0, frozen = R.seed(phi0, h)
    T, _ = R.solve_jacobi(T0, frozen, h)
    phi = np.copysign(T, phi0)
    Xs = R.nodes(n, lc, hc)
    r = np.sqrt(sum(x * x for x in Xs))
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.where(r > 0, Xs[0] / r, 0.0)
    (out,), stats = X.extend(phi, h, [np.asfortranarray(want)])
    assert stats["orphans"] == 0 and out.min() >= -1.0 and out.max() <= 1.0
    return float(np.abs(out - want)[r > 0.15].max())


@pytest.mark.parametrize("N", (2, 3))
def test_the_error_against_the_radial_field_falls_with_the_mesh_size(N):
    """seeds x/|x| on a circle and a sphere of radius 0.5 in [−1, 1]^N, crossing seed, ϕ a first-order distance; the maximum error
    over |x| > 0.15 (the characteristics meet at the centre).  Measured: DESIGN.md §7.28."""
    grids = ((33, 29), (65, 61), (129, 125)) if N == 2 else ((13, 12, 11), (25, 23, 21), (41, 38, 35))
    errs = [_radial_error(n, N) for n in grids]
    print(f"{N}-D: max error against x/|x| over |x| > 0.15 on {grids}: {errs}")
    assert errs[2] < errs[0]


def _orphans_by_hand(phi, frozen, cutoff=INF):
    g = np.abs(phi)
    n, count = phi.shape, 0
    for I in itertools.product(*[range(k) for k in n]):
        if frozen[I] or g[I] >= cutoff:
            continue
        smaller = False
        for d in range(len(n)):
            for step in (-1, 1):
                j = I[d] + step
                if 0 <= j < n[d] and g[I[:d] + (j,) + I[d + 1:]] < g[I]:
                    smaller = True
        count += not smaller
    return count


def test_planted_orphans_keep_their_values_and_are_counted():
    phi, n, lc, hc, h = X.planted_orphans()
    F = X.fields(n, lc, hc, 2)
    P = X.prepare(phi, h, F)
    assert P.stats["orphans"] == 4 == _orphans_by_hand(phi, P.frozen)
    out = X.solve_key_order(P)
    waves, _ = X.solve_waves(P)
    snap, _, _ = X.solve_tiles(P)
    assert _same(out, waves) and _same(out, snap)
    for f, w in zip(F, out):
        assert np.array_equal(_bits(w[P.orphan]), _bits(f[P.orphan])) and not np.isnan(w).any()
    # an orphan is a seed like any other: its neighbours may take its value, and a non-finite one is refused
    bad = [f.copy(order="F") for f in F]
    bad[1][tuple(np.argwhere(P.orphan)[0])] = np.nan
    with pytest.raises(X.Refused) as e:
        X.prepare(phi, h, bad)
    assert (e.value.reason, e.value.offenders) == (2, 1)


@pytest.mark.parametrize("name", ("partial_tiles", "two_circles"))
def test_the_cutoff_plateau_is_filled_or_orphaned(name):
    phi0, n, lc, hc, h = X.distance(name)
    c = 0.5 * float(np.abs(phi0).max())
    phi = np.asfortranarray(np.copysign(np.minimum(np.abs(phi0), c), phi0))         # what eikonal_(cutoff=c) leaves
    F = X.fields(n, lc, hc, 1)
    frozen = X.frozen_nodes(phi, h)
    (full,), _ = X.extend(phi0, h, F)
    (out,), stats = X.extend(phi, h, F, cutoff=c, fill=-7.5)
    plateau = ~frozen & (np.abs(phi) >= c)
    assert stats == {"frozen": int(frozen.sum()), "orphans": 0, "filled": int(plateau.sum())} and plateau.sum() > 0
    assert (out[plateau] == -7.5).all() and np.array_equal(_bits(out[~plateau]), _bits(full[~plateau]))
    # without the cutoff the inner nodes of the plateau have no smaller neighbour: orphans that keep their input
    (out2,), stats2 = X.extend(phi, h, F)
    assert stats2["filled"] == 0 and stats2["orphans"] == _orphans_by_hand(phi, frozen) > 0
    assert np.array_equal(_bits(out2[~plateau]), _bits(full[~plateau]))


def test_refusals_of_the_restatement():
    phi, n, lc, hc, h = X.distance("one_tile")
    F = X.fields(n, lc, hc, 2)
    p = phi.copy(order="F")
    p[1, 2, 3] = np.inf
    p[2, 2, 3] = np.nan
    with pytest.raises(X.Refused) as e:
        X.prepare(p, h, F)
    assert (e.value.reason, e.value.offenders) == (1, 2)
    fr = X.frozen_nodes(phi, h)
    bad = [f.copy(order="F") for f in F]
    for I in np.argwhere(fr)[:3]:
        bad[0][tuple(I)] = np.inf
    bad[1][tuple(np.argwhere(fr)[0])] = np.nan            # the same node in two fields counts once
    with pytest.raises(X.Refused) as e:
        X.prepare(phi, h, bad)
    assert (e.value.reason, e.value.offenders) == (2, 3)
    for kw in ({"rule": "mask", "mask": np.zeros(n, dtype=bool)}, {"rule": "inside"}):
        with pytest.raises(X.Refused) as e:
            X.prepare(np.abs(phi) + 1.0, h, F, **kw)
        assert e.value.reason == 3
    with pytest.raises(ValueError):
        X.prepare(phi, h, F, rule="inside", source="interface")
