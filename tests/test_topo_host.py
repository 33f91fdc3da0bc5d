"""The topological derivative and the nucleation step on the host: tests/_topo_ref.py states what include/lsm.h ("topological
derivative", "nucleation") says — the closed forms of the void's polarisation on the patch test, rigid motions, sign and ordering —
and T is the derivative it claims to be (a hole punched into a clamped plate, direct solves); the separable search is the
brute-force definition; the punch does not depend on the order of its list; the API refuses what needs no device, and the library
exports the entry points."""
import itertools
import math

import numpy as np
import pytest

import _elastic_ref as R
import _stress_ref as S
import _topo_ref as T

EPS = np.finfo(float).eps


def _grid(n, hc):
    h = tuple(x / (m - 1) for x, m in zip(hc, n))
    return h, np.meshgrid(*[np.arange(m) * hd for m, hd in zip(n, h)], indexing="ij")


def _patch(n, hc, plane, nu, A, seed=6):
    """the patch test of tests/test_stress_host.py: the linear field u = A x on random cell moduli"""
    N = len(n)
    h, x = _grid(n, hc)
    u = np.stack([sum(A[i][j] * x[j] for j in range(N)) for i in range(N)])
    E = np.asfortranarray(0.5 + np.random.default_rng(seed).random(tuple(m - 1 for m in n)))
    return S.Stress(R.Operator(E, h, R.k0(h, nu, plane)), nu, plane), u, E


def _close(got, want, scale):
    """a few dozen operations on values of size `scale`·max|A|: the patch test's 64 eps, times 4 as for its stresses"""
    assert np.abs(got - want).max() <= 256 * EPS * scale, float(np.abs(got - want).max() / (EPS * scale))


@pytest.mark.parametrize("nu", [0.3, -0.4, 0.0])
def test_closed_forms_in_plane_stress(nu):
    n, hc, s = (6, 5), (1.0, 0.5), 0.7
    # uniaxial stress t = E_C·s: the strain (s, −ν·s); 3t²/E_C — the stress concentration factor of a circular hole
    st, u, E = _patch(n, hc, "stress", nu, [[s, 0.0], [0.0, -nu * s]])
    sig = st.cells(u, S.STRESS)
    _close(sig[0], E * s, 1.0)
    _close(T.cells(st, u), 3.0 * sig[0] ** 2 / E, 4.0)
    # equibiaxial stress t: the strain (1 − ν)·s twice; 4t²/E_C
    st, u, E = _patch(n, hc, "stress", nu, [[(1 - nu) * s, 0.0], [0.0, (1 - nu) * s]])
    sig = st.cells(u, S.STRESS)
    _close(sig[1], sig[0], 1.0)
    _close(T.cells(st, u), 4.0 * sig[0] ** 2 / E, 4.0)
    # pure shear τ = E_C·μ·γ; 8τ²/E_C
    st, u, E = _patch(n, hc, "stress", nu, [[0.0, 0.9], [0.0, 0.0]])
    sig = st.cells(u, S.STRESS)
    assert not sig[0].any() and not sig[1].any()
    _close(T.cells(st, u), 8.0 * sig[2] ** 2 / E, 8.0)


@pytest.mark.parametrize("nu", [0.3, -0.4])
def test_closed_form_in_plane_strain(nu):
    """(1 − ν²)/E_C·((σ₁ + σ₂)² + 2(σ₁ − σ₂)²) in the in-plane principal stresses of a general linear field"""
    A = np.random.default_rng(5).standard_normal((2, 2))
    st, u, E = _patch((6, 5), (1.0, 0.5), "strain", nu, A)
    sxx, syy, sxy = st.cells(u, S.STRESS)
    want = (1 - nu * nu) / E * ((sxx + syy) ** 2 + 2.0 * ((sxx - syy) ** 2 + 4.0 * sxy ** 2))
    _close(T.cells(st, u), want, 64.0 * np.abs(A).max() ** 2)
    # the same form without the factor in plane stress
    st, u, E = _patch((6, 5), (1.0, 0.5), "stress", nu, A)
    sxx, syy, sxy = st.cells(u, S.STRESS)
    _close(T.cells(st, u), ((sxx + syy) ** 2 + 2.0 * ((sxx - syy) ** 2 + 4.0 * sxy ** 2)) / E, 64.0 * np.abs(A).max() ** 2)


@pytest.mark.parametrize("nu", [0.3, 0.0, -0.3])
def test_closed_forms_in_3d(nu):
    n, hc, s = (4, 5, 6), (1.0, 0.7, 0.9), 0.7
    st, u, E = _patch(n, hc, "stress", nu, [[s, 0, 0], [0, -nu * s, 0], [0, 0, -nu * s]])
    sig = st.cells(u, S.STRESS)
    _close(sig[0], E * s, 1.0)
    _close(T.cells(st, u), 3.0 * (1 - nu) * (9 + 5 * nu) / (2.0 * (7 - 5 * nu)) * sig[0] ** 2 / E, 4.0)
    # Novotny's form for a general linear field: 3(1−ν)/(2(7−5ν))·(10σ:ε − (1−5ν)/(1−2ν)·trσ·trε)
    A = np.random.default_rng(8).standard_normal((3, 3))
    st, u, E = _patch(n, hc, "stress", nu, A)
    sig, eps = st.cells(u, S.STRESS), st.cells(u, S.STRAIN)
    dot = sum(sig[k] * eps[k] for k in range(6))
    want = 3.0 * (1 - nu) / (2.0 * (7 - 5 * nu)) * (10.0 * dot - (1 - 5 * nu) / (1 - 2 * nu) * (sig[0] + sig[1] + sig[2]) * (eps[0] + eps[1] + eps[2]))
    _close(T.cells(st, u), want, 256.0 * np.abs(A).max() ** 2)


@pytest.mark.parametrize("n,hc", [((5, 4), (1.0, 0.6)), ((4, 3, 5), (1.0, 0.5, 0.8))])
def test_rigid_motions_cost_nothing(n, hc):
    """a translation by 0.375 gives exact zeros (tests/test_stress_host.py: every corner sum is exact); a linearised rotation rounding"""
    N = len(n)
    h, x = _grid(n, hc)
    st = S.Stress(R.Operator(np.ones(tuple(m - 1 for m in n)), h, R.k0(h)), 0.3)
    for i in range(N):
        u = np.zeros((N,) + n)
        u[i] = 0.375
        assert not T.cells(st, u).any() and not T.nodes(st, u).any()
    for i in range(N):
        for j in range(i + 1, N):
            u = np.zeros((N,) + n)
            u[i], u[j] = -x[j], x[i]
            assert np.abs(T.cells(st, u)).max() <= (64 * EPS) ** 2 * 64


@pytest.mark.parametrize("n,hc,plane,nu", [((7, 6), (1.0, 0.7), "stress", 0.3), ((6, 5), (1.0, 0.9), "strain", 0.3), ((6, 5), (1.0, 0.9), "stress", -0.4),
                                           ((4, 5, 4), (1.0, 1.1, 0.8), "stress", 0.25), ((4, 5, 4), (1.0, 1.1, 0.8), "stress", -0.3)])
def test_sign_and_ordering(n, hc, plane, nu):
    """T_C ≥ 0, and T_C ≥ E_C·w: a void costs at least the strain energy density it carried"""
    h, _ = _grid(n, hc)
    rng = np.random.default_rng(17)
    E = np.asfortranarray(0.2 + rng.random(tuple(m - 1 for m in n)))
    st = S.Stress(R.Operator(E, h, R.k0(h, nu, plane)), nu, plane)
    u = rng.standard_normal((len(n),) + n)
    t = T.cells(st, u)
    assert t.min() > 0.0 and np.all(t >= T.work(st, u))
    assert T.nodes(st, u).min() > 0.0


# ---- the derivative is a derivative

RADIUS = 0.08
# measured with this file's _hole_ratio (direct solves, float64): ΔJ/(T(centre)·π·r²) for a hole at (0.5, 0.5), (0.375, 0.5) and (0.5, 0.375) of
# the unit plate: 33²: 0.7333, 0.7227, 0.7365 (the staircase removes 0.754 of π·r²: over that area the ratios are 0.972, 0.958, 0.977);
# 65²: 1.0138, 0.9871, 1.0210 (0.983 of π·r²).  The band around the central hole's value is the spread over the three positions.
RATIO = {33: (0.7333, 0.7365 - 0.7227), 65: (1.0138, 1.0210 - 0.9871)}


def _hole_ratio(m, centre=(0.5, 0.5)):
    """a unit plate in plane stress, clamped at x = 0, pulled at x = 1, all material; one hole of radius RADIUS by the restated punch;
    (J_after − J_before)/(T(centre)·π·RADIUS²) and the fraction of π·RADIUS² that the cell moduli lose"""
    n, h = (m, m), (1.0 / (m - 1),) * 2
    bits, f, K = R.face_bits(n, 0, 0, 3), R.traction(n, h, 0, 1, (1.0, 0.0)), R.k0(h, 0.3, "stress")
    u0 = np.zeros((2,) + n)

    def state(phi):
        op = R.Operator(R.cell_coefficients(phi, h, 0.0, 1.0, 1e-3), h, K, bits)
        u = R.direct(op, f, u0)
        return op, u, R.compliance(op, f, u)

    phi = np.full(n, -1.0)
    op, u, J0 = state(phi)
    c = tuple(int(round(x * (m - 1))) for x in centre)
    t = T.nodes(S.Stress(op, 0.3, "stress"), u)[c]
    new, changed = T.punch(phi, [c[0] + m * c[1]], h, 0.0, RADIUS)
    op1, _, J1 = state(new)
    area = math.pi * RADIUS ** 2
    assert changed > 1 and J1 > J0 and t > 0
    return (J1 - J0) / (t * area), float(np.sum(op.E - op1.E)) / (1.0 - 1e-3) * h[0] * h[1] / area


def test_the_derivative_is_a_derivative():
    """the compliance change of the direct solve against T(centre)·(the area of the hole asked for, π·r²) at 33² (the hole 5 cells
    wide) and 65²: the finer one is closer to 1, and both lie in the band measured over three hole positions (RATIO)"""
    got = {m: _hole_ratio(m) for m in (33, 65)}
    print({m: (round(r, 4), round(a, 4)) for m, (r, a) in got.items()})
    assert abs(got[65][0] - 1.0) < abs(got[33][0] - 1.0)
    for m, (mid, margin) in RATIO.items():
        assert abs(got[m][0] - mid) <= margin, (m, got[m])


# ---- the search

def _brute(phi, t, threshold, level, clearance, w):
    """the definition, node by node over the window: O(nodes·window)"""
    n = phi.shape
    cand = T.candidates(phi, t, threshold, level, clearance)
    lin = lambda I: int(np.ravel_multi_index(I, n, order="F"))
    out = []
    for I in itertools.product(*[range(m) for m in n]):
        if not cand[I]:
            continue
        key = (float(t[I]) + 0.0, lin(I))
        best = key
        for J in itertools.product(*[range(max(0, i - wd), min(m, i + wd + 1)) for i, wd, m in zip(I, w, n)]):
            if cand[J]:
                best = min(best, (float(t[J]) + 0.0, lin(J)))
        if best == key:
            out.append(key[1])
    return np.array(sorted(out), dtype=np.int64)


def _tied_field(n, rng, levels=5):
    """few distinct values: ties everywhere, −0 and +0 among them, one NaN"""
    t = rng.integers(0, levels, size=n).astype(np.float64) - 1.0
    t[t == 0.0] = np.where(rng.random(int((t == 0.0).sum())) < 0.5, -0.0, 0.0)
    t[tuple(m // 2 for m in n)] = np.nan
    return t


@pytest.mark.parametrize("n,w", [((9, 12), (1, 1)), ((9, 12), (2, 2)), ((13, 11), (3, 1)), ((6, 5, 7), (1, 2, 1)), ((4, 4), (32, 32)), ((5, 6, 4), (2, 2, 2))])
def test_suppression_is_the_brute_force_definition(n, w):
    rng = np.random.default_rng(3)
    for t in (rng.standard_normal(n), _tied_field(n, rng), np.full(n, 0.25)):
        phi = -0.5 - rng.random(n)
        phi[(0,) * len(n)] = np.nan
        phi[(1,) * len(n)] = 0.5        # outside: never a candidate
        for threshold in (0.5, 10.0):
            idx, val = T.centres(phi, t, threshold, 0.0, 0.5, w)
            assert np.array_equal(idx, _brute(phi, t, threshold, 0.0, 0.5, w))
            assert np.array_equal(val.view(np.uint64), t.ravel(order="F")[idx].view(np.uint64))
            I = np.stack(np.unravel_index(idx, n, order="F"), axis=1)
            for a, b in itertools.combinations(range(len(idx)), 2):      # two centres: more than w_d nodes apart along some axis
                assert any(abs(int(I[a, d]) - int(I[b, d])) > w[d] for d in range(len(n)))


def test_suppression_edge_cases():
    n, rng = (9, 12), np.random.default_rng(4)
    phi, t = np.full(n, -1.0), rng.standard_normal(n)
    # a constant field: every key ties and the index decides — every other node has a smaller index in its window: node 0 alone
    for const in (np.zeros(n), np.where(rng.random(n) < 0.5, -0.0, 0.0)):
        idx, _ = T.centres(phi, const, 1.0, 0.0, 0.5, (2, 2))
        assert idx.tolist() == [0]
    # a threshold below every value, a clearance nobody meets, NaNs only: zero centres
    assert T.centres(phi, t, float(t.min()), 0.0, 0.5, (1, 1))[0].size == 0
    assert T.centres(phi, t, 10.0, 0.0, 1.5, (1, 1))[0].size == 0
    assert T.centres(phi, np.full(n, np.nan), 10.0, 0.0, 0.5, (1, 1))[0].size == 0
    assert T.centres(np.full(n, np.nan), t, 10.0, 0.0, 0.5, (1, 1))[0].size == 0
    # a window larger than the grid: the one global minimum
    idx, val = T.centres(phi, t, 10.0, 0.0, 0.5, (32, 32))
    assert idx.tolist() == [int(np.argmin(t.ravel(order="F")))] and val[0] == t.min()
    # max_holes keeps the lowest by (value, index); spacing: any two centres are more than `spacing` apart
    h = (0.1, 0.07)
    spacing = 0.25
    w = T.window(spacing, h)
    assert w == (3, 4)
    n = (33, 40)
    phi, t = np.full(n, -1.0), rng.standard_normal(n)
    idx, val = T.centres(phi, t, 10.0, 0.0, 0.5, w)
    assert idx.size > 3
    cut, cval = T.select(idx, val, 3)
    assert cval.tolist() == sorted(val.tolist())[:3] and set(cut.tolist()) <= set(idx.tolist())
    assert T.select(idx, val, 0)[0].size == 0 and T.select(idx, val)[0].size == idx.size
    X = np.stack(np.unravel_index(idx, n, order="F"), axis=1) * np.array(h)
    for a, b in itertools.combinations(range(len(idx)), 2):
        assert np.sqrt(np.sum((X[a] - X[b]) ** 2)) > spacing
    tie = np.maximum(np.floor(2.0 * t), -1.0)
    tidx, tval = T.centres(phi, tie, 10.0, 0.0, 0.5, (1, 1))
    low = np.flatnonzero(tval == tval.min())
    assert low.size > 2 and T.select(tidx, tval, 2)[0].tolist() == tidx[low[:2]].tolist()      # equal values: the smaller index first


# ---- the punch

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,h", [((9, 12), (0.1, 0.07)), ((6, 5, 7), (0.2, 0.25, 0.15))])
def test_punch_does_not_depend_on_the_order_of_the_list(n, h, dtype):
    rng = np.random.default_rng(9)
    phi = (-1.0 - rng.random(n)).astype(dtype)
    phi[(2,) * len(n)] = np.nan
    lin = lambda I: int(np.ravel_multi_index(I, n, order="F"))
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)
    disjoint = [lin((1,) * len(n)), lin(tuple(m - 2 for m in n))]
    overlapping = [lin(tuple(m // 2 for m in n)), lin(tuple(m // 2 + 1 for m in n)), lin(tuple(m // 2 for m in n))]      # a repeat as well
    for centres, radius in ((disjoint, 0.16), (overlapping, 0.31)):
        a, ca = T.punch(phi, centres, h, 0.0, radius)
        b, cb = T.punch(phi, centres[::-1], h, 0.0, radius)
        assert a.dtype == dtype and ca == cb > 0 and np.array_equal(bits(a), bits(b))
        assert np.isnan(a[(2,) * len(n)]) and ca == int((bits(a) != bits(phi)).sum())
        one_by_one = phi
        for c in centres:
            one_by_one, _ = T.punch(one_by_one, [c], h, 0.0, radius)
        assert np.array_equal(bits(one_by_one), bits(a))          # the maximum over the list is the list applied one by one
        assert np.all((a >= phi) | np.isnan(phi))


def test_punch_at_a_corner_and_below_the_mesh_size():
    n, h = (9, 12), (0.1, 0.07)
    phi = np.full(n, -1.0)
    new, changed = T.punch(phi, [0], h, 0.0, 0.25)                  # the corner node: the box is clipped to 3 × 4 nodes
    assert changed == 3 * 4 and not (new[3:, :] != -1.0).any() and not (new[:, 4:] != -1.0).any()
    assert new[0, 0] == 0.25 and new[2, 0] == 0.0 + (0.25 - math.sqrt((2 * 0.1) ** 2))
    assert (new[:3, :4] < 0).sum() == ((np.add.outer((np.arange(3) * 0.1) ** 2, (np.arange(4) * 0.07) ** 2)) > 0.25 ** 2).sum()
    c = 4 + 9 * 5
    new, changed = T.punch(phi, [c], h, 0.3, 0.05)                  # a radius below h: only the centre node can change
    assert changed == 1 and new[4, 5] == 0.3 + 0.05 and (new != -1.0).sum() == 1
    new, changed = T.punch(np.full(n, 1.0), [c], h, 0.3, 0.05)      # already above: nothing changes
    assert changed == 0
    new, changed = T.punch(phi, [], h, 0.0, 0.25)
    assert changed == 0 and np.array_equal(new, phi)


def test_nucleate_composes_the_three_steps():
    n, h = (33, 20), (0.05, 0.06)
    rng = np.random.default_rng(12)
    x = np.meshgrid(*[np.arange(m) * hd for m, hd in zip(n, h)], indexing="ij")
    phi = -np.minimum.reduce([x[0], x[1], (n[0] - 1) * h[0] - x[0], (n[1] - 1) * h[1] - x[1]])      # the box's signed distance
    t = rng.random(n)
    new, idx, val, found, changed = T.nucleate(phi, t, h, threshold=0.3, radius=0.12, max_holes=4)
    assert found >= idx.size == 4 and changed > 4 and val.tolist() == sorted(val.tolist()) and val.max() < 0.3
    I = np.stack(np.unravel_index(idx, n, order="F"), axis=1)
    assert np.all(phi[tuple(I.T)] <= -0.12) and np.all(new[tuple(I.T)] == 0.12)


# ---- the API and the exports

def test_the_api_refuses_what_needs_no_device():
    import lsm_amd as lsm

    class Op:      # stands for a closed operator
        ndim, levels = 2, 1

        def _handle(self):
            raise ValueError("the operator is closed")

    with pytest.raises(ValueError, match="closed"):
        lsm.ElasticitySolution(Op(), (None, None), None, 0, 0.0).topological_derivative()
    for fn in (lsm.nucleate_, lsm.find_nucleation_sites):
        with pytest.raises(TypeError, match="ROCMeshField"):
            fn(np.zeros((4, 4)), np.zeros((4, 4)), threshold=0.0, radius=0.1)
        with pytest.raises(TypeError):
            fn(np.zeros((4, 4)), np.zeros((4, 4)))      # threshold and radius are required keywords
        for bad in (dict(threshold=float("nan"), radius=0.1), dict(threshold=0.0, radius=0.0), dict(threshold=0.0, radius=float("inf")),
                    dict(threshold=0.0, radius=0.1, level=float("inf")), dict(threshold=0.0, radius=0.1, clearance=float("nan")),
                    dict(threshold=0.0, radius=0.1, spacing=float("inf")), dict(threshold=0.0, radius=0.1, max_holes=-1)):
            with pytest.raises(ValueError, match="finite|negative"):
                fn(None, None, **bad)
    assert lsm.Nucleation is not None


def test_the_nucleation_result_unravels_the_indices():
    import lsm_amd as lsm
    grid = lsm.CartesianGrid((0.0, 0.0), (1.0, 1.0), (5, 7))
    r = lsm.Nucleation(grid, np.array([7, 34], dtype=np.int64), np.array([0.5, 0.75]), 9, 3)
    assert r.centres.tolist() == [[2, 1], [4, 6]] and len(r) == 2 and r.found == 9 and r.changed == 3
    empty = lsm.Nucleation(grid, np.zeros(0, dtype=np.int64), np.zeros(0), 0)
    assert empty.centres.shape == (0, 2) and len(empty) == 0 and "0 of 0 centres" in repr(empty)


def test_the_library_exports_the_entry_points():
    import lsm_amd as lsm
    names = {"lsm_elastic_topo_cells", "lsm_elastic_topo", "lsm_nucleate_create", "lsm_nucleate_read", "lsm_nucleate_destroy", "lsm_nucleate_punch"}
    assert names <= set(lsm._lib.EXPORTS)
    lib = lsm._lib.lib()
    for name in names:
        assert hasattr(lib, name)
