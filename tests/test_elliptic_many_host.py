"""The two restatement functions of the multi-source fields (tests/_elliptic_many_ref.py) pinned on the CPU, and the Python refusals of
solve_many and its result that need no device.

  * energy_mutual(op, u, u) is Operator.energy(u) bit for bit; energy_mutual(op, u, v) and energy_mutual(op, v, u) are the same bits.
  * the polarisation identity e(u+v) − e(u) − e(v) = 2·m(u, v) at every node.  u and v are random multiples of 2⁻²⁰ below 1 in
    magnitude, so that u + v is exact and the identity is one about the arithmetic alone.  Each side is a combination of the 4·2N
    terms k̄·g_a·g_b/count (2N edges, the fields u+v, u, v and the pair).  A term is formed with at most 7 roundings (two differences,
    two quotients by h, two products, the quotient by the count), the sums over a node's edges add at most 2N and the combination 2:
    less than (9 + 2N)·2⁻⁵³·Σ|terms|.  The bar is (number of terms)·2⁻⁵³·Σ|terms| = 8N·2⁻⁵³·Σ|terms| (16 ≥ 13 in 2-D, 24 ≥ 15 in 3-D),
    Σ|terms| formed in the test by energy_mutual_abs.
  * the weighted sum against numpy's combination in the stated order (k ascending from +0), bit for bit."""
import types

import numpy as np
import pytest

import _elliptic_many_ref as M
import _elliptic_ref as R

SHAPES = [(10, 8), (6, 7, 5)]      # 9×7 and 5×6×4 cells


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _operator(n, seed=3):
    rng = np.random.default_rng(seed)
    h = tuple(1.0 / (max(n) - 1) * (1.0 + 0.1 * d) for d in range(len(n)))
    a = np.asfortranarray(0.5 + rng.random(tuple(m - 1 for m in n)))
    return R.Operator(a, h, c=0.7, fixed=R.face_mask(n, 0, 0)), rng


def _dyadic(rng, n):
    return np.asfortranarray(rng.integers(-2 ** 20, 2 ** 20, size=n).astype(np.float64) * 2.0 ** -20)


@pytest.mark.parametrize("n", SHAPES)
def test_mutual_of_u_with_itself_is_the_energy_density_and_it_is_symmetric(n):
    op, rng = _operator(n)
    u, v = rng.standard_normal(n), rng.standard_normal(n)
    assert np.array_equal(_bits(M.energy_mutual(op, u, u)), _bits(op.energy(u)))
    assert np.array_equal(_bits(M.energy_mutual(op, u, v)), _bits(M.energy_mutual(op, v, u)))
    assert np.any(M.energy_mutual(op, u, v) != op.energy(u))


@pytest.mark.parametrize("n", SHAPES)
def test_polarisation(n):
    op, rng = _operator(n)
    N = op.N
    u, v = _dyadic(rng, n), _dyadic(rng, n)
    assert np.array_equal((u + v) - v, u) and np.array_equal((u + v) - u, v)      # the sum is exact
    lhs = op.energy(u + v) - op.energy(u) - op.energy(v)
    rhs = 2.0 * M.energy_mutual(op, u, v)
    mag = M.energy_mutual_abs(op, u + v, u + v) + M.energy_mutual_abs(op, u, u) + M.energy_mutual_abs(op, v, v) + 2.0 * M.energy_mutual_abs(op, u, v)
    bound = 8 * N * 2.0 ** -53 * mag
    assert np.all(bound > 0)
    print(f"{n}: largest |e(u+v) − e(u) − e(v) − 2m| / bound = {float(np.max(np.abs(lhs - rhs) / bound)):.3e}")
    assert np.all(np.abs(lhs - rhs) <= bound)


@pytest.mark.parametrize("n", SHAPES)
def test_the_weighted_sum_is_numpys_combination_in_the_stated_order(n):
    op, rng = _operator(n)
    us = [rng.standard_normal(n) for _ in range(3)]
    es = [op.energy(u) for u in us]
    assert np.array_equal(_bits(M.energy_weighted(op, us[:1], (1.0,))), _bits(es[0]))
    assert np.array_equal(_bits(M.energy_weighted(op, us, (1.0, 1.0, 1.0))), _bits(((0.0 + 1.0 * es[0]) + 1.0 * es[1]) + 1.0 * es[2]))
    want = ((0.0 + 0.25 * es[0]) + -2.0 * es[1]) + 3.0 * es[2]
    assert np.array_equal(_bits(M.energy_weighted(op, us, (0.25, -2.0, 3.0))), _bits(want))
    assert not np.array_equal(_bits(want), _bits((3.0 * es[2] + -2.0 * es[1]) + 0.25 * es[0]))      # the order is part of the statement


# ---- the refusals that need no device
def _lsm():
    import lsm_amd
    return lsm_amd


def _closed_operator(lsm):
    """an EllipticOperator without a device, as close() leaves one: the checks of solve_many that come before the handle is touched"""
    op = object.__new__(lsm.EllipticOperator)
    op._h, op.levels, op.backend = None, 1, types.SimpleNamespace(ELLIPTIC_MAXCOLS=8)
    return op


def test_solve_many_refusals_without_a_device():
    lsm = _lsm()
    op = _closed_operator(lsm)
    f = np.zeros((9, 9))
    with pytest.raises(TypeError):
        op.solve_many(f)                      # not a sequence of sources
    with pytest.raises(TypeError):
        op.solve_many(1.0)
    with pytest.raises(ValueError, match="0 sources"):
        op.solve_many([])
    with pytest.raises(ValueError, match="9 sources"):
        op.solve_many([f] * 9)
    with pytest.raises(ValueError, match="one entry per source"):
        op.solve_many([f, f], u0=[None])
    with pytest.raises(ValueError, match="one entry per source"):
        op.solve_many([f, f], homogeneous=(False, True, False))
    with pytest.raises(TypeError):
        op.solve_many([f, f], u0=f)
    with pytest.raises(TypeError):
        op.solve_many([f, f], homogeneous=True)
    for kw in (dict(rtol=0.0), dict(rtol=float("nan")), dict(rtol=float("inf")), dict(max_iters=0)):
        with pytest.raises(ValueError, match="rtol"):
            op.solve_many([f], **kw)
    with pytest.raises(ValueError, match="closed"):
        op.solve_many([f, f])


def test_the_result_refuses_bad_weights_and_foreign_solutions_without_a_device():
    lsm = _lsm()
    op, other = _closed_operator(lsm), _closed_operator(lsm)
    cols = [lsm.EllipticSolution(op, None, None, k, 0.5 * k) for k in range(3)]
    many = lsm.EllipticMultiSolution(op, cols)
    assert len(many) == 3 and many[1] is cols[1] and list(many) == cols
    assert many.iterations == (0, 1, 2) and many.relres == (0.0, 0.5, 1.0) and many.operator is op and many.levels == 1
    for what in (many.energy_density, many.compliance):
        with pytest.raises(ValueError, match="weights for 3 columns"):
            what((1.0, 2.0))
        with pytest.raises(ValueError, match="finite"):
            what((1.0, float("inf"), 0.0))
    with pytest.raises(ValueError, match="another operator"):
        cols[0].mutual_energy_density(lsm.EllipticSolution(other, None, None, 0, 0.0))
    with pytest.raises(ValueError, match="another operator"):
        cols[0].mutual_energy_density(None)


def test_the_library_exports_the_batched_elliptic_entry_points():
    lsm = _lsm()
    names = {"lsm_elliptic_solve_many", "lsm_elliptic_energy_many", "lsm_elliptic_energy_mutual"}
    assert names <= set(lsm._lib.EXPORTS)
    lib = lsm._lib.lib()
    for name in names:
        getattr(lib, name)
    assert lsm.elliptic_solve_many is lsm.api.elliptic_solve_many
