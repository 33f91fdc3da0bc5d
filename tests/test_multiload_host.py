"""The two restatement functions of the multi-load fields (tests/_multiload_ref.py) pinned on the CPU.

  * energy_mutual(op, u, u) is Operator.energy(u) bit for bit.
  * Σ_I count_I·m_I(u, v) = 2^N·uᵀA v: every cell is seen from its 2^N corners.  Both sides are sums of the same T = 2^N·cells·R² products
    (R = 2^N·N), so they agree to T·2⁻⁵³·Σ|terms|, Σ|terms| formed with |K0|, |u|, |v|.
  * the polarisation identity e(u+v) − e(u) − e(v) = 2·m(u, v) at every node, to the same kind of bound: per node 2^N·R² products and
    the magnitudes of the four fields' terms.
  * the adjoint sensitivity.  With zero prescribed values, K u = b_f and K v = b_l, J(E) = ∏h·b_l·u has dJ/dE_C = −∏h·u_C·K0 v_C
    (mutual_cells).  Central differences in single cells at the relative steps 1e-3 and 5e-4, on 9×7 and 5×6×4 cells with a random E:
    the two step sizes leave max |FD(1e-3) − FD(5e-4)| = 1.72e-7·max|dJ/dE| (2-D) and 1.33e-7·max|dJ/dE| (3-D) against each other here;
    the bar on |analytic − FD(5e-4)| is 4× the larger, 6.9e-7·max|dJ/dE| (the truncation error of the finer step is a third of
    what the two leave against each other; the measured figure is printed)."""
import numpy as np
import pytest

import _elastic_ref as R
import _multiload_ref as M

SHAPES = [(10, 8), (6, 7, 5)]      # 9×7 and 5×6×4 cells
FD_BAR = 6.9e-7


def _operator(n, seed=3):
    rng = np.random.default_rng(seed)
    N = len(n)
    h = tuple(1.0 / (max(n) - 1) * (1.0 + 0.1 * d) for d in range(N))
    E = np.asfortranarray(0.5 + rng.random(tuple(m - 1 for m in n)))
    bits = R.face_bits(n, 0, 0, (1 << N) - 1)
    return R.Operator(E, h, R.k0(h), bits), rng


@pytest.mark.parametrize("n", SHAPES)
def test_mutual_of_u_with_itself_is_the_energy_density(n):
    op, rng = _operator(n)
    u = rng.standard_normal((op.N,) + op.n)
    a, b = M.energy_mutual(op, u, u), op.energy(u)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    e1 = M.energy_weighted(op, [u], [1.0])
    assert np.array_equal(e1.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("n", SHAPES)
def test_the_node_sums_of_the_mutual_density_give_the_bilinear_form(n):
    op, rng = _operator(n)
    N = op.N
    u, v = rng.standard_normal((N,) + op.n), rng.standard_normal((N,) + op.n)
    lhs = float(np.sum(op.count * M.energy_mutual(op, u, v)))
    rhs = float(2 ** N * (op.flat(u) @ (op.matrix() @ op.flat(v))))
    terms = 2 ** N * int(np.prod([m - 1 for m in n])) * (2 ** N * N) ** 2
    bound = terms * 2.0 ** -53 * float(np.sum(M.energy_mutual_abs(op, u, v)))
    print(f"{n}: Σ count·m = {lhs:.17g}, 2^N·uᵀAv = {rhs:.17g}, difference {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("n", SHAPES)
def test_polarisation(n):
    op, rng = _operator(n)
    N = op.N
    u, v = rng.standard_normal((N,) + op.n), rng.standard_normal((N,) + op.n)
    lhs = op.energy(u + v) - op.energy(u) - op.energy(v)
    rhs = 2.0 * M.energy_mutual(op, u, v)
    a, b = np.abs(u), np.abs(v)
    mag = (M.energy_mutual_abs(op, a + b, a + b) + M.energy_mutual_abs(op, a, a) + M.energy_mutual_abs(op, b, b) + 2.0 * M.energy_mutual_abs(op, a, b)) / op.count
    bound = 2 ** N * (2 ** N * N) ** 2 * 2.0 ** -53 * mag
    print(f"{n}: largest |e(u+v) − e(u) − e(v) − 2m| / bound = {float(np.max(np.abs(lhs - rhs) / bound)):.3e}")
    assert np.all(np.abs(lhs - rhs) <= bound)


def _objective(op, E, f, l, zero):
    o = R.Operator(E, op.h, op.K0, op.bits)
    return R.compliance(o, l, R.direct(o, f, zero))


@pytest.mark.parametrize("n", SHAPES)
def test_adjoint_sensitivity_against_central_differences(n):
    """dJ/dE_C = −∏h·u_C·K0 v_C for J = ∏h·b_l·u; the bar FD_BAR is stated in the module docstring"""
    op, rng = _operator(n)
    N = op.N
    zero = np.zeros((N,) + op.n)
    f, l = rng.standard_normal((N,) + op.n), rng.standard_normal((N,) + op.n)
    u, v = R.direct(op, f, zero), R.direct(op, l, zero)
    dJ = -float(np.prod(op.h)) * M.mutual_cells(op, u, v)
    scale = float(np.abs(dJ).max())
    cells = [tuple(int(rng.integers(0, m)) for m in op.E.shape) for _ in range(6)]
    worst_fd = worst = 0.0
    for c in cells:
        fd = []
        for rel in (1e-3, 5e-4):
            d = rel * op.E[c]
            Ep, Em = op.E.copy(), op.E.copy()
            Ep[c] += d
            Em[c] -= d
            fd.append((_objective(op, Ep, f, l, zero) - _objective(op, Em, f, l, zero)) / ((Ep[c] - Em[c])))
        worst_fd = max(worst_fd, abs(fd[0] - fd[1]) / scale)
        worst = max(worst, abs(dJ[c] - fd[1]) / scale)
    print(f"{n}: |FD(1e-3) − FD(5e-4)| ≤ {worst_fd:.3e}·max|dJ/dE|, |analytic − FD(5e-4)| ≤ {worst:.3e}·max|dJ/dE| (bar {FD_BAR:.1e})")
    assert worst <= FD_BAR
