"""Thermoelastic coupling on the host: tests/_thermo_ref.py states what include/lsm.h ("thermoelastic coupling") says, and what it states
is what the header claims it to be.

Free expansion.  With uniform E, α and θ the field u_i = ε*·(x_i − lc_i), ε* = α·θ (3-D, plane stress) or (1+ν)·α·θ (plane strain), has
A·u = b_th on every node: |A·u − b_th| ≤ 64·2⁻⁵³·max|b_th|, and its thermal stress vanishes, |σ| ≤ 64·2⁻⁵³·max|g_C|.  Measured
(5×4 plane stress, 5×4 plane strain, 4×4×3 with ν = −0.2): 6.4, 6.7 and 12.0 of the 64 units for A·u − b_th, 1.9, 3.2 and 5.6 for the stress.

Clamped block.  With u = 0 the normal stresses are the bits of −(E·(ab·θ)) and the shears are zero.

Elastic sensitivity.  z_C against central differences of J′ under E_C → E_C·(1 ± ε) with direct solves, at ε = 1e-3 and ε/2, on every
third cell; prescribed non-zero displacements, a mechanical load and a random T.  The bar is the finite difference's own resolution,
max(4·|FD_ε − FD_{ε/2}|, 1e-8·max|z|).  Measured, worst cell per grid, |FD_{ε/2} − z| against its bar: 5×4 plane stress 3.1e-8 against
3.7e-7 (max|z| 0.81), 5×4 plane strain 1.2e-9 against 1.4e-8 (max|z| 0.19), 4×4×3 1.0e-8 against 1.2e-7 (max|z| 0.47): a twelfth of
the bar, as a pure ε² truncation gives.

Heat source.  Σ m_I·q_I·δT_I against the central difference of J′ along a random δT (J′ is linear in T: the difference is exact to
rounding), under the same rule with |dJ′| for max|z|.  Measured: |FD − dJ′| ≤ 4e-11·|dJ′| on the three grids.

Consistency.  With α = 0 the sensitivity pass is −lsm_elastic_energy_mutual's restatement and the stress is the isothermal one, bit for bit;
with v = u it is −energy.  The library exports the five entry points; the API refuses what needs no device."""
import numpy as np
import pytest

import _elastic_ref as R
import _multiload_ref as ML
import _stress_ref as S
import _thermo_ref as TH

GRIDS = {
    "5x4_stress": dict(n=(5, 4), hc=(1.0, 0.6), nu=0.3, plane="stress"),
    "5x4_strain": dict(n=(5, 4), hc=(1.0, 0.6), nu=0.3, plane="strain"),
    "4x4x3_nu_neg": dict(n=(4, 4, 3), hc=(1.0, 0.9, 0.5), nu=-0.2, plane="stress"),
}
U = 2.0 ** -53


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _grid(g):
    n = g["n"]
    return n, tuple(x / (m - 1) for x, m in zip(g["hc"], n)), len(n)


def _random_problem(name, alpha_cells=True):
    """random cells in [1e-2, 1], a random T, α per cell (or a scalar), a clamped face with non-zero prescribed values, random f and l"""
    g = GRIDS[name]
    n, h, N = _grid(g)
    rng = np.random.default_rng(sum(map(ord, name)))
    cn = tuple(m - 1 for m in n)
    E = np.asfortranarray(1e-2 + 0.99 * rng.random(cn))
    alpha = np.asfortranarray(0.5 + rng.random(cn)) if alpha_cells else 0.8
    th = TH.coupling(E, h, g["nu"], g["plane"], R.face_bits(n, 0, 0, (1 << N) - 1), alpha, t_ref=0.25)
    T = rng.standard_normal(n)
    f, l = rng.standard_normal((N,) + n), rng.standard_normal((N,) + n)
    u0 = np.where(th.op.fixed, 0.05 * rng.standard_normal((N,) + n), 0.0)
    return th, T, f, l, u0, rng


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_free_expansion_balances_the_thermal_load_and_carries_no_stress(name):
    g = GRIDS[name]
    n, h, N = _grid(g)
    E = np.full(tuple(m - 1 for m in n), 0.7)
    th = TH.coupling(E, h, g["nu"], g["plane"], None, 1.3e-3, t_ref=1.25)
    T = np.full(n, 3.5)
    u, eps = th.free_expansion(3.5 - 1.25)
    assert eps == 1.3e-3 * 2.25 * ((1.0 + g["nu"]) if g["plane"] == "strain" and N == 2 else 1.0)
    b = R.rhs(th.op, th.load(T))
    assert np.abs(b).max() > 0.0
    res = float(np.abs(th.op.apply(u) - b).max()) / (U * float(np.abs(b).max()))
    gmax = float(np.abs(th.op.E * th.unit(T)).max())
    sig = float(np.abs(th.stress_cells(u, T, TH.STRESS)).max()) / (U * gmax)
    print(f"{name}: |A·u − b_th| {res:.2f}, |σ| {sig:.2f} units of 2⁻⁵³·scale (the bar is 64)")
    assert res <= 64.0 and sig <= 64.0
    # the isothermal stress of the same u is not small: the thermal term is what cancels it
    assert float(np.abs(th.st.cells(u, S.STRESS)[:N]).max()) > 0.5 * gmax


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_a_clamped_block_carries_minus_the_thermal_stress(name):
    th, T, _, _, _, _ = _random_problem(name)
    N = th.N
    zero = np.zeros((N,) + th.op.n)
    s = th.stress_cells(zero, T, TH.STRESS)
    want = -(th.op.E * ((th.alpha * th.beta) * th.theta(T)))
    for k in range(N):
        assert np.array_equal(_bits(s[k]), _bits(want))
    assert not s[N:].any()
    vm = th.stress_cells(zero, T, TH.VON_MISES)
    if N == 2 and th.plane == "stress":      # (−g, −g, 0): the von Mises value is |g|
        assert np.abs(vm - np.abs(want)).max() <= 4 * U * np.abs(want).max()
    else:                                    # hydrostatic: no deviatoric part
        assert not vm.any()


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_z_is_the_derivative_of_the_objective_in_the_cell_moduli(name):
    th, T, f, l, u0, _ = _random_problem(name)
    op = th.op
    u, v = th.state(f, T, u0), th.adjoint(l)
    z = th.sens_cells(u, v, T)

    def J(E):
        t2 = th.with_cells(E)
        return t2.objective(l, t2.state(f, T, u0))

    def fd(cell, eps):
        Ep, Em = op.E.copy(order="F"), op.E.copy(order="F")
        Ep[cell] *= 1.0 + eps
        Em[cell] *= 1.0 - eps
        return (J(Ep) - J(Em)) / (2.0 * eps)

    eps = 1e-3
    zmax = float(np.abs(z).max())
    worst = (0.0, 0.0)
    cells = list(np.ndindex(*op.E.shape))[::3]
    for cell in cells:
        a, b = fd(cell, eps), fd(cell, 0.5 * eps)
        err, bar = abs(b - z[cell]), max(4.0 * abs(a - b), 1e-8 * zmax)
        if worst[1] == 0.0 or err * worst[1] > worst[0] * bar:
            worst = (err, bar)
        assert err <= bar, (cell, err, bar)
    print(f"{name}: {len(cells)} cells, worst |FD − z| {worst[0]:.2e} against {worst[1]:.2e}, max|z| {zmax:.2e}")


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_the_source_is_the_derivative_of_the_objective_in_the_temperature(name):
    th, T, f, l, u0, rng = _random_problem(name)
    op = th.op
    v = th.adjoint(l)
    dT = rng.standard_normal(op.n)
    dJ = float(np.sum(op.m * th.source(v) * dT))
    J = lambda Tx: th.objective(l, th.state(f, Tx, u0))
    fd = lambda eps: (J(T + eps * dT) - J(T - eps * dT)) / (2.0 * eps)
    a, b = fd(1e-3), fd(0.5e-3)
    err, bar = abs(b - dJ), max(4.0 * abs(a - b), 1e-8 * abs(dJ))
    print(f"{name}: dJ′ {dJ:.6e}, |FD − dJ′| {err:.2e} against {bar:.2e}")
    assert dJ != 0.0 and err <= bar
    # count_I = 2^N·m_I: m_I·q_I is the plain sum over the cells of g′_C·2^−N, the derivative of v·b_th in T_I
    assert np.array_equal(op.count, op.m * 2.0 ** th.N)


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_without_expansion_the_passes_are_the_existing_ones(name):
    th, T, f, l, u0, rng = _random_problem(name)
    op, N = th.op, th.N
    u, v = rng.standard_normal((N,) + op.n), rng.standard_normal((N,) + op.n)
    for alpha in (0.0, np.zeros(th.st.cn)):
        cold = TH.Thermo(th.st, alpha, th.t_ref, th.nu, th.plane)
        assert np.array_equal(_bits(cold.sensitivity(u, v, T)), _bits(-ML.energy_mutual(op, u, v)))
        assert np.array_equal(_bits(cold.sensitivity(u, u, T)), _bits(-op.energy(u)))
        assert np.array_equal(_bits(cold.stress_cells(u, T, TH.STRESS)), _bits(th.st.cells(u, S.STRESS)))
        assert np.array_equal(_bits(cold.stress_cells(u, T, TH.VON_MISES)), _bits(th.st.cells(u, S.VON_MISES)))
        assert np.array_equal(_bits(cold.stress_nodes(u, T, TH.STRESS)), _bits(th.st.nodes(u, S.STRESS)))
        assert not cold.load(T).any() and not cold.source(v).any()
    minus = rng.standard_normal(op.n)
    assert np.array_equal(_bits(th.sensitivity(u, v, T, minus)), _bits(th.sensitivity(u, v, T) - minus))
    with pytest.raises(ValueError):
        th.stress_cells(u, T, S.STRAIN)


def test_von_mises_feels_the_temperature_in_plane_stress_only():
    for name in sorted(GRIDS):
        th, T, f, l, u0, rng = _random_problem(name)
        u = rng.standard_normal((th.N,) + th.op.n)
        hot, cold = th.stress_cells(u, T, TH.VON_MISES), th.st.cells(u, S.VON_MISES)
        rel = float(np.abs(hot - cold).max() / np.abs(cold).max())
        if th.N == 2 and th.plane == "stress":
            assert rel > 1e-3
        else:      # t_C cancels in the three differences, up to the rounding of ŝ − t
            assert rel <= 1e-12


def test_the_library_exports_the_entry_points():
    import lsm_amd as lsm
    names = {"lsm_elastic_thermal_load", "lsm_elastic_thermal_stress_cells", "lsm_elastic_thermal_stress", "lsm_elastic_thermal_source",
             "lsm_elastic_thermal_sensitivity"}
    assert names <= set(lsm._lib.EXPORTS)
    lib = lsm._lib.lib()
    for name in names:
        assert hasattr(lib, name)
    for name in ("Thermoelastic", "ThermoelasticSolution", "ThermoelasticSensitivity", "thermoelastic_solve"):
        assert name in lsm.__all__ and hasattr(lsm, name)


def test_the_api_refuses_what_needs_no_device():
    import lsm_amd as lsm
    with pytest.raises(TypeError, match="EllipticOperator"):
        lsm.Thermoelastic(object(), object(), alpha=1e-5)
    with pytest.raises(TypeError):
        lsm.Thermoelastic(None, None)      # alpha is required
