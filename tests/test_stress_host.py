"""Stress recovery on the host: tests/_stress_ref.py states what include/lsm.h ("stress recovery") says — the patch test, rigid
motions, the uniaxial bar — and its adjoint load and sensitivity are the derivatives they claim to be (central differences, the
homogeneity identity); the API refuses what needs no device, and the library exports the entry points."""
import numpy as np
import pytest

import _elastic_ref as R
import _stress_ref as S

# (n, hc, plane, ν): the shapes of the finite-difference checks
FD_CASES = [((7, 6), (1.0, 0.7), "stress", 0.3), ((6, 5), (1.0, 0.9), "strain", 0.3), ((4, 5, 4), (1.0, 1.1, 0.8), "stress", 0.25)]


def _grid(n, hc):
    h = tuple(x / (m - 1) for x, m in zip(hc, n))
    return h, np.meshgrid(*[np.arange(m) * hd for m, hd in zip(n, h)], indexing="ij")


def _problem(n, hc, plane, nu, seed, prescribed=0.0):
    """a clamped face x = 0 (with `prescribed` as the value of component 1 there), random cell moduli, a random load"""
    N = len(n)
    h, _ = _grid(n, hc)
    rng = np.random.default_rng(seed)
    E = np.asfortranarray(0.2 + rng.random(tuple(m - 1 for m in n)))
    bits = R.face_bits(n, 0, 0, (1 << N) - 1)
    f = rng.standard_normal((N,) + n)
    u0 = np.zeros((N,) + n)
    if prescribed:
        u0[1][R.face_mask(n, 0, 0)] = prescribed * np.linspace(0.0, 1.0, int(R.face_mask(n, 0, 0).sum()))      # not a rigid motion
    return h, E, bits, f, u0, rng


@pytest.mark.parametrize("n,hc,plane", [((6, 5), (1.0, 0.5), "stress"), ((6, 5), (1.0, 0.5), "strain"), ((4, 5, 6), (1.0, 0.7, 0.9), "stress")])
def test_patch_test_a_linear_field_gives_its_gradient_and_stress(n, hc, plane):
    N = len(n)
    h, x = _grid(n, hc)
    A = np.random.default_rng(5).standard_normal((N, N))
    u = np.stack([sum(A[i, j] * x[j] for j in range(N)) for i in range(N)])
    E = np.asfortranarray(0.5 + np.random.default_rng(6).random(tuple(m - 1 for m in n)))
    st = S.Stress(R.Operator(E, h, R.k0(h, 0.3, plane)), 0.3, plane)
    tol = 64 * np.finfo(float).eps * np.abs(A).max()
    G = st.gradient(u)
    for i in range(N):
        for j in range(N):
            assert np.abs(G[i][j] - A[i, j]).max() <= tol
    lam, mu = R.material(0.3, N, plane)
    sig = st.cells(u, S.STRESS)
    for k, (i, j) in enumerate(S.voigt(N)):
        exact = E * (lam * np.trace(A) + 2 * mu * A[i, i]) if i == j else E * mu * (A[i, j] + A[j, i])
        assert np.abs(sig[k] - exact).max() <= 4 * tol
    eps = st.cells(u, S.STRAIN)
    for k, (i, j) in enumerate(S.voigt(N)):
        assert np.abs(eps[k] - (A[i, i] if i == j else A[i, j] + A[j, i])).max() <= 4 * tol


@pytest.mark.parametrize("n,hc", [((5, 4), (1.0, 0.6)), ((4, 3, 5), (1.0, 0.5, 0.8))])
def test_rigid_motions_carry_no_strain(n, hc):
    """a translation gives exact zeros: in 2-D for any value (the corner sum passes through ∓u, ∓2u only); in 3-D the sum along axis 2
    passes through ∓3u, so the zero is exact where 3u is a double (0.375) and a rounding of 3u otherwise (0.37)"""
    N = len(n)
    h, x = _grid(n, hc)
    st = S.Stress(R.Operator(np.ones(tuple(m - 1 for m in n)), h, R.k0(h)), 0.3)
    for i in range(N):
        u = np.zeros((N,) + n)
        u[i] = 0.37 if N == 2 else 0.375
        assert all(not c.any() for c in st.cells(u, S.STRAIN)) and not st.cells(u, S.VON_MISES).any()      # exact zeros
        u[i] = 0.37
        assert np.abs(st.cells(u, S.STRAIN)).max() <= 4 * np.finfo(float).eps * 0.37 * max(st.c)
    for i in range(N):
        for j in range(i + 1, N):
            u = np.zeros((N,) + n)
            u[i], u[j] = -x[j], x[i]
            assert np.abs(st.cells(u, S.STRAIN)).max() <= 64 * np.finfo(float).eps


@pytest.mark.parametrize("n,hc,plane", [((13, 9), (2.0, 1.0), "stress"), ((13, 9), (2.0, 1.0), "strain"), ((9, 6, 5), (2.0, 1.0, 0.8), "stress")])
def test_uniaxial_bar_recovers_the_traction(n, hc, plane):
    """test_elastic_host's bar under the traction t: σ_xx = t and von Mises = |t| in plane stress and in 3-D; in plane strain
    σ_zz = ν·t, so von Mises = |t|·sqrt(1 − ν + ν²)"""
    N = len(n)
    h, _ = _grid(n, hc)
    E, nu, t = 3.0, 0.3, -0.7
    bits = R.face_bits(n, 0, 0, 1)
    bits[(0,) * N] |= (1 << N) - 2
    if N == 3:
        bits[0, n[1] - 1, 0] |= 4
    tv = [0.0] * N
    tv[0] = t
    op = R.Hierarchy(np.full(tuple(m - 1 for m in n), E), h, nu, plane, bits).ops[0]
    u = R.direct(op, R.traction(n, h, 0, 1, tv), np.zeros((N,) + n))
    st = S.Stress(op, nu, plane)
    sig = st.cells(u, S.STRESS)
    assert np.abs(sig[0] - t).max() <= 1e-8 * abs(t)
    assert np.abs(sig[1:]).max() <= 1e-8 * abs(t)
    vm = abs(t) * (np.sqrt(1 - nu + nu * nu) if (N == 2 and plane == "strain") else 1.0)
    assert np.abs(st.cells(u, S.VON_MISES) - vm).max() <= 1e-8 * abs(t)
    if N == 2 and plane == "strain":
        _, sn, _ = st.unit(u)
        assert np.abs(E * sn[2] - nu * t).max() <= 1e-8 * abs(t)
    assert np.abs(st.nodes(u, S.VON_MISES) - vm).max() <= 1e-8 * abs(t)


LOAD_FD_BAR, SENS_FD_BAR = 1.7e-7, 6.5e-9


@pytest.mark.parametrize("p", [2.0, 3.5, 8.0])
@pytest.mark.parametrize("n,hc,plane,nu", FD_CASES)
def test_the_load_is_the_derivative_of_the_aggregate_in_u(n, hc, plane, nu, p):
    """central differences of J′ along a random direction v at step 1e-6 against Σ (m·f)·v, for an arbitrary u.  Measured on
    these nine cases: 2.4e-10 … 1.7e-8 relative (the largest at p = 3.5); the bar is 10× the largest."""
    N = len(n)
    h, E, bits, _, _, rng = _problem(n, hc, plane, nu, 11)
    op = R.Operator(E, h, R.k0(h, nu, plane), bits)
    st = S.Stress(op, nu, plane)
    u, v = rng.standard_normal((N,) + n), rng.standard_normal((N,) + n)
    sref = float(st.norm(u, 2.0, 1.0)[1])
    g = op.m * st.load(u, p, sref)
    eps = 1e-6
    fd = (float(st.norm(u + eps * v, p, sref)[0]) - float(st.norm(u - eps * v, p, sref)[0])) / (2 * eps)
    an = float(np.sum(g * v))
    rel = abs(fd - an) / abs(an)
    print(f"load FD {n} {plane} p={p}: {rel:.2e}")
    assert rel <= LOAD_FD_BAR


@pytest.mark.parametrize("prescribed", [0.0, 0.05])
@pytest.mark.parametrize("n,hc,plane,nu", FD_CASES)
def test_the_cell_sensitivity_is_the_derivative_in_the_moduli(n, hc, plane, nu, prescribed):
    """central differences of J′ (sref held) in the cell moduli along a random relative direction δ at step 1e-5, each state a
    direct solve, against Σ_C δ_C·(p·r^p − E_C·λᵀK0u), with and without a prescribed non-rigid displacement; p = 6.  Measured on
    these six cases: 1.5e-10 … 6.5e-10 relative; the bar is 10× the largest."""
    N, p = len(n), 6.0
    h, E, bits, f, u0, rng = _problem(n, hc, plane, nu, 12, prescribed)
    K = R.k0(h, nu, plane)

    def state(Ec):
        op = R.Operator(Ec, h, K, bits)
        return S.Stress(op, nu, plane), R.direct(op, f, u0)

    st, u = state(E)
    sref = float(st.norm(u, 2.0, 1.0)[1])
    cell = st.sens_cells(u, st.adjoint(u, p, sref), p, sref)
    delta = rng.standard_normal(E.shape)
    eps = 1e-5
    Jp, Jm = [float(s.norm(uu, p, sref)[0]) for s, uu in (state(E * (1 + eps * delta)), state(E * (1 - eps * delta)))]
    fd, an = (Jp - Jm) / (2 * eps), float(np.sum(delta * cell))
    rel = abs(fd - an) / abs(an)
    print(f"sensitivity FD {n} {plane} prescribed={prescribed}: {rel:.2e}")
    assert rel <= SENS_FD_BAR


@pytest.mark.parametrize("n,hc,plane,nu", FD_CASES)
def test_homogeneity_scaling_every_modulus_leaves_the_stress(n, hc, plane, nu):
    """with zero prescribed values Σ_I count_I·d_I = 0 (to the direct solves' rounding); a prescribed non-rigid displacement breaks it"""
    p = 8.0
    rel = {}
    for prescribed in (0.0, 0.05):
        h, E, bits, f, u0, _ = _problem(n, hc, plane, nu, 13, prescribed)
        op = R.Operator(E, h, R.k0(h, nu, plane), bits)
        st = S.Stress(op, nu, plane)
        u = R.direct(op, f, u0)
        J, smax = st.norm(u, 2.0, 1.0)
        d = st.sensitivity(u, st.adjoint(u, p, float(smax)), p, float(smax), 1.0)
        s = st.cells(u, S.VON_MISES)
        rel[prescribed] = abs(st.homogeneity(d)) / float(np.sum(op.count * st.node_mean(p * np.power(s / smax, p))))
    print(f"homogeneity {n} {plane}: {rel}")
    assert rel[0.0] <= 1e-10
    assert rel[0.05] >= 1e-4


def test_the_zero_strain_cell_has_a_finite_load():
    n, hc = (5, 4), (1.0, 0.75)
    h, _ = _grid(n, hc)
    st = S.Stress(R.Operator(np.ones((4, 3)), h, R.k0(h)), 0.3)
    u = np.random.default_rng(2).standard_normal((2,) + n)
    u[:, :2, :2] = 0.25      # cell (0, 0) is translated: zero strain
    for p in (2.0, 3.5, 64.0):
        f = st.load(u, p, float(st.norm(u, 2.0, 1.0)[1]))
        assert np.all(np.isfinite(f)) and st.cells(u, S.VON_MISES)[0, 0] == 0.0


def test_the_api_refuses_what_needs_no_device():
    import lsm_amd as lsm
    assert lsm.StressSensitivity is not None

    class Op:      # stands for an open operator: reaching the device is an error here
        ndim, levels = 2, 1

        def _handle(self):
            raise AssertionError("the refusal came after a device call")

    sol = lsm.ElasticitySolution(Op(), (None, None), None, 0, 0.0)
    for p in (1.9, 64.5, float("nan"), float("inf"), -3.0):
        with pytest.raises(ValueError, match="p must"):
            sol.stress_norm(p=p)
        with pytest.raises(ValueError, match="p must"):
            sol.stress_sensitivity(p=p)
    for sref in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="sref"):
            sol.stress_norm(sref=sref)
        with pytest.raises(ValueError, match="sref"):
            sol.stress_sensitivity(sref=sref)
    with pytest.raises(ValueError, match="rtol"):
        sol.stress_sensitivity(rtol=0.0)
    with pytest.raises(ValueError, match="no load|without a load"):
        sol.compliance()
    closed = lsm.ElasticityOperator.__new__(lsm.ElasticityOperator)
    closed._h, closed.ndim, closed.levels = None, 2, 1
    gone = lsm.ElasticitySolution(closed, (None, None), None, 0, 0.0)
    for call in (gone.strain, gone.stress, gone.von_mises, gone.stress_max, gone.stress_norm, gone.stress_sensitivity,
                 lambda: closed.with_displacement(np.zeros((2, 9, 9)))):
        with pytest.raises(ValueError, match="closed"):
            call()


def test_the_library_exports_the_stress_entry_points():
    import lsm_amd as lsm
    names = {"lsm_elastic_stress_cells", "lsm_elastic_stress", "lsm_elastic_stress_norm", "lsm_elastic_stress_load", "lsm_elastic_stress_sensitivity"}
    assert names <= set(lsm._lib.EXPORTS)
    lib = lsm._lib.lib()
    for name in names:
        assert hasattr(lib, name)
    assert (lsm._lib.STRESS_STRAIN, lsm._lib.STRESS_STRESS, lsm._lib.STRESS_VON_MISES) == (0, 1, 2)
