"""elasticity_modes without a device: the restatement (tests/_modes_ref.py) against dense / shift-invert eigenvalues, its iteration
counts against its own case table, the mass and the start vector against closed forms, the warning of the documentation about equal
densities, the exported symbols, and the Python API's refusals on fake fields.

The eigenvalue bar (relative error ≤ rtol) is loose by about four decades — the error is second order in the residual, the measured
largest is 5.4e-10 — and the residual bars are the sharp ones: the recursive relres ≤ rtol and the true residual, with A x in the
stated order, ≤ 2·rtol·λ·‖M x‖₂ (tests/test_gpu_elliptic.py's bar for a recursive residual)."""
import numpy as np
import pytest

import _elastic_ref as E
import _modes_ref as R

NAMES = list(R.cases())


@pytest.mark.parametrize("rtol", [1e-6, 1e-8])
@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_reaches_the_exact_eigenvalues_in_the_tables_iterations(name, rtol):
    s = R.solved(name, rtol)
    cs, op, Mn = s["case"], s["hier"].ops[0], s["mass"]
    err = float(np.max(np.abs(s["lam"] - s["exact"]) / s["exact"]))
    ortho = R.ortho_defect(op, Mn, s["X"])
    true = max(tr / (lam * mn) for tr, mn, lam in (R.true_residual(op, Mn, x, lam) + (lam,) for x, lam in zip(s["X"], s["lam"])))
    print(f"{name} rtol {rtol:g}: {s['iters']} iterations, {s['applies']} V-cycles, eigenvalue error {err:.1e}, relres {s['relres'].max():.2e}, "
          f"true residual {true:.2e}, |XᵀMX − I| {ortho:.1e}, dropped {s['dropped']}, λ {s['lam']}")
    assert s["converged"] and s["dropped"] == 0
    assert err <= rtol
    assert s["relres"].max() <= rtol and true <= 2 * rtol
    assert np.all(np.diff(s["lam"]) >= 0)
    assert s["iters"] == cs["iters"][0 if rtol == 1e-6 else 1]
    assert ortho <= 1e-13
    if rtol == 1e-6:
        assert ortho <= max(2 * cs["ortho"], 1e-15) and cs["ortho"] <= max(2 * ortho, 1e-15)       # the table's figure is this run's
    for x in s["X"]:
        assert not np.any(x[op.fixed])


def test_a_warm_start_needs_no_iteration():
    s = R.solved("33x33_m4", 1e-6)
    again = R.lobpcg(s["hier"], s["mass"], 4, s["X"], 1e-6, 10)
    assert again["iters"] == 0 and again["converged"]


def test_the_mass_of_a_uniform_field_is_the_integral_of_the_density():
    for n, h in (((9, 12), (0.1, 0.25)), ((6, 5, 7), (0.5, 0.25, 0.125))):
        N = len(n)
        op = E.Operator(np.ones(tuple(k - 1 for k in n)), h, E.k0(h))
        rho = R.density_cells(np.full(n, -1.0), h, 0.0, 2.5, 1e-6)
        assert np.all(rho == 2.5)
        Mn = R.mass(op, rho)
        cells = int(np.prod([k - 1 for k in n]))
        assert abs(Mn.sum() - 2.5 * cells) <= 1e-13 * 2.5 * cells        # ∫ρ/∏h: every cell gives 2^N nodes 2^−N of its density
        inner = Mn[(slice(1, -1),) * N]
        assert np.all(inner == 2.5) and Mn.flat[0] == 2.5 * 2.0 ** -N
        assert np.all(R.mean_density(op, rho) == 2.5)


def test_the_default_start_is_splitmix64_and_zero_on_fixed_components():
    def one(t):
        z = (t + 0x9E3779B97F4A7C15) & R.MASK64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & R.MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & R.MASK64
        z ^= z >> 31
        return 2.0 * ((z >> 11) * 2.0 ** -53) - 1.0

    assert int(R.splitmix64(np.array([0], dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF      # the generator's first output from state 0
    n = (5, 4)
    bits = E.face_bits(n, 0, 0, 1)
    op = E.Operator(np.ones((4, 3)), (0.25, 0.25), E.k0((0.25, 0.25)), bits)
    x = R.default_start(op, 3)
    assert x.shape == (3, 2) + n and np.all(np.abs(x) < 1.0)
    for k, i, i0, i1 in ((0, 0, 1, 0), (2, 1, 4, 3), (1, 0, 3, 2), (1, 1, 0, 0)):
        assert x[k, i, i0, i1] == one(k * 2 * 20 + i * 20 + i0 + 5 * i1)
    assert np.all(x[:, 0, 0, :] == 0.0) and np.all(x[:, 1, 0, :] != 0.0)


def test_equal_densities_put_spurious_void_modes_below_the_first_true_one():
    """what the documentation warns of: at 33×33 with ρ_out = ρ_in and E_out = 1e-3·E_in there is a cluster of modes living in the holes
    at 0.16 … 0.25 under the structure's first eigenvalue 0.331; with ρ_out = 1e-6 the first mode is the structure's"""
    s = R.solved("33x33_m4", 1e-6)
    cs, op = s["case"], s["hier"].ops[0]
    assert abs(s["exact"][0] - 0.3310154) < 1e-6
    heavy = R.mass(op, R.density_cells(cs["phi"], cs["h"], 0.0, 1.0, 1.0))
    lam = R.exact(op, heavy, 8)
    print("ρ_out = ρ_in:", lam, " ρ_out = 1e-6:", s["exact"])
    assert np.sum(lam < s["exact"][0]) >= 6 and 0.15 < lam[0] < 0.17 and 0.24 < lam[5] < 0.26


def test_the_sensitivity_is_the_energy_minus_the_kinetic_term():
    s = R.solved("5x5_one_level_m2", 1e-8)
    op, rho, lam = s["hier"].ops[0], s["rho"], s["lam"][0]
    u = s["X"][0] / np.sqrt(np.prod(s["case"]["h"]))
    g = R.sensitivity(op, rho, u, lam)
    assert np.array_equal(g, op.energy(u) - (lam * R.mean_density(op, rho)) * (u[0] * u[0] + u[1] * u[1]))
    # Σ over the nodes of (cells around I)·g_I·∏h/2^N = ∏h·(uᵀA u − λ uᵀM u) = 0 for an eigenpair normalised to ∏h·uᵀM u = 1
    total = float(np.sum(op.count * g)) * 2.0 ** -op.N * float(np.prod(op.h))
    assert abs(total) <= 1e-7 * lam


def test_the_library_exports_the_modes_entry_points():
    import lsm_amd as lsm
    names = {"lsm_elastic_modes_create", "lsm_elastic_modes_mass", "lsm_elastic_modes_solve", "lsm_elastic_modes_vectors", "lsm_elastic_modes_store",
             "lsm_elastic_modes_sensitivity", "lsm_elastic_modes_destroy"}
    assert names <= set(lsm._lib.EXPORTS)
    assert callable(lsm.elasticity_modes) and hasattr(lsm.ElasticityOperator, "modes") and hasattr(lsm, "ElasticityModes")


# ---- the Python API without a device

def _fake_field(lsm, n, band=False, slab=None):
    import types
    grid = lsm.CartesianGrid((0.0,) * len(n), (1.0,) * len(n), n)
    cls = lsm.api.ROCNarrowBandMeshField if band else lsm.api.ROCMeshField
    f = cls.__new__(cls)
    f.mesh = grid
    b = lsm.NeumannBC()
    f.bcs = tuple((b.to_c(), b.to_c()) for _ in n) if hasattr(b, "to_c") else None
    f.backend = types.SimpleNamespace(slab=slab)
    return f


def test_the_api_refuses_what_needs_no_device():
    import lsm_amd as lsm
    ok = _fake_field(lsm, (9, 9))
    clamp = (lsm.face_mask(ok.mesh, 0, 0), 0.0)
    for m in (0, 9, -1):
        with pytest.raises(ValueError, match="between 1 and 8"):
            lsm.elasticity_modes(ok, m, dirichlet=clamp)
    for m in (2.0, "2", True, None):
        with pytest.raises(TypeError, match="integer"):
            lsm.elasticity_modes(ok, m, dirichlet=clamp)
    for kw in (dict(rho_in=0.0), dict(rho_out=-1.0), dict(rho_in=float("nan")), dict(rho_out=float("inf")), dict(rho=-np.ones((8, 8))),
               dict(rho=np.full((8, 8), np.nan)), dict(rtol=0.0), dict(rtol=float("inf")), dict(rtol=float("nan")), dict(max_iters=0)):
        with pytest.raises(ValueError, match="elasticity_modes"):
            lsm.elasticity_modes(ok, 2, dirichlet=clamp, **kw)
    with pytest.raises(ValueError, match="give the cell densities"):
        lsm.elasticity_modes(ok, 2, dirichlet=clamp, E=np.ones((8, 8)))
    # elasticity_solve's refusals come through unchanged
    with pytest.raises(ValueError, match="no fixed"):
        lsm.elasticity_modes(ok, 2)
    with pytest.raises(ValueError, match="nu must be"):
        lsm.elasticity_modes(ok, 2, dirichlet=clamp, nu=0.5)
    with pytest.raises(ValueError, match="NarrowBand"):
        lsm.elasticity_modes(_fake_field(lsm, (9, 9), band=True), 2, dirichlet=clamp)
    with pytest.raises(ValueError, match="slab"):
        lsm.elasticity_modes(_fake_field(lsm, (9, 9), slab=(0, 4)), 2, dirichlet=clamp)
    with pytest.raises(TypeError):
        lsm.elasticity_modes(lsm.MeshField(np.zeros((9, 9)), ok.mesh), 2, dirichlet=clamp)


def test_a_modes_object_refuses_a_closed_operator_and_too_many_modes():
    import types
    import lsm_amd as lsm
    op = lsm.ElasticityOperator.__new__(lsm.ElasticityOperator)
    op._h, op._phi, op._level, op.free_dofs, op.ndim = None, object(), 0.0, 5, 2
    op.backend, op.mesh = types.SimpleNamespace(), lsm.CartesianGrid((0.0, 0.0), (1.0, 1.0), (3, 3))
    with pytest.raises(ValueError, match="exceeds the 5 free components"):
        lsm.ElasticityModes(op, 2)
    md = lsm.ElasticityModes.__new__(lsm.ElasticityModes)
    md._h, md.operator, md.m = object(), op, 1
    for use in (md.vectors, md.mass, lambda: md.mode(0), lambda: md.sensitivity(0), md.solve):
        with pytest.raises(ValueError, match="ElasticityOperator is closed"):
            use()
    md._h = None
    with pytest.raises(ValueError, match="ElasticityModes object is closed"):
        md.mass()
