"""elasticity_modes without a device: the restatement (tests/_modes_ref.py) against dense / shift-invert eigenvalues, its iteration
counts against its own case table, the mass and the start vector against closed forms, the warning of the documentation about equal
densities, the exported symbols, and the Python API's refusals on fake fields.

The eigenvalue bar (relative error ≤ rtol) is loose by about four decades — the error is second order in the residual, the measured
largest is 5.4e-10 — and the residual bars are the sharp ones: the recursive relres ≤ rtol and the true residual, with A x in the
stated order, ≤ 2·rtol·λ·‖M x‖₂ (tests/test_gpu_elliptic.py's bar for a recursive residual).

For tests/test_gpu_modes_edges.py: the restated Jacobi against eigh and in long double, the trace against solves cut short, the locked
start, and the conditions under which a single iterate is defined to rounding, per step case (its print-out lists the yardsticks, the
Gram gaps and every relres)."""
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


# ---- single iterations: what tests/test_gpu_modes_edges.py relies on

def test_the_restated_jacobi_solves_the_small_problems_as_eigh_does_and_in_long_double_further():
    rng = np.random.default_rng(3)
    q, m = 9, 3
    S = rng.standard_normal((q, 40))
    GM = S @ S.T
    GA = S @ np.diag(rng.random(40) + 0.5) @ S.T
    C0, th0, d0 = R.rayleigh_ritz(GA, GM, m)
    C1, th1, d1 = R.rayleigh_ritz_jacobi(GA, GM, m)
    C2, th2, d2 = R.rayleigh_ritz_jacobi(GA, GM, m, dt=R.LD)
    assert d0 == d1 == d2 == 0 and C2.dtype == R.LD
    sg = np.sign(np.sum(C0 * C1, axis=0))
    err64 = max(float(np.abs(C0 * sg - C1).max()), float(np.abs(th0 - th1).max() / th0.max()))
    # the pencil's residual GA·C − GM·C·θ and the M-orthonormality, both evaluated in long double
    GAl, GMl = GA.astype(R.LD), GM.astype(R.LD)
    res = {k: float(np.abs(GAl @ C - (GMl @ C) * th).max() / np.abs(GAl).max()) for k, (C, th) in (("eigh", (C0.astype(R.LD), th0.astype(R.LD))),
                                                                                                   ("jacobi", (C1.astype(R.LD), th1.astype(R.LD))), ("ld", (C2, th2)))}
    orth = float(np.abs(C2.T @ GMl @ C2 - np.eye(m)).max())
    print(f"eigh against jacobi {err64:.1e}; residuals {res}; long-double orthonormality {orth:.1e}")
    assert err64 <= 1e-11 and res["eigh"] <= 1e-12 and res["jacobi"] <= 1e-12
    assert res["ld"] <= 1e-16 and orth <= 1e-16             # three decades under float64's rounding: the sweeps ran in long double
    w, V = R.em_jacobi(GM)
    assert np.all(np.diff(w) >= 0) and np.abs(V.T @ GM @ V - np.diag(w)).max() <= 1e-13 * w.max()
    # two equal columns: one direction is dropped, fewer than m are left
    G2 = np.array([[2.0, 2.0], [2.0, 2.0]])
    for rr in (R.rayleigh_ritz, R.rayleigh_ritz_jacobi):
        with pytest.raises(R.NotPositive) as e:
            rr(3.0 * G2, G2, 2)
        assert e.value.args == (1,)


def test_a_trace_changes_nothing_and_its_record_k_is_the_solve_stopped_after_k_iterations():
    b = R.base("9x12_m8")
    hier, Mn = b["hier"], b["mass"]
    full = R.lobpcg(hier, Mn, 8, None, 1e-6, 600)
    traced = R.lobpcg(hier, Mn, 8, None, 1e-6, 600, trace=True)
    assert full["iters"] == traced["iters"] == R.ITERS["9x12_m8"][0] and len(traced["steps"]) == full["iters"] + 1
    assert np.array_equal(full["X"], traced["X"]) and np.array_equal(full["lam"], traced["lam"])
    for k in (0, 1, 3):
        cut, rec = R.lobpcg(hier, Mn, 8, None, 1e-6, k), traced["steps"][k]
        assert cut["iters"] == k and not cut["converged"]
        assert np.array_equal(cut["X"], rec["X"]) and np.array_equal(cut["lam"], rec["lam"]) and np.array_equal(cut["relres"], rec["relres"])
        assert cut["applies"] == rec["applies"] == 8 * k and cut["dropped"] == rec["dropped"]
    assert traced["steps"][-1]["act"] == () and traced["steps"][0]["act"] == tuple(range(8))


def test_the_locked_start_holds_exact_eigenvectors_and_perturbed_ones():
    r = R.step_ref("9x12_m4_lock02")
    op, Mn, x0 = r["hier"].ops[0], r["mass"], r["x0"]
    assert x0.shape == (4, 2, 9, 12) and not np.any(x0[:, op.fixed])
    lam = R.exact(op, Mn, 8)
    for k in range(4):
        rq = float(np.sum(x0[k] * op.apply_free(x0[k])) / np.sum(Mn[None] * x0[k] * x0[k]))
        tr, mn = R.true_residual(op, Mn, x0[k], rq)
        print(f"column {k}: Rayleigh quotient {rq:.6g} (λ_k {lam[k]:.6g}), relative residual {tr / (rq * mn):.2e}")
        if k in (0, 2):
            assert abs(rq - lam[k]) <= 1e-12 * lam[k] and tr <= 1e-11 * rq * mn
        else:
            want = (lam[k] + 0.09 * lam[4 + k] + 0.01 * lam[3 + k]) / 1.1        # the eigenvectors are M-orthonormal
            assert abs(rq - want) <= 1e-10 * want and tr >= 0.1 * rq * mn


@pytest.mark.parametrize("name", list(R.step_cases()))
def test_the_step_cases_are_well_defined(name):
    """what makes an iterate comparable to rounding: the three restatements (float64 with eigh, float64 with the device's Jacobi, long
    double) take the same decisions at every step up to the last observed one, none of them near its threshold, and differ by rounding"""
    r = R.step_ref(name)
    cs, rtol = r["case"], R.STEP_RTOL
    m, locked = cs["m"], cs["locked"] or ()
    assert len(r["steps"]) == max(cs["ks"]) + 1 and cs["ks"][0] == 0
    for k, s in enumerate(r["steps"]):
        ld = s["ld"]
        rel = ld["relres"].astype(np.float64)
        gap = ld["mu"][0] / ld["mu"][1]
        yx, yl = (s["yard_x"] / s["scale"]).astype(np.float64), (s["yard_lam"] / ld["lam"]).astype(np.float64)
        print(f"{name} k = {k}{'' if k in cs['ks'] else ' (not observed)'}: active {ld['act']}, dropped {ld['dropped']}, V-cycles {ld['applies']}, smallest/largest of the "
              f"M-Gram {gap:.1e}, relres {np.array2string(rel, precision=1)}, yardstick in max|x| {np.array2string(yx, precision=1)}, in λ {np.array2string(yl, precision=1)}")
        for v in ("eigh", "jacobi"):
            assert s[v]["act"] == ld["act"] and s[v]["dropped"] == ld["dropped"] == 0 and s[v]["applies"] == ld["applies"]
            assert min(s[v]["mu"]) >= 1e-9 * max(s[v]["mu"])
        assert gap >= 1e-9
        assert len(ld["act"]) == m - len(locked)
        assert all(rel[j] >= 10 * rtol if j in ld["act"] else rel[j] <= rtol / 10 for j in range(m))
        assert np.all(yx <= 1e-10) and np.all(yl <= 1e-10)
        assert not np.any(ld["X"][:, r["hier"].ops[0].fixed])
    acts = [s["ld"]["act"] for s in r["steps"]]
    if name.startswith("9x12_m4_lock02"):
        assert set(acts) == {(1, 3)}
    if name == "9x12_m4_lock12":
        assert set(acts) == {(0, 3)}
    if name == "6x5x7_m3_lock1":
        assert acts == [(1, 2)] + [(0, 2)] * 4
    if name == "5x5_one_level_m2_lock0":
        assert r["hier"].levels == 1 and set(acts) == {(1,)}
    if name in ("190x180_m2", "30x29x27_m2"):
        nt = len(cs["n"]) * int(np.prod(cs["n"]))
        assert 256 * 256 < nt <= 2048 * 256
        ref = E.prototype(cs["n"])[0].ops[0]
        mine = r["hier"].ops[0]
        assert np.array_equal(ref.E, mine.E) and np.array_equal(ref.bits, mine.bits) and np.array_equal(ref.K0, mine.K0)


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
