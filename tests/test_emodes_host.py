"""elliptic_modes without a device: the restatement (tests/_emodes_ref.py: _modes_ref's LOBPCG through a one-component adapter over
_elliptic_ref) against dense eigenvalues and, on the boxes, the closed form; its iteration counts against its own case table; the
mass, the start and the sensitivity against closed forms; the warning of the documentation about equal densities; the exported
symbols and the Python API's refusals on fake fields.

The bars are tests/test_modes_host.py's: relative eigenvalue error ≤ 1e-9 against dense eigh (second order in the residual), the
recursive relres ≤ rtol, the true residual ≤ 2·rtol·λ·‖M x‖₂, no direction dropped, the table's iteration counts exactly.

For tests/test_gpu_emodes_steps.py: the conditions under which a single iterate is defined to rounding, per step case."""
import numpy as np
import pytest

import _elliptic_ref as EL
import _emodes_ref as M

NAMES = list(M.cases())
RUNS = [(n, 1e-6) for n in NAMES] + [(n, 1e-8) for n in M.TIGHT]


@pytest.mark.parametrize("name,rtol", RUNS)
def test_the_restatement_reaches_the_dense_eigenvalues_in_the_tables_iterations(name, rtol):
    s = M.solved(name, rtol)
    cs, op, Mn = s["case"], s["hier"].ops[0], s["mass"]
    err = float(np.max(np.abs(s["lam"] - s["exact"]) / s["exact"]))
    ortho = M.ortho_defect(op, Mn, s["X"])
    true = max(tr / (lam * mn) for tr, mn, lam in (M.true_residual(op, Mn, x, lam) + (lam,) for x, lam in zip(s["X"], s["lam"])))
    print(f"{name} rtol {rtol:g}: {s['iters']} iterations, {s['applies']} V-cycles, eigenvalue error {err:.1e}, relres {s['relres'].max():.2e}, "
          f"true residual {true:.2e}, |XᵀMX − I| {ortho:.1e}, dropped {s['dropped']}, λ {s['lam']}")
    assert s["converged"] and s["dropped"] == 0
    assert err <= 1e-9
    assert s["relres"].max() <= rtol and true <= 2 * rtol
    assert np.all(np.diff(s["lam"]) >= 0)
    assert s["iters"] == cs["iters"][0 if rtol == 1e-6 else 1]
    assert ortho <= 1e-13
    if rtol == 1e-6:
        assert ortho <= max(2 * cs["ortho"], 1e-15) and cs["ortho"] <= max(2 * ortho, 1e-15)       # the table's figure is this run's
    for x in s["X"]:
        assert not np.any(x[op.fixed])


def test_the_case_table_reaches_every_path():
    c = M.cases()
    assert len(c) == 12 and set(M.TIGHT) <= set(c) and len(M.TIGHT) == 3
    assert sum(v["closed"] is not None for v in c.values()) == 3
    assert any(v["fixed"] is None for v in c.values()) and any(v["dtype"] == np.float32 for v in c.values())
    assert any(v["precond"] == "jacobi" and EL.coarsen_shape(v["n"]) is None for v in c.values())          # one level
    assert any(v["a"] is not None and v["rho"] is not None and np.ndim(v["c"]) for v in c.values())
    assert any(v["m"] == 8 for v in c.values()) and any(v["m"] == 1 for v in c.values())
    assert any(n % 2 == 0 for n in c["64x48_m4"]["n"])
    mem = c["membrane41_m4"]
    assert np.array_equal(mem["fixed"], mem["phi"] >= 0) and mem["fixed"][0, 0] and not mem["fixed"][20, 20]
    lam = M.base("membrane41_m4")["exact"]
    assert abs(lam[1] - lam[2]) <= 1e-12 * lam[1] and lam[1] - lam[0] > 1.0      # an exact double pair


@pytest.mark.parametrize("name", [k for k, v in M.cases().items() if v["closed"]])
def test_the_boxes_have_the_closed_forms_eigenvalues(name):
    b = M.base(name)
    cs = b["case"]
    want = M.closed_form(cs["n"], cs["h"], cs["m"], cs["closed"] == "dirichlet", cs["c"])
    err = float(np.max(np.abs(b["exact"] - want) / want))
    print(f"{name}: dense against the closed form {err:.1e}; λ {want}")
    assert err <= 1e-12
    if cs["closed"] == "natural":
        assert abs(want[0] - cs["c"]) == 0.0 and abs(b["exact"][0] - cs["c"]) <= 1e-12 * cs["c"]       # λ₀ = c: the constant mode


def test_a_constant_c_shifts_the_spectrum_of_unit_density_by_exactly_c():
    n, h = (9, 7), (0.125, 0.125)
    a = EL.cell_coefficients(EL.two_holes(n, h), h, 0.0, 1.0, 1e-3)
    fixed = EL.face_mask(n, 0, 0)
    rho = np.ones((8, 6))
    lam = [M.exact(op, M.mass(op, rho), 5) for op in (EL.Operator(a, h, 0.0, fixed), EL.Operator(a, h, 0.7, fixed))]
    assert np.max(np.abs(lam[1] - lam[0] - 0.7)) <= 1e-11 * lam[1].max()


def test_unit_density_gives_the_operators_node_mass_bit_for_bit():
    for n, h in (((9, 12), (0.1, 0.25)), ((6, 5, 7), (0.5, 0.25, 0.125))):
        op = EL.Operator(np.ones(tuple(k - 1 for k in n)), h)
        Mn = M.mass(op, np.ones(tuple(k - 1 for k in n)))
        assert np.array_equal(Mn.view(np.uint64), np.ascontiguousarray(op.m).view(np.uint64))
        rho = M.density_cells(np.full(n, -1.0), h, 0.0, 2.5, 1e-6)
        assert np.all(rho == 2.5) and np.all(M.mean_density(op, rho) == 2.5)
        cells = int(np.prod([k - 1 for k in n]))
        assert abs(M.mass(op, rho).sum() - 2.5 * cells) <= 1e-13 * 2.5 * cells
        cnt = M.cell_count(op)
        assert cnt.flat[0] == 1 and cnt[(1,) * len(n)] == 2 ** len(n)


def test_the_default_start_is_splitmix64_of_k_nn_plus_id_and_zero_on_fixed_nodes():
    def one(t):
        z = (t + 0x9E3779B97F4A7C15) & ((1 << 64) - 1)
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & ((1 << 64) - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & ((1 << 64) - 1)
        z ^= z >> 31
        return 2.0 * ((z >> 11) * 2.0 ** -53) - 1.0

    assert int(M.splitmix64(np.array([0], dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF
    n = (5, 4)
    op = EL.Operator(np.ones((4, 3)), (0.25, 0.25), 0.0, EL.face_mask(n, 0, 0))
    x = M.default_start(op, 3)
    assert x.shape == (3,) + n and np.all(np.abs(x) < 1.0)
    for k, i0, i1 in ((0, 1, 0), (2, 4, 3), (1, 3, 2)):
        assert x[k, i0, i1] == one(k * 20 + i0 + 5 * i1)
    assert np.all(x[:, 0, :] == 0.0) and np.all(x[:, 1:, :] != 0.0)


def test_a_warm_start_needs_no_iteration():
    s = M.solved("33x33_m4", 1e-6)
    again = M.lobpcg(s["hier"], s["mass"], 4, s["X"], 1e-6, 10)
    assert again["iters"] == 0 and again["converged"]


def test_equal_densities_put_a_spurious_void_mode_below_the_first_true_one():
    """what the documentation warns of: at 33×33 with ρ_out = ρ_in and a_out = 1e-3·a_in the first "mode" lives in the holes at 0.26,
    against the domain's 2.09 with ρ_out = 1e-6"""
    s = M.solved("33x33_m4", 1e-6)
    cs, op = s["case"], s["hier"].ops[0]
    assert abs(s["exact"][0] - 2.0916) < 1e-3
    heavy = M.mass(op, M.density_cells(cs["phi"], cs["h"], 0.0, 1.0, 1.0))
    lam = M.exact(op, heavy, 4)
    print("ρ_out = ρ_in:", lam, " ρ_out = 1e-6:", s["exact"])
    assert 0.25 < lam[0] < 0.27 and np.sum(lam < s["exact"][0]) >= 2


def test_the_sensitivity_is_the_energy_minus_the_kinetic_term_and_sums_to_zero_without_c():
    s = M.solved("33x33_m4", 1e-8)
    op, rho, lam = s["hier"].ops[0], s["rho"], s["lam"][0]
    h = s["case"]["h"]
    u = s["X"][0] / np.sqrt(np.prod(h))
    g = M.sensitivity(op, rho, u, lam)
    assert np.array_equal(g, op.energy(u) - (lam * M.mean_density(op, rho)) * (u * u))
    # Σ over the nodes of (cells around I)·g_I·∏h/2^N = ∏h·(uᵀA u − λ uᵀM u) = 0 for an eigenpair with c = 0 normalised to ∏h·uᵀM u = 1
    total = float(np.sum(M.cell_count(op) * g)) * 2.0 ** -op.N * float(np.prod(h))
    print(f"the weighted sum of g: {total:.2e} (λ {lam:.6g})")
    assert abs(total) <= 1e-7 * lam


def test_the_library_exports_the_scalar_modes_entry_points():
    import lsm_amd as lsm
    names = {"lsm_elliptic_modes_create", "lsm_elliptic_modes_mass", "lsm_elliptic_modes_apply", "lsm_elliptic_modes_solve", "lsm_elliptic_modes_vectors",
             "lsm_elliptic_modes_store", "lsm_elliptic_modes_sensitivity", "lsm_elliptic_modes_destroy"}
    assert names <= set(lsm._lib.EXPORTS)
    assert callable(lsm.elliptic_modes) and hasattr(lsm.EllipticOperator, "modes") and hasattr(lsm, "EllipticModes")
    assert "rho_out" in lsm.elliptic_modes.__doc__ and "dirichlet=(ϕ.values() >= 0, 0.0)" in lsm.elliptic_modes.__doc__


# ---- single iterations: what tests/test_gpu_emodes_steps.py relies on

@pytest.mark.parametrize("name", list(M.step_cases()))
def test_the_step_cases_are_well_defined(name):
    """tests/test_modes_host.py's conditions: the three restatements (float64 with eigh, float64 with the device's Jacobi, long double)
    take the same decisions at every step, none of them near its threshold, and differ by rounding"""
    r = M.step_ref(name)
    cs, rtol = r["case"], M.STEP_RTOL
    m, locked = cs["m"], cs["locked"] or ()
    assert len(r["steps"]) == max(cs["ks"]) + 1 and cs["ks"] == (0, 1, 2)
    for k, s in enumerate(r["steps"]):
        ld = s["ld"]
        rel = ld["relres"].astype(np.float64)
        gap = ld["mu"][0] / ld["mu"][1]
        yx, yl = (s["yard_x"] / s["scale"]).astype(np.float64), (s["yard_lam"] / ld["lam"]).astype(np.float64)
        print(f"{name} k = {k}: active {ld['act']}, V-cycles {ld['applies']}, smallest/largest of the M-Gram {gap:.1e}, relres {np.array2string(rel, precision=1)}, "
              f"yardstick in max|x| {np.array2string(yx, precision=1)}, in λ {np.array2string(yl, precision=1)}")
        for v in ("eigh", "jacobi"):
            assert s[v]["act"] == ld["act"] and s[v]["dropped"] == ld["dropped"] == 0 and s[v]["applies"] == ld["applies"]
            assert min(s[v]["mu"]) >= 1e-9 * max(s[v]["mu"])
        assert gap >= 1e-9
        assert len(ld["act"]) == m - len(locked)
        assert all(rel[j] >= 10 * rtol if j in ld["act"] else rel[j] <= rtol / 10 for j in range(m))
        assert np.all(yx <= 1e-10) and np.all(yl <= 1e-10)
        assert not np.any(ld["X"][:, r["hier"].ops[0].fixed])
    acts = {s["ld"]["act"] for s in r["steps"]}
    if name == "9x12_m4_lock02":
        assert acts == {(1, 3)}
    if name == "6x5x7_m3_lock1":
        assert acts == {(0, 2)} and len(cs["n"]) == 3


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
        with pytest.raises(ValueError, match="elliptic_modes: m must be between 1 and 8"):
            lsm.elliptic_modes(ok, m, dirichlet=clamp)
    for m in (2.0, "2", True, None):
        with pytest.raises(TypeError, match="elliptic_modes: m must be an integer"):
            lsm.elliptic_modes(ok, m, dirichlet=clamp)
    for kw in (dict(rho_in=0.0), dict(rho_out=-1.0), dict(rho_in=float("nan")), dict(rho_out=float("inf")), dict(rho=-np.ones((8, 8))),
               dict(rho=np.full((8, 8), np.nan)), dict(rtol=0.0), dict(rtol=float("inf")), dict(rtol=float("nan")), dict(max_iters=0)):
        with pytest.raises(ValueError, match="elliptic_modes"):
            lsm.elliptic_modes(ok, 2, dirichlet=clamp, **kw)
    with pytest.raises(ValueError, match="cell coefficients `a`, not from ϕ: give the cell densities"):
        lsm.elliptic_modes(ok, 2, dirichlet=clamp, a=np.ones((8, 8)))
    # elliptic_solve's refusals come through unchanged
    with pytest.raises(ValueError, match="no fixed node and c = 0"):
        lsm.elliptic_modes(ok, 2)
    with pytest.raises(ValueError, match="c must be finite and not negative"):
        lsm.elliptic_modes(ok, 2, c=-1.0)
    with pytest.raises(ValueError, match="NarrowBand"):
        lsm.elliptic_modes(_fake_field(lsm, (9, 9), band=True), 2, dirichlet=clamp)
    with pytest.raises(ValueError, match="slab"):
        lsm.elliptic_modes(_fake_field(lsm, (9, 9), slab=(0, 4)), 2, dirichlet=clamp)
    with pytest.raises(TypeError):
        lsm.elliptic_modes(lsm.MeshField(np.zeros((9, 9)), ok.mesh), 2, dirichlet=clamp)
    # the elasticity messages keep their name
    with pytest.raises(ValueError, match="elasticity_modes: m must be between 1 and 8"):
        lsm.elasticity_modes(ok, 0, dirichlet=clamp)
    with pytest.raises(ValueError, match="elasticity_modes: the operator was built from cell moduli `E`"):
        lsm.elasticity_modes(ok, 2, dirichlet=clamp, E=np.ones((8, 8)))


def test_a_modes_object_refuses_a_closed_operator_and_too_many_modes():
    import types
    import lsm_amd as lsm
    op = lsm.EllipticOperator.__new__(lsm.EllipticOperator)
    op._h, op._phi, op._level, op.free_nodes = None, object(), 0.0, 5
    op.backend, op.mesh = types.SimpleNamespace(), lsm.CartesianGrid((0.0, 0.0), (1.0, 1.0), (3, 3))
    with pytest.raises(ValueError, match="exceeds the 5 free nodes"):
        lsm.EllipticModes(op, 2)
    md = lsm.EllipticModes.__new__(lsm.EllipticModes)
    md._h, md.operator, md.m = object(), op, 1
    for use in (md.vectors, md.mass, lambda: md.mode(0), lambda: md.sensitivity(0), md.solve):
        with pytest.raises(ValueError, match="EllipticOperator is closed"):
            use()
    md._h = None
    with pytest.raises(ValueError, match="EllipticModes object is closed"):
        md.mass()
