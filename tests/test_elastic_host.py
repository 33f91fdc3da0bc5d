"""elasticity_solve without a device: the restatement (tests/_elastic_ref.py) is pinned against closed forms — K0's null space,
the patch test, the uniaxial bar in plane stress, plane strain and 3-D — and has the properties the device tests rely on: a
symmetric positive V-cycle and fewer V-cycle than Jacobi iterations on every case of tests/test_gpu_elastic.py and
tests/test_gpu_elastic_edges.py, a per-level damping whose power iteration agrees with eigvalsh, and a first iterate that shows the
preconditioner.  The Python API refuses what needs no device, and the library exports the entry points."""
import numpy as np
import pytest

import _elastic_ref as R


@pytest.mark.parametrize("h,plane", [((0.1, 0.1), "stress"), ((0.1, 0.1), "strain"), ((0.25, 0.07), "stress"), ((0.25, 0.07), "strain"),
                                     ((0.1, 0.1, 0.1), "stress"), ((0.3, 0.11, 0.05), "stress")])
def test_k0_is_symmetric_and_annihilates_the_rigid_modes(h, plane):
    K = R.k0(h, 0.3, plane)
    big = np.abs(K).max()
    assert np.abs(K - K.T).max() <= 1e-14 * big
    modes = R.rigid_modes(h)
    N = len(h)
    assert len(modes) == N + N * (N - 1) // 2
    for v in modes:
        assert np.abs(K @ v).max() <= 1e-14 * big * max(1.0, np.abs(v).max())
    w = np.linalg.eigvalsh(K)
    assert w.min() >= -1e-13 * big and int((w > 1e-10 * big).sum()) == K.shape[0] - len(modes)


def _boundary(n):
    m = np.zeros(n, dtype=bool)
    for d in range(len(n)):
        m |= R.face_mask(n, d, 0) | R.face_mask(n, d, 1)
    return m


@pytest.mark.parametrize("n,hc,plane", [((9, 7), (1.0, 0.5), "stress"), ((9, 7), (1.0, 0.5), "strain"), ((6, 5, 7), (1.0, 0.7, 0.9), "stress")])
def test_patch_test_a_linear_field_is_reproduced(n, hc, plane):
    N = len(n)
    h = tuple(x / (m - 1) for x, m in zip(hc, n))
    G = np.random.default_rng(3).standard_normal((N, N))
    x = np.meshgrid(*[np.arange(m) * hd for m, hd in zip(n, h)], indexing="ij")
    exact = np.stack([sum(G[i, j] * x[j] for j in range(N)) for i in range(N)])
    bits = _boundary(n).astype(np.uint8) * np.uint8((1 << N) - 1)
    hier = R.Hierarchy(np.full(tuple(m - 1 for m in n), 2.5), h, 0.3, plane, bits)
    u0 = np.where(hier.ops[0].fixed, exact, 0.0)
    u = R.direct(hier.ops[0], np.zeros((N,) + n), u0)
    assert np.abs(u - exact).max() <= 1e-10 * np.abs(exact).max()
    up, it, rel, ok = R.pcg(hier, np.zeros((N,) + n), u0, 1e-12, 500, "mg")
    assert ok and np.abs(up - exact).max() <= 1e-9 * np.abs(exact).max()


@pytest.mark.parametrize("n,hc,plane", [((13, 9), (2.0, 1.0), "stress"), ((13, 9), (2.0, 1.0), "strain"), ((9, 6, 5), (2.0, 1.0, 0.8), "stress")])
def test_uniaxial_bar_pins_the_material_and_the_load_convention(n, hc, plane):
    """a roller on x = 0, the transverse offsets (and in 3-D the rotation about x) pinned at single nodes, traction t on x = L
    through f = 2t/h_x: u_x = t·x/E', u_⊥ = −ν'·t·x_⊥/E' with (E', ν') = (E, ν), or (E/(1−ν²), ν/(1−ν)) in plane strain"""
    N = len(n)
    h = tuple(x / (m - 1) for x, m in zip(hc, n))
    E, nu, t = 3.0, 0.3, 0.7
    bits = R.face_bits(n, 0, 0, 1)
    bits[(0,) * N] |= (1 << N) - 2
    if N == 3:
        bits[0, n[1] - 1, 0] |= 4
    tv = [0.0] * N
    tv[0] = t
    hier = R.Hierarchy(np.full(tuple(m - 1 for m in n), E), h, nu, plane, bits)
    u = R.direct(hier.ops[0], R.traction(n, h, 0, 1, tv), np.zeros((N,) + n))
    Ee, ne = (E / (1 - nu * nu), nu / (1 - nu)) if (N == 2 and plane == "strain") else (E, nu)
    x = np.meshgrid(*[np.arange(m) * hd for m, hd in zip(n, h)], indexing="ij")
    exact = np.stack([t * x[0] / Ee] + [-ne * t * x[d] / Ee for d in range(1, N)])
    assert np.abs(u - exact).max() <= 1e-8 * np.abs(exact).max()


def test_the_v_cycle_is_symmetric_and_positive_on_the_free_components():
    n = (9, 12)
    h = (1.0 / 11, 1.0 / 11)
    bits = R.face_bits(n, 0, 0, 3)
    bits[5, 7] = 2
    hier = R.Hierarchy(R.cell_coefficients(R.two_holes(n, h), h, 0.0, 1.0, 1e-3), h, 0.3, "stress", bits)
    op = hier.ops[0]
    assert hier.levels == 3
    free = np.flatnonzero(op.flat(op.free))
    M = np.zeros((free.size, free.size))
    for k, j in enumerate(free):
        e = np.zeros(op.flat(op.free).size)
        e[j] = 1.0
        M[:, k] = op.flat(hier.vcycle(op.unflat(e)))[free]
    assert np.abs(M - M.T).max() <= 1e-12 * np.abs(M).max()
    assert np.linalg.eigvalsh(0.5 * (M + M.T)).min() > 0


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_mg_needs_fewer_iterations_than_jacobi_in_the_restatement(name):
    """what tests/test_gpu_elastic.py relies on, established on the CPU"""
    s = R.solved(name)
    op = s["hier"].ops[0]
    line = [name, "levels", s["hier"].levels]
    for pc in ("mg", "jacobi"):
        u, it, rel, ok = s[pc]
        assert ok, (name, pc, it, rel)
        tr, bn = R.true_residual(op, s["f"], R.pcg(s["hier"], s["f"], s["u0"], 1e-8, 3000, pc)[0])
        if bn == 0.0:
            bn = R.true_residual(op, s["f"], s["u0"])[0]
        line += [pc, it, "recursive %.6e true %.6e" % (rel, tr / bn), "|u − direct| %.3e" % np.abs(u - s["direct"]).max()]
        assert tr <= 2e-8 * bn
    print(*line)
    assert s["mg"][1] < s["jacobi"][1]


def test_print_the_iteration_table():
    """DESIGN.md §7.18's table from the restatement (rtol 1e-8, ν = 0.3, plane stress in 2-D, contrast 1e-3): the V-cycle with
    ω = 0.6 and ω = 0.8 and Jacobi PCG; the largest grids are left to tools/elastic_bench.py --table"""
    for n, hc in R.TABLE:
        if int(np.prod(n)) > 20000:
            continue
        hier, f, u0 = R.prototype(n, hc)
        row = [hier.levels]
        for pc, om in (("mg", 0.6), ("mg", 0.8), ("jacobi", 0.6)):
            if pc == "mg" and om == 0.8 and len(n) == 3:
                row.append("-")         # not a convergent smoother in 3-D: thousands of iterations
                continue
            u, it, rel, ok = R.pcg(hier, f, u0, 1e-8, 3000, pc, om)
            row.append(it if ok else "no convergence")
        print("x".join(map(str, n)), *row)
        assert row[1] < row[3]


# ---- what tests/test_gpu_elastic_edges.py relies on
EPS = 2.0 ** -52


def _all_names():
    return sorted(R.cases()) + R.edge_case_names()


def _hier(name):
    """the case's hierarchy; a big case's without its solves"""
    return R.any_solved(name)["hier"]


@pytest.mark.parametrize("name", _all_names())
def test_the_power_iteration_gives_the_symbol_bound_of_eigvalsh(name):
    """The device's host code bounds λmax(D⁻¹A) of a level by 500 power steps from (1, 0.9, 0.8) per corner frequency
    (symbol_lambda_power restates it operation for operation); the restatement takes the eigenvalues (symbol_lambda).  On every
    level of every case |power − eigvalsh| ≤ 1e-14·λ, so the two dampings agree to rounding, and wherever the damping falls below
    ω = 0.6 its product with λ is SAFE = 1.9.  Measured over the 143 levels (λ from 1.71 to 4.34): at most 9.3e-16·λ."""
    hier = _hier(name)
    row = [name]
    for lev, op in enumerate(hier.ops):
        lam, lam_p = R.symbol_lambda(op.K0, op.N), R.symbol_lambda_power(op.K0, op.N)
        om = hier.omega(lev)
        row.append(f"{'x'.join(map(str, op.n))}: λ {lam:.6f} (power − eigvalsh {abs(lam_p - lam) / lam:.1e}·λ) ω {om:.6f}")
        assert abs(lam_p - lam) <= 1e-14 * lam
        assert om == R.level_omega(op.K0, op.N) and om <= R.OMEGA
        assert abs(R.device_omegas([op.K0], op.N)[0] - om) <= 1e-14 * om
        if om < R.OMEGA:
            assert abs(om * lam - R.SAFE) <= 1e-14 * R.SAFE and abs(om * lam_p - R.SAFE) <= 1e-14 * R.SAFE
        else:
            assert R.OMEGA * lam <= R.SAFE
    print(*row, sep="\n  ")


def test_the_stretched_cases_have_a_damping_of_their_own_per_level():
    """the figures the device test's case list quotes"""
    want = {"5x5x5_flat_clamp": [0.444], "5x4x5_flat_rollers": [0.449], "4x6x21_clamp": [0.6, 0.483, 0.460, 0.454], "12x10x8_far_rollers": [0.6, 0.6, 0.573]}
    for name, oms in want.items():
        hier = _hier(name)
        assert [round(hier.omega(l), 3) for l in range(hier.levels)] == oms, name


@pytest.mark.parametrize("name,precond", R.FIRST_ITERATE_PAIRS)
def test_the_first_iterate_shows_the_preconditioner(name, precond):
    """From u0 = 0 with zero prescribed values a solve at rtol = 0.97 stops after exactly one iteration for every right-hand side
    whose relative residual after the restatement's first iteration is ≤ 0.95 (2 % of margin against a device-to-restatement
    difference near 1e-15); at most two right-hand sides of a case fail that, never the normal one.  Measured: no right-hand side
    of these cases fails it; the worst relative residual per case, mg: 33x33_clamp 0.469, 65x20_aniso_rollers 0.734, 17c_clamp
    0.335, 24x33x10_patch 0.862, 24x33x10_aniso_given_E 0.933, 4x4_clamp 0.551, 5x5_rollers 0.319, 4x5x4_clamp 0.242,
    5x5x5_flat_clamp 0.521, 5x4x5_flat_rollers 0.391, 6x5_clamp 0.714, 4x40_side 0.435, 4x6x21_clamp 0.786, 9x12_pin 0.684,
    24x10_far_clamp 0.757, 12x10x8_far_rollers 0.700, 12x9_nu_neg 0.780; jacobi: 9x12_pin 0.948, 12x10x8_far_rollers 0.556.
    The long-double u₁ (first_iterate_ld) and the float64 one (pcg on the assembled matrix, scipy's P) agree to
    0.5e-16 … 2.9e-15 of max|u|: that spread is the device test's yardstick, and 64 ε bounds it here — two statements of the
    V-cycle that differed in a weight, a bit or a damping would differ by 1e-3 of max|u| or more."""
    s = R.any_solved(name)
    hier = s["hier"]
    op = hier.ops[0]
    assert s["case"]["dtype"] == np.float64
    runs, left_out = R.first_iterate_runs(hier, precond)
    print(f"{name} {precond}: left out {left_out}")
    assert len(left_out) <= R.FIRST_LEFT_OUT and "normal" in [r[0] for r in runs] and len(runs) >= 3
    for fname, f, u, rel in runs:
        b = R.rhs(op, f)
        if fname != "normal":
            assert np.count_nonzero(b) == 1 and b.max() == 1.0 and op.free[np.unravel_index(np.argmax(b), b.shape)]
        uld = R.first_iterate_ld(hier, f, precond)
        assert uld.dtype == np.longdouble and np.finfo(np.longdouble).eps < EPS
        spread = float(np.abs(u - uld).max() / np.abs(uld).max())
        print(f"{name} {precond} {fname}: relative residual after iteration 1: {rel:.3f}, float64 against long double: {spread:.2e}·max|u|")
        assert rel <= R.FIRST_RELRES
        assert spread <= 64 * EPS


def test_64x48_upper_patch_fails_the_first_iterate_condition():
    """why it is not among the first-iterate cases: its patch sits on the upper face of the even axis, no coarse level has a fixed
    component, and one V-cycle leaves 1.92 of the residual for the normal right-hand side and more than 1 for three impulses"""
    runs, left_out = R.first_iterate_runs(R.solved("64x48_upper_patch")["hier"], "mg")
    print(left_out)
    assert "normal" in [n for n, _ in left_out] and len(left_out) > R.FIRST_LEFT_OUT
    assert "64x48_upper_patch" not in R.FIRST_ITERATE


_EDGE_LEVELS = {"4x4_clamp": [(4, 4)], "5x5_rollers": [(5, 5)], "4x5x4_clamp": [(4, 5, 4)], "5x5x5_flat_clamp": [(5, 5, 5)], "5x4x5_flat_rollers": [(5, 4, 5)],
                "6x5_clamp": [(6, 5), (3, 5)], "4x40_side": [(4, 40), (4, 20), (4, 10), (4, 5)], "4x6x21_clamp": [(4, 6, 21), (4, 3, 11), (4, 3, 6), (4, 3, 3)],
                "9x12_pin": [(9, 12), (5, 6), (5, 3)], "24x10_far_clamp": [(24, 10), (12, 5), (6, 5), (3, 5)], "6x6x6_far_clamp": [(6, 6, 6), (3, 3, 3)],
                "12x10x8_far_rollers": [(12, 10, 8), (6, 5, 4), (3, 5, 4)]}
_NO_COARSE_FIXED = ("24x10_far_clamp", "6x6x6_far_clamp", "12x10x8_far_rollers", "64x48_devfield")       # the last: 64x48_upper_patch's bits
_WORKGROUPS = {"300x230": (270, 540), "45x41x37": (267, 800), "600x500": (1172, 2344)}


@pytest.mark.parametrize("name", R.edge_case_names())
def test_the_edge_cases_converge_and_the_v_cycle_needs_fewer_iterations(name):
    """the restatement on the cases of tests/test_gpu_elastic_edges.py, rtol 1e-8: iterations mg / jacobi
      4x4_clamp 7/23, 5x5_rollers 8/30, 4x5x4_clamp 11/53, 5x5x5_flat_clamp 12/58, 5x4x5_flat_rollers 15/71, 6x5_clamp 13/37,
      4x40_side 12/55, 4x6x21_clamp 57/243, 9x12_pin 16/88, 24x10_far_clamp 30/151, 12x10x8_far_rollers 25/123, 12x9_nu_neg 17/82
    so mg < jacobi wherever both run (the test prints the others).  The bits of a coarse level are those of fine node 2J: the lone
    bit of 9x12_pin at (4, 11) is gone from level 1 on, and the three far cases (and 64x48_upper_patch's bits) leave no fixed component on any coarse level.  The
    launch shapes are not solved here (the device test does, on the device's K0): their workgroup counts are what is checked."""
    s = R.edge_solved(name)
    cs, hier = s["case"], s["hier"]
    op = hier.ops[0]
    if name in _EDGE_LEVELS:
        assert [o.n for o in hier.ops] == _EDGE_LEVELS[name]
    for lev, c in enumerate(hier.ops[1:], 1):
        fine = hier.ops[lev - 1]
        sl = tuple(slice(None, None, 2) if a != b else slice(None) for a, b in zip(fine.n, c.n))
        assert np.array_equal(c.bits, fine.bits[sl])
        assert c.fixed.any() == (name not in _NO_COARSE_FIXED)
    if name == "9x12_pin":
        assert [int(o.fixed[1].sum()) for o in hier.ops] == [1, 0, 0] and op.bits[4, 11] == 2
    if cs.get("big"):
        nn = int(np.prod(op.n))
        assert (-(-nn // 256), -(-op.N * nn // 256)) == _WORKGROUPS[name] and s["mg"] is None and s["jacobi"] is None
        assert 256 < -(-nn // 256) < 2048
        return
    for pc in ("mg", "jacobi"):
        if s[pc] is None:
            assert pc == "jacobi" and cs["solve"] == "mg"
            continue
        u, it, rel, ok = s[pc]
        print(f"{name} {pc}: {it} iterations, relres {rel:.3e}, |u − direct| {np.abs(u - s['direct']).max():.3e}, levels {[o.n for o in hier.ops]}")
        assert ok and it < 3000
    if s["jacobi"] is not None:
        assert s["mg"][1] < s["jacobi"][1]
    if cs.get("u0") is not None:
        assert np.count_nonzero(s["u0"][op.free]) == int(op.free.sum())


def test_the_budget_cases_need_at_least_eight_iterations():
    """test_an_exact_iteration_budget_converges_and_one_less_does_not solves with max_iters = it − 1 ≥ 1, beyond the first chunk of 4"""
    for name in ("24x33x10_patch", "64x48_upper_patch"):
        for pc in ("mg", "jacobi"):
            assert R.solved(name)[pc][1] >= 8


# ---- the Python API without a device

def _fake_field(lsm, n, band=False, slab=None, bc=None):
    import types
    grid = lsm.CartesianGrid((0.0,) * len(n), (1.0,) * len(n), n)
    cls = lsm.api.ROCNarrowBandMeshField if band else lsm.api.ROCMeshField
    f = cls.__new__(cls)
    f.mesh = grid
    b = bc or lsm.NeumannBC()
    f.bcs = tuple((b.to_c(), b.to_c()) for _ in n) if hasattr(b, "to_c") else None
    f.backend = types.SimpleNamespace(slab=slab)
    return f


def test_the_api_refuses_what_needs_no_device():
    import lsm_amd as lsm
    ok = _fake_field(lsm, (9, 9))
    clamp = (lsm.face_mask(ok.mesh, 0, 0), 0.0)
    f = (0.0, 1.0)
    for kw, exc in ((dict(nu=0.5), ValueError), (dict(nu=-1.0), ValueError), (dict(nu=float("nan")), ValueError), (dict(plane="shell"), ValueError),
                    (dict(E_in=0.0), ValueError), (dict(E_out=float("inf")), ValueError), (dict(precond="ilu"), ValueError),
                    (dict(E=-np.ones((8, 8))), ValueError), (dict(E=np.ones((9, 9))), ValueError)):
        with pytest.raises(exc):
            lsm.elasticity_solve(ok, f, dirichlet=clamp, **kw)
    with pytest.raises(ValueError, match="no fixed"):
        lsm.elasticity_solve(ok, f)
    roller = np.zeros((9, 9, 2), dtype=bool)
    roller[0, :, 0] = True
    with pytest.raises(ValueError, match="no fixed"):           # component 1 is free everywhere: a translation is in the null space
        lsm.elasticity_solve(ok, f, dirichlet=(roller, 0.0))
    with pytest.raises(ValueError, match="every"):
        lsm.elasticity_solve(ok, f, dirichlet=(np.ones((9, 9), dtype=bool), 0.0))
    with pytest.raises(TypeError):
        lsm.elasticity_solve(ok, f, dirichlet=(np.zeros((9, 9)), 0.0))
    with pytest.raises(TypeError):
        lsm.elasticity_solve(lsm.MeshField(np.zeros((9, 9)), ok.mesh), f, dirichlet=clamp)
    with pytest.raises(ValueError, match="1 dimensional"):
        lsm.elasticity_solve(_fake_field(lsm, (9,)), f, dirichlet=clamp)
    with pytest.raises(ValueError, match="NarrowBand"):
        lsm.elasticity_solve(_fake_field(lsm, (9, 9), band=True), f, dirichlet=clamp)
    with pytest.raises(ValueError, match="slab"):
        lsm.elasticity_solve(_fake_field(lsm, (9, 9), slab=(0, 4)), f, dirichlet=clamp)
    with pytest.raises(ValueError, match="at least 3"):
        lsm.elasticity_solve(_fake_field(lsm, (9, 2)), f, dirichlet=(np.zeros((9, 2), dtype=bool), 0.0))


def test_the_library_exports_the_elastic_entry_points():
    import lsm_amd as lsm
    names = {"lsm_elastic_create", "lsm_elastic_stiffness", "lsm_elastic_apply", "lsm_elastic_solve", "lsm_elastic_energy", "lsm_elastic_compliance",
             "lsm_elastic_cells", "lsm_elastic_destroy"}
    assert names <= set(lsm._lib.EXPORTS)
