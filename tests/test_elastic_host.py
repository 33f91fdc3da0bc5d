"""elasticity_solve without a device: the restatement (tests/_elastic_ref.py) is pinned against closed forms — K0's null space,
the patch test, the uniaxial bar in plane stress, plane strain and 3-D — and has the properties the device tests rely on: a
symmetric positive V-cycle and fewer V-cycle than Jacobi iterations on every case of tests/test_gpu_elastic.py.  The Python API
refuses what needs no device, and the library exports the entry points."""
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
