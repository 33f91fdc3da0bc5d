"""elliptic_modes on the device (csrc/lsm_elliptic.hip and csrc/lobpcg.h through the Python API) against the restatement
(tests/_emodes_ref.py).

Bit for bit: the block apply against Operator.apply_free (per column, and a block call's column against the single-column call), the
node mass, the stored mode's single rounding, the sensitivity given the device's stored u and λ, two solves from the default start,
and elliptic_solve's u before and after a modes() call.  Against tests/test_gpu_modes.py's bars, per case of the shared table at rtol
1e-6 (three of them at 1e-8 as well):
  * relres ≤ rtol; the true residual of the device's vectors(), recomputed by Operator.apply in the stated order, is
    ≤ 2·rtol·λ_k·‖M x_k‖₂ per column;
  * |λ − exact|/exact ≤ rtol, exact the closed form where the case has one, else the dense eigenvalues;
  * max |XᵀM X − I| ≤ 100× the restatement's own figure in the case table, floored at 1e-12;
  * iterations ≤ the restatement's count in the case table + max(3, a tenth of it).
The two shapes beyond 2048 workgroups of 256 threads check the block apply, the true residual and the orthonormality only."""
import numpy as np
import pytest

import _elliptic_ref as EL
import _emodes_ref as M

pytestmark = pytest.mark.gpu

NAMES = list(M.cases())
RUNS = [(n, 1e-6) for n in NAMES] + [(n, 1e-8) for n in M.TIGHT]
BIG = [(1025, 600), (96, 96, 64)]


def _lsm():
    import lsm_amd
    return lsm_amd


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _field(lsm, cs):
    n = cs["n"]
    mf = lsm.MeshField(np.asfortranarray(cs["phi"]), lsm.CartesianGrid((0.0,) * len(n), cs["hc"], n), dtype=cs["dtype"])
    phi = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=mf, bc=lsm.NeumannBC()).current_state()
    assert tuple(phi.mesh.meshsize()) == tuple(cs["h"])
    return phi


def _operator(lsm, cs, precond=None):
    return lsm.EllipticOperator(_field(lsm, cs), a_in=cs["a_in"], a_out=cs["a_out"], a=cs["a"], c=cs["c"],
                                dirichlet=None if cs["fixed"] is None else (cs["fixed"], 0.0), precond=precond or cs["precond"])


def _modes(op, cs, **kw):
    kw.setdefault("max_iters", 600)
    return op.modes(cs["m"] if "m" not in kw else kw.pop("m"), rho_in=cs["rho_in"], rho_out=cs["rho_out"], rho=cs["rho"], **kw)


def _big_case(n):
    hc = tuple((k - 1.0) / (max(n) - 1.0) for k in n)
    h = tuple(x / (k - 1) for x, k in zip(hc, n))
    return dict(n=n, hc=hc, h=h, phi=EL.two_holes(n, h), a=None, a_in=1.0, a_out=1e-3, c=0.0, fixed=EL.face_mask(n, 0, 0), m=2, rho_in=1.0, rho_out=1e-6, rho=None,
                dtype=np.float64, precond="mg")


def _check_vectors(op, Mn, md, rtol, what):
    """the true residual per column and the orthonormality of the device's vectors(); returns max |XᵀM X − I|"""
    X = md.vectors()
    assert not np.any(X[:, op.fixed])
    for k, x in enumerate(X):
        tr, mn = M.true_residual(op, Mn, x, md.eigenvalues[k])
        print(f"{what} mode {k}: λ {md.eigenvalues[k]:.12g}, relres {md.relres[k]:.3e}, true residual {tr / (md.eigenvalues[k] * mn):.3e}")
        assert md.relres[k] <= rtol
        assert tr <= 2 * rtol * md.eigenvalues[k] * mn
    return M.ortho_defect(op, Mn, X)


def _apply_block(dev, md, cols):
    """the device's block apply of host columns (each n-shaped): (ncols,) + n"""
    b, t = dev.backend, dev.backend.torch
    n = cols[0].shape
    x = t.from_numpy(np.concatenate([c.reshape(-1, order="F") for c in cols])).to(b.device)
    y = b.emodes_apply(md._handle(), len(cols), x).cpu().numpy()
    nn = cols[0].size
    return np.stack([y[k * nn:(k + 1) * nn].reshape(n, order="F") for k in range(len(cols))])


def _check_block_apply(dev, md, op, seed):
    rng = np.random.default_rng(seed)
    cols = [np.where(op.free, rng.standard_normal(op.n) * 10.0 ** rng.integers(-3, 4), 0.0) for _ in range(8)]
    want = np.stack([op.apply_free(c) for c in cols])
    for ncols in (1, 3, 8):
        got = _apply_block(dev, md, cols[:ncols])
        assert np.array_equal(_bits(got), _bits(want[:ncols])), ncols
    # column k of a block call is the single-column call
    one = _apply_block(dev, md, cols[5:6])
    assert np.array_equal(_bits(one[0]), _bits(want[5]))
    assert np.all(_bits(want[:, op.fixed]) == 0)


@pytest.mark.parametrize("name", ["64x48_m4", "box9x11x8_dirichlet_m3", "membrane41_m4", "20x14x9_given_m2", "17c_void_c1_m4"])
def test_the_block_apply_is_the_restatements_bits_per_column(name):
    lsm = _lsm()
    b = M.base(name)
    cs = b["case"]
    dev = _operator(lsm, cs)
    md = _modes(dev, cs, m=1, rtol=1e-2)
    _check_block_apply(dev, md, b["hier"].ops[0], 5)
    md.close()
    dev.close()


@pytest.mark.parametrize("name", ["64x48_m4", "membrane41_m4", "20x14x9_given_m2", "17c_void_f32_m3", "box17x13_natural_c_m4"])
def test_the_mass_is_the_restatements_bits(name):
    lsm = _lsm()
    b = M.base(name)
    cs = b["case"]
    dev = _operator(lsm, cs)
    md = _modes(dev, cs, m=1, rtol=1e-2)
    assert np.array_equal(_bits(md.mass()), _bits(b["mass"]))
    if cs["rho"] is None and cs["rho_out"] == cs["rho_in"] == 1.0:
        assert np.array_equal(_bits(md.mass()), _bits(b["hier"].ops[0].m))        # ρ ≡ 1: the operator's node mass
    md.close()
    dev.close()


@pytest.mark.parametrize("name,rtol", RUNS)
def test_every_case_against_exact_and_the_restatements_counts(name, rtol):
    lsm = _lsm()
    b = M.base(name)
    cs = b["case"]
    dev = _operator(lsm, cs)
    md = _modes(dev, cs, rtol=rtol)
    op, Mn = b["hier"].ops[0], b["mass"]
    assert np.array_equal(_bits(dev.cells()), _bits(op.a))
    assert np.array_equal(_bits(md.mass()), _bits(Mn))
    ortho = _check_vectors(op, Mn, md, rtol, name)
    exact = M.closed_form(cs["n"], cs["h"], cs["m"], cs["closed"] == "dirichlet", cs["c"]) if cs["closed"] else b["exact"]
    err = float(np.max(np.abs(md.eigenvalues - exact) / exact))
    itref = cs["iters"][0 if rtol == 1e-6 else 1]
    print(f"{name} rtol {rtol:g}: {md.iterations} iterations (restatement {itref}), eigenvalue error {err:.2e}, |XᵀMX − I| {ortho:.2e} "
          f"(restatement {cs['ortho']:.1e}), stats {md.stats}")
    assert err <= rtol
    assert np.allclose(md.frequencies, np.sqrt(md.eigenvalues) / (2 * np.pi), rtol=1e-15)
    assert ortho <= max(100 * cs["ortho"], 1e-12)
    assert md.iterations <= itref + max(3, itref / 10)
    assert md.stats[0] == md.iterations and md.stats[2] == 0 and md.stats[3] == 0
    md.close()
    dev.close()


@pytest.mark.parametrize("name", ["33x33_m4", "17c_void_f32_m3", "membrane41_m4", "20x14x9_given_m2", "box17x13_natural_c_m4"])
def test_modes_and_sensitivities_are_normalised_rounded_once_and_the_restatements_bits(name):
    lsm = _lsm()
    b = M.base(name)
    cs = b["case"]
    dev = _operator(lsm, cs)
    md = _modes(dev, cs)
    op, Mn = b["hier"].ops[0], b["mass"]
    X = md.vectors()
    vol = 1.0
    for hd in cs["h"]:
        vol = vol * hd
    scale = 1.0 / np.sqrt(vol)
    nn = int(np.prod(cs["n"]))
    for k in range(cs["m"]):
        uf = md.mode(k)
        assert isinstance(uf, lsm.api.ROCMeshField)
        u = uf.values()
        assert u.dtype == cs["dtype"]
        assert np.array_equal(_bits(u), _bits((X[k] * scale).astype(cs["dtype"])))       # rounded once
        assert np.all(_bits(u[op.fixed]) == 0)                                            # exact (positive) zeros
        u64 = u.astype(np.float64)
        norm = vol * float(np.sum(Mn * u64 * u64))
        print(f"{name} mode {k}: ∏h·Σ M u² − 1 = {norm - 1:.2e}")
        # float64: 4 ulp per node of summation on top of the orthonormality; float32: the relative rounding of u, twice, whatever nn
        assert abs(norm - 1.0) <= (4 * 2.0 ** -52 * nn if cs["dtype"] == np.float64 else 4 * 2.0 ** -24)
        g = md.sensitivity(k).values()
        want = M.sensitivity(op, b["rho"], u64, md.eigenvalues[k]).astype(cs["dtype"])
        assert g.dtype == cs["dtype"] and np.array_equal(_bits(g), _bits(want))
    md.close()
    dev.close()


def test_a_warm_start_returns_at_once_and_two_cold_solves_are_bit_identical():
    lsm = _lsm()
    for name in ("33x33_m4", "17c_void_c1_m4"):
        cs = M.base(name)["case"]
        dev = _operator(lsm, cs)
        md = _modes(dev, cs)
        X, lam, it = md.vectors(), md.eigenvalues.copy(), md.iterations
        assert X.shape == (cs["m"],) + cs["n"]
        md.solve(x0=X, max_iters=600)
        assert md.iterations == 0
        assert np.allclose(md.eigenvalues, lam, rtol=1e-12, atol=0)
        md.solve(max_iters=600)
        assert md.iterations == it
        assert np.array_equal(_bits(md.eigenvalues), _bits(lam)) and np.array_equal(_bits(md.vectors()), _bits(X))
        other = _modes(dev, cs)
        assert np.array_equal(_bits(other.eigenvalues), _bits(lam)) and np.array_equal(_bits(other.vectors()), _bits(X))
        other.close()
        md.close()
        dev.close()


def test_the_default_start_is_the_restatements():
    """a solve at a huge finite rtol stops before the first iteration: X is the Rayleigh–Ritz rotation of the start, and spans it"""
    lsm = _lsm()
    b = M.base("9x12_m8")
    cs = b["case"]
    dev = _operator(lsm, cs)
    md = _modes(dev, cs, rtol=1e300)
    assert md.iterations == 0
    op = b["hier"].ops[0]
    X0 = M.default_start(op, 8).reshape(8, -1)
    X = md.vectors().reshape(8, -1)
    coef, res, rank, _ = np.linalg.lstsq(X0.T, X.T, rcond=None)
    assert rank == 8 and np.abs(X0.T @ coef - X.T).max() <= 1e-12 * np.abs(X).max()
    md.close()
    dev.close()


def test_the_jacobi_preconditioner_converges_under_the_same_residual_bars():
    lsm = _lsm()
    b = M.base("20x14_m1")
    cs = b["case"]
    dev = _operator(lsm, cs, precond="jacobi")
    md = _modes(dev, cs, m=2, max_iters=3000)
    op, Mn = b["hier"].ops[0], b["mass"]
    ortho = _check_vectors(op, Mn, md, 1e-6, "20x14 jacobi")
    want = M.exact(op, Mn, 2)
    print(f"20x14 jacobi: {md.iterations} iterations, |XᵀMX − I| {ortho:.2e}")
    assert np.max(np.abs(md.eigenvalues - want) / want) <= 1e-6 and ortho <= 1e-12
    md.close()
    dev.close()


def test_a_modes_call_leaves_the_solver_bit_identical_and_needs_its_operator():
    lsm = _lsm()
    for name in ("24x33x10_patch", "64x48_blob"):
        cs = EL.cases()[name]
        n = cs["n"]
        mf = lsm.MeshField(np.asfortranarray(cs["phi"]), lsm.CartesianGrid((0.0,) * len(n), cs["hc"], n), dtype=cs["dtype"])
        phi = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=mf, bc=lsm.NeumannBC()).current_state()
        dev = lsm.EllipticOperator(phi, a_in=cs["a_in"], a_out=cs["a_out"], c=cs["c"], dirichlet=(cs["fixed"], cs["g"]))
        before = dev.solve(cs["f"], rtol=1e-8)
        md = dev.modes(2, rtol=1e-4)
        after = dev.solve(cs["f"], rtol=1e-8)
        assert after.iterations == before.iterations and after.relres == before.relres
        assert np.array_equal(_bits(after.u.values()), _bits(before.u.values()))
        dev.close()
        for use in (md.vectors, md.mass, lambda: md.mode(0), lambda: md.sensitivity(0), md.solve):
            with pytest.raises(ValueError, match="closed"):
                use()
        md.close()
    with pytest.raises(ValueError, match="give the cell densities"):
        lsm.EllipticOperator(phi, a=1.0, dirichlet=(cs["fixed"], 0.0)).modes(2)


def test_an_overrun_returns_the_last_iterate_and_leaves_the_object_reusable():
    lsm = _lsm()
    b = M.base("33x33_m4")
    cs = b["case"]
    dev = _operator(lsm, cs)
    with pytest.raises(lsm.LsmNotConvergedError, match="lsm_elliptic_modes_solve.*no convergence within max_iters.*X is the last iterate") as e:
        _modes(dev, cs, rtol=1e-10, max_iters=2)
    err = e.value
    md = err.modes
    assert err.iterations == 2 and np.all(err.eigenvalues > 0) and np.all(np.diff(err.eigenvalues) >= 0) and err.relres.max() > 1e-10
    assert md.stats[0] == 2 and md.stats[1] == 8 and md.stats[3] >= 1
    X = md.vectors()
    assert X.shape == (4, 33, 33) and np.all(np.isfinite(X))
    ref = M.lobpcg(b["hier"], b["mass"], 4, None, 1e-10, 2)
    assert np.allclose(err.eigenvalues, ref["lam"], rtol=1e-9, atol=0)                      # the restatement's second iterate
    assert M.ortho_defect(b["hier"].ops[0], b["mass"], X) <= 1e-12
    assert np.all(np.isfinite(md.mode(0).values())) and np.all(np.isfinite(md.sensitivity(0).values()))
    md.solve(max_iters=600)
    assert md.iterations <= cs["iters"][0] + 3 and np.max(np.abs(md.eigenvalues - b["exact"]) / b["exact"]) <= 1e-6
    md.close()
    dev.close()


def test_the_c_abi_refuses_what_the_header_lists():
    lsm = _lsm()
    L = lsm._lib
    cs = M.base("5x5_jacobi_m2")["case"]
    dev = _operator(lsm, cs)
    b, t = dev.backend, dev.backend.torch
    phi = dev._phi.buf
    assert dev.free_nodes == 20

    def invalid(call):
        with pytest.raises(lsm.LsmError, match=r"\(-1\)") as e:
            call()
        assert not isinstance(e.value, lsm.LsmNotConvergedError)

    for m in (0, 9, -3):
        invalid(lambda: b.emodes_create(dev._handle(), phi, 0.0, 1.0, 1e-6, None, m))
    for rin, rout in ((0.0, 1e-6), (1.0, -1.0), (float("nan"), 1e-6), (1.0, float("inf"))):
        invalid(lambda: b.emodes_create(dev._handle(), phi, 0.0, rin, rout, None, 2))
    invalid(lambda: b.emodes_create(dev._handle(), phi, float("nan"), 1.0, 1e-6, None, 2))
    invalid(lambda: b.emodes_create(dev._handle(), None, 0.0, 1.0, 1e-6, None, 2))
    bad = t.ones(16, dtype=t.float64, device=b.device)
    bad[5] = float("nan")
    invalid(lambda: b.emodes_create(dev._handle(), None, 0.0, 1.0, 1e-6, bad, 2))
    bad[5] = 0.0
    invalid(lambda: b.emodes_create(dev._handle(), None, 0.0, 1.0, 1e-6, bad, 2))
    with pytest.raises(ValueError, match="must be finite and positive"):
        dev.modes(2, rho=bad)
    # 3·m above the free nodes: 4×4 nodes fixed on two opposite faces leave 8
    n4 = (4, 4)
    small = dict(cs, n=n4, hc=(1.0, 1.0), h=(1.0 / 3, 1.0 / 3), phi=np.full(n4, -1.0), fixed=EL.face_mask(n4, 0, 0) | EL.face_mask(n4, 0, 1), precond="mg")
    tiny = _operator(lsm, small)
    assert tiny.free_nodes == 8
    invalid(lambda: tiny.backend.emodes_create(tiny._handle(), tiny._phi.buf, 0.0, 1.0, 1e-6, None, 3))
    with pytest.raises(ValueError, match="exceeds"):
        tiny.modes(3)
    two = tiny.modes(2, rtol=1e-8)
    want = M.exact(EL.Operator(np.ones((3, 3)), small["h"], 0.0, small["fixed"]), two.mass(), 2)
    assert np.max(np.abs(two.eigenvalues - want) / want) <= 1e-8
    two.close()
    tiny.close()
    md = b.emodes_create(dev._handle(), phi, 0.0, 1.0, 1e-6, None, 2)
    x = t.zeros(9 * 25, dtype=t.float64, device=b.device)
    for ncols in (0, 9, -1):
        invalid(lambda: b.emodes_apply(md, ncols, x))
    invalid(lambda: L.check(b.h, b.lib.lsm_elliptic_modes_apply(md, 1, b.ptr(x), b.ptr(x)), "lsm_elliptic_modes_apply"))
    for rtol, mx in ((0.0, 10), (-1.0, 10), (float("nan"), 10), (float("inf"), 10), (1e-6, 0)):
        invalid(lambda: b.emodes_solve(md, 2, None, rtol, mx))
    invalid(lambda: b.emodes_vectors(md, 2 * 25))                  # no solve has run
    invalid(lambda: b.emodes_store(md, 0, phi))
    x0 = t.ones(2 * 25, dtype=t.float64, device=b.device)
    x0[37] = float("inf")          # column 1, node (2, 2): free
    invalid(lambda: b.emodes_solve(md, 2, x0, 1e-6, 10))
    code, lam, rel, it, stats = b.emodes_solve(md, 2, None, 1e-10, 2)       # an overrun: λ, relres and iters are still written
    assert code == L.ERR_NOT_CONVERGED and it == 2 and stats[0] == 2 and stats[3] >= 1
    assert np.all(np.isfinite(lam)) and np.all(lam > 0) and lam[0] <= lam[1] and np.all(np.isfinite(rel)) and rel.max() > 1e-10
    assert b.emodes_vectors(md, 2 * 25).isfinite().all()              # the last iterate
    for k in (-1, 2):
        invalid(lambda: b.emodes_store(md, k, phi))
        invalid(lambda: b.emodes_sensitivity(md, k, phi))
    b.emodes_destroy(md)
    with pytest.raises(ValueError, match="x0 must be finite"):
        dev.modes(2, x0=np.full((2, 5, 5), np.nan))
    with pytest.raises(ValueError, match="x0 has shape"):
        dev.modes(2, x0=np.zeros((2, 1, 5, 5)))
    dev.close()


@pytest.mark.parametrize("n", BIG)
def test_grid_stride_shapes(n):
    """more nodes than 2048 × 256 threads: the second trip of the grid-stride loops in the block apply, the index arithmetic and the
    Gram pass's capped grid"""
    lsm = _lsm()
    assert int(np.prod(n)) > 2048 * 256
    cs = _big_case(n)
    dev = _operator(lsm, cs)
    md = _modes(dev, cs, rtol=1e-6, max_iters=1000)
    op = EL.Operator(EL.cell_coefficients(cs["phi"], cs["h"], 0.0, 1.0, 1e-3), cs["h"], 0.0, cs["fixed"])
    assert np.array_equal(_bits(dev.cells()), _bits(op.a))
    Mn = M.mass(op, M.density_cells(cs["phi"], cs["h"], 0.0, 1.0, 1e-6))
    assert np.array_equal(_bits(md.mass()), _bits(Mn))
    _check_block_apply(dev, md, op, 11)
    ortho = _check_vectors(op, Mn, md, 1e-6, str(n))
    print(f"{n}: {md.iterations} iterations, levels {dev.levels}, |XᵀMX − I| {ortho:.2e}, stats {md.stats}")
    assert ortho <= 1e-12 and md.eigenvalues[0] <= md.eigenvalues[1]
    md.close()
    dev.close()
