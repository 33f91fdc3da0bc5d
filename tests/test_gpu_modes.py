"""elasticity_modes on the device (csrc/lsm_elastic.hip through the Python API) against the restatement (tests/_modes_ref.py).

Bit for bit: the node mass, the stored mode's single rounding, the sensitivity given the device's stored u and λ (on the device's K0),
two solves from the default start, and elasticity_solve's u before and after a modes() call.  Against bars, per case of the shared
table at rtol 1e-6 (three of them at 1e-8 as well):
  * relres ≤ rtol; the true residual of the device's vectors(), recomputed by Operator.apply in the stated order, is
    ≤ 2·rtol·λ_k·‖M x_k‖₂ per column (tests/test_gpu_elliptic.py's bar for a recursive residual);
  * |λ − exact|/exact ≤ rtol (second order in the residual: loose by about four decades);
  * max |XᵀM X − I| ≤ 100× the restatement's own figure in the case table, floored at 1e-12;
  * iterations ≤ the restatement's count in the case table + max(3, a tenth of it): the Gram sums are ordered differently.
The two shapes beyond 2048 workgroups of 256 threads check the true residual and the orthonormality only: neither `exact` nor the
restatement's solve is affordable there."""
import numpy as np
import pytest

import _elastic_ref as E
import _modes_ref as R

pytestmark = pytest.mark.gpu

NAMES = list(R.cases())
RUNS = [(n, 1e-6) for n in NAMES] + [(n, 1e-8) for n in R.TIGHT]


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


def _mask(cs):
    return np.stack([(cs["bits"] >> i) & 1 != 0 for i in range(len(cs["n"]))], axis=-1)


def _operator(lsm, cs, precond=None):
    return lsm.ElasticityOperator(_field(lsm, cs), E_in=cs["E_in"], E_out=cs["E_out"], nu=cs["nu"], plane=cs["plane"], dirichlet=(_mask(cs), 0.0),
                                  precond=precond or cs["precond"])


def _modes(op, cs, **kw):
    kw.setdefault("max_iters", 600)
    return op.modes(cs["m"] if "m" not in kw else kw.pop("m"), rho_in=cs["rho_in"], rho_out=cs["rho_out"], rho=cs["rho"], **kw)


def _level0(dev, ref):
    """the restatement's level-0 operator on the device's K0"""
    return E.Operator(ref.E, ref.h, dev.stiffness(0), ref.bits)


def _values(u):
    return np.stack([c.values() for c in u])


def _check_vectors(op, Mn, md, rtol, what):
    """the true residual per column and the orthonormality of the device's vectors(); returns max |XᵀM X − I|"""
    X = md.vectors()
    assert not np.any(X[:, op.fixed])
    for k, x in enumerate(X):
        tr, mn = R.true_residual(op, Mn, x, md.eigenvalues[k])
        print(f"{what} mode {k}: λ {md.eigenvalues[k]:.12g}, relres {md.relres[k]:.3e}, true residual {tr / (md.eigenvalues[k] * mn):.3e}")
        assert md.relres[k] <= rtol
        assert tr <= 2 * rtol * md.eigenvalues[k] * mn
    return R.ortho_defect(op, Mn, X)


@pytest.mark.parametrize("name", ["64x48_m4", "24x33x10_m4", "24x33x10_given_rho_m2", "17c_f32_m3"])
def test_the_mass_is_the_restatements_bits(name):
    lsm = _lsm()
    b = R.base(name)
    cs = b["case"]
    dev = _operator(lsm, cs)
    md = _modes(dev, cs, m=1)
    assert np.array_equal(_bits(md.mass()), _bits(b["mass"]))
    md.close()
    dev.close()


@pytest.mark.parametrize("name,rtol", RUNS)
def test_every_case_against_exact_and_the_restatements_counts(name, rtol):
    lsm = _lsm()
    b = R.base(name)
    cs = b["case"]
    dev = _operator(lsm, cs)
    md = _modes(dev, cs, rtol=rtol)
    op, Mn = _level0(dev, b["hier"].ops[0]), b["mass"]
    assert np.array_equal(_bits(md.mass()), _bits(Mn))
    ortho = _check_vectors(op, Mn, md, rtol, name)
    err = float(np.max(np.abs(md.eigenvalues - b["exact"]) / b["exact"]))
    itref = cs["iters"][0 if rtol == 1e-6 else 1]
    print(f"{name} rtol {rtol:g}: {md.iterations} iterations (restatement {itref}), eigenvalue error {err:.2e}, |XᵀMX − I| {ortho:.2e} "
          f"(restatement {cs['ortho']:.1e}), stats {md.stats}")
    assert err <= rtol
    assert np.allclose(md.frequencies, np.sqrt(md.eigenvalues) / (2 * np.pi), rtol=1e-15)
    assert ortho <= max(100 * cs["ortho"], 1e-12)
    assert md.iterations <= itref + max(3, itref / 10)
    md.close()
    dev.close()


@pytest.mark.parametrize("name", ["33x33_m4", "17c_f32_m3", "64x48_blob_roller_m3", "24x33x10_given_rho_m2"])
def test_modes_and_sensitivities_are_normalised_rounded_once_and_the_restatements_bits(name):
    lsm = _lsm()
    b = R.base(name)
    cs = b["case"]
    dev = _operator(lsm, cs)
    md = _modes(dev, cs)
    op, Mn = _level0(dev, b["hier"].ops[0]), b["mass"]
    X = md.vectors()
    vol = 1.0
    for hd in cs["h"]:
        vol = vol * hd
    scale = 1.0 / np.sqrt(vol)
    for k in range(cs["m"]):
        u = _values(md.mode(k))
        assert u.dtype == cs["dtype"]
        assert np.array_equal(_bits(u), _bits((X[k] * scale).astype(cs["dtype"])))       # rounded once
        assert np.all(_bits(u[op.fixed]) == 0)                                            # exact (positive) zeros
        u64 = u.astype(np.float64)
        norm = vol * float(np.sum(Mn[None] * u64 * u64))
        print(f"{name} mode {k}: ∏h·Σ M|u|² − 1 = {norm - 1:.2e}")
        assert abs(norm - 1.0) <= (1e-12 if cs["dtype"] == np.float64 else 4 * 2.0 ** -24)
        g = md.sensitivity(k).values()
        want = R.sensitivity(op, b["rho"], u64, md.eigenvalues[k]).astype(cs["dtype"])
        assert g.dtype == cs["dtype"] and np.array_equal(_bits(g), _bits(want))
    md.close()
    dev.close()


def test_a_warm_start_returns_at_once_and_two_cold_solves_are_bit_identical():
    lsm = _lsm()
    for name in ("33x33_m4", "17c_m6"):
        cs = R.base(name)["case"]
        dev = _operator(lsm, cs)
        md = _modes(dev, cs)
        X, lam, it = md.vectors(), md.eigenvalues.copy(), md.iterations
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


def test_the_jacobi_preconditioner_converges_under_the_same_residual_bars():
    lsm = _lsm()
    b = R.base("20x14_m1")
    cs = b["case"]
    dev = _operator(lsm, cs, precond="jacobi")
    md = _modes(dev, cs, m=2, max_iters=3000)
    op, Mn = _level0(dev, b["hier"].ops[0]), b["mass"]
    ortho = _check_vectors(op, Mn, md, 1e-6, "20x14 jacobi")
    want = R.exact(op, Mn, 2)
    print(f"20x14 jacobi: {md.iterations} iterations, |XᵀMX − I| {ortho:.2e}")
    assert np.max(np.abs(md.eigenvalues - want) / want) <= 1e-6 and ortho <= 1e-12
    md.close()
    dev.close()


def test_a_modes_call_leaves_the_solver_unchanged_and_needs_its_operator():
    lsm = _lsm()
    cs = E.cases()["24x33x10_patch"]
    s = dict(f=cs["f"])
    n = cs["n"]
    mf = lsm.MeshField(np.asfortranarray(cs["phi"]), lsm.CartesianGrid((0.0,) * len(n), cs["hc"], n), dtype=cs["dtype"])
    phi = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=mf, bc=lsm.NeumannBC()).current_state()
    dev = lsm.ElasticityOperator(phi, E_in=cs["E_in"], E_out=cs["E_out"], nu=cs["nu"], plane=cs["plane"], dirichlet=(_mask(cs), tuple(cs["g"])))
    before = dev.solve(s["f"], rtol=1e-8)
    md = dev.modes(2, rtol=1e-4)
    after = dev.solve(s["f"], rtol=1e-8)
    assert after.iterations == before.iterations
    assert np.array_equal(_bits(_values(after.u)), _bits(_values(before.u)))
    with pytest.raises(ValueError, match="give the cell densities"):
        lsm.ElasticityOperator(phi, E=1.0, dirichlet=(_mask(cs), 0.0)).modes(2)
    dev.close()
    for use in (md.vectors, md.mass, lambda: md.mode(0), lambda: md.sensitivity(0), md.solve):
        with pytest.raises(ValueError, match="closed"):
            use()
    md.close()


def test_the_c_abi_refuses_what_the_header_lists():
    lsm = _lsm()
    L = lsm._lib
    cs = R.base("5x5_one_level_m2")["case"]
    dev = _operator(lsm, cs)
    b, t = dev.backend, dev.backend.torch
    phi = dev._phi.buf
    assert dev.free_dofs == 40

    def invalid(call):
        with pytest.raises(lsm.LsmError, match=r"\(-1\)") as e:
            call()
        assert not isinstance(e.value, lsm.LsmNotConvergedError)

    for m in (0, 9, -3):
        invalid(lambda: b.modes_create(dev._handle(), phi, 0.0, 1.0, 1e-6, None, m))
    for rin, rout in ((0.0, 1e-6), (1.0, -1.0), (float("nan"), 1e-6), (1.0, float("inf"))):
        invalid(lambda: b.modes_create(dev._handle(), phi, 0.0, rin, rout, None, 2))
    invalid(lambda: b.modes_create(dev._handle(), phi, float("nan"), 1.0, 1e-6, None, 2))
    invalid(lambda: b.modes_create(dev._handle(), None, 0.0, 1.0, 1e-6, None, 2))
    bad = t.ones(16, dtype=t.float64, device=b.device)
    bad[5] = float("nan")
    invalid(lambda: b.modes_create(dev._handle(), None, 0.0, 1.0, 1e-6, bad, 2))
    bad[5] = 0.0
    invalid(lambda: b.modes_create(dev._handle(), None, 0.0, 1.0, 1e-6, bad, 2))
    with pytest.raises(ValueError, match="must be finite and positive"):
        dev.modes(2, rho=bad)
    # 3·m above the free components: 4×4 nodes clamped on two opposite faces leave 16
    n4 = (4, 4)
    small = dict(cs, n=n4, hc=(1.0, 1.0), h=(1.0 / 3, 1.0 / 3), phi=np.full(n4, -1.0), bits=E.face_bits(n4, 0, 0, 3) | E.face_bits(n4, 0, 1, 3))
    tiny = _operator(lsm, small)
    assert tiny.free_dofs == 16
    invalid(lambda: tiny.backend.modes_create(tiny._handle(), tiny._phi.buf, 0.0, 1.0, 1e-6, None, 6))
    with pytest.raises(ValueError, match="exceeds"):
        tiny.modes(6)
    two = tiny.modes(2, rtol=1e-8)
    want = R.exact(E.Operator(np.ones((3, 3)), small["h"], tiny.stiffness(0), small["bits"]), two.mass(), 2)
    assert np.max(np.abs(two.eigenvalues - want) / want) <= 1e-8
    two.close()
    tiny.close()
    md = b.modes_create(dev._handle(), phi, 0.0, 1.0, 1e-6, None, 2)
    for rtol, mx in ((0.0, 10), (-1.0, 10), (float("nan"), 10), (float("inf"), 10), (1e-6, 0)):
        invalid(lambda: b.modes_solve(md, 2, None, rtol, mx))
    invalid(lambda: b.modes_vectors(md, 2 * 2 * 25))                  # no solve has run
    x0 = t.ones(2 * 2 * 25, dtype=t.float64, device=b.device)
    x0[62] = float("inf")          # column 1, component 0, node (2, 2): free
    invalid(lambda: b.modes_solve(md, 2, x0, 1e-6, 10))
    code, lam, rel, it, stats = b.modes_solve(md, 2, None, 1e-10, 2)       # an overrun: λ, relres and iters are still written
    assert code == L.ERR_NOT_CONVERGED and it == 2 and stats[0] == 2 and stats[3] >= 1
    assert np.all(np.isfinite(lam)) and np.all(lam > 0) and lam[0] <= lam[1] and np.all(np.isfinite(rel)) and rel.max() > 1e-10
    assert b.modes_vectors(md, 2 * 2 * 25).isfinite().all()              # the last iterate
    b.modes_destroy(md)
    with pytest.raises(lsm.LsmNotConvergedError) as e:
        dev.modes(2, rtol=1e-10, max_iters=2)
    assert e.value.iterations == 2 and np.all(e.value.eigenvalues > 0) and e.value.relres.max() > 1e-10 and e.value.modes.vectors().shape == (2, 2, 5, 5)
    e.value.modes.close()
    with pytest.raises(ValueError, match="x0 must be finite"):
        dev.modes(2, x0=np.full((2, 2, 5, 5), np.nan))
    with pytest.raises(ValueError, match="x0 has shape"):
        dev.modes(2, x0=np.zeros((2, 5, 5)))
    dev.close()


@pytest.mark.parametrize("n", [(1025, 600), (96, 96, 64)])
def test_grid_stride_shapes(n):
    """more nodes than 2048 × 256 threads: the second trip of the grid-stride loops, the index arithmetic and the Gram pass's capped grid"""
    lsm = _lsm()
    assert int(np.prod(n)) > 2048 * 256
    hier, _, _ = E.prototype(n)
    ref = hier.ops[0]
    cs = dict(n=n, hc=tuple((k - 1.0) / (max(n) - 1.0) for k in n), h=ref.h, phi=E.two_holes(n, ref.h), dtype=np.float64)
    phi = _field(lsm, cs)
    dev = lsm.ElasticityOperator(phi, dirichlet=(lsm.face_mask(phi.mesh, 0, 0), 0.0))
    md = dev.modes(2, rtol=1e-6, max_iters=1000)
    op = _level0(dev, ref)
    Mn = R.mass(op, R.density_cells(cs["phi"], ref.h, 0.0, 1.0, 1e-6))
    assert np.array_equal(_bits(md.mass()), _bits(Mn))
    ortho = _check_vectors(op, Mn, md, 1e-6, str(n))
    print(f"{n}: {md.iterations} iterations, levels {dev.levels}, |XᵀMX − I| {ortho:.2e}, stats {md.stats}")
    assert ortho <= 1e-12 and md.eigenvalues[0] <= md.eigenvalues[1]
    md.close()
    dev.close()
