"""homogenize on the device (csrc/lsm_homog.hip through the Python API) against the restatement (tests/_homog_ref.py).

With the device's K0 handed to the restatement, bit for bit: the cell array (ElasticityOperator.cells()'s as well), A x for a random
x, the M loads, energy_cells(p, q) for every p ≤ q and sensitivity(W) on the device's own correctors, corrector(k) at the image
nodes.  The tensor against math.fsum of the device's own cell integrands, to (ncells − 1)·2⁻⁵³·Σ|t|/ncells per entry: the worst-case
rounding of any summation order.  The solves per corrector and preconditioner under tests/test_gpu_elastic.py's bars (the correctors
are kept in float64 on a float32 handle too, so that file's float32 term is zero here).  One V-cycle against a long-double
restatement to 16× the float64 restatement's own rounding.  Observed on an MI355X: DESIGN.md §7.23."""
import math

import numpy as np
import pytest

import _elastic_ref as RE
import _homog_ref as R

pytestmark = pytest.mark.gpu

RTOL = 1e-8
NAMES = sorted(R.cases())


def _lsm():
    import lsm_amd
    return lsm_amd


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _field(lsm, cs, bc=None):
    n = cs["n"]
    mf = lsm.MeshField(np.asfortranarray(cs["phi"]), lsm.CartesianGrid((0.0,) * len(n), cs["hc"], n), dtype=cs["dtype"])
    phi = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=mf, bc=lsm.NeumannBC() if bc is None else bc).current_state()
    assert tuple(phi.mesh.meshsize()) == tuple(cs["h"])
    return phi


def _kwargs(cs):
    return dict(E_in=cs["E_in"], E_out=cs["E_out"], E=cs["E"], nu=cs["nu"], plane=cs["plane"], level=cs["level"])


def _device_hierarchy(dev, cs):
    """the restatement's hierarchy on the device's own K0 and dampings, after comparing each level's K0 with the closed form"""
    k0s, h, m = [], list(cs["h"]), tuple(x - 1 for x in cs["n"])
    for l in range(dev.levels):
        K = dev.stiffness(l)
        want = RE.k0(tuple(h), cs["nu"], cs["plane"])
        assert np.abs(K - want).max() <= 8 * 2.0 ** -52 * np.abs(want).max(), (l, np.abs(K - want).max())
        k0s.append(K)
        nxt = R.coarsen_shape(m)
        if nxt is not None:
            m, co = nxt
            h = [x * 2.0 if c else x for x, c in zip(h, co)]
    with pytest.raises(_lsm().LsmError):
        dev.stiffness(dev.levels)
    hier = R.build_case(cs, k0s, R.device_omegas(k0s, len(cs["n"])))
    assert hier.levels == dev.levels
    return hier


def _sym(rng, M):
    W = rng.standard_normal((M, M))
    return W + W.T


def check_tensor(dev, M):
    """the tensor against math.fsum of the device's own cell integrands; symmetric in storage; two calls give the same bits"""
    C = dev.backend.homog_tensor(dev._handle())
    assert np.array_equal(_bits(C), _bits(C.T))
    assert np.array_equal(_bits(C), _bits(dev.backend.homog_tensor(dev._handle())))
    worst = 0.0
    for q in range(M):
        for p in range(q + 1):
            t = dev.energy_cells(p, q).reshape(-1)
            nc = t.size
            want = math.fsum(t) / nc
            bound = (nc - 1) * 2.0 ** -53 * math.fsum(np.abs(t)) / nc
            worst = max(worst, abs(C[p, q] - want) / bound if bound > 0 else 0.0)
            assert abs(C[p, q] - want) <= bound, (p, q, C[p, q], want, bound)
    return C, worst


@pytest.mark.parametrize("name", NAMES)
def test_cells_apply_loads_integrands_and_sensitivity_are_the_restatements_bits(name):
    lsm = _lsm()
    s = R.solved(name)
    cs = s["case"]
    N, M = len(cs["n"]), R.nstrains(len(cs["n"]))
    phi = _field(lsm, cs)
    dev = lsm.homogenize(phi, rtol=RTOL, max_iters=3000, **_kwargs(cs))
    assert dev.levels == s["hier"].levels and dev.free_dofs == N * int(np.prod(dev.cells_shape)) - N
    hier = _device_hierarchy(dev, cs)
    op = hier.ops[0]
    assert np.array_equal(_bits(dev.cells()), _bits(op.E))
    if cs["E"] is None:
        el = lsm.ElasticityOperator(phi, E_in=cs["E_in"], E_out=cs["E_out"], nu=cs["nu"], plane=cs["plane"], level=cs["level"],
                                    dirichlet=(lsm.face_mask(phi.mesh, 0, 0), 0.0))
        assert np.array_equal(_bits(dev.cells()), _bits(el.cells()))
        el.close()
    rng = np.random.default_rng(11)
    x = rng.standard_normal((N,) + op.m)
    assert np.array_equal(_bits(dev.apply(x)), _bits(op.apply(x)))
    for k in range(M):
        assert np.array_equal(_bits(dev.load(k)), _bits(op.load(k))), k
    chi = dev.correctors()
    assert chi.shape == (M, N) + op.m and not chi[(slice(None), slice(None)) + (0,) * N].any()
    for q in range(M):
        for p in range(q + 1):
            assert np.array_equal(_bits(dev.energy_cells(p, q)), _bits(op.energy_cells(chi, p, q))), (p, q)
    W = _sym(rng, M)
    g = dev.sensitivity(W).values()
    assert g.dtype == cs["dtype"]
    assert np.array_equal(_bits(g), _bits(op.sensitivity(chi, W).astype(cs["dtype"])))
    for k in (0, M - 1):
        u = np.stack([c.values() for c in dev.corrector(k)])
        assert np.array_equal(_bits(u), _bits(np.stack([R.image(chi[k, i]) for i in range(N)]).astype(cs["dtype"])))
    C, worst = check_tensor(dev, M)
    assert np.array_equal(_bits(C), _bits(dev.tensor))
    print(f"{name}: tensor within {worst:.3f} of its summation bound, iterations {dev.iterations}")
    dev.close()


@pytest.mark.parametrize("name,precond", [(k, "mg") for k in NAMES] + [(k, "jacobi") for k in NAMES if R.cases()[k]["both"]])
def test_solve_against_the_restatement(name, precond):
    lsm = _lsm()
    s = R.solved(name)
    cs = s["case"]
    M = R.nstrains(len(cs["n"]))
    dev = lsm.homogenize(_field(lsm, cs), rtol=RTOL, max_iters=3000, precond=precond, **_kwargs(cs))
    op = _device_hierarchy(dev, cs).ops[0]
    chi = dev.correctors()
    chiref, itref = s[precond]
    for k in range(M):
        f = op.load(k)
        tr, bn = R.true_residual(op, f, chi[k])
        dref, ddev = float(np.abs(chiref[k] - s["direct"][k]).max()), float(np.abs(chi[k] - s["direct"][k]).max())
        print(f"{name} {precond} χ{k}: {dev.iterations[k]} iterations (restatement {itref[k]}), relres {dev.relres[k]:.3e}, true residual {tr / bn:.3e}·‖f‖, "
              f"|χ − direct| {ddev:.3e} (restatement {dref:.3e}), levels {dev.levels}")
        assert dev.relres[k] <= RTOL
        assert tr <= 2 * RTOL * bn
        assert ddev <= 4 * dref
        assert dev.iterations[k] <= itref[k] + 2
    if precond == "mg" and dev.levels > 1 and cs["both"]:
        jac = lsm.homogenize(_field(lsm, cs), rtol=RTOL, max_iters=3000, precond="jacobi", **_kwargs(cs))
        assert max(dev.iterations) < min(jac.iterations)
        jac.close()
    dev.close()


def _closed_form_cases():
    out = {}
    for name, n, axis, layers in (("laminate_17x9_axis0", (17, 9), 0, 4), ("laminate_17x9_axis1", (17, 9), 1, 3), ("laminate_9x7x5_axis0", (9, 7, 5), 0, 2)):
        m = tuple(x - 1 for x in n)
        out[name] = (n, R.laminate_cells(m, 1.0, 0.1, layers, axis), "stress", R.laminate_tensor(1.0, 0.1, layers / m[axis], 0.3, len(n), "stress", axis))
    for name, n, plane in (("uniform_7x6_stress", (7, 6), "stress"), ("uniform_7x6_strain", (7, 6), "strain"), ("uniform_5x4x6", (5, 4, 6), "stress")):
        out[name] = (n, np.full(tuple(x - 1 for x in n), 2.5, order="F"), plane, 2.5 * R.c0_tensor(0.3, len(n), plane))
    return out


@pytest.mark.parametrize("name", sorted(_closed_form_cases()))
def test_laminates_and_uniform_cells_have_their_closed_forms(name):
    lsm = _lsm()
    n, E, plane, want = _closed_form_cases()[name]
    hc = tuple((x - 1.0) / (max(n) - 1.0) for x in n)
    h = tuple(x / (nd - 1) for x, nd in zip(hc, n))
    cs = dict(n=n, hc=hc, h=h, phi=np.zeros(n, order="F"), dtype=np.float64)
    hier = R.Hierarchy(E, h, 0.3, plane)
    chiref, _ = R.correctors(hier, "pcg", RTOL, "mg")
    eref = np.abs(hier.ops[0].tensor(chiref) - want)
    dev = lsm.homogenize(_field(lsm, cs), E=E, plane=plane, rtol=RTOL)
    err = np.abs(dev.tensor - want)
    bound = np.maximum(100 * eref, 64 * 2.0 ** -53 * np.abs(want).max())
    print(f"{name}: max|C − closed form| {err.max():.2e} (restatement's PCG {eref.max():.2e}), iterations {dev.iterations}")
    assert (err <= bound).all()
    dev.close()


@pytest.mark.parametrize("name", R.FIRST_ITERATE)
def test_the_first_iterate_is_the_restatements_to_rounding(name):
    """a solve at rtol 0.97 stops after one iteration: x₁ = α·M b shows one V-cycle at every node and component"""
    lsm = _lsm()
    cs = R.cases()[name]
    dev = lsm.Homogenization(_field(lsm, cs), **_kwargs(cs))
    hier = _device_hierarchy(dev, cs)
    runs, left_out = R.first_iterate_runs(hier)
    print(f"{name}: dampings {[float(hier.omega(l)) for l in range(hier.levels)]}, left out {[(k, float(r)) for k, _, _, r in left_out]}")
    assert len(runs) >= 3 and runs[0][0] == "load0"
    for fname, f, xref, rel in runs:
        x, it, relres = dev.solve_rhs(f, rtol=R.FIRST_RTOL)
        xld = R.first_iterate_ld(hier, f)
        scale = float(np.abs(xld).max())
        yard = max(float(np.abs(xref - xld).max()), 2.0 ** -53 * scale)
        err = float(np.abs(x - xld).max())
        print(f"{name} {fname}: {it} iteration(s), relres {relres:.3f} (restatement {rel:.3f}), |x_dev − x_ld| {err / scale:.2e}·max|x|, yardstick {yard / scale:.2e}·max|x|, "
              f"ratio {err / yard:.2f}")
        assert it == 1
        assert err <= 16 * yard
    dev.close()


@pytest.mark.parametrize("name,precond", [(k, pc) for k in ("13x9", "9x5x7") for pc in ("mg", "jacobi")])
def test_a_guess_at_the_pinned_node_is_ignored(name, precond):
    """solve_rhs from a guess that is not zero at node 0, in every component: the bits, iterations and residual of the same guess with
    zeros there, and zero at the pin.  These two of R.FIRST_ITERATE have odd axes, which leave a coarsest level that one workgroup cannot hold in 2-D."""
    lsm = _lsm()
    cs = R.cases()[name]
    N = len(cs["n"])
    dev = lsm.Homogenization(_field(lsm, cs), precond=precond, **_kwargs(cs))
    pin = (slice(None),) + (0,) * N
    f = dev.load(0)
    x0 = np.random.default_rng(5).standard_normal(f.shape) * min(cs["h"])
    x0[pin] = 0.0
    xz, itz, relz = dev.solve_rhs(f, x0, rtol=RTOL, max_iters=3000)
    x0[pin] = 1.0 + np.arange(N)
    xp, itp, relp = dev.solve_rhs(f, x0, rtol=RTOL, max_iters=3000)
    print(f"{name} {precond}: {itz} iterations, relres {relz:.3e}, levels {dev.levels}")
    assert itz > 1 and itp == itz and relp == relz
    assert np.array_equal(_bits(xp), _bits(xz)) and not xp[pin].any()
    dev.close()


def test_a_non_finite_right_hand_side_is_refused_and_changes_nothing():
    lsm = _lsm()
    cs = R.cases()["13x9"]
    dev = lsm.homogenize(_field(lsm, cs), rtol=RTOL, **_kwargs(cs))
    chi, C = dev.correctors(), dev.backend.homog_tensor(dev._handle())
    f = dev.load(0)
    f[1, 3, 4] = np.nan
    with pytest.raises(lsm.LsmError, match=r"\(1 entries are not\)"):
        dev.solve_rhs(f, rtol=RTOL)
    assert np.array_equal(_bits(dev.correctors()), _bits(chi))
    assert np.array_equal(_bits(dev.backend.homog_tensor(dev._handle())), _bits(C)) and np.array_equal(_bits(dev.tensor), _bits(C))
    dev.close()


@pytest.mark.parametrize("n", [(801, 701), (90, 90, 70)])
def test_grid_stride_shapes(n):
    """more nodes than 2048 × 256 threads, without a solve: the second trip of the grid-stride loops and the index arithmetic"""
    lsm = _lsm()
    N, M = len(n), R.nstrains(len(n))
    assert int(np.prod([x - 1 for x in n])) > 2048 * 256
    hc = tuple((x - 1.0) / (max(n) - 1.0) for x in n)
    h = tuple(x / (nd - 1) for x, nd in zip(hc, n))
    cs = dict(n=n, hc=hc, h=h, phi=R.inclusion(n, h, 0.09 if N == 2 else 0.1), E=None, E_in=1.0, E_out=1e-3, nu=0.3, plane="stress", level=0.0, dtype=np.float64)
    dev = lsm.Homogenization(_field(lsm, cs), **_kwargs(cs))
    op = R.Operator(R.cell_coefficients(cs["phi"], h, 0.0, 1.0, 1e-3), h, dev.stiffness(0))
    assert np.array_equal(_bits(dev.cells()), _bits(op.E))
    rng = np.random.default_rng(11)
    x = rng.standard_normal((N,) + op.m)
    assert np.array_equal(_bits(dev.apply(x)), _bits(op.apply(x)))
    for k in range(M):
        assert np.array_equal(_bits(dev.load(k)), _bits(op.load(k))), k
    chi = rng.standard_normal((M, N) + op.m) * min(h)
    dev.with_correctors(chi)
    assert np.array_equal(_bits(dev.correctors()), _bits(chi))
    pairs = [(p, q) for q in range(M) for p in range(q + 1)] if N == 2 else [(0, 0), (1, 4), (5, 5)]      # 3-D: three of the 21 pairs, for the restatement's time
    for p, q in pairs:
        assert np.array_equal(_bits(dev.energy_cells(p, q)), _bits(op.energy_cells(chi, p, q))), (p, q)
    W = _sym(rng, M)
    assert np.array_equal(_bits(dev.sensitivity(W).values()), _bits(op.sensitivity(chi, W)))
    _, worst = check_tensor(dev, M)
    print(f"{n}: tensor within {worst:.3f} of its summation bound")
    dev.close()


def test_warm_start_failure_and_refusals():
    lsm = _lsm()
    cs = R.cases()["13x9"]
    phi = _field(lsm, cs)
    dev = lsm.homogenize(phi, rtol=RTOL, **_kwargs(cs))
    chi, C = dev.correctors(), dev.tensor.copy()
    assert min(dev.iterations) > 1
    # a warm start from the converged correctors takes no iteration, on this object and on a new one
    dev.solve(chi0=chi, rtol=RTOL)
    assert dev.iterations == [0, 0, 0] and np.array_equal(_bits(dev.correctors()), _bits(chi))
    new = lsm.homogenize(phi, chi0=chi, rtol=RTOL, **_kwargs(cs))
    assert new.iterations == [0, 0, 0] and np.array_equal(_bits(new.tensor), _bits(C))
    new.close()
    # max_iters = 1 does not suffice: the stored correctors are untouched
    with pytest.raises(lsm.LsmNotConvergedError, match="max_iters"):
        dev.solve(rtol=RTOL, max_iters=1)
    assert np.array_equal(_bits(dev.correctors()), _bits(chi)) and np.array_equal(_bits(dev.tensor), _bits(C))
    dev.close()
    with pytest.raises(ValueError, match="closed"):
        dev.correctors()
    # refusals, each with a message
    bad = cs["phi"].copy()
    bad[3, 4] = np.nan
    with pytest.raises(ValueError, match="phi must be finite"):
        lsm.homogenize(_field(lsm, dict(cs, phi=bad)))
    Ebad = np.ones((12, 8))
    Ebad[2, 2] = np.nan
    with pytest.raises(ValueError, match="finite and positive"):
        lsm.homogenize(phi, E=Ebad)
    t = phi.backend.torch
    with pytest.raises(lsm.LsmError, match="finite and positive") as ei:
        phi.backend.homog_create(None, 0.0, 1.0, 1e-3, t.from_numpy(Ebad.reshape(-1, order="F").copy()).to(phi.backend.device), 0.3, 0, 0)
    assert ei.value.reason == 2 and ei.value.detail == 1
    g1 = lsm.CartesianGrid((0.0,), (1.0,), (16,))
    p1 = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(np.linspace(-1, 1, 16), g1), bc=lsm.NeumannBC()).current_state()
    with pytest.raises(ValueError, match="1 dimensional"):
        lsm.homogenize(p1)
    with pytest.raises(lsm.LsmError, match="1-dimensional"):
        p1.backend.homog_create(p1.buf, 0.0, 1.0, 1e-3, None, 0.3, 0, 0)
    # (an axis with fewer than 2 cells cannot reach the device: a handle has at least 4 nodes per dimension; tests/test_homog_host.py
    # has the refusal.)  ϕ needs no PeriodicBC, and one does no harm: only the cells are read
    pp = _field(lsm, cs, bc=(lsm.PeriodicBC(), lsm.NeumannBC()))
    per = lsm.homogenize(pp, rtol=RTOL, **_kwargs(cs))
    assert np.array_equal(_bits(per.tensor), _bits(C))
    per.close()


def test_an_update_func_sets_the_speed_to_the_sensitivity_and_a_step_runs():
    lsm = _lsm()
    cs = R.cases()["33x33_soft"]
    n = cs["n"]
    W = np.diag([1.0, 1.0, 0.0])      # the sum of the two normal stiffnesses
    seen = {}

    def update(coeff, phi, t):
        hom = lsm.homogenize(phi, rtol=RTOL, chi0=seen.get("chi"), **_kwargs(cs))
        g = hom.sensitivity(W)
        coeff.set_values(g)
        seen["chi"], seen["g"], seen["speed"] = hom.correctors(), g.buf.clone(), coeff.fields[0].clone()
        hom.close()

    grid = lsm.CartesianGrid((0.0,) * len(n), cs["hc"], n)
    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(lsm.MeshField(np.zeros(n), grid), update),), ic=lsm.MeshField(cs["phi"], grid), bc=lsm.NeumannBC(),
                              integrator=lsm.RK3())
    before = eq.current_state().values()
    lsm.integrate_(eq, 1e-9)
    assert "g" in seen and bool((seen["g"] == seen["speed"]).all())
    assert float(seen["speed"].abs().max()) > 0
    after = eq.current_state().values()
    assert np.isfinite(after).all() and not np.array_equal(after, before)
