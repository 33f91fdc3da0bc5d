"""homogenize_conductivity on the device (csrc/lsm_hcond.hip through the Python API) against the restatement (tests/_hcond_ref.py).

Bit for bit: the cell array (EllipticOperator.cells()'s as well), A x for a random x, the N loads, energy_cells(p, q) for every p ≤ q
and sensitivity(W) on the device's own correctors, corrector(k) at the image nodes.  The tensor against math.fsum of the device's own
cell integrands, to (ncells − 1)·2⁻⁵³·Σ|t|/ncells per entry: the worst-case rounding of any summation order.  The solves per corrector
and preconditioner under tests/test_gpu_elliptic.py's bar (iterations ≤ the restatement's + 2; the correctors are kept in float64 on
a float32 handle too).  One V-cycle against a long-double restatement to 16× the float64 restatement's own rounding.  Laminates and
uniform cells against their closed forms at tests/test_hcond_host.py's floor.  Observed on an MI355X: DESIGN.md §7.24."""
import math

import numpy as np
import pytest

import _hcond_ref as R

pytestmark = pytest.mark.gpu

RTOL = 1e-8
NAMES = sorted(R.cases())
FLOOR = 64 * 2.0 ** -53


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
    return dict(a_in=cs["a_in"], a_out=cs["a_out"], a=cs["a"], level=cs["level"])


def _sym(rng, N):
    W = rng.standard_normal((N, N))
    return W + W.T


def check_tensor(dev):
    """the tensor against math.fsum of the device's own cell integrands; symmetric in storage; two calls give the same bits"""
    N = dev.ndim
    K = dev.backend.hcond_tensor(dev._handle())
    assert K.shape == (N, N) and np.array_equal(_bits(K), _bits(K.T))
    assert np.array_equal(_bits(K), _bits(dev.backend.hcond_tensor(dev._handle())))
    worst = 0.0
    for q in range(N):
        for p in range(q + 1):
            t = dev.energy_cells(p, q).reshape(-1)
            nc = t.size
            want = math.fsum(t) / nc
            bound = (nc - 1) * 2.0 ** -53 * math.fsum(np.abs(t)) / nc
            worst = max(worst, abs(K[p, q] - want) / bound if bound > 0 else 0.0)
            assert abs(K[p, q] - want) <= bound, (p, q, K[p, q], want, bound)
    return K, worst


def check_operator(lsm, dev, op, chi, dtype, rng):
    """cells, A x, the loads, the cell integrands and the sensitivity of `chi` (the device's stored correctors): the restatement's bits"""
    N = op.N
    assert np.array_equal(_bits(dev.cells()), _bits(op.a))
    x = rng.standard_normal(op.m)
    assert np.array_equal(_bits(dev.apply(x)), _bits(op.apply(x)))
    for k in range(N):
        assert np.array_equal(_bits(dev.load(k)), _bits(op.load(k))), k
    for q in range(N):
        for p in range(q + 1):
            assert np.array_equal(_bits(dev.energy_cells(p, q)), _bits(op.energy_cells(chi, p, q))), (p, q)
    W = _sym(rng, N)
    g = dev.sensitivity(W).values()
    assert g.dtype == dtype
    assert np.array_equal(_bits(g), _bits(op.sensitivity(chi, W).astype(dtype)))


@pytest.mark.parametrize("name", NAMES)
def test_cells_apply_loads_integrands_and_sensitivity_are_the_restatements_bits(name):
    lsm = _lsm()
    s = R.solved(name)
    cs = s["case"]
    N = len(cs["n"])
    phi = _field(lsm, cs)
    dev = lsm.homogenize_conductivity(phi, rtol=RTOL, max_iters=3000, **_kwargs(cs))
    op = s["hier"].ops[0]
    assert dev.levels == s["hier"].levels and dev.free_dofs == int(np.prod(dev.cells_shape)) - 1 and dev.cells_shape == op.m
    if cs["a"] is None:
        el = lsm.EllipticOperator(phi, a_in=cs["a_in"], a_out=cs["a_out"], level=cs["level"], dirichlet=(lsm.face_mask(phi.mesh, 0, 0), 0.0))
        assert np.array_equal(_bits(dev.cells()), _bits(el.cells()))
        el.close()
    chi = dev.correctors()
    assert chi.shape == (N,) + op.m and chi.dtype == np.float64 and not chi[(slice(None),) + (0,) * N].any()
    check_operator(lsm, dev, op, chi, cs["dtype"], np.random.default_rng(11))
    for k in range(N):
        u = dev.corrector(k).values()
        assert u.dtype == cs["dtype"] and np.array_equal(_bits(u), _bits(R.image(chi[k]).astype(cs["dtype"])))
    K, worst = check_tensor(dev)
    assert np.array_equal(_bits(K), _bits(dev.tensor))
    print(f"{name}: tensor within {worst:.3f} of its summation bound, iterations {dev.iterations}, K = {K.tolist()}")
    dev.close()


@pytest.mark.parametrize("name,precond", [(k, pc) for k in NAMES for pc in ("mg", "jacobi")])
def test_solve_against_the_restatement(name, precond):
    lsm = _lsm()
    s = R.solved(name)
    cs = s["case"]
    N = len(cs["n"])
    dev = lsm.homogenize_conductivity(_field(lsm, cs), rtol=RTOL, max_iters=3000, precond=precond, **_kwargs(cs))
    op = s["hier"].ops[0]
    chi = dev.correctors()
    chiref, itref = s[precond]
    for k in range(N):
        f = op.load(k)
        tr, bn = R.true_residual(op, f, chi[k])
        dref, ddev = float(np.abs(chiref[k] - s["direct"][k]).max()), float(np.abs(chi[k] - s["direct"][k]).max())
        print(f"{name} {precond} χ{k}: {dev.iterations[k]} iterations (restatement {itref[k]}), relres {dev.relres[k]:.3e}, true residual {tr / bn:.3e}·‖f‖, "
              f"|χ − direct| {ddev:.3e} (restatement {dref:.3e}), levels {dev.levels}")
        assert dev.relres[k] <= RTOL
        assert tr <= 2 * RTOL * bn
        assert dev.iterations[k] <= itref[k] + 2
    dev.close()


@pytest.mark.parametrize("name", NAMES)
def test_mg_needs_fewer_iterations_than_jacobi(name):
    lsm = _lsm()
    cs = R.cases()[name]
    it = {}
    for pc in ("mg", "jacobi"):
        dev = lsm.homogenize_conductivity(_field(lsm, cs), rtol=RTOL, max_iters=3000, precond=pc, **_kwargs(cs))
        it[pc], levels = dev.iterations, dev.levels
        dev.close()
    print(f"{name}: mg {it['mg']}, jacobi {it['jacobi']}, levels {levels}")
    if levels > 1:
        assert max(it["mg"]) < min(it["jacobi"])
    else:
        assert max(it["mg"]) <= min(it["jacobi"])


def _closed_form_cases():
    out = {}
    for n, axis, layers in (((17, 9), 0, 4), ((17, 9), 1, 3), ((9, 7, 5), 0, 2), ((9, 7, 5), 1, 5), ((5, 7, 9), 2, 5)):
        m = tuple(x - 1 for x in n)
        out[f"laminate_{'x'.join(map(str, n))}_axis{axis}"] = (n, R.laminate_cells(m, 1.0, 0.1, layers, axis), R.laminate_tensor(1.0, 0.1, layers / m[axis], len(n), axis))
    for n in ((7, 6), (5, 4, 6)):
        out[f"uniform_{'x'.join(map(str, n))}"] = (n, np.full(tuple(x - 1 for x in n), 2.5, order="F"), 2.5 * np.eye(len(n)))
    return out


@pytest.mark.parametrize("name", sorted(_closed_form_cases()))
def test_laminates_and_uniform_cells_have_their_closed_forms(name):
    """the floor is tests/test_hcond_host.py's, 64·2⁻⁵³·max|K|.  The error of K^H is quadratic in the corrector's, at most rtol²·κ(A)
    relative: rtol = 1e-12 keeps it below 2⁻⁵³ for any κ these small cells can have, so the floor is left to the arithmetic."""
    lsm = _lsm()
    n, a, want = _closed_form_cases()[name]
    hc = tuple((x - 1.0) / (max(n) - 1.0) for x in n)
    h = tuple(x / (nd - 1) for x, nd in zip(hc, n))
    cs = dict(n=n, hc=hc, h=h, phi=np.zeros(n, order="F"), dtype=np.float64)
    dev = lsm.homogenize_conductivity(_field(lsm, cs), a=a, rtol=1e-12)
    err = np.abs(dev.tensor - want).max()
    print(f"{name}: max|K − closed form| {err / np.abs(want).max():.2e}·max|K|, iterations {dev.iterations}")
    if name.startswith("uniform"):
        assert dev.iterations == [0] * len(n) and not dev.correctors().any()
        for k in range(len(n)):
            assert not dev.load(k).any()
    assert err <= FLOOR * np.abs(want).max()
    dev.close()


@pytest.mark.parametrize("name", R.FIRST_ITERATE)
def test_the_first_iterate_is_the_restatements_to_rounding(name):
    """a solve at rtol 0.97 stops after one iteration: x₁ = α·M b shows one V-cycle at every node.  Observed ratios: DESIGN.md §7.24."""
    lsm = _lsm()
    cs = R.cases()[name]
    dev = lsm.ConductivityHomogenization(_field(lsm, cs), **_kwargs(cs))
    hier = R.build_case(cs)
    assert hier.levels == dev.levels
    runs, left_out = R.first_iterate_runs(hier)
    assert not left_out and runs[0][0] == "load0" and len(runs) == 3 + len(cs["n"])
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
    """solve_rhs from a guess that is not zero at node 0: the bits, iterations and residual of the same guess with zero there, and
    zero at the pin.  These two of R.FIRST_ITERATE have odd axes, which leave a coarsest level that one workgroup cannot hold in 2-D."""
    lsm = _lsm()
    cs = R.cases()[name]
    dev = lsm.ConductivityHomogenization(_field(lsm, cs), precond=precond, **_kwargs(cs))
    pin = (0,) * len(cs["n"])
    f = dev.load(0)
    x0 = np.random.default_rng(5).standard_normal(f.shape) * min(cs["h"])
    x0[pin] = 0.0
    xz, itz, relz = dev.solve_rhs(f, x0, rtol=RTOL, max_iters=3000)
    x0[pin] = 1.0
    xp, itp, relp = dev.solve_rhs(f, x0, rtol=RTOL, max_iters=3000)
    print(f"{name} {precond}: {itz} iterations, relres {relz:.3e}, levels {dev.levels}")
    assert itz > 1 and itp == itz and relp == relz
    assert np.array_equal(_bits(xp), _bits(xz)) and xp[pin] == 0.0
    dev.close()


@pytest.mark.parametrize("n", [(801, 701), (90, 90, 70)])
def test_grid_stride_shapes(n):
    """more nodes than 2048 × 256 threads, without a solve: the second trip of the grid-stride loops and the index arithmetic"""
    lsm = _lsm()
    N = len(n)
    assert int(np.prod([x - 1 for x in n])) > 2048 * 256
    hc = tuple((x - 1.0) / (max(n) - 1.0) for x in n)
    h = tuple(x / (nd - 1) for x, nd in zip(hc, n))
    cs = dict(n=n, hc=hc, h=h, phi=R.inclusion(n, h, 0.09 if N == 2 else 0.1), a=None, a_in=1.0, a_out=1e-3, level=0.0, dtype=np.float64)
    dev = lsm.ConductivityHomogenization(_field(lsm, cs), **_kwargs(cs))
    op = R.Operator(R.cell_coefficients(cs["phi"], h, 0.0, 1.0, 1e-3), h)
    rng = np.random.default_rng(11)
    chi = rng.standard_normal((N,) + op.m) * min(h)
    dev.with_correctors(chi)
    assert np.array_equal(_bits(dev.correctors()), _bits(chi))
    check_operator(lsm, dev, op, chi, np.float64, rng)
    _, worst = check_tensor(dev)
    print(f"{n}: tensor within {worst:.3f} of its summation bound")
    dev.close()


def test_warm_start_failure_and_refusals():
    lsm = _lsm()
    cs = R.cases()["13x9"]
    phi = _field(lsm, cs)
    dev = lsm.homogenize_conductivity(phi, rtol=RTOL, **_kwargs(cs))
    chi, K = dev.correctors(), dev.tensor.copy()
    assert min(dev.iterations) > 1
    # a warm start from the converged correctors takes no iteration, on this object and on a new one
    dev.solve(chi0=chi, rtol=RTOL)
    assert dev.iterations == [0, 0] and np.array_equal(_bits(dev.correctors()), _bits(chi))
    new = lsm.homogenize_conductivity(phi, chi0=chi, rtol=RTOL, **_kwargs(cs))
    assert new.iterations == [0, 0] and np.array_equal(_bits(new.tensor), _bits(K))
    new.close()
    # max_iters = 1 does not suffice: the stored correctors are untouched
    with pytest.raises(lsm.LsmNotConvergedError, match="max_iters"):
        dev.solve(rtol=RTOL, max_iters=1)
    assert np.array_equal(_bits(dev.correctors()), _bits(chi)) and np.array_equal(_bits(dev.tensor), _bits(K))
    with pytest.raises(ValueError, match="symmetric"):
        dev.sensitivity(np.array([[1.0, 2.0], [0.0, 1.0]]))
    with pytest.raises(ValueError):
        dev.load(2)
    dev.close()
    with pytest.raises(ValueError, match="closed"):
        dev.correctors()
    # refusals, each with a message
    bad = cs["phi"].copy()
    bad[3, 4] = np.nan
    with pytest.raises(ValueError, match="phi must be finite"):
        lsm.homogenize_conductivity(_field(lsm, dict(cs, phi=bad)))
    abad = np.ones((12, 8))
    abad[2, 2] = np.nan
    with pytest.raises(ValueError, match="finite and positive"):
        lsm.homogenize_conductivity(phi, a=abad)
    with pytest.raises(ValueError, match="precond"):
        lsm.homogenize_conductivity(phi, precond="ilu")
    t = phi.backend.torch
    with pytest.raises(lsm.LsmError, match="finite and positive") as ei:
        phi.backend.hcond_create(None, 0.0, 1.0, 1e-3, t.from_numpy(abad.reshape(-1, order="F").copy()).to(phi.backend.device), 0)
    assert ei.value.reason == 2 and ei.value.detail == 1
    g1 = lsm.CartesianGrid((0.0,), (1.0,), (16,))
    p1 = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(np.linspace(-1, 1, 16), g1), bc=lsm.NeumannBC()).current_state()
    with pytest.raises(ValueError, match="1 dimensional"):
        lsm.homogenize_conductivity(p1)
    with pytest.raises(lsm.LsmError, match="1-dimensional"):
        p1.backend.hcond_create(p1.buf, 0.0, 1.0, 1e-3, None, 0)
    # (an axis with fewer than 2 cells cannot reach the device: a handle has at least 4 nodes per dimension; tests/test_hcond_host.py has
    # the refusal, with the band field and the slab.)  ϕ needs no PeriodicBC, and one does no harm: only the cells are read
    pp = _field(lsm, cs, bc=(lsm.PeriodicBC(), lsm.NeumannBC()))
    per = lsm.homogenize_conductivity(pp, rtol=RTOL, **_kwargs(cs))
    assert np.array_equal(_bits(per.tensor), _bits(K))
    per.close()
    # elliptic_solve keeps refusing a periodic dimension
    with pytest.raises(ValueError, match="[Pp]eriodic"):
        lsm.EllipticOperator(pp, dirichlet=(lsm.face_mask(pp.mesh, 1, 0), 0.0))


def test_an_update_func_sets_the_speed_to_the_sensitivity_and_a_step_runs():
    lsm = _lsm()
    cs = R.cases()["33x33_soft"]
    n = cs["n"]
    W = np.eye(2)      # the trace of K^H
    seen = {}

    def update(coeff, phi, t):
        hom = lsm.homogenize_conductivity(phi, rtol=RTOL, chi0=seen.get("chi"), **_kwargs(cs))
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
