"""Stress recovery on the device (csrc/lsm_elastic.hip through the Python API) against the restatement (tests/_stress_ref.py) on the
device's own K0 and cell moduli.

Bit for bit, for a random displacement (not a solution) through with_displacement: the three cell arrays and the three kinds of node
field, on every shape of _stress_ref.field_cases() — a handle takes 4 nodes per dimension at least, so 4×4, 5×4 and 4×4×4 stand
for the 3×3, 4×3 and 3×3×3 one would start from; 9×12, 5×4×6 and 4×6×21 have interior nodes — and on the two launch shapes beyond
2048 workgroups of 256 threads; smax as well.  A float32 handle: the inputs rounded to float32 first, the outputs rounded once.

To rounding: J′, the adjoint load and the sensitivity pass (λ given as fields) differ from numpy in the order of the grand sum and
in pow.  tests/test_gpu_elastic_edges.py's bar: |x_dev − x_ld|∞ ≤ 16·max(|x_f64 − x_ld|∞, 2⁻⁵³·|x_ld|∞) per case, x_ld the
restatement in long double and x_f64 the restatement in float64; the ratios are printed.  p ∈ {2, 3.5, 8, 64}, sref = smax and 1;
cell (0, 0, …) of every case is translated, so it has zero strain and the load must be finite there.  A float32 handle rounds the
sensitivity field once more: half a float32 ulp of the value, 2⁻²⁴·|d|, is taken off the difference before it is measured.

End to end on four small solved problems (a cantilever with a hole at contrast 1e-3): stress_sensitivity against the restatement
with direct solves, under 4× what the restatement's own PCG at the same rtol leaves (tests/test_gpu_elastic.py's convention); the
homogeneity identity |Σ count·d| / Σ count·|p·r^p| under 4× the restatement's value at that rtol; the adjoint solve in no more than the
state solve's iterations + 2 (the restatement: 15/15, 16/16, 13/12, 15/15).

The new calls between two solves of one operator (and between two modes solves) change no bit of either; the C ABI refuses what
include/lsm.h says it refuses."""
import ctypes as C

import numpy as np
import pytest

import _elastic_ref as R
import _stress_ref as S
import test_gpu_elastic as T
from _elliptic_ref import LD

pytestmark = pytest.mark.gpu

FIELD_CASES = S.field_cases()
SOLVED_CASES = S.solved_cases()
RTOL = 1e-8


def _open(lsm, cs):
    """(the device operator, the restatement on its K0 and cells)"""
    dev = lsm.ElasticityOperator(T._field(lsm, cs), **T._kwargs(cs))
    op = R.Operator(dev.cells(), cs["h"], dev.stiffness(0), cs["bits"])
    return dev, S.Stress(op, cs["nu"], cs["plane"])


def _random_u(cs, seed=31):
    """a random displacement, rounded to the storage type; the corners of cell (0, 0, …) share one value: zero strain there"""
    n = tuple(cs["n"])
    u = np.random.default_rng(seed).standard_normal((len(n),) + n)
    u[(slice(None),) + (slice(0, 2),) * len(n)] = 0.375
    return u.astype(cs["dtype"]).astype(np.float64)


def _cell_arrays(dev, sol, what, cn):
    flat = dev.backend.elastic_stress_cells(dev._handle(), [c.buf for c in sol.u], what).cpu().numpy()
    nc = int(np.prod(cn))
    return np.stack([flat[k * nc:(k + 1) * nc].reshape(cn, order="F") for k in range(flat.size // nc)])


@pytest.mark.parametrize("name", sorted(FIELD_CASES))
def test_the_cell_arrays_and_node_fields_are_the_restatements_bits(name):
    lsm = T._lsm()
    cs = FIELD_CASES[name]
    dev, st = _open(lsm, cs)
    u = _random_u(cs)
    sol = dev.with_displacement(u)
    assert np.array_equal(T._bits(T._values(sol.u)), T._bits(u.astype(cs["dtype"])))
    with pytest.raises(ValueError, match="load"):
        sol.compliance()
    for what in (S.STRAIN, S.STRESS, S.VON_MISES):
        want = st.cells(u, what)
        got = _cell_arrays(dev, sol, what, st.cn)
        assert np.array_equal(T._bits(got), T._bits(want.reshape(got.shape))), (name, what)
    assert st.cells(u, S.VON_MISES)[(0,) * len(cs["n"])] == 0.0
    for what, fields in ((S.STRAIN, sol.strain()), (S.STRESS, sol.stress()), (S.VON_MISES, (sol.von_mises(),))):
        want = st.nodes(u, what).astype(cs["dtype"])
        got = T._values(fields)
        assert got.dtype == cs["dtype"] and len(fields) == (1 if what == S.VON_MISES else len(S.voigt(len(cs["n"]))))
        assert np.array_equal(T._bits(got), T._bits(want.reshape(got.shape))), (name, what)
    assert np.array_equal(T._bits(np.float64(sol.stress_max())), T._bits(np.float64(st.norm(u, 2.0, 1.0)[1])))
    dev.close()


def _yard(f64, ld):
    return max(float(np.abs(f64.astype(LD) - ld).max()), 2.0 ** -53 * float(np.abs(ld).max()))


@pytest.mark.parametrize("name", S.AGGREGATE)
def test_the_aggregate_the_load_and_the_sensitivity_pass_to_rounding(name):
    lsm = T._lsm()
    cs = FIELD_CASES[name]
    N, n = len(cs["n"]), tuple(cs["n"])
    dev, st = _open(lsm, cs)
    b, h = dev.backend, dev._handle()
    u = _random_u(cs)
    lam = np.random.default_rng(37).standard_normal((N,) + n).astype(cs["dtype"]).astype(np.float64)
    sol, adj = dev.with_displacement(u), dev.with_displacement(lam)
    ub, lb = [c.buf for c in sol.u], [c.buf for c in adj.u]
    smax = float(st.norm(u, 2.0, 1.0)[1])
    nn = int(np.prod(n))
    worst = {}
    for p in (2.0, 3.5, 8.0, 64.0):
        for sref in (smax, 1.0):
            J, mx = b.elastic_stress_norm(h, ub, p, sref)
            assert np.array_equal(T._bits(np.float64(mx)), T._bits(np.float64(smax)))
            J64, Jld = st.norm(u, p, sref)[0], st.norm(u, p, sref, LD)[0]
            rJ = abs(LD(J) - Jld) / _yard(np.asarray(J64), np.asarray(Jld))
            f = b.elastic_stress_load(h, ub, p, sref).cpu().numpy()
            f = np.stack([f[i * nn:(i + 1) * nn].reshape(n, order="F") for i in range(N)])
            assert np.all(np.isfinite(f))
            f64, fld = st.load(u, p, sref), st.load(u, p, sref, LD)
            rf = float(np.abs(f.astype(LD) - fld).max()) / _yard(f64, fld)
            scale = 1.0 / (p * float(J64))
            g = lsm.ROCMeshField(b, sol.u[0].mesh, sol.u[0].bcs)
            b.elastic_stress_sensitivity(h, ub, lb, p, sref, scale, g.buf)
            d64, dld = st.sensitivity(u, lam, p, sref, scale), st.sensitivity(u, lam, p, sref, scale, LD)
            half = 2.0 ** -24 * np.abs(dld) if cs["dtype"] == np.float32 else 0.0      # the one rounding to a float32 field: half an ulp at most
            rd = float(np.maximum(np.abs(g.values().astype(LD) - dld) - half, 0.0).max()) / _yard(d64, dld)
            print(f"{name} p={p} sref={sref:.3g}: J′ {float(rJ):.2f}, load {rf:.2f}, sensitivity {rd:.2f} yardsticks")
            worst[p, sref] = (float(rJ), rf, rd)
    assert max(max(v) for v in worst.values()) <= 16.0, worst
    dev.close()


_REF = {}


def _reference(name, dev, st, cs):
    if name not in _REF:
        hier = T._device_hierarchy(dev, cs)
        f, u0 = cs["f"], np.zeros((len(cs["n"]),) + tuple(cs["n"]))
        direct = S.sensitivity_by(st, hier, f, u0, 8.0, cs["dtype"], "direct")
        s = st.cells(R.direct(st.op, f, u0), S.VON_MISES)
        den = float(np.sum(st.op.count * st.node_mean(8.0 * np.power(s / direct[3], 8.0))))      # Σ count·|p·r^p|
        _REF[name] = (direct, S.sensitivity_by(st, hier, f, u0, 8.0, cs["dtype"], "mg", RTOL), den)
    return _REF[name]


@pytest.mark.parametrize("name", sorted(SOLVED_CASES))
def test_stress_sensitivity_end_to_end(name):
    lsm = T._lsm()
    cs = SOLVED_CASES[name]
    dev, st = _open(lsm, cs)
    op, p = st.op, 8.0
    (dd, Gd, _, _, _, _), (dp, Gp, _, _, itu, ita), den = _reference(name, dev, st, cs)
    sol = dev.solve(cs["f"], rtol=RTOL, max_iters=3000)
    res = sol.stress_sensitivity(p=p, rtol=RTOL, max_iters=3000)
    d = res.field.values().astype(np.float64)
    err, err_ref = float(np.abs(d - dd).max()), float(np.abs(dp - dd).max())
    hom, hom_ref = abs(st.homogeneity(d)) / den, abs(st.homogeneity(dp)) / den
    print(f"{name}: G_p {res.value:.12g} (direct {Gd:.12g}, restatement's PCG {Gp:.12g}); |d − direct| {err:.3e} (restatement {err_ref:.3e}) of {np.abs(dd).max():.3e}; "
          f"homogeneity {hom:.3e} (restatement {hom_ref:.3e}); iterations state {sol.iterations}, adjoint {res.iterations} (restatement {itu}, {ita})")
    assert res.value == sol.stress_norm(p) and res.p == p and res.sref == sol.stress_max()
    assert res.adjoint.iterations == res.iterations and res.adjoint.relres <= RTOL
    lam = T._values(res.adjoint.u)
    assert not lam[op.fixed].any()      # zero on the fixed components, whatever the state prescribes
    assert err <= 4 * err_ref
    assert hom <= 4 * hom_ref
    assert res.iterations <= sol.iterations + 2
    dev.close()


@pytest.mark.parametrize("name", ["17x9_stress", "9x7x5"])
def test_the_stress_calls_leave_later_solves_and_modes_unaffected(name):
    lsm = T._lsm()
    cs = SOLVED_CASES[name]
    f2 = np.random.default_rng(41).standard_normal((len(cs["n"]),) + tuple(cs["n"]))

    def run(between):
        dev, _ = _open(lsm, cs)
        m1 = dev.modes(2, rtol=1e-6)
        a = dev.solve(cs["f"], rtol=RTOL)
        if between:
            a.strain(), a.stress(), a.von_mises(), a.stress_max(), a.stress_norm(4.0), a.stress_norm(8.0, sref=1.0)
            a.stress_sensitivity(p=8.0)
            dev.with_displacement(f2).stress_sensitivity(p=3.5, sref=2.0)
        b = dev.solve(f2, rtol=RTOL)
        m2 = dev.modes(2, rtol=1e-6)
        out = (T._values(a.u), T._values(b.u), a.iterations, b.iterations, m1.eigenvalues, m2.eigenvalues)
        dev.close()
        return out

    plain, mixed = run(False), run(True)
    for x, y in zip(plain, mixed):
        assert np.array_equal(T._bits(np.asarray(x, dtype=np.float64)), T._bits(np.asarray(y, dtype=np.float64)))


def test_with_displacement_takes_fields_and_a_zero_state_has_no_stress():
    lsm = T._lsm()
    cs = FIELD_CASES["9x12_strain_level"]
    dev, st = _open(lsm, cs)
    u = _random_u(cs)
    a = dev.with_displacement(u)
    b = dev.with_displacement(a.u)          # N ROCMeshFields: copied
    c = dev.with_displacement(tuple(u))     # N host arrays
    assert all(x.buf.data_ptr() != y.buf.data_ptr() for x, y in zip(a.u, b.u))
    want = T._bits(a.von_mises().values())
    assert np.array_equal(T._bits(b.von_mises().values()), want) and np.array_equal(T._bits(c.von_mises().values()), want)
    with pytest.raises(ValueError, match="components"):
        dev.with_displacement((u[0],))
    zero = dev.with_displacement(np.zeros_like(u))
    assert zero.stress_max() == 0.0 and zero.stress_norm() == 0.0 and zero.stress_norm(4.0, sref=1.0) == 0.0
    res = zero.stress_sensitivity()
    assert res.value == 0.0 and res.adjoint is None and res.iterations == 0 and not res.field.values().any()
    dev.close()
    with pytest.raises(ValueError, match="closed"):
        a.von_mises()


def test_the_c_abi_refuses_what_the_header_says():
    lsm = T._lsm()
    cs = FIELD_CASES["9x12_strain_level"]
    dev, st = _open(lsm, cs)
    b, h, lib = dev.backend, dev._handle(), dev.backend.lib
    u = _random_u(cs)
    sol, adj = dev.with_displacement(u), dev.with_displacement(u[::-1])
    u0, u1 = [b.ptr(c.buf) for c in sol.u]
    l0, l1 = [b.ptr(c.buf) for c in adj.u]
    outs = [lsm.ROCMeshField(b, sol.u[0].mesh, sol.u[0].bcs) for _ in range(3)]
    o0, o1, o2 = [b.ptr(c.buf) for c in outs]
    big = b.torch.zeros(3 * u[0].size, dtype=b.torch.float64, device=b.device)
    pb, res, nan, inf = b.ptr(big), (C.c_double * 2)(), float("nan"), float("inf")
    bad = [
        lib.lsm_elastic_stress_cells(h, u0, u1, None, 3, pb), lib.lsm_elastic_stress_cells(h, u0, u1, None, -1, pb),
        lib.lsm_elastic_stress_cells(h, u0, None, None, S.STRAIN, pb), lib.lsm_elastic_stress_cells(h, u0, u0, None, S.STRAIN, pb),
        lib.lsm_elastic_stress_cells(h, u0, u1, None, S.STRAIN, None), lib.lsm_elastic_stress_cells(h, u0, u1, None, S.STRAIN, u1),
        lib.lsm_elastic_stress(h, u0, u1, None, 7, o0, o1, o2, None, None, None), lib.lsm_elastic_stress(h, u0, u1, None, S.STRESS, o0, o1, None, None, None, None),
        lib.lsm_elastic_stress(h, u0, u1, None, S.STRESS, o0, o1, o1, None, None, None), lib.lsm_elastic_stress(h, u0, u1, None, S.STRAIN, o0, o1, u0, None, None, None),
        lib.lsm_elastic_stress(h, u0, u1, None, S.VON_MISES, None, None, None, None, None, None), lib.lsm_elastic_stress(h, u0, u1, None, S.VON_MISES, u1, None, None, None, None, None),
        lib.lsm_elastic_stress(h, None, u1, None, S.VON_MISES, o0, None, None, None, None, None),
    ]
    for p, sref in ((1.999, 1.0), (64.001, 1.0), (nan, 1.0), (inf, 1.0), (8.0, 0.0), (8.0, -1.0), (8.0, inf), (8.0, nan)):
        bad += [lib.lsm_elastic_stress_norm(h, u0, u1, None, p, sref, res), lib.lsm_elastic_stress_load(h, u0, u1, None, p, sref, pb),
                lib.lsm_elastic_stress_sensitivity(h, u0, u1, None, l0, l1, None, p, sref, 1.0, o0)]
    bad += [lib.lsm_elastic_stress_norm(h, u0, u0, None, 8.0, 1.0, res), lib.lsm_elastic_stress_norm(h, u0, u1, None, 8.0, 1.0, None),
            lib.lsm_elastic_stress_load(h, u0, None, None, 8.0, 1.0, pb), lib.lsm_elastic_stress_load(h, u0, u1, None, 8.0, 1.0, None),
            lib.lsm_elastic_stress_load(h, u0, u1, None, 8.0, 1.0, u0),
            lib.lsm_elastic_stress_sensitivity(h, u0, u1, None, l0, l1, None, 8.0, 1.0, inf, o0), lib.lsm_elastic_stress_sensitivity(h, u0, u1, None, l0, l1, None, 8.0, 1.0, nan, o0),
            lib.lsm_elastic_stress_sensitivity(h, u0, u1, None, l0, l0, None, 8.0, 1.0, 1.0, o0), lib.lsm_elastic_stress_sensitivity(h, u0, u1, None, l0, None, None, 8.0, 1.0, 1.0, o0),
            lib.lsm_elastic_stress_sensitivity(h, u0, u1, None, l0, l1, None, 8.0, 1.0, 1.0, None), lib.lsm_elastic_stress_sensitivity(h, u0, u1, None, l0, l1, None, 8.0, 1.0, 1.0, l1),
            lib.lsm_elastic_stress_sensitivity(h, u0, u1, None, l0, l1, None, 8.0, 1.0, 1.0, u0)]
    assert bad == [lsm._lib.ERR_INVALID] * len(bad), bad
    b.sync()
    assert not T._values(outs).any() and not big.any().item()      # nothing ran
    # the same calls with the offending argument put right go through
    assert lib.lsm_elastic_stress_norm(h, u0, u1, None, 2.0, 1.0, res) == 0 and lib.lsm_elastic_stress_norm(h, u0, u1, None, 64.0, 1.0, res) == 0
    assert lib.lsm_elastic_stress(h, u0, u1, None, S.STRESS, o0, o1, o2, None, None, None) == 0
    dev.close()
