"""Thermoelastic coupling on the device (csrc/lsm_elastic.hip through the Python API) against the restatement (tests/_thermo_ref.py) on the
device's own K0 and cell moduli.

Bit for bit, for random T, u and v (not solutions): the thermal load, the heat-adjoint source, both thermal stress cell arrays and their
node fields, and the sensitivity field with and without `minus`, with a scalar alpha and with alpha per cell, on every shape of
_stress_ref.field_cases() — 4×4, 5×4, 4×4×4, 9×12, 5×4×6, 4×6×21, both planes, a negative ν, one float32 handle (inputs rounded to float32
first, output fields rounded once) — and on the two launch shapes beyond 2048 workgroups of 256 threads (one alpha variant each).

End to end on the two smallest cases of _stress_ref.solved_cases() and the 3-D one, with a heat problem added (the face x = 0 held at 0.5,
a uniform source, the conductivity from the same ϕ): T, u, the two adjoints and the sensitivity field against the restatement with
direct solves, each under 4× what the restatement's own PCG at the same rtol leaves (tests/test_gpu_elastic.py's convention); the
elastic solve is the hand-composed elastic_op.solve(f + thermal_load(T)) bit for bit (u, iterations, relres); a given-T solve skips the
heat adjoint; uniform heating on rollers reaches ε*·(x − lc) under the same bar.

The new calls between two solves of either operator change no bit of either; the C ABI refuses what include/lsm.h says it refuses."""
import numpy as np
import pytest

import _elastic_ref as R
import _elliptic_many_ref as EM
import _elliptic_ref as EL
import _stress_ref as S
import _thermo_ref as TH
import test_gpu_elastic as T

pytestmark = pytest.mark.gpu

FIELD_CASES = S.field_cases()
SOLVED_CASES = S.solved_cases()
RTOL = 1e-8
T_REF = 0.25


def _open(lsm, cs, alpha, t_ref=T_REF):
    """(the device operator, the restatement of the coupling on its K0 and cells)"""
    dev = lsm.ElasticityOperator(T._field(lsm, cs), **T._kwargs(cs))
    return dev, TH.coupling(dev.cells(), cs["h"], cs["nu"], cs["plane"], cs["bits"], alpha, t_ref, dev.stiffness(0))


def _round(a, cs):
    return np.asarray(a).astype(cs["dtype"]).astype(np.float64)


def _device_field(lsm, dev, a):
    f = lsm.ROCMeshField(dev.backend, dev.mesh, dev.bcs)
    f.copy_(np.asfortranarray(a))
    return f


def _alphas(cs, name):
    """the scalar and the per-cell expansion coefficient (host); a big shape runs one of them"""
    cn = tuple(m - 1 for m in cs["n"])
    cells = np.asfortranarray(0.5 + np.random.default_rng(43).random(cn))
    return {"1025x600": [cells], "96x96x64": [0.8]}.get(name, [0.8, cells])


def _nodes(flat, n, comps):
    nn = int(np.prod(n))
    return np.stack([flat[k * nn:(k + 1) * nn].reshape(n, order="F") for k in range(comps)])


@pytest.mark.parametrize("name", sorted(FIELD_CASES))
def test_every_pass_is_the_restatements_bits(name):
    lsm = T._lsm()
    cs = FIELD_CASES[name]
    N, n = len(cs["n"]), tuple(cs["n"])
    M = N * (N + 1) // 2
    rng = np.random.default_rng(47)
    u, v = _round(rng.standard_normal((N,) + n), cs), _round(rng.standard_normal((N,) + n), cs)
    temp, minus = _round(rng.standard_normal(n), cs), _round(rng.standard_normal(n), cs)
    for alpha in _alphas(cs, name):
        dev, th = _open(lsm, cs, alpha)
        b, h = dev.backend, dev._handle()
        a_dev = alpha if np.ndim(alpha) == 0 else b.node_array(alpha, "alpha", th.st.cn)
        su, sv = dev.with_displacement(u), dev.with_displacement(v)
        ub, vb = [c.buf for c in su.u], [c.buf for c in sv.u]
        tf, mf = _device_field(lsm, dev, temp), _device_field(lsm, dev, minus)
        tag = (name, "scalar" if np.ndim(alpha) == 0 else "cells")

        got = _nodes(b.elastic_thermal_load(h, tf.buf, T_REF, a_dev).cpu().numpy(), n, N)
        assert np.array_equal(T._bits(got), T._bits(th.load(temp))), tag
        got = b.elastic_thermal_source(h, vb, a_dev).cpu().numpy().reshape(n, order="F")
        assert np.array_equal(T._bits(got), T._bits(th.source(v))), tag
        nc = int(np.prod(th.st.cn))
        for what, comps in ((S.STRESS, M), (S.VON_MISES, 1)):
            flat = b.elastic_thermal_stress_cells(h, ub, tf.buf, T_REF, a_dev, what).cpu().numpy()
            assert flat.size == comps * nc
            want = th.stress_cells(u, temp, what)
            assert np.array_equal(T._bits(flat), T._bits(np.concatenate([x.reshape(-1, order="F") for x in want.reshape((comps,) + th.st.cn)]))), tag + (what,)
            outs = [lsm.ROCMeshField(b, dev.mesh, dev.bcs) for _ in range(comps)]
            b.elastic_thermal_stress(h, ub, tf.buf, T_REF, a_dev, what, [c.buf for c in outs])
            got = T._values(outs)
            want = th.stress_nodes(u, temp, what).astype(cs["dtype"]).reshape(got.shape)
            assert got.dtype == cs["dtype"] and np.array_equal(T._bits(got), T._bits(want)), tag + (what,)
        g = lsm.ROCMeshField(b, dev.mesh, dev.bcs)
        d = th.sensitivity(u, v, temp)
        for mfield, want in ((None, d), (mf, d - minus)):      # the restatement's definition of `minus` (tests/test_thermo_host.py pins it)
            b.elastic_thermal_sensitivity(h, ub, vb, tf.buf, T_REF, a_dev, None if mfield is None else mfield.buf, g.buf)
            assert np.array_equal(T._bits(g.values()), T._bits(want.astype(cs["dtype"]))), tag + (mfield is not None,)
        dev.close()


# ---- end to end

def _heat_kwargs(cs):
    return dict(a_in=1.0, a_out=1e-3, dirichlet=(EL.face_mask(tuple(cs["n"]), 0, 0), 0.5), level=cs.get("level", 0.0))


def _objective_load(cs):
    """l: a unit traction along x on the face opposite the clamp — l·u is the mean axial displacement of the tip"""
    t = [0.0] * len(cs["n"])
    t[0] = 1.0
    return R.traction(cs["n"], cs["h"], 0, 1, t)


def _alpha_of(name, cs):
    if name == "17x9_strain":
        return np.asfortranarray(1e-2 * (0.5 + np.random.default_rng(53).random(tuple(m - 1 for m in cs["n"]))))
    return 1e-2


def _coupled(th, eh, hh, cs, f, l, u0, solver):
    """(T, u, v, w, d) of the restatement with solver = "direct" (the reference) or its own PCG at RTOL (T, u, v, w, minus and d rounded to the
    storage type, as the handle stores them)"""
    eop, hop = eh.ops[0], hh.ops[0]
    rnd = (lambda a: np.asarray(a, dtype=np.float64)) if solver == "direct" else (lambda a: _round(a, cs))

    def heat(src, t0):
        if solver == "direct":
            return EL.direct(hop, src, t0)
        x, _, _, ok = EL.pcg(hh, src, t0, RTOL, 3000, "mg")
        assert ok
        return x

    def elastic(load, x0):
        if solver == "direct":
            return R.direct(eop, load, x0)
        x, _, _, ok = R.pcg(eh, load, x0, RTOL, 3000, "mg")
        assert ok
        return x

    temp = rnd(heat(1.0, np.where(hop.fixed, 0.5, 0.0)))
    u = rnd(elastic(np.asarray(f, dtype=np.float64) + th.load(temp), u0))
    v = rnd(elastic(l, np.zeros_like(u0)))
    w = rnd(heat(th.source(v), np.zeros(hop.n)))
    d = rnd(th.sensitivity(u, v, temp, rnd(EM.energy_mutual(hop, temp, w))))
    return temp, u, v, w, d


_REF = {}


def _reference(name, dev, hdev, th, cs, f, l):
    if name not in _REF:
        eh = T._device_hierarchy(dev, cs)
        hop = EL.Operator(hdev.cells(), cs["h"], 0.0, EL.face_mask(tuple(cs["n"]), 0, 0))
        hh = EL.Hierarchy(hop)
        u0 = R.build_case(cs)[2]
        _REF[name] = (_coupled(th, eh, hh, cs, f, l, u0, "direct"), _coupled(th, eh, hh, cs, f, l, u0, "mg"), hop)
    return _REF[name]


@pytest.mark.parametrize("name", ["17x9_stress", "17x9_strain", "9x7x5"])
def test_solve_and_sensitivity_end_to_end(name):
    lsm = T._lsm()
    cs = SOLVED_CASES[name]
    alpha = _alpha_of(name, cs)
    phi = T._field(lsm, cs)
    dev = lsm.ElasticityOperator(phi, **T._kwargs(cs))
    hdev = lsm.EllipticOperator(phi, **_heat_kwargs(cs))
    th = TH.coupling(dev.cells(), cs["h"], cs["nu"], cs["plane"], cs["bits"], alpha, T_REF, dev.stiffness(0))
    f, l = cs["f"], _objective_load(cs)
    direct, pcg, hop = _reference(name, dev, hdev, th, cs, f, l)
    co = lsm.Thermoelastic(hdev, dev, alpha=alpha, T_ref=T_REF)
    sol = co.solve(1.0, f, rtol=RTOL, max_iters=3000)
    res = sol.sensitivity(l, rtol=RTOL, max_iters=3000)
    assert sol.temperature is not None and sol.T is sol.temperature.u and sol.coupling is co
    got = (sol.T.values(), T._values(sol.displacement.u), T._values(res.adjoint.u), res.heat_adjoint.u.values(), res.field.values())
    for what, x, xd, xp in zip(("T", "u", "v", "w", "d"), got, direct, pcg):
        err, ref = float(np.abs(x.astype(np.float64) - xd).max()), float(np.abs(xp - xd).max())
        print(f"{name} {what}: |device − direct| {err:.3e} (restatement's PCG {ref:.3e}) of {np.abs(xd).max():.3e}")
        assert err <= 4 * ref, (name, what)
    assert res.iterations == res.adjoint.iterations and res.heat_iterations == res.heat_adjoint.iterations
    assert res.adjoint.relres <= RTOL and res.heat_adjoint.relres <= RTOL
    assert not T._values(res.adjoint.u)[th.op.fixed].any() and not res.heat_adjoint.u.values()[hop.fixed].any()
    u64 = got[1].astype(np.float64)
    want = R.compliance(th.op, l, u64)
    assert abs(res.value - want) <= 1e-12 * float(np.prod(cs["h"])) * float(np.abs(R.rhs(th.op, l) * u64).sum())
    # the elastic solve is the hand-composed one, bit for bit
    hand = dev.solve(dev._load(f) + co.thermal_load(sol.T), rtol=RTOL, max_iters=3000)
    assert np.array_equal(T._bits(T._values(hand.u)), T._bits(got[1]))
    assert (hand.iterations, hand.relres) == (sol.displacement.iterations, sol.displacement.relres)
    # the thermal stress of the solution is the restatement's of the device's T and u
    temp64 = got[0].astype(np.float64)
    want = th.stress_nodes(u64, temp64, S.STRESS).astype(cs["dtype"])
    assert np.array_equal(T._bits(T._values(sol.stress())), T._bits(want))
    assert np.array_equal(T._bits(sol.von_mises().values()), T._bits(th.stress_nodes(u64, temp64, S.VON_MISES).astype(cs["dtype"])))
    # a given temperature does not depend on the design: no heat adjoint, nothing subtracted
    given = co.solve(T=sol.T, f=f, rtol=RTOL, max_iters=3000)
    assert given.temperature is None and given.T is sol.T
    assert np.array_equal(T._bits(T._values(given.displacement.u)), T._bits(got[1]))
    gres = given.sensitivity(l, rtol=RTOL, max_iters=3000)
    assert gres.heat_adjoint is None and gres.heat_iterations == 0
    v64 = T._values(gres.adjoint.u).astype(np.float64)
    assert np.array_equal(T._bits(gres.field.values()), T._bits(th.sensitivity(u64, v64, temp64).astype(cs["dtype"])))
    with pytest.raises(ValueError, match="either"):
        co.solve(1.0, f, T=sol.T)
    co.close()


@pytest.mark.parametrize("name", ["17x9_stress", "17x9_strain", "9x7x5"])
def test_uniform_heating_on_rollers_is_the_free_expansion(name):
    lsm = T._lsm()
    base = SOLVED_CASES[name]
    n, N = tuple(base["n"]), len(base["n"])
    bits = np.zeros(n, dtype=np.uint8)
    for d in range(N):
        bits |= R.face_bits(n, d, 0, 1 << d)
    cs = dict(base, E=np.full(tuple(m - 1 for m in n), 0.7, order="F"), bits=np.asfortranarray(bits), g=np.zeros(N), f=None)
    phi = T._field(lsm, cs)
    dev = lsm.ElasticityOperator(phi, **T._kwargs(cs))
    hdev = lsm.EllipticOperator(phi, **_heat_kwargs(cs))
    alpha, temp = 1.3e-3, 3.5
    th = TH.coupling(dev.cells(), cs["h"], cs["nu"], cs["plane"], cs["bits"], alpha, T_REF, dev.stiffness(0))
    want, eps = th.free_expansion(temp - T_REF)
    co = lsm.Thermoelastic(hdev, dev, alpha=alpha, T_ref=T_REF)
    sol = co.solve(T=temp, rtol=RTOL, max_iters=3000)
    eh = T._device_hierarchy(dev, cs)
    ref, _, _, ok = R.pcg(eh, th.load(np.full(n, temp)), np.zeros((N,) + n), RTOL, 3000, "mg")
    assert ok
    err, err_ref = float(np.abs(T._values(sol.displacement.u) - want).max()), float(np.abs(ref - want).max())
    print(f"{name}: ε* {eps:.6e}, |u − ε*·x| {err:.3e} (restatement's PCG {err_ref:.3e}) of {np.abs(want).max():.3e}")
    assert err <= 4 * err_ref
    co.close()


@pytest.mark.parametrize("name", ["17x9_stress", "9x7x5"])
def test_the_thermal_calls_leave_later_solves_of_both_operators_unaffected(name):
    lsm = T._lsm()
    cs = SOLVED_CASES[name]
    n, N = tuple(cs["n"]), len(cs["n"])
    rng = np.random.default_rng(59)
    f2, q2, l = rng.standard_normal((N,) + n), rng.standard_normal(n), _objective_load(cs)

    def run(between):
        phi = T._field(lsm, cs)
        dev = lsm.ElasticityOperator(phi, **T._kwargs(cs))
        hdev = lsm.EllipticOperator(phi, **_heat_kwargs(cs))
        co = lsm.Thermoelastic(hdev, dev, alpha=1e-2, T_ref=T_REF)
        a, ta = dev.solve(cs["f"], rtol=RTOL), hdev.solve(1.0, rtol=RTOL)
        if between:
            sol = co.solve(1.0, cs["f"], rtol=RTOL)
            sol.stress(), sol.von_mises(), co.thermal_load(ta.u)
            sol.sensitivity(l, rtol=RTOL)
            co.solve(T=q2, f=f2, rtol=RTOL).sensitivity(l, rtol=RTOL)
        b, tb = dev.solve(f2, rtol=RTOL), hdev.solve(q2, rtol=RTOL)
        out = (T._values(a.u), T._values(b.u), ta.u.values(), tb.u.values(), a.iterations, b.iterations, ta.iterations, tb.iterations)
        co.close()
        return out

    plain, mixed = run(False), run(True)
    for x, y in zip(plain, mixed):
        assert np.array_equal(T._bits(np.asarray(x, dtype=np.float64)), T._bits(np.asarray(y, dtype=np.float64)))


def test_the_constructor_wants_one_backend_and_one_mesh():
    lsm = T._lsm()
    cs = SOLVED_CASES["17x9_stress"]
    phi, other = T._field(lsm, cs), T._field(lsm, cs)
    dev, hdev, hother = lsm.ElasticityOperator(phi, **T._kwargs(cs)), lsm.EllipticOperator(phi, **_heat_kwargs(cs)), lsm.EllipticOperator(other, **_heat_kwargs(cs))
    with pytest.raises(ValueError, match="backend"):
        lsm.Thermoelastic(hother, dev, alpha=1e-5)
    for bad in (float("nan"), np.full((3, 3), 1e-5), np.full(tuple(m - 1 for m in cs["n"]), np.inf)):
        with pytest.raises(ValueError, match="alpha"):
            lsm.Thermoelastic(hdev, dev, alpha=bad)
    with pytest.raises(ValueError, match="T_ref"):
        lsm.Thermoelastic(hdev, dev, alpha=1e-5, T_ref=float("inf"))
    sol = lsm.thermoelastic_solve(phi, 1.0, cs["f"], alpha=1e-2, T_ref=T_REF, heat=_heat_kwargs(cs), elastic=T._kwargs(cs), rtol=RTOL)
    ref = lsm.Thermoelastic(hdev, dev, alpha=1e-2, T_ref=T_REF).solve(1.0, cs["f"], rtol=RTOL)
    assert np.array_equal(T._bits(T._values(sol.displacement.u)), T._bits(T._values(ref.displacement.u)))
    sol.coupling.close()
    for op in (dev, hdev, hother):
        op.close()


def test_the_c_abi_refuses_what_the_header_says():
    lsm = T._lsm()
    cs = FIELD_CASES["9x12_strain_level"]
    dev, th = _open(lsm, cs, 0.8)
    b, h, lib = dev.backend, dev._handle(), dev.backend.lib
    rng = np.random.default_rng(61)
    n = tuple(cs["n"])
    su, sv = dev.with_displacement(rng.standard_normal((2,) + n)), dev.with_displacement(rng.standard_normal((2,) + n))
    u0, u1 = [b.ptr(c.buf) for c in su.u]
    v0, v1 = [b.ptr(c.buf) for c in sv.u]
    tf, mf = _device_field(lsm, dev, rng.standard_normal(n)), _device_field(lsm, dev, rng.standard_normal(n))
    tp, mp = b.ptr(tf.buf), b.ptr(mf.buf)
    outs = [lsm.ROCMeshField(b, dev.mesh, dev.bcs) for _ in range(3)]
    o0, o1, o2 = [b.ptr(c.buf) for c in outs]
    big = b.torch.zeros(3 * int(np.prod(n)), dtype=b.torch.float64, device=b.device)
    cells = b.torch.full((int(np.prod(th.st.cn)),), 0.8, dtype=b.torch.float64, device=b.device)
    pb, pc, nan, inf, a = b.ptr(big), b.ptr(cells), float("nan"), float("inf"), 0.8
    Z = (None,) * 3
    bad = [
        lib.lsm_elastic_thermal_load(h, None, 0.0, a, None, pb), lib.lsm_elastic_thermal_load(h, tp, nan, a, None, pb), lib.lsm_elastic_thermal_load(h, tp, inf, a, None, pb),
        lib.lsm_elastic_thermal_load(h, tp, 0.0, nan, None, pb), lib.lsm_elastic_thermal_load(h, tp, 0.0, inf, None, pb), lib.lsm_elastic_thermal_load(h, tp, 0.0, a, None, None),
        lib.lsm_elastic_thermal_load(h, tp, 0.0, a, None, tp), lib.lsm_elastic_thermal_load(h, tp, 0.0, a, pc, pc),
        lib.lsm_elastic_thermal_stress_cells(h, u0, u1, None, tp, 0.0, a, None, S.STRAIN, pb), lib.lsm_elastic_thermal_stress_cells(h, u0, u1, None, tp, 0.0, a, None, 3, pb),
        lib.lsm_elastic_thermal_stress_cells(h, u0, u0, None, tp, 0.0, a, None, S.STRESS, pb), lib.lsm_elastic_thermal_stress_cells(h, u0, None, None, tp, 0.0, a, None, S.STRESS, pb),
        lib.lsm_elastic_thermal_stress_cells(h, u0, u1, None, None, 0.0, a, None, S.STRESS, pb), lib.lsm_elastic_thermal_stress_cells(h, u0, u1, None, u1, 0.0, a, None, S.STRESS, pb),
        lib.lsm_elastic_thermal_stress_cells(h, u0, u1, None, tp, nan, a, None, S.STRESS, pb), lib.lsm_elastic_thermal_stress_cells(h, u0, u1, None, tp, 0.0, nan, None, S.STRESS, pb),
        lib.lsm_elastic_thermal_stress_cells(h, u0, u1, None, tp, 0.0, a, None, S.STRESS, None), lib.lsm_elastic_thermal_stress_cells(h, u0, u1, None, tp, 0.0, a, None, S.STRESS, tp),
        lib.lsm_elastic_thermal_stress(h, u0, u1, None, tp, 0.0, a, None, S.STRAIN, o0, o1, o2, *Z), lib.lsm_elastic_thermal_stress(h, u0, u1, None, tp, 0.0, a, None, -1, o0, o1, o2, *Z),
        lib.lsm_elastic_thermal_stress(h, u0, u1, None, tp, 0.0, a, None, S.STRESS, o0, o1, None, *Z), lib.lsm_elastic_thermal_stress(h, u0, u1, None, tp, 0.0, a, None, S.STRESS, o0, o1, o1, *Z),
        lib.lsm_elastic_thermal_stress(h, u0, u1, None, tp, 0.0, a, None, S.STRESS, o0, o1, u0, *Z), lib.lsm_elastic_thermal_stress(h, u0, u1, None, tp, 0.0, a, None, S.STRESS, o0, o1, tp, *Z),
        lib.lsm_elastic_thermal_stress(h, u0, u1, None, tp, 0.0, a, None, S.VON_MISES, None, None, None, *Z), lib.lsm_elastic_thermal_stress(h, u0, u1, None, None, 0.0, a, None, S.VON_MISES, o0, None, None, *Z),
        lib.lsm_elastic_thermal_stress(h, u0, u1, None, tp, inf, a, None, S.VON_MISES, o0, None, None, *Z), lib.lsm_elastic_thermal_stress(h, u0, u1, None, tp, 0.0, inf, None, S.VON_MISES, o0, None, None, *Z),
        lib.lsm_elastic_thermal_source(h, v0, v0, None, a, None, pb), lib.lsm_elastic_thermal_source(h, v0, None, None, a, None, pb), lib.lsm_elastic_thermal_source(h, v0, v1, None, nan, None, pb),
        lib.lsm_elastic_thermal_source(h, v0, v1, None, a, None, None), lib.lsm_elastic_thermal_source(h, v0, v1, None, a, None, v1),
        lib.lsm_elastic_thermal_sensitivity(h, u0, u0, None, v0, v1, None, tp, 0.0, a, None, mp, o0), lib.lsm_elastic_thermal_sensitivity(h, u0, u1, None, v0, None, None, tp, 0.0, a, None, mp, o0),
        lib.lsm_elastic_thermal_sensitivity(h, u0, u1, None, v0, v1, None, None, 0.0, a, None, mp, o0), lib.lsm_elastic_thermal_sensitivity(h, u0, u1, None, v0, v1, None, u0, 0.0, a, None, mp, o0),
        lib.lsm_elastic_thermal_sensitivity(h, u0, u1, None, v0, v1, None, tp, nan, a, None, mp, o0), lib.lsm_elastic_thermal_sensitivity(h, u0, u1, None, v0, v1, None, tp, 0.0, inf, None, mp, o0),
        lib.lsm_elastic_thermal_sensitivity(h, u0, u1, None, v0, v1, None, tp, 0.0, a, None, mp, None), lib.lsm_elastic_thermal_sensitivity(h, u0, u1, None, v0, v1, None, tp, 0.0, a, None, mp, mp),
        lib.lsm_elastic_thermal_sensitivity(h, u0, u1, None, v0, v1, None, tp, 0.0, a, None, mp, tp), lib.lsm_elastic_thermal_sensitivity(h, u0, u1, None, v0, v1, None, tp, 0.0, a, None, mp, u1),
        lib.lsm_elastic_thermal_sensitivity(h, u0, u1, None, v0, v1, None, tp, 0.0, a, None, mp, v0),
    ]
    assert bad == [lsm._lib.ERR_INVALID] * len(bad), bad
    b.sync()
    assert not T._values(outs).any() and not big.any().item()      # nothing ran
    # the same calls with the offending argument put right go through; a non-finite scalar alpha is not read beside a cell array; u and v may be the same fields
    assert lib.lsm_elastic_thermal_load(h, tp, 0.0, nan, pc, pb) == 0 and lib.lsm_elastic_thermal_source(h, v0, v1, None, nan, pc, pb) == 0
    assert lib.lsm_elastic_thermal_stress(h, u0, u1, None, tp, 0.0, a, None, S.STRESS, o0, o1, o2, *Z) == 0
    assert lib.lsm_elastic_thermal_sensitivity(h, u0, u1, None, u0, u1, None, tp, 0.0, a, None, None, o0) == 0
    b.sync()
    # a non-finite temperature propagates
    hot = rng.standard_normal(n)
    hot[3, 4] = nan
    got = _nodes(b.elastic_thermal_load(h, _device_field(lsm, dev, hot).buf, 0.0, a).cpu().numpy(), n, 2)
    assert np.isnan(got[:, 2:5, 3:6]).all() and np.isfinite(got[:, 5:, :]).all()
    dev.close()
