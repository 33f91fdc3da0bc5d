"""One FAST stage with the folded advection factor (a WENO5 line returns three times its value; the plain variants carry cdt
in the factor and sum the lines straight into the stage base) and the Eikonal tail on the undivided Godunov sum
(csrc/stage_math.h, csrc/stage_kernel.h) against the oracle: every coefficient kind the factor is folded into, every base
mode, f32 storage, the general variant with a second output, the untouched branch of unequal spacings, the band stage
with one lane per node, and three RK3 steps.

The stress fields and the separable velocity are those of test_gpu_weno_forms.py (spacing 1/8: exact zeros, -0.0, w₂ = -w₃,
both ends of FAST's range, flat data; u_d and ϕ change sign inside some waves and keep it across others), plus a field that
is zero everywhere.
"""
import numpy as np
import pytest

from test_gpu_parity import TOL_100, TOL_STAGE, _run_stage
from test_gpu_weno_forms import H, _coords, _fields, _sphere, _velocity

pytestmark = pytest.mark.gpu

SHAPES = [(40, 12, 10),    # ragged x tile, two y tiles, one short march chunk
          (70, 21, 45),
          (300, 9),
          (70,)]
_ID = lambda s: "x".join(map(str, s))

_CASES = {}


@pytest.fixture(scope="module")
def hip():
    import _hip
    yield _hip
    _CASES.clear()


def _case(hip, shape, dtype=np.float64):
    key = (shape, np.dtype(dtype).name)
    if key not in _CASES:
        nd = len(shape)
        _CASES[key] = hip.Case(shape, "neumann", lc=(0.0,) * nd, hc=tuple((n - 1) * H for n in shape), mode="fast", dtype=dtype)
    return _CASES[key]


def _all_fields(shape):
    out = _fields(shape)
    out["zero"] = np.zeros(shape, order="F")
    return out


def _velocities(shape):
    nd = len(shape)
    rng = np.random.default_rng(31)
    # a field velocity that changes sign from node to node in places and is smooth elsewhere
    cs = np.meshgrid(*_coords(shape), indexing="ij", sparse=True)
    fld = []
    for d in range(nd):
        smooth = np.broadcast_to(np.sin(1.3 * cs[d] + 0.4 * d) * np.cos(0.7 * cs[(d + 1) % nd] - 0.2), shape)
        fld.append(np.asfortranarray(smooth + 0.05 * rng.standard_normal(shape)))
    out = {"sep": _velocity(shape), "const": ("const", (0.7, -0.4, 0.9)[:nd]), "field": ("field", fld)}
    if nd >= 2:
        L = [(n - 1) * H for n in shape]
        out["rot"] = ("rot", 1.3, 0.45 * L[0], 0.55 * L[1])          # the centre inside the grid: both signs of both components
    return out


def _check(got, want, what, failures, tol=TOL_STAGE):
    scale = np.abs(want).max()
    err = np.abs(got - want).max() if np.isfinite(got).all() else np.inf
    print(f"{what:60s} max|Δ| = {err:.3e} = {err / scale if scale > 0 else err:.2e}·max|ϕ|")
    if not err <= tol * scale:
        failures.append((what, float(err), float(scale)))


@pytest.mark.parametrize("shape", SHAPES, ids=_ID)
def test_stage_on_stress_fields_every_velocity_kind(hip, orc, shape):
    """WENO5 + Eikonal (current sign), base ψ, every field × every velocity kind; the four base modes on the sphere."""
    c = _case(hip, shape)
    assert all(c.grid.meshsize(d) == H for d in range(len(shape)))
    failures = []
    fields = _all_fields(shape)
    for vname, vel in _velocities(shape).items():
        specs = [("adv", vel, "weno5"), ("eik", None)]
        for name, phi in fields.items():
            got, want, _, _ = _run_stage(c, orc, specs, phi, 0, t=0.4)
            if name == "zero":
                assert np.array_equal(got, want) and not got.any(), (vname, name)
                continue
            _check(got, want, f"{_ID(shape)} {vname} {name}", failures)
        for base_mode in (1, 2, 3):
            got, want, _, _ = _run_stage(c, orc, specs, fields["sphere"], base_mode, t=0.4)
            _check(got, want, f"{_ID(shape)} {vname} sphere base {base_mode}", failures)
    assert not failures, failures


@pytest.mark.parametrize("shape", [(40, 12, 10), (300, 9)], ids=_ID)
def test_advection_alone_and_with_frozen_sign(hip, orc, shape):
    """The folded factor without the Eikonal term (the advection sum is the whole update) and beside the frozen-sign Eikonal
    term, whose tail is the old one."""
    c = _case(hip, shape)
    failures = []
    phi = _fields(shape)["sphere"]
    for vname, vel in _velocities(shape).items():
        for base_mode in (0, 1, 2, 3):
            got, want, _, _ = _run_stage(c, orc, [("adv", vel, "weno5")], phi, base_mode, t=0.4)
            _check(got, want, f"{_ID(shape)} adv {vname} base {base_mode}", failures)
        got, want, _, _ = _run_stage(c, orc, [("adv", vel, "weno5"), ("eik", phi)], phi, 1, t=0.4)
        _check(got, want, f"{_ID(shape)} adv+frozen {vname}", failures)
    assert not failures, failures


def test_f32_storage(hip, orc):
    """float storage: the arithmetic is the fp64 one on widened values; the result is rounded to float on store."""
    shape = (40, 12, 10)
    c = _case(hip, shape, np.float32)
    phi = np.asfortranarray(_fields(shape)["sphere"].astype(np.float32).astype(np.float64))
    specs = [("adv", _velocity(shape), "weno5"), ("eik", None)]
    for base_mode in (0, 2):
        # the oracle sees the float values of both inputs (ϕⁿ = 0.9ψ + 0.01 is rounded on upload)
        got, want, _, _ = _run_stage(c, orc, specs, phi, base_mode, t=0.4)
        scale = np.abs(want).max()
        # inputs: ϕⁿ rounded to float on upload (2^-24 relative, times base_a <= 1); output rounded to float
        assert np.abs(got - want).max() <= (2.0 ** -24 + 2.0 ** -24 + TOL_STAGE) * scale, (base_mode, np.abs(got - want).max())


@pytest.mark.parametrize("shape", [(70, 21, 45), (300, 9)], ids=_ID)
def test_rk2_stage_with_second_output_runs_the_general_variant(hip, orc, shape):
    c = _case(hip, shape)
    failures = []
    for vname, vel in _velocities(shape).items():
        specs = [("adv", vel, "weno5"), ("eik", None)]
        for name in ("sphere", "saw0", "kink"):
            got, want, got2, want2 = _run_stage(c, orc, specs, _fields(shape)[name], 0, with_out2=True, t=0.4)
            _check(got, want, f"{_ID(shape)} out {vname} {name}", failures)
            _check(got2, want2, f"{_ID(shape)} out2 {vname} {name}", failures)
    assert not failures, failures


@pytest.mark.parametrize("shape", SHAPES, ids=_ID)
def test_general_variant_agrees_with_the_plain_one(hip, orc, shape):
    """LSM_STAGE_GENERIC=1 keeps Ladv and cdt·Ladv apart where the plain variant sums the lines into the base: rounding only."""
    c = _case(hip, shape)
    vels = _velocities(shape)
    vels.pop("field")                           # a field velocity has no plain variant
    bad = []
    for vname, vel in vels.items():
        specs = [("adv", vel, "weno5"), ("eik", None)]
        for name in ("sphere", "saw0", "kink", "sphere*1e+30", "constant"):
            phi = _fields(shape)[name]
            for base_mode in (0, 1, 2, 3):
                c.be.set_tuning("LSM_STAGE_GENERIC", 0)
                plain, want, _, _ = _run_stage(c, orc, specs, phi, base_mode, t=0.4)
                c.be.set_tuning("LSM_STAGE_GENERIC", 1)
                try:
                    general, _, _, _ = _run_stage(c, orc, specs, phi, base_mode, t=0.4)
                finally:
                    c.be.set_tuning("LSM_STAGE_GENERIC", 0)
                scale = np.abs(want).max()
                d = np.abs(plain - general).max()
                print(f"{_ID(shape)} {vname} {name} base {base_mode}: |plain - general| = {d / scale:.2e}·max|ϕ|")
                if not d <= 4e-16 * scale or not np.abs(general - want).max() <= TOL_STAGE * scale:
                    bad.append((vname, name, base_mode, float(d / scale)))
    assert not bad, bad


def test_unequal_spacings_take_the_old_tail(hip, orc):
    shape = (40, 12, 10)
    c = hip.Case(shape, "neumann", lc=(0.0, 0.0, 0.0), hc=(39 * 0.125, 11 * 0.25, 9 * 0.0625), mode="fast")
    assert len({c.grid.meshsize(d) for d in range(3)}) == 3
    failures = []
    xs = [np.arange(n) * c.grid.meshsize(d) for d, n in enumerate(shape)]
    X = np.meshgrid(*xs, indexing="ij")
    phi = np.asfortranarray(np.sqrt((X[0] - 2.4) ** 2 + (X[1] - 1.3) ** 2 + (X[2] - 0.3) ** 2) - 0.9)
    for vname, vel in (("const", ("const", (0.7, -0.4, 0.9))), ("rot", ("rot", 1.3, 2.0, 1.2))):
        for base_mode in (0, 2):
            got, want, _, _ = _run_stage(c, orc, [("adv", vel, "weno5"), ("eik", None)], phi, base_mode, t=0.4)
            _check(got, want, f"unequal h {vname} base {base_mode}", failures)
    assert not failures, failures


@pytest.mark.parametrize("vname", ["const", "rot"])
def test_band_stage_against_the_dense_stage_on_the_band(hip, orc, vname):
    """The band stage (one lane per band node where it applies, csrc/stage_brick.h) and the dense stage read the same array:
    on the band's nodes they evaluate the same node update."""
    from lsm_amd import _lib as L
    shape = (70, 21, 45)
    nd = len(shape)
    mk = lambda: hip.Case(shape, "neumann", lc=(0.0,) * nd, hc=tuple((n - 1) * H for n in shape), mode="fast")
    c, cd = mk(), mk()                                 # the band lives on its own handle; the dense stage runs on a second one
    be = c.be
    phi = _fields(shape)["sphere"]
    psi = c.pad(phi)
    vals = c.to_dev(psi)
    mask, halo, sa, sb = (be.alloc_mask() for _ in range(4))
    MC = 16
    tiles = be.alloc_tiles(MC)
    hlist, hcount = be.alloc_halo_list(1 << 16)
    be.band_update(vals, mask, True, 3, sa, sb, halo, tiles, MC, hlist, hcount)
    band = be.mask_to_host(mask).astype(bool)
    assert 1000 < band.sum() < band.size // 2
    psi = c.to_host(vals)                              # what both stages read
    vel = _velocities(shape)[vname]
    ot, arr = c.terms([("adv", vel, "weno5"), ("eik", None)])
    cdt = 1.7e-3
    want = np.full_like(psi, np.nan)
    orc.stage_padded(c.grid, c.bc, c.olay, ot, psi, None, want, None, L.BASE_PSI, cdt, 0.0, 0.4)
    out_b, out_d = c.to_dev(np.zeros_like(psi)), cd.to_dev(np.zeros_like(psi))
    be.stage_band(arr, 2, vals, None, out_b, None, L.BASE_PSI, cdt, 0.0, 0.4, mask, tiles, MC)
    _, arr_d = cd.terms([("adv", vel, "weno5"), ("eik", None)])
    cd.be.stage(arr_d, 2, cd.to_dev(psi), None, out_d, None, L.BASE_PSI, cdt, 0.0, 0.4)
    gb, gd, w = c.interior(c.to_host(out_b)), cd.interior(cd.to_host(out_d)), c.interior(want)
    scale = np.abs(w[band]).max()
    print(f"band {vname}: |band - dense| = {np.abs(gb[band] - gd[band]).max() / scale:.2e}, |band - oracle| = {np.abs(gb[band] - w[band]).max() / scale:.2e}")
    assert np.abs(gb[band] - w[band]).max() <= TOL_STAGE * scale
    assert np.abs(gb[band] - gd[band]).max() <= 4e-16 * scale
    assert np.all(gb[~band] == 0.0)


def test_three_rk3_steps_at_48_cubed(hip, orc):
    """Three steps of the headline equation against the oracle, at three hundredths of the 100-step bar."""
    shape = (48, 48, 48)
    c = hip.Case(shape, "neumann", lc=(0, 0, 0), hc=(1, 1, 1), mode="fast")
    x, y, z = c.grid.coords()
    s2 = lambda a: np.sin(np.pi * a) * np.sin(np.pi * a)
    s = lambda a: np.sin(2 * np.pi * a)
    tables = [[2 * s2(x), s(y), s(z)], [-s(x), s2(y), s(z)], [-s(x), s(y), s2(z)]]
    X, Y, Z = np.meshgrid(x, y, z, indexing="ij")
    phi = np.asfortranarray(np.sqrt((X - 0.35) ** 2 + (Y - 0.35) ** 2 + (Z - 0.35) ** 2) - 0.15)
    specs = [("adv", ("sep", tables, ("cos", 3.0)), "weno5"), ("eik", None)]
    ref = phi.copy(order="F")
    dense = c.dense_terms(specs)
    _, arr = c.terms(specs)
    d_phi = c.to_dev(np.nan_to_num(c.pad(phi, fill=False), nan=0.0))
    b1, b2 = c.be.alloc(), c.be.alloc()
    tc = 0.0
    for _ in range(3):
        dtc = orc.compute_cfl(c.grid, c.bc, ref, dense, tc)
        assert c.be.compute_cfl_local(arr, 2, d_phi, tc) == dtc
        dt = 0.5 * dtc
        orc.advance(orc.RK3, c.grid, c.bc, ref, dense, tc, dt)
        c.be.advance_single("rk3", arr, 2, d_phi, b1, b2, tc, dt, None)
        tc += dt
    got = c.interior(c.to_host(d_phi))
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"3 RK3 steps at 48³: max|Δ| = {err:.2e}·max|ϕ|")
    assert err <= 3 * TOL_100 / 100
