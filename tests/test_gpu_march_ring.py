"""One FAST stage of the 3-D WENO5 kernels against the oracle on shapes chosen for the march ring (csrc/stage_kernel.h,
LSM_LDS7 / LSM_ZD): seven LDS slots, one per copy of the 7-fold unrolled plane loop, and the march line carried as a register
ring of first differences with the centre values written to LDS four planes ahead.

Shapes: columns shorter than the ring and clamped at both faces, exits from each of the seven unrolled copies
((40, 12, nz), nz = 4, 5, 7, 8, 13, 15), several short march chunks with their 4-plane prologue and seams ((70, 21, 45)) and
ragged tiles in x and y ((33, 9, 23)).  lsm_create refuses grids with fewer than 4 nodes in a dimension, so the 2-plane
column is checked to be refused (tests/test_march_ring_model.py runs the ring's model on it) and 4 planes is the shortest
column that reaches the kernel.  NeumannBC clamps both march faces (the repeated plane gives an interval of exactly 0);
PeriodicBC reads the ghost planes and clamps nothing.  The separable velocity of
test_gpu_weno_forms changes the sign of its march-axis table along the column: a wave switches between the two compile-time
directions of the line from one plane to the next.  The ring serves the plain dense WENO5 + Eikonal kernels (constant, rotation
and separable velocities); the field velocity, WENO5 alone and the band keep the two-slot value ring and run beside them on the
same shapes.
"""
import numpy as np
import pytest

from test_gpu_parity import TOL_100, TOL_STAGE, _run_stage
from test_gpu_stage_tail import _velocities
from test_gpu_stage_tail import test_band_stage_against_the_dense_stage_on_the_band as _band_stage_case
from test_gpu_weno_forms import H, _fields, _velocity

pytestmark = pytest.mark.gpu

SHAPES = [(40, 12, nz) for nz in (4, 5, 7, 8, 13, 15)] + [(70, 21, 45), (33, 9, 23)]
_ID = lambda s: "x".join(map(str, s))

_CASES = {}


@pytest.fixture(scope="module")
def hip():
    import _hip
    yield _hip
    _CASES.clear()


def _case(hip, shape, bc, dtype=np.float64):
    key = (shape, bc, np.dtype(dtype).name)
    if key not in _CASES:
        _CASES[key] = hip.Case(shape, bc, lc=(0.0,) * 3, hc=tuple((n - 1) * H for n in shape), mode="fast", dtype=dtype)
    return _CASES[key]


def _check(got, want, what, failures, tol=TOL_STAGE):
    scale = np.abs(want).max()
    err = np.abs(got - want).max() if np.isfinite(got).all() else np.inf
    print(f"{what:60s} max|Δ| = {err:.3e} = {err / scale if scale > 0 else err:.2e}·max|ϕ|")
    if not err <= tol * scale:
        failures.append((what, float(err), float(scale)))


@pytest.mark.parametrize("bc", ["neumann", "periodic"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ID)
def test_stage_on_ring_shapes(hip, orc, shape, bc):
    """WENO5 + Eikonal (current sign): every stress field with the separable velocity, three of them with the other kinds, the
    four base modes on the sphere; WENO5 alone (two slots, the value ring) on the sphere."""
    c = _case(hip, shape, bc)
    assert all(c.grid.meshsize(d) == H for d in range(3))
    fields = _fields(shape)
    failures = []
    for vname, vel in _velocities(shape).items():
        specs = [("adv", vel, "weno5"), ("eik", None)]
        names = list(fields) if vname == "sep" else ["sphere", "saw2", "sphere*1e+30"]
        for name in names:
            got, want, _, _ = _run_stage(c, orc, specs, fields[name], 0, t=0.4)
            _check(got, want, f"{_ID(shape)} {bc} {vname} {name}", failures)
        got, want, _, _ = _run_stage(c, orc, [("adv", vel, "weno5")], fields["sphere"], 0, t=0.4)
        _check(got, want, f"{_ID(shape)} {bc} {vname} sphere, advection alone", failures)
    specs = [("adv", _velocity(shape), "weno5"), ("eik", None)]
    for base_mode in (1, 2, 3):
        got, want, _, _ = _run_stage(c, orc, specs, fields["sphere"], base_mode, t=0.4)
        _check(got, want, f"{_ID(shape)} {bc} sep sphere base {base_mode}", failures)
    assert not failures, failures


def test_two_plane_column_is_refused(hip):
    """(40, 12, 2): no handle, no launch — the kernel never sees a column shorter than 4 planes."""
    from lsm_amd import _lib as L
    with pytest.raises(L.LsmError, match="at least 4 nodes"):
        hip.Case((40, 12, 2), "neumann", lc=(0.0,) * 3, hc=(39 * H, 11 * H, H), mode="fast")


def test_f32_storage(hip, orc):
    shape = (40, 12, 13)
    c = _case(hip, shape, "neumann", np.float32)
    phi = np.asfortranarray(_fields(shape)["sphere"].astype(np.float32).astype(np.float64))
    specs = [("adv", _velocity(shape), "weno5"), ("eik", None)]
    for base_mode in (0, 2):
        got, want, _, _ = _run_stage(c, orc, specs, phi, base_mode, t=0.4)
        scale = np.abs(want).max()
        # ϕⁿ rounded to float on upload (2^-24 relative, times base_a <= 1); the output rounded to float
        assert np.abs(got - want).max() <= (2.0 ** -24 + 2.0 ** -24 + TOL_STAGE) * scale, (base_mode, np.abs(got - want).max())


@pytest.mark.parametrize("bc", ["neumann", "periodic"])
@pytest.mark.parametrize("shape,mb,me", [((70, 21, 45), 5, 38), ((40, 12, 15), 3, 11), ((40, 12, 15), 6, 7)], ids=lambda v: str(v))
def test_plane_range_strictly_inside_the_grid(hip, orc, shape, mb, me, bc):
    """lsm_stage_planes on [mb, me), as the slab steps use it: the planes of the range equal the full stage's, the others stay."""
    from lsm_amd import _lib as L
    c = _case(hip, shape, bc)
    phi = _fields(shape)["saw2"]
    failures = []
    for vname in ("sep", "field"):
        specs = [("adv", _velocities(shape)[vname], "weno5"), ("eik", None)]
        ot, arr = c.terms(specs)
        psi = c.pad(phi)
        phin = c.pad(np.asfortranarray(phi * 0.9 + 0.01))
        cdt = 1.7e-3
        want = np.full_like(psi, np.nan)
        orc.stage_padded(c.grid, c.bc, c.olay, ot, psi, phin, want, None, L.BASE_RK3_S2, cdt, 0.0, 0.4)
        d_out = c.to_dev(np.zeros_like(psi))
        c.be.stage_planes(arr, len(specs), c.to_dev(psi), c.to_dev(phin), d_out, None, L.BASE_RK3_S2, cdt, 0.0, 0.4, mb, me)
        got, w = c.interior(c.to_host(d_out)), c.interior(want)
        _check(got[:, :, mb:me], w[:, :, mb:me], f"{_ID(shape)} {bc} {vname} planes [{mb}, {me})", failures)
        assert not got[:, :, :mb].any() and not got[:, :, me:].any()
    assert not failures, failures


@pytest.mark.parametrize("vname", ["const", "rot"])
def test_band_stage(hip, orc, vname):
    """The band stage of test_gpu_stage_tail (one lane per band node, and the dense stage it is compared with) on (70, 21, 45)."""
    _band_stage_case(hip, orc, vname)


def test_three_rk3_steps(hip, orc):
    """Three RK3 steps of WENO5 + Eikonal on (70, 21, 45), three 16-plane chunks, at three hundredths of the 100-step bar."""
    shape = (70, 21, 45)
    c = _case(hip, shape, "neumann")
    phi = _fields(shape)["sphere"]
    specs = [("adv", _velocity(shape), "weno5"), ("eik", None)]
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
    print(f"3 RK3 steps at {_ID(shape)}: max|Δ| = {err:.2e}·max|ϕ|")
    assert err <= 3 * TOL_100 / 100
