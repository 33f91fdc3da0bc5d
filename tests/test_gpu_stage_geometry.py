"""Oracle parity of the stage kernels at the launch shapes a LARGE grid takes.

`launch_tiled` (stage_kernel.h) shortens the march chunk from 64 planes to 8 until a 3-D launch has 2048 tiles, and the graded
tail (static, or dynamic through the ticket counters) needs chunks longer than 16 planes and four chunk layers: on the grids
of tests/test_gpu_parity.py, tests/test_gpu_f32.py and the goldens none of that is ever on, and `launch_pairs` leaves 8-plane
chunks only from about 512³ on.  This module compares `lsm_stage`, `lsm_stage_planes` and `lsm_advance_rk3` with the CPU
oracle (`oracle.stage_padded`, `oracle.advance`) on rough, non-symmetric fields

  1. on grids of 10⁵–10⁶ nodes with the large-grid geometry FORCED through the tuning switches (`LSM_STAGE_MC`,
     `LSM_STAGE_TAIL`, `LSM_STAGE_TAIL_DYN`, `LSM_STAGE_MC2`; `launch_pairs` honours `LSM_STAGE_MC` for this), edge values of
     the switches included;
  2. with DEFAULT tuning at 250 × 253 × 250 and at the headline's 512³, where the defaults turn those paths on, the oracle
     running on up to 16 threads (asserted bitwise equal to its one-thread run here).

Every interior node of every case is compared.  Tolerances are the project's: STRICT bitwise for every combination without a
curvature term; 1e-13·max|want| per stage otherwise and 3× that for an RK3 step; float32 storage equal to the rounded fp64
oracle in STRICT and within 2.4e-7·max|want| in FAST.

Which path a launch takes cannot be seen from its result.  tests/_stage_geometry.py mirrors the launch arithmetic and states
each case's class, tests/test_stage_geometry_table.py asserts the claims without a GPU, and
profiles/stage_geometry/kernel_trace_summary.json records one `rocprofv3 --kernel-trace` run on an MI355X in which the
workgroup count of one launch per class (mc 64, static tail, dynamic tail, pairs at mc > 8, 2-D) equals the mirror's.

A check of the checks (tried once on a scratch build, not committed): with the tail tiles of `stage_tile` handing `node_update`
the march line's entry G + 1 instead of G as the centre value — values only, every address as it is — all 144 cases here that
launch a tail fail (first mismatch in the first tail chunk, e.g. plane 128 of dyn25_mc32) while the 32 without one, and all of
tests/test_gpu_parity.py and tests/test_gpu_f32.py, still pass.

Cost, measured once on an MI355X host with the oracle on 16 threads (pytest --durations): the forced-geometry cases 9 s together,
250 × 253 × 250 12 s (three tests), the 512³ headline step 7 s, the three 512³ single-term stages 4 s each — 40 s in all, against
91 s of tests/test_gpu_fullsize.py in the same run.  The 512³ single-term stages therefore stay at 512³.
"""
import ctypes as C

import numpy as np
import pytest

import _stage_geometry as G
from test_gpu_parity import PAIRS, TOL_STAGE, _fix_specs, _rand_field

pytestmark = pytest.mark.gpu

F32 = np.float32
TOL_F32_FAST = 2.4e-7          # test_pair_kernels_match_the_oracle_and_the_one_node_kernels
SENTINEL = -7.25               # exact in float32; no result of these fields comes near it
CDT, CDT2 = 1.7e-3, 0.85e-3

BC_N = "neumann"
BC_P = ["neumann", "symmetry", "periodic"]                                   # march axis periodic: ghost planes read on both faces
BC_EN = ["periodic", "neumann", (("extrapolation", 2), "neumann")]           # weighted ghosts below, NeumannBC above
BC_NE = ["neumann", "periodic", ("neumann", ("extrapolation", 2))]           # ... and the other way round: the last tail chunk looks ahead into them
BCS3 = [BC_N, BC_P, BC_EN, BC_NE]
_bcid = lambda b: str(b).replace(" ", "").replace("'", "")


@pytest.fixture(scope="module")
def hip():
    import _hip
    return _hip


def _nthreads(orc):
    return min(16, orc.max_threads())


@pytest.fixture(scope="module", autouse=True)
def threaded_orc(orc):
    """The whole module runs the oracle on up to 16 threads (its node loop is pointwise: test_threaded_oracle_is_the_one_thread_oracle
    asserts the results equal the one-thread run's bit for bit), and on one again afterwards."""
    orc.set_threads(_nthreads(orc))
    yield orc
    orc.set_threads(1)


def _r32(p):
    return p.astype(F32).astype(np.float64)


def _rough(shape, seed, dtype=np.float64):
    phi = _rand_field(shape, seed, smooth=False)
    return np.asfortranarray(_r32(phi)) if np.dtype(dtype) == F32 else phi


def _tables(c):
    """SEPARABLE velocity whose components change sign inside waves and across them (test_plain_and_general_kernel_variants_agree)."""
    s2 = lambda a: np.sin(np.pi * a) * np.sin(np.pi * a)
    s = lambda a: np.sin(2 * np.pi * a)
    return [[(2 * s2(x) if k == d else (-1) ** d * s(x)) for k, x in enumerate(c.grid.coords())] for d in range(c.nd)]


def _terms(name, c, phi, seed=5):
    nd = c.nd
    if name == "sep+eik":                                                     # the headline pair: WENO5 by a SEPARABLE·cos field + Eikonal
        return [("adv", ("sep", _tables(c), ("cos", 3.0)), "weno5"), ("eik", None)]
    if name == "rot+eik":                                                     # ... by a ROTATION field, frozen sign
        return [("adv", ("rot", 1.3, 0.45, 0.55), "weno5"), ("eik", phi)]
    if name == "nm+curv":                                                     # BASELINE config 3's pair: the LDS ring with LEAD = 1
        return [("nm", ("const", (0.1,))), ("curv", ("const", (-0.1,)))]
    if name == "all4":                                                        # two passes
        return [("adv", ("rot", 1.0, 0.5, 0.5), "weno5"), ("eik", None), ("nm", ("const", (0.3,))), ("curv", ("const", (-0.05,)))]
    if name == "field":                                                       # FIELD coefficients: the general kernel variant
        rng = np.random.default_rng(seed)
        u = [np.asfortranarray(rng.standard_normal(c.grid.shape)) for _ in range(nd)]
        return [("adv", ("field", u), "weno5"), ("nm", ("field", [np.asfortranarray(rng.standard_normal(c.grid.shape))]))]
    return _fix_specs(PAIRS[name], nd, phi)


def _has_curv(specs):
    return any(s[0] == "curv" for s in specs)


class _Stage:
    """One lsm_stage problem: inputs on both sides, the oracle's result per base mode (computed once), GPU launches at will."""

    def __init__(self, c, orc, specs, phi, out2=False, t=0.4):
        self.c, self.orc, self.specs, self.out2, self.t = c, orc, specs, out2, t
        self.ot, self.arr = c.terms(specs)
        r = _r32 if c.dtype == F32 else (lambda p: p)
        self.psi = r(c.pad(phi))                                              # what the device holds
        self.phin = r(c.pad(np.asfortranarray(phi * 0.9 + 0.01)))
        self.d_psi, self.d_phin = c.to_dev(self.psi), c.to_dev(self.phin)
        self._want = {}
        inside = np.zeros(int(c.lay.total))
        c._view(inside)[tuple(slice(int(c.olay.g[d]), int(c.olay.g[d] + c.olay.n[d])) for d in range(c.nd))] = 1.0
        self._g = int(c.olay.g[c.nd - 1])
        self._inside = inside

    def want(self, base_mode):
        if base_mode not in self._want:
            c = self.c
            w = np.full_like(self.psi, np.nan)
            w2 = np.full_like(self.psi, np.nan) if self.out2 else None
            self.orc.stage_padded(c.grid, c.bc, c.olay, self.ot, self.psi, self.phin, w, w2, base_mode, CDT, CDT2, self.t)
            self._want[base_mode] = (c.interior(w), c.interior(w2) if self.out2 else None)
        return self._want[base_mode]

    def run(self, base_mode, planes=None, stream=None):
        """Launch into sentinel-filled outputs; returns the interiors and asserts that nothing outside the plane range was written."""
        c = self.c
        n = c.grid.shape[-1]
        m0, m1 = planes or (0, n)
        outs = [c.be.alloc() for _ in range(2 if self.out2 else 1)]
        for o in outs:
            o.fill_(SENTINEL)                                                 # the alignment padding of the layout too
        args = (c.be.h, self.arr, len(self.specs), c.be.ptr(self.d_psi), c.be.ptr(self.d_phin), c.be.ptr(outs[0]),
                c.be.ptr(outs[1]) if self.out2 else None, base_mode, CDT, CDT2, self.t)
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else None
        if stream is not None:
            c.torch.cuda.synchronize()                                        # the sentinel fill ran on torch's stream
        from lsm_amd import _lib as L
        if planes is None and stream is None:
            c.be.stage(self.arr, len(self.specs), self.d_psi, self.d_phin, outs[0], outs[1] if self.out2 else None, base_mode, CDT, CDT2, self.t)
        elif planes is None:
            L.check(c.be.h, c.be.lib.lsm_stage(*args, sp), "lsm_stage")
        else:
            L.check(c.be.h, c.be.lib.lsm_stage_planes(*args, m0, m1, sp), "lsm_stage_planes")
        if stream is not None:
            stream.synchronize()
        res = []
        for o in outs:
            flat = o.cpu().numpy().astype(np.float64)
            written = self._inside.copy()
            v = c._view(written)
            idx = [slice(None)] * c.nd
            idx[-1] = slice(0, self._g + m0)
            v[tuple(idx)] = 0.0
            idx[-1] = slice(self._g + m1, None)
            v[tuple(idx)] = 0.0
            stray = (written == 0.0) & (flat != SENTINEL)
            assert not stray.any(), f"{int(stray.sum())} elements outside planes [{m0}, {m1}) of the interior were written (first flat index {int(np.argmax(stray))})"
            res.append(c.interior(np.asfortranarray(c._view(flat).copy())))
        return res[0], (res[1] if self.out2 else None)


def _report(bad, got, want, launch, m_off):
    """Where a comparison failed: count, the first mismatching node (lowest plane first), its chunk, the planes touched."""
    idx = np.argwhere(bad)
    first = idx[np.lexsort(tuple(idx[:, d] for d in range(idx.shape[1])))[0]]          # lowest plane (row in 2-D) first
    planes = np.unique(idx[:, -1]) + m_off
    msg = f"{len(idx)} nodes differ; first {tuple(int(i) for i in first)} (+{m_off} along the march axis): got {got[tuple(first)]!r} want {want[tuple(first)]!r}; " \
          f"planes {planes.min()}..{planes.max()} ({len(planes)} of them: {planes[:12].tolist()}...)"
    if launch is not None:
        k, ch = launch.chunk_of(int(first[-1]) + m_off)
        msg += f"; chunk {k} = planes [{ch[0]}, {ch[1]}) {'TAIL' if ch[2] else 'long'} of {launch.kernel} mc {launch.mc} tail {launch.tail} {launch.mc_tail}"
    return msg


def _assert_parity(got, want, mode, curv, f32=False, launch=None, m_off=0, label="", factor=1.0):
    scale = float(np.abs(want).max())
    if f32:
        w = _r32(want)
        bad = (got != w) if mode == "strict" and not curv else ~(np.abs(got - w) <= TOL_F32_FAST * scale)
        want = w
    elif mode == "strict" and not curv:
        bad = got != want
    else:
        bad = ~(np.abs(got - want) <= factor * TOL_STAGE * scale)
    err = float(np.nanmax(np.abs(got - want)))
    print(f"{label}: max|Δ| = {err:.3e} ({err / scale:.2e} of max|want|)")
    assert not bad.any(), f"{label}: max|Δ| = {err:.3e}; " + _report(bad, got, want, launch, m_off)


def _set(c, tuning):
    for k, v in tuning.items():
        c.be.set_tuning(k, v)


def _check_stage(st, mode, base_modes, tuning, launch, planes=None, label="", stream=None):
    c = st.c
    _set(c, tuning)
    f32 = c.dtype == F32
    m0, m1 = planes or (0, c.grid.shape[-1])
    for bm in base_modes:
        want, want2 = st.want(bm)
        got, got2 = st.run(bm, planes=planes, stream=stream)
        sl = (Ellipsis, slice(m0, m1))
        _assert_parity(got[sl], want[sl], mode, _has_curv(st.specs), f32, launch, m0, f"{label} base {bm}")
        if st.out2:
            _assert_parity(got2[sl], want2[sl], mode, _has_curv(st.specs), f32, launch, m0, f"{label} base {bm} out2")


# ---- the reference stays the reference ----------------------------------------------------------------------------------

def test_threaded_oracle_is_the_one_thread_oracle(hip, orc):
    shape = (45, 38, 33)
    c = hip.Case(shape, BC_EN, lc=(0.0,) * 3, hc=(1.0,) * 3, mode="strict")
    phi = _rough(shape, 31)
    res = {}
    try:
        for nt in (1, _nthreads(orc)):
            orc.set_threads(nt)
            for name in ("sep+eik", "nm+curv"):
                specs = _terms(name, c, phi)
                ot, _ = c.terms(specs)
                psi, phin = c.pad(phi), c.pad(np.asfortranarray(0.9 * phi + 0.01))
                w = np.full_like(psi, np.nan)
                orc.stage_padded(c.grid, c.bc, c.olay, ot, psi, phin, w, None, 2, CDT, 0.0, 0.4)
                ref = phi.copy(order="F")
                orc.advance(orc.RK3, c.grid, c.bc, ref, c.dense_terms(specs), 0.1, 2.0e-3)
                cfl = orc.compute_cfl(c.grid, c.bc, phi, c.dense_terms(specs), 0.1)
                res[nt, name] = (c.interior(w), ref, cfl)
    finally:
        orc.set_threads(_nthreads(orc))                                       # the module's setting (threaded_orc)
    for name in ("sep+eik", "nm+curv"):
        a, b = res[1, name], res[_nthreads(orc), name]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and not np.isnan(a[0]).any(), name


# ---- 1. forced geometry on small grids ------------------------------------------------------------------------------------

_ROWS = [k for k, v in G.GEOMETRY.items() if v[1] is None]


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("row", _ROWS)
def test_headline_pair_under_forced_geometry(hip, orc, mode, row):
    """WENO5 advection by a SEPARABLE·cos velocity + Eikonal on every row of the geometry table (tests/_stage_geometry.py): long
    chunks of 64 / 32 / 24 / 14 / 7 / 1 planes, static and dynamic tails of 16 / 7 / 5 / 1 planes, with and without spare
    workgroups, 3 and 4 chunk layers; the march-axis boundary kind changes from row to row."""
    shape, _, tuning, _ = G.GEOMETRY[row]
    bc = BCS3[_ROWS.index(row) % 4]
    c = hip.Case(shape, bc, lc=(0.0,) * 3, hc=(1.0,) * 3, mode=mode)
    phi = _rough(shape, 40 + _ROWS.index(row))
    st = _Stage(c, orc, _terms("sep+eik", c, phi), phi)
    launch = G.launch(shape, G.COMBO_HEADLINE, mode=mode, tuning=tuning)
    base_modes = (0, 1, 2, 3) if row in ("dyn25_mc32", "static_mc32", "dyn_mc64", "tail7") else (0, 2)
    _check_stage(st, mode, base_modes, tuning, launch, label=f"{row} {mode}")


TERM_ROWS = ["dyn25_mc32", "static_mc32", "static_mc64", "tail5", "mc7_static"]


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("row", TERM_ROWS)
@pytest.mark.parametrize("terms", ["rot+eik", "nm+curv", "all4", "field"])
def test_term_combinations_under_forced_geometry(hip, orc, mode, row, terms):
    """The other kernels of the family on long chunks and tails: ROTATION velocity with a frozen sign, NormalMotion + curvature (three
    LDS planes resident), the four-term stage in two passes, FIELD coefficients (general variant) — each with every march-axis
    boundary kind."""
    shape, _, tuning, _ = G.GEOMETRY[row]
    for bc in (BCS3[(TERM_ROWS.index(row) + k) % 4] for k in range(2)):
        c = hip.Case(shape, bc, lc=(0.0,) * 3, hc=(1.0,) * 3, mode=mode)
        phi = _rough(shape, 60 + TERM_ROWS.index(row))
        specs = _terms(terms, c, phi)
        st = _Stage(c, orc, specs, phi)
        launch = G.launches(shape, specs, mode=mode, tuning=tuning)[0]
        assert launch.kernel == "tiled" and launch.tail == G.GEOMETRY[row][3]["tail"]
        _check_stage(st, mode, (0, 2) if terms != "nm+curv" else (0, 1, 2, 3), tuning, launch, label=f"{terms} {row} {_bcid(bc)} {mode}")


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("row", ["dyn25_mc32", "static_mc32", "dyn_mc64"])
def test_second_output_and_generic_variant_under_forced_geometry(hip, orc, mode, row):
    """`out2` (RK2's second accumulation; in FAST it takes the general kernel variant) and LSM_STAGE_GENERIC 0 / 1."""
    shape, _, tuning, _ = G.GEOMETRY[row]
    c = hip.Case(shape, BC_EN, lc=(0.0,) * 3, hc=(1.0,) * 3, mode=mode)
    phi = _rough(shape, 70)
    launch = G.launch(shape, G.COMBO_HEADLINE, mode=mode, tuning=tuning)
    st2 = _Stage(c, orc, _terms("sep+eik", c, phi), phi, out2=True)
    _check_stage(st2, mode, (0, 3), tuning, launch, label=f"out2 {row} {mode}")
    st4 = _Stage(c, orc, _terms("all4", c, phi), phi, out2=True)              # the second pass accumulates into out2
    _check_stage(st4, mode, (0,), tuning, launch, label=f"out2 all4 {row} {mode}")
    for name in ("sep+eik", "rot+eik", "nm+curv"):
        st = _Stage(c, orc, _terms(name, c, phi), phi)
        for generic in (1, 0):
            _check_stage(st, mode, (0, 2), dict(tuning, LSM_STAGE_GENERIC=generic), launch, label=f"generic {generic} {name} {row} {mode}")


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("row", ["dyn25_mc32", "static_mc32", "tail7_x3", "mc7"])
def test_float32_storage_under_forced_geometry(hip, orc, mode, row):
    """float32 storage (values widen on load, fp64 arithmetic, one rounding on store): STRICT equals the rounded fp64 oracle."""
    shape, _, tuning, _ = G.GEOMETRY[row]
    c = hip.Case(shape, BC_NE, lc=(0.0,) * 3, hc=(1.0,) * 3, mode=mode, dtype=F32)
    phi = _rough(shape, 80, F32)
    st = _Stage(c, orc, _terms("sep+eik", c, phi), phi)
    _check_stage(st, mode, (0, 1, 2), tuning, G.launch(shape, G.COMBO_HEADLINE, mode=mode, tuning=tuning), label=f"f32 {row} {mode}")


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("row", ["planes_dyn", "planes_dyn8", "planes_static"])
@pytest.mark.parametrize("terms", ["sep+eik", "nm+curv"])
def test_plane_ranges_with_a_tail_write_their_planes_only(hip, orc, mode, row, terms):
    """lsm_stage_planes on a range that starts inside the grid and is long enough for the tail: the planes of the range equal the
    oracle's, and every other element of the output — planes outside the range, ghost layers, alignment padding — still holds
    the sentinel it was filled with (`_Stage.run`)."""
    shape, planes, tuning, _ = G.GEOMETRY[row]
    c = hip.Case(shape, BC_P if terms == "sep+eik" else BC_EN, lc=(0.0,) * 3, hc=(1.0,) * 3, mode=mode)
    phi = _rough(shape, 90)
    specs = _terms(terms, c, phi)
    launch = G.launches(shape, specs, mode=mode, tuning=tuning, mb=planes[0], me=planes[1])[0]
    _check_stage(_Stage(c, orc, specs, phi), mode, (0, 2), tuning, launch, planes=planes, label=f"{terms} {row} {mode}")


@pytest.mark.parametrize("mode", ["strict", "fast"])
def test_ticket_ring_alternating_geometries(hip, orc, mode):
    """44 launches in a row on one handle, alternating two plane ranges whose dynamic tails draw 16 and 8 tickets — every slot of
    the 16-counter ring serves both — with a launch on a caller's stream (static tail) in between: a counter left non-zero by one
    geometry would shift the other's tickets, so every output is compared with its oracle result."""
    import torch
    shape, pa, tuning, _ = G.GEOMETRY["planes_dyn"]
    _, pb, _, _ = G.GEOMETRY["planes_dyn8"]
    la = G.launch(shape, G.COMBO_HEADLINE, mode=mode, tuning=tuning, mb=pa[0], me=pa[1])
    lb = G.launch(shape, G.COMBO_HEADLINE, mode=mode, tuning=tuning, mb=pb[0], me=pb[1])
    assert (la.tail, lb.tail) == ("dynamic", "dynamic") and (la.tail_wgs, lb.tail_wgs) == (16, 8)
    c = hip.Case(shape, BC_N, lc=(0.0,) * 3, hc=(1.0,) * 3, mode=mode)
    phi = _rough(shape, 95)
    st = _Stage(c, orc, _terms("sep+eik", c, phi), phi)
    side = torch.cuda.Stream()
    for rep in range(44):
        planes, launch = ((pa, la), (pb, lb), (pb, lb))[rep % 3] if rep % 7 else (pa, la)      # A B B A B B ... and AA at the multiples of 7
        _check_stage(st, mode, (0,), tuning, launch, planes=planes, label=f"launch {rep} {mode}")
        if rep in (10, 27):
            side.wait_stream(torch.cuda.current_stream())
            torch.cuda.synchronize()
            ls = G.launch(shape, G.COMBO_HEADLINE, mode=mode, tuning=tuning, mb=pa[0], me=pa[1], own_stream=False)
            _check_stage(st, mode, (0,), tuning, ls, planes=pa, label=f"side stream after launch {rep} {mode}", stream=side)


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("bcspec", [BC_N, BC_P, BC_EN], ids=_bcid)
@pytest.mark.parametrize("row", ["dyn25_mc32", "static_mc32", "dyn_mc64", "tail7"])
def test_rk3_step_under_forced_geometry(hip, orc, mode, bcspec, row):
    """lsm_advance_rk3 from zeroed ghosts on long chunks and tails.  With NeumannBC on every face a FAST step fills no ghost at all
    (x / y served by the loads, the march CLAMPED at the boundary planes: the first chunk's prologue and the last tail chunk's
    look-ahead meet the clamp); periodic and ExtrapolationBC(2) faces are filled and their ghost planes read."""
    shape, _, tuning, _ = G.GEOMETRY[row]
    c = hip.Case(shape, bcspec, lc=(0.0,) * 3, hc=(1.0,) * 3, mode=mode)
    _set(c, tuning)
    phi = _rough(shape, 100)
    specs = _terms("sep+eik", c, phi)
    ref = phi.copy(order="F")
    tc, dt = 0.1, 2.0e-3
    orc.advance(orc.RK3, c.grid, c.bc, ref, c.dense_terms(specs), tc, dt)
    _, arr = c.terms(specs)
    d_phi = c.to_dev(np.nan_to_num(c.pad(phi, fill=False), nan=0.0))
    b1, b2 = c.be.alloc(), c.be.alloc()
    c.be.advance_single("rk3", arr, len(specs), d_phi, b1, b2, tc, dt, None)
    got = c.interior(c.to_host(d_phi))
    _assert_parity(got, ref, mode, False, launch=G.launch(shape, G.COMBO_HEADLINE, mode=mode, tuning=tuning),
                   label=f"rk3 {row} {_bcid(bcspec)} {mode}", factor=3.0)


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("bcspec", ["periodic", "neumann"])
@pytest.mark.parametrize("shape", [(270, 100), (300, 50)])
def test_2d_rows_per_chunk(hip, orc, mode, bcspec, shape):
    """2-D: LSM_STAGE_MC2 = 1, 8, 64 rows per chunk on rows longer than one 256-node tile."""
    c = hip.Case(shape, bcspec, lc=(0.0,) * 2, hc=(1.0,) * 2, mode=mode)
    phi = _rough(shape, 110)
    for name in ("sep+eik", "nm+curv", "rot+eik"):
        specs = _terms(name, c, phi)
        st = _Stage(c, orc, specs, phi)
        for mc2 in (1, 8, 64):
            launch = G.launches(shape, specs, mode=mode, tuning={"LSM_STAGE_MC2": mc2})[0]
            _check_stage(st, mode, (0, 2), {"LSM_STAGE_MC2": mc2}, launch, label=f"2-D {name} mc2 {mc2} {shape} {bcspec} {mode}")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("shape,bcspec", [((256, 11, 150), BC_P), ((130, 20, 150), BC_EN)], ids=_bcid)
@pytest.mark.parametrize("name", list(PAIRS))
def test_pair_kernels_on_long_chunks(hip, orc, name, shape, bcspec, dtype):
    """The two-nodes-per-thread kernels (FAST, a single upwind / NormalMotion / Eikonal term) at 64, 32 and 7 planes per chunk
    (LSM_STAGE_MC; they end at 8 on every grid below about 512³ otherwise): against the oracle, and bit for bit against the
    one-node kernels (LSM_PAIRS = 0: the 64×8 tile with the same chunks and a graded tail)."""
    dt = np.dtype(dtype)
    c = hip.Case(shape, bcspec, lc=(0.0,) * 3, hc=(1.0,) * 3, mode="fast", dtype=dt)
    phi = _rough(shape, 120, dt)
    specs = _terms(name, c, phi)
    st = _Stage(c, orc, specs, phi)
    for mc in (64, 32, 7):
        tuning = {"LSM_STAGE_MC": mc, "LSM_PAIRS": 1}
        launch = G.launches(shape, specs, tuning=tuning)[0]
        assert launch.kernel == "pairs" and launch.mc == mc
        one = G.launches(shape, specs, tuning=dict(tuning, LSM_PAIRS=0))[0]
        assert one.kernel == "wide" and one.mc == mc
        for bm in (0, 1, 2, 3):
            _check_stage(st, "fast", (bm,), tuning, launch, label=f"pairs {name} mc {mc} {shape} {dtype}")
            _set(c, tuning)
            got, _ = st.run(bm)
            _set(c, dict(tuning, LSM_PAIRS=0))
            ref, _ = st.run(bm)
            bad = got != ref
            assert not bad.any(), f"pairs vs one node, {name} mc {mc} base {bm}: " + _report(bad, got, ref, launch, 0)
        _check_stage(st, "fast", (0, 2), dict(tuning, LSM_PAIRS=0), one, label=f"one-node {name} mc {mc} {shape} {dtype}")


def test_set_tuning_refuses_values_outside_the_documented_range(hip):
    from lsm_amd import _lib as L
    c = hip.Case((16, 16, 16), BC_N, mode="fast")
    for name, hi in (("LSM_STAGE_MC", 65536), ("LSM_STAGE_MC2", 65536), ("LSM_STAGE_TAIL", 65536), ("LSM_STAGE_TAIL_DYN", 1000)):
        before = c.be.get_tuning(name)
        for v in (-1, hi + 1, -2 ** 31, 2 ** 31 - 1):
            with pytest.raises(L.LsmError, match=name):
                c.be.set_tuning(name, v)
        assert c.be.get_tuning(name) == before
        c.be.set_tuning(name, hi)
        assert c.be.get_tuning(name) == hi
        c.be.set_tuning(name, before)


STEP_SWITCHES = [("LSM_XREDIRECT", 0), ("LSM_MREDIRECT", 0), ("LSM_GHOST_FULL_DEPTH", 1)]


@pytest.mark.parametrize("switch,value", STEP_SWITCHES)
@pytest.mark.parametrize("shape,bcspec", [
    ((21, 19, 17), "neumann"), ((70, 20), "neumann"), ((40, 18, 12), "periodic"),
    ((36, 17, 11), [("neumann", "symmetry"), "periodic", ("extrapolation", 2)]),
    ((36, 17, 11), [("extrapolation", 2), ("symmetry", "neumann"), "neumann"]),
    ((67, 13, 10), ["periodic", ("extrapolation", 3), "symmetry"]),
], ids=_bcid)
def test_rk3_step_under_each_step_level_switch(hip, orc, switch, value, shape, bcspec):
    """include/lsm.h: "the whole GPU test suite passes under each" switch — here the FAST RK3 step of
    test_advance_matches_literal_reference_loop's mixed boundary conditions with the ghosts materialised instead of redirected
    (LSM_XREDIRECT = 0, LSM_MREDIRECT = 0) and with every ghost layer filled (LSM_GHOST_FULL_DEPTH = 1), at that test's tolerance."""
    nd = len(shape)
    c = hip.Case(shape, bcspec, mode="fast")
    c.be.set_tuning(switch, value)
    assert c.be.get_tuning(switch) == value
    phi = _rough(shape, 130)
    specs = _fix_specs([("adv", ("rot", 1.0, 0.0, 0.0), "weno5"), ("eik", None)], nd, phi)
    ref = phi.copy(order="F")
    tc, dt = 0.1, 2.0e-3
    orc.advance(orc.RK3, c.grid, c.bc, ref, c.dense_terms(specs), tc, dt)
    _, arr = c.terms(specs)
    d_phi = c.to_dev(np.nan_to_num(c.pad(phi, fill=False), nan=0.0))
    b1, b2 = c.be.alloc(), c.be.alloc()
    c.be.advance_single("rk3", arr, len(specs), d_phi, b1, b2, tc, dt, None)
    _assert_parity(c.interior(c.to_host(d_phi)), ref, "fast", False, label=f"{switch}={value} {shape}", factor=3.0)


# ---- 2. default tuning at sizes where the defaults turn the paths on --------------------------------------------------------

MID = (250, 253, 250)


def _free_or_skip(gib):
    import torch
    torch.cuda.empty_cache()
    if torch.cuda.mem_get_info()[0] < gib * 2 ** 30:
        pytest.skip(f"needs {gib} GiB of free device memory")


@pytest.mark.parametrize("terms,bcspec", [("sep+eik", BC_N), ("nm+curv", ("extrapolation", 2))], ids=_bcid)
def test_250_cubed_stage_default_tuning(hip, threaded_orc, terms, bcspec):
    """250 × 253 × 250 with no switch set: 32-plane chunks, 7 long layers, a dynamic tail of 16 + 10 planes, partial tiles in x and y
    (tests/_stage_geometry.py, DEFAULT_GEOMETRY) — one lsm_stage per base mode in STRICT and in FAST against one oracle evaluation."""
    orc = threaded_orc
    _free_or_skip(4)
    phi = _rough(MID, 140)
    want = None
    for mode in ("fast", "strict"):
        c = hip.Case(MID, bcspec, lc=(0.0,) * 3, hc=(1.0,) * 3, mode=mode)
        specs = _terms(terms, c, phi)
        st = _Stage(c, orc, specs, phi)
        if want is not None:
            st._want = want                                                   # the oracle does not depend on the device's mode
        launch = G.launches(MID, specs, mode=mode)[0]
        G.check(launch, G.DEFAULT_GEOMETRY[MID, G.passes(specs)[0][0]])
        _check_stage(st, mode, (0, 1, 2, 3), {}, launch, label=f"250³ {terms} {mode}")
        want = st._want


def test_250_cubed_rk3_step_default_tuning(hip, threaded_orc):
    """... and one lsm_advance_rk3 of the headline pair from zeroed ghosts (FAST: no ghost fill, the march clamped at both faces)."""
    orc = threaded_orc
    _free_or_skip(4)
    phi = _rough(MID, 141)
    ref = None
    for mode in ("fast", "strict"):
        c = hip.Case(MID, BC_N, lc=(0.0,) * 3, hc=(1.0,) * 3, mode=mode)
        specs = _terms("sep+eik", c, phi)
        tc, dt = 0.1, 1.0e-3
        if ref is None:
            ref = phi.copy(order="F")
            orc.advance(orc.RK3, c.grid, c.bc, ref, c.dense_terms(specs), tc, dt)
        _, arr = c.terms(specs)
        d_phi, b1, b2 = c.be.alloc(), c.be.alloc(), c.be.alloc()
        c.be.upload(d_phi, phi)                                               # ghost layers stay zero
        c.be.advance_single("rk3", arr, len(specs), d_phi, b1, b2, tc, dt, None)
        _assert_parity(c.be.download(d_phi).astype(np.float64), ref, mode, False, launch=G.launch(MID, G.COMBO_HEADLINE, mode=mode),
                       label=f"250³ rk3 {mode}", factor=3.0)


def _bench_sphere(c):
    """bench.py's initial field, ϕ = |x − (0.35, 0.35, 0.35)| − 0.15 at the grid's nodes, built plane by plane."""
    x, y, z = c.grid.coords()
    n = c.grid.shape
    out = np.empty(n, dtype=np.float64, order="F")
    xy = (x[:, None] - 0.35) ** 2 + (y[None, :] - 0.35) ** 2
    for k in range(n[2]):
        out[:, :, k] = np.sqrt(xy + (z[k] - 0.35) ** 2) - 0.15
    return out


def test_512_cubed_headline_step_matches_the_oracle(hip, threaded_orc):
    """The shape the project's number is measured on: bench.py's headline equation (vortex-deformation WENO5 advection + Eikonal,
    NeumannBC, FAST) and its initial sphere at 512³ — 64-plane chunks, 7 long layers, a dynamic tail of 4 × 16 planes.
    lsm_compute_cfl equals the oracle's bitwise, then one RK3 step with Δt = half of it against oracle.advance."""
    import lsm_amd
    orc = threaded_orc
    _free_or_skip(8)
    n = (512, 512, 512)
    G.check(G.launch(n, G.COMBO_HEADLINE), G.DEFAULT_GEOMETRY[n, G.COMBO_HEADLINE])
    c = hip.Case(n, "neumann", lc=(0.0,) * 3, hc=(1.0,) * 3, mode="fast")
    tables = lsm_amd.vortex_deformation(lsm_amd.CartesianGrid((0, 0, 0), (1, 1, 1), n)).tables
    specs = [("adv", ("sep", tables, ("cos", 3.0)), "weno5"), ("eik", None)]
    phi = _bench_sphere(c)
    dense = c.dense_terms(specs)
    _, arr = c.terms(specs)
    d_phi, b1, b2 = c.be.alloc(), c.be.alloc(), c.be.alloc()
    c.be.upload(d_phi, phi)                                                   # ghost layers stay zero
    want_cfl = orc.compute_cfl(c.grid, c.bc, phi, dense, 0.0)
    got_cfl = c.be.compute_cfl_local(arr, len(specs), d_phi, 0.0)
    assert got_cfl == want_cfl, (got_cfl, want_cfl)
    dt = 0.5 * want_cfl
    c.be.advance_single("rk3", arr, len(specs), d_phi, b1, b2, 0.0, dt, None)
    got = c.be.download(d_phi)
    del d_phi, b1, b2
    orc.advance(orc.RK3, c.grid, c.bc, phi, dense, 0.0, dt)                   # in place: phi is the reference now
    _assert_parity(got, phi, "fast", False, launch=G.launch(n, G.COMBO_HEADLINE), label="512³ headline rk3", factor=3.0)


BIG_SINGLE = (512, 512, 512)


@pytest.mark.parametrize("name", ["upwind", "nm", "eik_current"])
def test_512_cubed_single_term_stage_on_the_pair_kernels(hip, threaded_orc, name):
    """A single upwind / NormalMotion / Eikonal term at a size where the pair kernels keep their default 64-plane chunks."""
    orc = threaded_orc
    _free_or_skip(8)
    n = BIG_SINGLE
    c = hip.Case(n, "neumann", lc=(0.0,) * 3, hc=(1.0,) * 3, mode="fast")
    phi = _bench_sphere(c)
    phi += 0.004 * np.sin(40.0 * np.linspace(0.0, 1.0, n[0]))[:, None, None] * np.cos(23.0 * np.linspace(0.0, 1.0, n[2]))[None, None, :]     # not symmetric
    specs = _terms(name, c, phi)
    launch = G.launches(n, specs)[0]
    G.check(launch, G.DEFAULT_GEOMETRY[n, G.passes(specs)[0][0]])
    ot, arr = c.terms(specs)
    psi = c.pad(phi)
    del phi
    want = np.full_like(psi, np.nan)
    orc.stage_padded(c.grid, c.bc, c.olay, ot, psi, None, want, None, 0, CDT, 0.0, 0.4)
    want = c.interior(want)
    d_psi = c.to_dev(psi)
    del psi
    d_out = c.be.alloc()
    c.be.stage(arr, len(specs), d_psi, None, d_out, None, 0, CDT, 0.0, 0.4)
    got = c.be.download(d_out)
    del d_psi, d_out
    _assert_parity(got, want, "fast", False, launch=launch, label=f"512³ {name}")
