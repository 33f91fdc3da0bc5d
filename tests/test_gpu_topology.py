"""The topological derivative and the nucleation step on the device (csrc/lsm_elastic.hip, csrc/lsm_nucleate.hip through the Python
API and the C ABI) against the restatement (tests/_topo_ref.py) on the device's own K0 and cell moduli.

Bit for bit: the cell array T_C and the node field for a random displacement on the field cases of tests/_stress_ref.py (both planes,
given moduli, a level ≠ 0, a float32 handle, and its two launch shapes beyond 2048 workgroups of 256 threads, where the kernels
stride); the centre list on the shapes and inputs listed at SEARCH_CASES; the punched ϕ and `changed` on the same shapes.  Two
solves of one operator are bit-identical with and without the new calls in between; the C ABI refuses what include/lsm.h says it
refuses and then runs nothing.

End to end on a 65×33 cantilever that is all material: topological_derivative() → nucleate_; the outside components grow by exactly
the number of punched centres, ϕ is the restatement's bit for bit and volume() is _measure_ref's exact sum over it to 1e-12, the bar
tests/test_gpu_field_ops.py holds the device's volume to (tests/test_gpu_components.py, which the drop is compared like, has integer
sums only)."""
import ctypes as C

import numpy as np
import pytest

import _elastic_ref as R
import _measure_ref as M
import _stress_ref as S
import _topo_ref as TR
import test_gpu_elastic as T

pytestmark = pytest.mark.gpu

FIELD_CASES = S.field_cases()


def _open(lsm, cs):
    dev = lsm.ElasticityOperator(T._field(lsm, cs), **T._kwargs(cs))
    op = R.Operator(dev.cells(), cs["h"], dev.stiffness(0), cs["bits"])
    return dev, S.Stress(op, cs["nu"], cs["plane"])


def _random_u(cs, seed=31):
    n = tuple(cs["n"])
    u = np.random.default_rng(seed).standard_normal((len(n),) + n)
    u[(slice(None),) + (slice(0, 2),) * len(n)] = 0.375      # cell (0, 0, …) is translated: T_C = 0 there
    return u.astype(cs["dtype"]).astype(np.float64)


# ----------------------------------------------------------------------------- the T field

@pytest.mark.parametrize("name", sorted(FIELD_CASES))
def test_the_cells_and_the_node_field_are_the_restatements_bits(name):
    lsm = T._lsm()
    cs = FIELD_CASES[name]
    dev, st = _open(lsm, cs)
    u = _random_u(cs)
    sol = dev.with_displacement(u)
    want = TR.cells(st, u)
    got = dev.backend.elastic_topo_cells(dev._handle(), [c.buf for c in sol.u]).cpu().numpy().reshape(st.cn, order="F")
    assert np.array_equal(T._bits(got), T._bits(want))
    assert want[(0,) * len(cs["n"])] == 0.0 and want.max() > 0.0
    field = sol.topological_derivative()
    got = field.values()
    want = st.node_mean(want).astype(cs["dtype"])
    assert got.dtype == cs["dtype"] and np.array_equal(T._bits(got), T._bits(want))
    nan = u.copy()
    nan[0][tuple(m // 2 for m in cs["n"])] = np.nan      # a non-finite u propagates to the cells around the node, and no further
    got = dev.with_displacement(nan).topological_derivative().values()
    assert np.isnan(got).sum() == np.isnan(TR.nodes(st, nan)).sum() > 0
    dev.close()
    with pytest.raises(ValueError, match="closed"):
        sol.topological_derivative()


@pytest.mark.parametrize("name", ["17x9_stress", "9x7x5"])
def test_the_calls_leave_later_solves_unaffected(name):
    lsm = T._lsm()
    cs = S.solved_cases()[name]
    f2 = np.random.default_rng(41).standard_normal((len(cs["n"]),) + tuple(cs["n"]))

    def run(between):
        dev, _ = _open(lsm, cs)
        a = dev.solve(cs["f"], rtol=1e-8)
        if between:
            a.topological_derivative()
            dev.backend.elastic_topo_cells(dev._handle(), [c.buf for c in a.u])
            dev.with_displacement(f2).topological_derivative()
        b = dev.solve(f2, rtol=1e-8)
        out = (T._values(a.u), T._values(b.u), a.iterations, b.iterations)
        dev.close()
        return out

    for x, y in zip(run(False), run(True)):
        assert np.array_equal(T._bits(np.asarray(x, dtype=np.float64)), T._bits(np.asarray(y, dtype=np.float64)))


def test_the_c_abi_of_the_t_field_refuses_what_the_header_says():
    lsm = T._lsm()
    cs = FIELD_CASES["9x12_strain_level"]
    dev, st = _open(lsm, cs)
    b, h, lib = dev.backend, dev._handle(), dev.backend.lib
    sol = dev.with_displacement(_random_u(cs))
    u0, u1 = [b.ptr(c.buf) for c in sol.u]
    out = lsm.ROCMeshField(b, sol.u[0].mesh, sol.u[0].bcs)
    out.buf.zero_()
    o0 = b.ptr(out.buf)
    big = b.torch.zeros(int(np.prod(st.cn)), dtype=b.torch.float64, device=b.device)
    pb = b.ptr(big)
    bad = [lib.lsm_elastic_topo_cells(h, u0, None, None, pb), lib.lsm_elastic_topo_cells(h, u0, u0, None, pb), lib.lsm_elastic_topo_cells(h, u0, u1, None, None),
           lib.lsm_elastic_topo_cells(h, u0, u1, None, u1), lib.lsm_elastic_topo_cells(h, None, u1, None, pb), lib.lsm_elastic_topo_cells(None, u0, u1, None, pb),
           lib.lsm_elastic_topo(h, u0, None, None, o0), lib.lsm_elastic_topo(h, u0, u0, None, o0), lib.lsm_elastic_topo(h, u0, u1, None, None),
           lib.lsm_elastic_topo(h, u0, u1, None, u0), lib.lsm_elastic_topo(h, u0, u1, None, u1), lib.lsm_elastic_topo(None, u0, u1, None, o0)]
    assert bad == [lsm._lib.ERR_INVALID] * len(bad), bad
    b.sync()
    assert not out.buf.any().item() and not big.any().item()      # nothing ran
    assert lib.lsm_elastic_topo(h, u0, u1, None, o0) == 0 and lib.lsm_elastic_topo_cells(h, u0, u1, None, pb) == 0
    b.sync()
    assert out.buf.any().item() and big.any().item()
    dev.close()


# ----------------------------------------------------------------------------- the search and the punch

def _grid_case(n, hc, dtype=np.float64):
    return dict(n=n, hc=hc, h=tuple(x / (m - 1) for x, m in zip(hc, n)), dtype=dtype)


# name → (n, hc, spacing, the window it must give, dtype)
SEARCH_CASES = {
    "9x12_w1": ((9, 12), (0.8, 1.1), 0.05, (1, 1), np.float64),
    "9x12_w2": ((9, 12), (0.8, 1.1), 0.15, (2, 2), np.float64),
    "9x12_w2_f32": ((9, 12), (0.8, 1.1), 0.15, (2, 2), np.float32),
    "33x20_w5": ((33, 20), (3.2, 1.9), 0.45, (5, 5), np.float64),                   # the halo of a column tile: 5 lines on either side of 16
    "33x20_w20": ((33, 20), (3.2, 1.9), 1.95, (20, 20), np.float64),                # a window as wide as the grid in y, wider than a tile
    "6x5x7_w121": ((6, 5, 7), (1.0, 0.4, 1.2), 0.15, (1, 2, 1), np.float64),
    "4x4_w32": ((4, 4), (0.3, 0.3), 3.15, (32, 32), np.float64),                    # the window beyond the grid
    "300x230_w2": ((300, 230), (29.9, 22.9), 0.15, (2, 2), np.float64),            # many workgroups, a partial last tile on every axis
    "300x230_w16_f32": ((300, 230), (29.9, 22.9), 1.55, (16, 16), np.float32),
    "45x41x37_w213": ((45, 41, 37), (4.4, 8.0, 2.16), 0.15, (2, 1, 3), np.float64),
}


def _fields(lsm, cs, phi, t):
    """(ϕ, t) as two fields of one backend holding the given values rounded to the storage type"""
    p = T._field(lsm, cs, np.asfortranarray(phi.astype(cs["dtype"])))
    q = lsm.ROCMeshField(p.backend, p.mesh, p.bcs).copy_(np.asfortranarray(t.astype(cs["dtype"])))
    return p, q


def _inputs(n, dtype, rng):
    """name → (ϕ, t, threshold): the stored values"""
    rnd = lambda a: a.astype(dtype)
    inside = np.full(n, -1.0)
    mixed = -1.0 + 1.2 * rng.random(n)                       # a fifth of the nodes fail the clearance
    ties = rng.integers(0, 4, size=n).astype(np.float64) - 1.0      # four values: ties across every tile boundary, ±0 among them
    ties[ties == 0.0] = np.where(rng.random(int((ties == 0.0).sum())) < 0.5, -0.0, 0.0)
    nans = rng.standard_normal(n)
    nans[rng.random(n) < 0.1] = np.nan
    pn = mixed.copy()
    pn[rng.random(n) < 0.1] = np.nan
    t = rng.standard_normal(n)
    return {"random": (rnd(mixed), rnd(t), 0.5), "constant": (rnd(inside), rnd(np.full(n, 0.25)), 1.0), "ties": (rnd(mixed), rnd(ties), 1.5),
            "nans": (rnd(pn), rnd(nans), 0.5), "no_candidate": (rnd(inside), rnd(t), float(rnd(t).min())), "all_candidates": (rnd(inside), rnd(t), 1e30)}


@pytest.mark.parametrize("name", sorted(SEARCH_CASES))
def test_the_centre_list_is_the_restatements(name):
    lsm = T._lsm()
    n, hc, spacing, w, dtype = SEARCH_CASES[name]
    cs = _grid_case(n, hc, dtype)
    assert TR.window(spacing, cs["h"]) == w
    rng = np.random.default_rng(5)
    level, clearance = 0.125, 0.25
    p = q = None
    for kind, (phi, t, threshold) in _inputs(n, dtype, rng).items():
        if p is None:
            p, q = _fields(lsm, cs, phi, t)
        else:
            p.copy_(np.asfortranarray(phi)), q.copy_(np.asfortranarray(t))
        idx, val = p.backend.nucleate_find(p.buf, q.buf, threshold, level, clearance, spacing)
        widx, wval = TR.centres(phi, t, threshold, level, clearance, w)
        assert idx.dtype == np.int64 and np.array_equal(idx, widx), (name, kind)
        assert np.array_equal(T._bits(val), T._bits(wval)), (name, kind)
        assert (idx.size == 0) == (kind == "no_candidate") and (kind != "constant" or idx.tolist() == [0])
        res = lsm.find_nucleation_sites(p, q, threshold=threshold, radius=0.5 * spacing, clearance=clearance, level=level, max_holes=3)
        sidx, sval = TR.select(widx, wval, 3)
        assert np.array_equal(res.indices, sidx) and np.array_equal(T._bits(res.values), T._bits(sval)) and res.found == widx.size and res.changed == 0
        assert np.array_equal(res.centres, np.stack(np.unravel_index(sidx, n, order="F"), axis=1).reshape(-1, len(n)))
    assert np.array_equal(T._bits(p.values()), T._bits(phi))      # the search writes nothing


def test_the_centre_counts_of_more_than_8192_chunks():
    """(4097, 8194) nodes, 8197 chunks: the scan of the centres per chunk (csrc/scan.h with 64-bit offsets) runs a second round,
    which receives a carry.  ϕ = −1 (material, a clearance of 1 to the level), t = 1 but for 90 nodes below the threshold, any
    two farther apart than the window of 3 nodes (spacing 2.5, h = 1): each is the only candidate of its window, so a centre.
    Half lie in the first chunks, half in rows 8191..8193.  A dropped carry writes the centres of chunk 8192 and beyond over the
    first ones, or loses them from the count."""
    import _chunk_carry as CC
    lsm = T._lsm()
    cs = _grid_case(CC.N, tuple(float(m - 1) for m in CC.N), np.float32)
    I, J, lin = CC.isolated_nodes()
    t = np.ones(CC.N, dtype=np.float32, order="F")
    values = (-(1.0 + np.arange(len(lin))[::-1] / 128.0)).astype(np.float32)      # exact in float32, descending along the list
    t[I, J] = values
    spacing = 2.5
    assert TR.window(spacing, cs["h"]) == (3, 3)
    p, q = _fields(lsm, cs, np.full(CC.N, -1.0, dtype=np.float32, order="F"), t)
    idx, val = p.backend.nucleate_find(p.buf, q.buf, 0.5, 0.0, 0.25, spacing)
    print(f"{idx.size} centres, {int((idx // CC.CHUNK >= CC.SCAN).sum())} of them in chunks >= {CC.SCAN}")
    assert idx.dtype == np.int64 and np.array_equal(idx, lin) and np.array_equal(T._bits(val), T._bits(values.astype(np.float64)))
    assert (idx // CC.CHUNK >= CC.SCAN).any() and (idx // CC.CHUNK < 20).any()


def _padded_bits(f):
    t = f.backend.torch
    return f.buf.view(t.int64 if f.buf.dtype == t.float64 else t.int32).clone()


def _ghost_mask(f):
    t = f.backend.torch
    m = t.ones(f.buf.shape, dtype=t.bool, device=f.buf.device)
    f.backend.interior(m).zero_()
    return m


def _lists(n):
    """name → (linear indices, radius in units of the smallest h): a corner, a face, two overlapping balls in both orders with a
    repeat, a radius below h, the empty list"""
    lin = lambda I: int(np.ravel_multi_index(I, n, order="F"))
    mid = tuple(m // 2 for m in n)
    face = (0,) + mid[1:]
    near = tuple(min(m // 2 + 2, m - 1) for m in n)
    return {"corner": ([0, lin(tuple(m - 1 for m in n))], 2.6), "face": ([lin(face)], 3.2), "overlap": ([lin(mid), lin(near), lin(mid)], 3.7),
            "overlap_reversed": ([lin(mid), lin(near), lin(mid)][::-1], 3.7), "below_h": ([lin(mid), lin(near)], 0.7), "empty": ([], 2.0)}


@pytest.mark.parametrize("name", ["9x12_w2", "9x12_w2_f32", "33x20_w5", "6x5x7_w121", "4x4_w32", "300x230_w16_f32", "45x41x37_w213"])
def test_the_punch_is_the_restatements_bits(name):
    lsm = T._lsm()
    n, hc, _, _, dtype = SEARCH_CASES[name]
    cs = _grid_case(n, hc, dtype)
    rng = np.random.default_rng(6)
    phi0 = (-1.0 + 1.1 * rng.random(n)).astype(dtype)      # all below the level: every centre that is a number rises
    phi0[tuple(m // 2 for m in n)] = np.nan      # a centre on a NaN node: it stays NaN
    phi0[tuple(m // 2 - 1 for m in n)] = np.nan
    p, _ = _fields(lsm, cs, np.nan_to_num(phi0), np.nan_to_num(phi0))
    b, level = p.backend, 0.125
    ghosts = _ghost_mask(p)
    results = {}
    for kind, (centres, r) in _lists(n).items():
        radius = r * min(cs["h"])
        p.copy_(np.asfortranarray(phi0))
        before = _padded_bits(p)
        changed = b.nucleate_punch(p.buf, np.array(centres, dtype=np.int64), level, radius)
        b.sync()
        want, wchanged = TR.punch(phi0, centres, cs["h"], level, radius)
        got = p.values()
        assert got.dtype == dtype and np.array_equal(T._bits(got), T._bits(want)), (name, kind)
        assert changed == wchanged and (changed > 0) == (kind != "empty"), (name, kind, changed, wchanged)
        assert np.array_equal(_padded_bits(p)[ghosts].cpu().numpy(), before[ghosts].cpu().numpy())      # the ABI call leaves the ghosts alone
        assert np.isnan(got[tuple(m // 2 for m in n)]) and np.isnan(got[tuple(m // 2 - 1 for m in n)])
        if kind == "below_h":
            assert changed <= len(centres) and int((T._bits(got) != T._bits(phi0)).sum()) == changed
        results[kind] = got
    assert np.array_equal(T._bits(results["overlap"]), T._bits(results["overlap_reversed"]))


def test_the_c_abi_of_the_nucleation_refuses_what_the_header_says():
    lsm = T._lsm()
    n, hc, spacing, _, dtype = SEARCH_CASES["9x12_w2"]
    cs = _grid_case(n, hc, dtype)
    rng = np.random.default_rng(7)
    phi0, t0 = -1.0 - rng.random(n), rng.standard_normal(n)
    p, q = _fields(lsm, cs, phi0, t0)
    b, lib = p.backend, p.backend.lib
    h, nan, inf = min(cs["h"]), float("nan"), float("inf")
    out, count, changed = C.c_void_p(), C.c_int64(-7), C.c_int64(-7)
    pp, pq = b.ptr(p.buf), b.ptr(q.buf)
    create = lambda *a: lib.lsm_nucleate_create(b.h, *a, C.byref(out), C.byref(count))
    bad = [create(None, pq, 0.5, 0.0, 0.1, spacing), create(pp, None, 0.5, 0.0, 0.1, spacing),
           create(pp, pq, nan, 0.0, 0.1, spacing), create(pp, pq, inf, 0.0, 0.1, spacing), create(pp, pq, 0.5, nan, 0.1, spacing),
           create(pp, pq, 0.5, 0.0, -inf, spacing), create(pp, pq, 0.5, 0.0, 0.1, nan), create(pp, pq, 0.5, 0.0, 0.1, inf),
           create(pp, pq, 0.5, 0.0, 0.1, 0.0), create(pp, pq, 0.5, 0.0, 0.1, -1.0),      # w = 0
           create(pp, pq, 0.5, 0.0, 0.1, 32.5 * h),                                       # w = 33
           lib.lsm_nucleate_create(b.h, pp, pq, 0.5, 0.0, 0.1, spacing, None, C.byref(count)),
           lib.lsm_nucleate_create(b.h, pp, pq, 0.5, 0.0, 0.1, spacing, C.byref(out), None)]
    assert bad == [lsm._lib.ERR_INVALID] * len(bad), bad
    assert out.value is None and count.value == -7
    assert create(pp, pq, 0.5, 0.0, 0.1, 31.5 * h) == 0 and count.value == 1      # w = 32 is taken: the one global minimum of the candidates
    lib.lsm_nucleate_destroy(out)
    lib.lsm_nucleate_destroy(None)
    for fn, kw in ((lsm.find_nucleation_sites, dict(spacing=0.0)), (lsm.nucleate_, dict(spacing=32.5 * h))):
        with pytest.raises(ValueError, match="window"):
            fn(p, q, threshold=0.5, radius=0.1, **kw)
    cen = b.torch.tensor([5, 40], dtype=b.torch.int64, device=b.device)
    off = b.torch.tensor([5, n[0] * n[1]], dtype=b.torch.int64, device=b.device)
    neg = b.torch.tensor([-1], dtype=b.torch.int64, device=b.device)
    punch = lambda c, k, level, radius: lib.lsm_nucleate_punch(b.h, pp, b.ptr(c) if c is not None else None, k, level, radius, C.byref(changed))
    bad = [punch(cen, 2, nan, 0.2), punch(cen, 2, inf, 0.2), punch(cen, 2, 0.0, 0.0), punch(cen, 2, 0.0, -0.1), punch(cen, 2, 0.0, nan), punch(cen, 2, 0.0, inf),
           punch(cen, -1, 0.0, 0.2), punch(None, 2, 0.0, 0.2), punch(off, 2, 0.0, 0.2), punch(neg, 1, 0.0, 0.2),
           lib.lsm_nucleate_punch(b.h, None, b.ptr(cen), 2, 0.0, 0.2, C.byref(changed)), lib.lsm_nucleate_punch(b.h, pp, b.ptr(cen), 2, 0.0, 0.2, None)]
    assert bad == [lsm._lib.ERR_INVALID] * len(bad), bad
    b.sync()
    assert np.array_equal(T._bits(p.values()), T._bits(phi0)) and changed.value == 0      # nothing was written
    assert punch(None, 0, 0.0, 0.2) == 0 and changed.value == 0                           # an empty list is fine, and changes nothing
    assert np.array_equal(T._bits(p.values()), T._bits(phi0))
    assert punch(cen, 2, 0.0, 0.2) == 0 and changed.value == TR.punch(phi0, [5, 40], cs["h"], 0.0, 0.2)[1] > 0


def test_the_api_refuses_bands_periodic_and_1d_fields():
    lsm = T._lsm()
    grid = lsm.CartesianGrid((0.0, 0.0), (1.0, 1.0), (12, 12))
    vals = np.asfortranarray(np.full((12, 12), -1.0))

    def state(bc, ic=None):
        ic = lsm.MeshField(vals, grid) if ic is None else ic
        return lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=ic, bc=bc).current_state()

    kw = dict(threshold=0.5, radius=0.1)
    per = state(lsm.PeriodicBC())
    fine = lsm.CartesianGrid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (17, 18, 16))
    band = state(lsm.NeumannBC(), lsm.NarrowBandMeshField(lsm.MeshField(lambda x: np.sqrt((x[0] - 0.5) ** 2 + (x[1] - 0.5) ** 2 + (x[2] - 0.5) ** 2) - 0.3, fine), nlayers=2))
    one = state(lsm.NeumannBC(), lsm.MeshField(lambda x: x[0] - 0.3, lsm.CartesianGrid((0,), (1,), (33,))))
    ok = state(lsm.NeumannBC())
    other = state(lsm.NeumannBC())
    for fn in (lsm.nucleate_, lsm.find_nucleation_sites):
        with pytest.raises(ValueError, match="PeriodicBC"):
            fn(per, per, **kw)
        with pytest.raises(ValueError, match="NarrowBandMeshField"):
            fn(band, band, **kw)
        with pytest.raises(ValueError, match="1 dimensional"):
            fn(one, one, **kw)
        with pytest.raises(ValueError, match="backend"):
            fn(ok, other, **kw)
        with pytest.raises(TypeError, match="ROCMeshField"):
            fn(ok, vals, **kw)
    with pytest.raises(lsm.LsmError, match="periodic"):
        per.backend.nucleate_find(per.buf, per.buf, 0.5, 0.0, 0.1, 0.2)
    assert not (ok.values() != -1.0).any()


# ----------------------------------------------------------------------------- end to end

def test_a_full_cantilever_gets_its_holes():
    lsm = T._lsm()
    n, hc = (65, 33), (2.0, 1.0)
    h = tuple(x / (m - 1) for x, m in zip(hc, n))
    x = np.meshgrid(*[np.arange(m) * hd for m, hd in zip(n, h)], indexing="ij")
    dist = np.minimum.reduce([x[0], x[1], hc[0] - x[0], hc[1] - x[1]])
    phi0 = np.asfortranarray(-(0.5 * h[0] + dist))            # all material: the signed distance of a box half a cell larger
    t = [0.0, 0.0]
    t[1] = -1.0
    cs = dict(n=n, hc=hc, h=h, phi=phi0, E=None, E_in=1.0, E_out=1e-3, nu=0.3, plane="stress", level=0.0, bits=np.asfortranarray(R.face_bits(n, 0, 0, 3)),
              g=np.zeros(2), f=R.traction(n, h, 0, 1, t), dtype=np.float64)
    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(phi0, lsm.CartesianGrid((0.0, 0.0), hc, n)), bc=lsm.NeumannBC())
    phi = eq.current_state()
    assert tuple(phi.mesh.meshsize()) == h
    dev = lsm.ElasticityOperator(phi, **T._kwargs(cs))
    sol = dev.solve(cs["f"], rtol=1e-8, max_iters=3000)
    field = sol.topological_derivative()
    tv = field.values()
    assert tv.min() >= 0.0
    assert lsm.components(phi, side="outside").count == 0
    v0 = lsm.volume(eq)
    radius, threshold, holes = 0.1, float(np.quantile(tv, 0.25)), 2      # three centres are found: max_holes cuts
    phi.ghosts_dirty = False
    res = lsm.nucleate_(phi, field, threshold=threshold, radius=radius, max_holes=holes)
    want, widx, wval, wfound, wchanged = TR.nucleate(phi0, tv, h, threshold=threshold, radius=radius, max_holes=holes)
    assert phi.ghosts_dirty                                    # the ghosts are refilled before the next stencil reads them, as after remove_components_
    assert len(res) == holes < res.found == wfound and res.changed == wchanged > holes
    assert np.array_equal(res.indices, widx) and np.array_equal(T._bits(res.values), T._bits(wval))
    assert np.array_equal(T._bits(phi.values()), T._bits(want))
    assert lsm.components(phi, side="outside").count == len(res)
    v1, r0, r1 = lsm.volume(eq), M.volume(phi0, h), M.volume(want, h)
    print(f"centres {res.centres.tolist()} of {res.found}; volume {v0:.6f} -> {v1:.6f} (restatement {r0:.6f} -> {r1:.6f})")
    assert v1 == pytest.approx(r1, rel=1e-12) and r1 < r0
    assert abs((v0 - v1) - (r0 - r1)) <= 2e-12 * r0
    again = lsm.find_nucleation_sites(phi, field, threshold=threshold, radius=radius)
    assert not set(again.indices.tolist()) & set(res.indices.tolist())      # a punched centre is no candidate any more
    dev.close()
