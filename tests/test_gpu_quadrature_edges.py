"""quadrature on the device (csrc/lsm_quad.hip) at the launch shapes and edges tests/test_gpu_quadrature.py does not reach,
node for node against the restatement tests/_quad_ref.py (whole grids, or the cells passed to _compare(cells=...)), against the
closed form of the stripes1 fixture, and row against row on the stripes3 fixture (tests/test_quadrature_host.py checks the
fixtures' conditions on the CPU).  Tolerances are _compare's: 1e-12 on coordinates, 1e-12·max(1, max |w|) on weights.

  A  classify / compaction: several chunks of 4096 cells, a partial last chunk, a chunk with nothing in it
  B  chunk_scan_kernel (csrc/scan.h): a second round of 8192 values in the node-offset scan and in the scan of count != 0 (the
     row with `nonzero` set)
  C  quad_cells_kernel: more than 2^20 candidates, so a workgroup takes a second cell (an empty candidate on either trip)
  D  more than 8192 chunks: the scan of the chunk counts carries into chunk 8192
  E  subdivision to the depth limit and the fallback in 3-D and with h_x != h_y (the first longest side is not a tie)
  F  quadrature_order 3, 9, 20 in 1-D, 2-D, 3-D
  G  boundary conditions and float32 storage in 3-D; bands with garbage off the band in 2-D and 3-D
"""
import itertools
import time
import warnings

import numpy as np
import pytest

from test_gpu_quadrature import _SHAPES, _compare, _device, _grid_vals, _lin, _lsm, _ref
from test_quadrature_host import KINKS, kink, restated, row_pattern, stripes1, stripes1_closed_form, stripes3

pytestmark = pytest.mark.gpu

CHUNK, SCAN, GRID = 4096, 8192, 1 << 20     # QUAD_CHUNK, values per round of chunk_scan_kernel, the cell kernel's launch cap


def _quad(lsm, phi, k, q, surface):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return lsm.quadrature(phi, interpolation_order=k, quadrature_order=q, surface=surface)


def _structure(q):
    """what holds for every result, whatever the restatement says; returns the linear indices of the cut and the full cells"""
    c, f = _lin(q.cells, q.mesh.n), _lin(q.full_cells, q.mesh.n)
    assert len(c) == q.ncut and len(f) == q.nfull
    assert (np.diff(c) > 0).all() and (np.diff(f) > 0).all()
    assert np.intersect1d(c, f).size == 0
    assert q.offsets[0] == 0 and (np.diff(q.offsets) >= 0).all() and q.offsets[-1] == q.nnodes == len(q.weights)
    return c, f


def _close(what, dX, dW, wmax):
    print(f"{what}: coords {dX:.3e}, weights {dW:.3e} (max |w| {wmax:.3e})")
    assert dX <= 1e-12 and dW <= 1e-12 * max(1.0, wmax)


# ----------------------------------------------------------------------------- A: chunks of the classify and compaction kernels

_CHUNKED = {
    # name: (n, f, lc, hc, k, q, chunks holding cut cells, chunks holding full cells (volume), number of chunks)
    "1d": ((9001,), lambda X: np.sin(40 * X[0] + 0.3) - 0.2, (0.0,), (3.0,), 3, 3, {0, 1, 2}, {0, 1, 2}, 3),
    "2d": ((97, 131), lambda X: np.hypot((X[0] - 0.11) / 0.83, X[1] + 0.07) - 0.73, None, None, 2, 3, {0, 1, 2}, {0, 1, 2}, 4),
    "3d": ((18, 17, 17), lambda X: np.sqrt(((X[0] - 0.35) / 0.9) ** 2 + (X[1] + 0.08) ** 2 + ((X[2] - 0.3) / 1.1) ** 2) - 0.62,
           None, None, 3, 1, {0, 1}, {0}, 2),      # q = 1: at q = 2 the restatement takes 5 s for the surface rule
}


@pytest.mark.parametrize("name", sorted(_CHUNKED))
@pytest.mark.parametrize("surface", [False, True])
def test_chunks(name, surface):
    """several chunks, the last one partial (1-D: 808 cells, 3-D: 256) or with nothing cut or full in it (2-D: 192 cells)"""
    lsm = _lsm()
    n, f, lc, hc, k, qo, cut_chunks, full_chunks, nchunk = _CHUNKED[name]
    vals, lc, hc = _grid_vals(n, f, lc, hc)
    ncell = int(np.prod([m - 1 for m in n]))
    assert -(-ncell // CHUNK) == nchunk and ncell % CHUNK != 0
    q = _quad(lsm, _device(lsm, vals, lc, hc, lsm.ExtrapolationBC(k)), k, qo, surface)
    c, fl = _structure(q)
    assert set(c // CHUNK) == cut_chunks and set(fl // CHUNK) == (set() if surface else full_chunks)
    assert q.ncut > 0 and (surface or q.nfull > 0)
    print(f"{name}: {ncell} cells, {q.ncut} cut, {q.nfull} full, {q.nnodes} nodes")
    _compare(q, _ref(vals, lc, hc, k, k), qo, surface, restated=restated(("chunks", name, surface), vals, lc, hc, k, qo, surface))


# ----------------------------------------------------------------------------- B, C: scan rounds, the second cell of a workgroup

def _stripes1_case(n, surface, sample):
    """k = 1, q = 1: every cell is cut and has the one node of the closed form; the restatement on the cells `sample`"""
    lsm = _lsm()
    vals, lc, hc = stripes1(n)
    ncell = int(np.prod([m - 1 for m in n]))
    t0 = time.perf_counter()
    q = _quad(lsm, _device(lsm, vals, lc, hc, lsm.ExtrapolationBC(1)), 1, 1, surface)
    print(f"stripes1{n}: ncut = {q.ncut}, nnodes = {q.nnodes}, {time.perf_counter() - t0:.2f} s on the device side")
    c, _ = _structure(q)
    assert q.ncut == ncell and q.nfull == 0 and q.nfallback == 0
    assert np.array_equal(c, np.arange(ncell)) and np.array_equal(q.offsets, np.arange(ncell + 1))
    X, W = stripes1_closed_form(n, surface)
    _close("device vs closed form", np.abs(q.coords - X).max(), np.abs(q.weights - W).max(), np.abs(W).max())
    dims = tuple(m - 1 for m in n)
    lin = np.unique(np.asarray(sample, dtype=np.int64))
    assert lin[0] == 0 and lin[-1] == ncell - 1
    cells = [tuple(int(v) for v in I) for I in zip(*np.unravel_index(lin, dims, order="F"))]
    _compare(q, _ref(vals, lc, hc, 1, 1), 1, surface, cells=cells)


@pytest.mark.parametrize("surface", [False, True])
def test_second_scan_round_every_cell_cut(surface):
    """9025 candidates: the scans of the node counts and of count != 0 run a second round of 8192 values"""
    ncell = 95 * 95
    assert SCAN < ncell < 2 * SCAN
    _stripes1_case((96, 96), surface, list(range(0, ncell, 7)) + list(range(8188, 8197)) + [ncell - 1])


def _pairs(ncell):
    """about 500 cells: pairs (ci, ci + 2^20) of one workgroup, the ends of both trips, the first and the last candidate"""
    second = ncell - GRID
    assert 1024 <= second < GRID
    first = np.unique(np.concatenate([np.linspace(0, second - 1, 247).astype(np.int64), [0, 1, second - 1]]))
    return np.concatenate([first, first + GRID, [GRID - 1, ncell - 1]])


@pytest.mark.parametrize("n", [(1025, 1100), (106, 106, 106)])
@pytest.mark.parametrize("surface", [False, True])
def test_second_cell_of_a_workgroup_every_cell_cut(n, surface):
    """more than 2^20 cut cells (the smallest such grids of these widths): quad_cells_kernel's loop runs a second trip in both
    passes, on LDS the first cell left behind"""
    _stripes1_case(n, surface, _pairs(int(np.prod([m - 1 for m in n]))))


def _stripes3_case(ny, qo, surface, rows):
    """k = 3, constant along y: the counts and the cells from the row pattern, the restatement node for node on `rows`, every
    row against the middle row"""
    lsm = _lsm()
    vals, lc, hc = stripes3(ny)
    nrow, mid, hy = ny - 1, (ny - 1) // 2, (hc[1] - lc[1]) / (ny - 1)
    ref = _ref(vals, lc, hc, 3, 3)
    cand, cut, full = row_pattern(ref, mid, qo, surface)
    cols, counts = np.array(sorted(cut)), np.array([len(cut[i][1]) for i in sorted(cut)])
    assert len(cand) == 18 and len(cols) == 12 and len(full) == (0 if surface else 6)
    t0 = time.perf_counter()
    q = _quad(lsm, _device(lsm, vals, lc, hc, lsm.ExtrapolationBC(3)), 3, qo, surface)
    print(f"stripes3({ny}): {len(cand) * nrow} candidates, ncut = {q.ncut}, nnodes = {q.nnodes}, nfull = {q.nfull}, "
          f"{time.perf_counter() - t0:.2f} s on the device side")
    _structure(q)
    assert q.ncut == 12 * nrow and q.nfull == len(full) * nrow and q.nfallback == 0 and q.nnodes == counts.sum() * nrow
    assert np.array_equal(q.cells[:, 0].reshape(nrow, 12), np.broadcast_to(cols, (nrow, 12)))
    assert np.array_equal(q.cells[:, 1], np.repeat(np.arange(nrow), 12))
    if not surface:
        assert np.array_equal(q.full_cells[:, 0].reshape(nrow, 6), np.broadcast_to(np.array(full), (nrow, 6)))
        assert np.array_equal(q.full_cells[:, 1], np.repeat(np.arange(nrow), 6))
    assert np.array_equal(np.diff(q.offsets).reshape(nrow, 12), np.broadcast_to(counts, (nrow, 12)))
    _compare(q, ref, qo, surface, cells=[(i, j) for j in sorted(set(rows) | {mid}) for i in range(60)])
    m = int(counts.sum())
    X, W = q.coords.reshape(nrow, m, 2), q.weights.reshape(nrow, m)
    dy = (X[:, :, 1] - (np.arange(nrow) * hy)[:, None]) - (X[mid, :, 1] - mid * hy)
    _close("rows vs the middle row", max(np.abs(X[:, :, 0] - X[mid, :, 0]).max(), np.abs(dy).max()), np.abs(W - W[mid]).max(),
           np.abs(W).max())
    return np.array([i not in cut for i in cand])      # which candidates of a row are empty


@pytest.mark.parametrize("surface", [False, True])
def test_second_scan_round_with_empty_candidates(surface):
    """8442 candidates, a third of them without nodes: the slots (scan of count != 0) and the node offsets differ, and both cross
    8192 in row 455"""
    ny = 470
    assert SCAN // 18 == 455
    _stripes3_case(ny, 2, surface, [0, 1, 2, 454, 455, 456, ny - 3, ny - 2])


@pytest.mark.parametrize("surface", [False, True])
def test_second_cell_of_a_workgroup_with_empty_candidates(surface):
    """1 080 000 candidates (3 % over 2^20): workgroups whose first candidate is empty and whose second is not, and the reverse
    (the emit pass skips an empty candidate with `continue`)"""
    ny = 60001
    ncand = 18 * (ny - 1)
    assert GRID + 1024 <= ncand <= 1.05 * GRID
    row = GRID // 18
    empty = _stripes3_case(ny, 1, surface, [0, 1, row - 1, row, row + 1, ny - 3, ny - 2])
    first, second = np.tile(empty, ny - 1)[:ncand - GRID], np.tile(empty, ny - 1)[GRID:]
    assert (first & ~second).any() and (~first & second).any() and (~first & ~second).any()


# ----------------------------------------------------------------------------- D: more than 8192 chunks

def test_chunk_scan_beyond_8192_chunks():
    """4096 x 8193 cells: 8193 chunks, one per cell row; a disc near the first rows and one crossing the last cell row, so the
    scan of the chunk counts runs a second round whose only chunk holds cut and full cells and receives a carry"""
    lsm = _lsm()
    n, lc, hc = (4097, 8194), (0.0, 0.0), (1.0, 2.5)
    ncell = (n[0] - 1) * (n[1] - 1)
    assert ncell == (SCAN + 1) * CHUNK
    t0 = time.perf_counter()
    vals = np.ones(n, order="F")
    windows = []
    for cx, cy, r in ((1500.3, 7.4, 6.2), (2901.6, n[1] - 1 - 2.7, 6.3)):
        i0, i1, j0, j1 = int(cx) - 9, int(cx) + 11, max(int(cy) - 9, 0), min(int(cy) + 11, n[1])
        I, J = np.meshgrid(np.arange(i0, i1), np.arange(j0, j1), indexing="ij")
        vals[i0:i1, j0:j1] = np.minimum(1.0, np.hypot(I - cx, J - cy) - r)
        windows.append((i0, i1, j0, j1))
    assert (vals[0] == 1.0).all() and all((vals[a:b, c:d] != 0.0).all() for a, b, c, d in windows)
    h = [(hc[d] - lc[d]) / (n[d] - 1) for d in range(2)]
    last = n[1] - 2
    phi = _device(lsm, vals, lc, hc, lsm.ExtrapolationBC(1))
    print(f"field and upload: {time.perf_counter() - t0:.2f} s")
    for surface in (False, True):
        # k = 1: the coefficients are the corner values
        cut, full = [], []
        for a, b, c, d in windows:
            w = vals[a:b, c:d]
            corners = np.stack([w[:-1, :-1], w[1:, :-1], w[:-1, 1:], w[1:, 1:]])
            mn, mx = corners.min(axis=0), corners.max(axis=0)
            lin = (a + np.arange(b - a - 1))[:, None] + (n[0] - 1) * (c + np.arange(d - c - 1))[None, :]
            cut.append(lin[(mn < 0.0) & (mx > 0.0)])
            full.append(lin[mx < 0.0])
        cut, full = np.sort(np.concatenate(cut)), np.sort(np.concatenate(full))
        t1 = time.perf_counter()
        q = _quad(lsm, phi, 1, 1, surface)
        print(f"surface = {surface}: ncut = {q.ncut}, nfull = {q.nfull}, nnodes = {q.nnodes}, {time.perf_counter() - t1:.2f} s")
        c, f = _structure(q)
        assert np.array_equal(c, cut) and np.array_equal(f, full if not surface else full[:0])
        assert (c // CHUNK == SCAN).any() and (c // CHUNK < 20).any() and (surface or (f // CHUNK == SCAN).any())
        cells = [(int(v % (n[0] - 1)), last) for v in cut if v // (n[0] - 1) == last]
        assert len(cells) >= 2
        _compare(q, _ref(vals, lc, hc, 1, 1), 1, surface, cells=cells)
        assert q.total() == pytest.approx(q.weights.sum() + q.nfull * h[0] * h[1], rel=1e-12)
    print(f"{ncell} cells: {time.perf_counter() - t0:.2f} s in all")


# ----------------------------------------------------------------------------- E: subdivision and fallback off the square grid

@pytest.mark.parametrize("name,qo", [("kink3d", 2), ("kink2d_aniso", 4), ("kink2d_aniso", 20)])
@pytest.mark.parametrize("surface", [False, True])
def test_depth_limit_and_fallback(name, qo, surface):
    lsm = _lsm()
    vals, lc, hc = kink(name)
    phi = _device(lsm, vals, lc, hc, lsm.ExtrapolationBC(3))
    with pytest.warns(UserWarning, match="subdivision limit"):
        q = lsm.quadrature(phi, interpolation_order=3, quadrature_order=qo, surface=surface)
    _structure(q)
    key = (name, surface) if qo == KINKS[name][2] else (name, surface, qo)
    _compare(q, _ref(vals, lc, hc, 3, 3), qo, surface, restated=restated(key, vals, lc, hc, 3, qo, surface))
    assert q.nfallback > 0


# ----------------------------------------------------------------------------- F: high quadrature orders

@pytest.mark.parametrize("N,k", [(1, 2), (1, 5), (2, 5)])
@pytest.mark.parametrize("qo", [3, 9, 20])
@pytest.mark.parametrize("surface", [False, True])
def test_high_orders_1d_2d(N, k, qo, surface):
    lsm = _lsm()
    vals, lc, hc = _grid_vals({1: (23,), 2: (9, 8)}[N], _SHAPES[N])
    q = _quad(lsm, _device(lsm, vals, lc, hc, lsm.ExtrapolationBC(k)), k, qo, surface)
    _structure(q)
    _compare(q, _ref(vals, lc, hc, k, k), qo, surface)


@pytest.mark.parametrize("qo", [3, 9])
@pytest.mark.parametrize("surface", [False, True])
def test_high_orders_3d(qo, surface):
    lsm = _lsm()
    vals, lc, hc = _grid_vals((5, 6, 5), _SHAPES[3])
    q = _quad(lsm, _device(lsm, vals, lc, hc, lsm.ExtrapolationBC(3)), 3, qo, surface)
    _structure(q)
    _compare(q, _ref(vals, lc, hc, 3, 3), qo, surface, restated=restated(("orders3d", qo, surface), vals, lc, hc, 3, qo, surface))


@pytest.mark.parametrize("surface", [False, True])
def test_order_20_in_3d(surface):
    """up to 72 000 nodes in a cell, lifted 64 at a time.  The restatement on four cut cells: the first, the last and the two
    with the most nodes at q = 3.  Elsewhere the node count: a cell with one node at q = 1 is one box whose base has no root (a
    base with a root has two pieces, so two nodes), so every line through a base node has the end signs of that one and the
    cell has 20³ nodes (volume) or 20² (surface)"""
    lsm = _lsm()
    vals, lc, hc = _grid_vals((5, 6, 5), _SHAPES[3])
    phi = _device(lsm, vals, lc, hc, lsm.ExtrapolationBC(3))
    ref = _ref(vals, lc, hc, 3, 3)
    cut3, _, _ = restated(("orders3d", 3, surface), vals, lc, hc, 3, 3, surface)
    cut1, full1, _ = restated(("orders3d", 1, surface), vals, lc, hc, 3, 1, surface)
    cells = sorted(cut3, key=lambda I: I[::-1])
    most = sorted(cells, key=lambda I: -len(cut3[I][1]))[:2]
    q = _quad(lsm, phi, 3, 20, surface)
    _structure(q)
    assert [tuple(int(v) for v in I) for I in q.cells] == cells and [tuple(int(v) for v in I) for I in q.full_cells] == full1
    _compare(q, ref, 20, surface, cells=[cells[0], cells[-1], *most])
    single = np.array([I in cut1 and len(cut1[I][1]) == 1 for I in cells])
    assert single.any()
    assert (np.diff(q.offsets)[single] == (400 if surface else 8000)).all()
    print(f"q = 20: {q.ncut} cut cells, {q.nnodes} nodes, at most {np.diff(q.offsets).max()} in a cell, {single.sum()} single-piece cells")


# ----------------------------------------------------------------------------- G: boundary conditions, float32, bands in 3-D

@pytest.mark.parametrize("bc,P", [("neumann", 0), ("linear", 1)])
@pytest.mark.parametrize("surface", [False, True])
def test_interface_across_the_boundary_3d(bc, P, surface):
    from test_gpu_isosurface import FIELDS
    lsm = _lsm()
    n, f, lc, hc = FIELDS["sphere_leaving"]
    vals, lc, hc = _grid_vals(n, f, lc, hc)
    phi = _device(lsm, vals, lc, hc, lsm.NeumannBC() if bc == "neumann" else lsm.LinearExtrapolationBC())
    q = _quad(lsm, phi, 3, 2, surface)
    _structure(q)
    assert (q.cells[:, 0] == n[0] - 2).any()         # cut cells on the face the sphere leaves through
    _compare(q, _ref(vals, lc, hc, P, 3), 2, surface)


def test_float32_storage_3d():
    lsm = _lsm()
    vals, lc, hc = _grid_vals((9, 10, 8), _SHAPES[3])
    v32 = np.asfortranarray(vals.astype(np.float32))
    phi = _device(lsm, v32, lc, hc, lsm.ExtrapolationBC(3), dtype=np.float32)
    for surface in (False, True):
        q = _quad(lsm, phi, 3, 4, surface)
        _structure(q)
        _compare(q, _ref(np.asfortranarray(v32.astype(np.float64)), lc, hc, 3, 3), 4, surface)


def _band(lsm, vals, lc, hc, mask, garbage):
    """a band field whose mask is `mask`, with garbage off it, and the halo list of that mask (as after any change of the mask
    from outside: tiles, then the halo search)"""
    from test_gpu_isosurface import _set_band
    grid = lsm.CartesianGrid(lc, hc, vals.shape)
    nb = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.NarrowBandMeshField(lsm.MeshField(vals, grid), nlayers=3),
                              bc=lsm.ExtrapolationBC(3)).current_state()
    _set_band(nb, mask, garbage=garbage)
    b = nb.backend
    b.band_retile(nb.mask, nb.tiles, nb.MC)
    b.band_status(nb._hcount)
    b.band_halo(nb.buf, nb.mask, nb.halo, nb.tiles, nb.MC, nb._hlist, nb._hcount)
    nb._check_halo()
    return nb


def _all_in(mask, cells, lo, hi):
    """per cell: every node I + (lo..hi)^N is in the grid and in the mask"""
    out = np.ones(len(cells), dtype=bool)
    for J in itertools.product(range(lo, hi + 1), repeat=mask.ndim):
        idx = cells + np.array(J)
        ok = ((idx >= 0) & (idx < np.array(mask.shape))).all(axis=1)
        out &= ok
        out[ok] &= mask[tuple(idx[ok].T)]
    return out


@pytest.mark.parametrize("n", [(41, 41), (17, 16, 15)])
def test_bands_read_band_values_only(n):
    lsm = _lsm()
    N = len(n)
    vals, lc, hc = _grid_vals(n, _SHAPES[N])
    dense = _quad(lsm, _device(lsm, vals, lc, hc, lsm.ExtrapolationBC(3)), 3, 4, True)
    assert dense.ncut > 0
    # (i) the narrowest band |ϕ| < w that holds the 4^N stencil nodes (offsets -1..2) of every dense cut cell
    stencil = np.zeros(n, dtype=bool)
    for J in itertools.product(range(-1, 3), repeat=N):
        idx = dense.cells + np.array(J)
        assert ((idx >= 0) & (idx < np.array(n))).all()          # the interface stays away from the boundary
        stencil[tuple(idx.T)] = True
    mask = np.abs(vals) <= np.abs(vals[stencil]).max()
    assert stencil[mask].sum() == stencil.sum() and not mask.all()
    garbage = np.random.default_rng(7).choice([-7.0, 7.0], size=n)
    qb = _quad(lsm, _band(lsm, vals, lc, hc, mask, garbage), 3, 4, True)
    for x, y in ((dense.cells, qb.cells), (dense.offsets, qb.offsets), (dense.coords, qb.coords), (dense.weights, qb.weights)):
        assert np.array_equal(x, y)
    # (ii) the same band cut at x = 0: cells whose whole stencil is on the band keep the dense nodes bit for bit
    ax0 = np.linspace(lc[0], hc[0], n[0]).reshape((-1,) + (1,) * (N - 1))
    half = mask & (ax0 < 0.0)
    qh = _quad(lsm, _band(lsm, vals, lc, hc, half, garbage), 3, 4, True)
    _structure(qh)
    assert _all_in(half, qh.cells, 0, 1).all()                   # active cells: the 2^N corners on the band
    whole = _all_in(half, dense.cells, -1, 2)
    inner = _all_in(half, qh.cells, -1, 2)
    assert whole.any() and not whole.all() and inner.any() and not inner.all()
    assert np.array_equal(qh.cells[inner], dense.cells[whole])
    for i, j in zip(np.flatnonzero(inner), np.flatnonzero(whole)):
        a, b = slice(qh.offsets[i], qh.offsets[i + 1]), slice(dense.offsets[j], dense.offsets[j + 1])
        assert np.array_equal(qh.coords[a], dense.coords[b]) and np.array_equal(qh.weights[a], dense.weights[b])
    print(f"{n}: band of {mask.sum()} of {mask.size} nodes, {dense.ncut} cut cells; half band: {qh.ncut} cells, {inner.sum()} with their whole stencil")
