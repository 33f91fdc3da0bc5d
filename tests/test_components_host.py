"""components on the host: the restatement (tests/_cc_ref.py) against scipy.ndimage.label with the Kuhn structure element and
against the vertex-connected pieces of the reference volume mesh (tests/_vol_ref.py); the identities of the statistics; the
flip rule of remove_components_; the ABI rows.  Every comparison is for equality."""
import os
import re

import numpy as np
import pytest

import _cc_ref as R
import _vol_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CC_SYMBOLS = ("lsm_cc_create", "lsm_cc_read", "lsm_cc_flip", "lsm_cc_destroy")

GRIDS = ((9, 8), (23, 17), (7, 6, 5), (11, 9, 10))
FRACTIONS = (0.2, 0.35, 0.5, 0.7)


def kuhn_structure(N):
    """scipy's structure element of the Kuhn adjacency: the centre and ±d, d ∈ {0,1}^N without 0"""
    s = np.zeros((3,) * N, dtype=bool)
    s[(1,) * N] = True
    for d in R.kuhn_offsets(N):
        s[tuple(1 + k for k in d)] = True
        s[tuple(1 - k for k in d)] = True
    return s


def test_the_kuhn_structure_has_6_and_14_neighbours():
    assert int(kuhn_structure(2).sum()) == 7 and int(kuhn_structure(3).sum()) == 15
    assert len(R.kuhn_offsets(2)) == 3 and len(R.kuhn_offsets(3)) == 7


@pytest.mark.parametrize("n", GRIDS + ((45, 19), (13, 12, 11)), ids=str)
@pytest.mark.parametrize("side", R.SIDES)
def test_restatement_against_scipy(n, side):
    ndi = pytest.importorskip("scipy.ndimage")
    for k, frac in enumerate(FRACTIONS):
        vals = R.random_field(n, frac, 100 + k)[0]
        mine = R.labels(vals, 0.0, side)
        theirs, K = ndi.label(R.in_set(vals, 0.0, side), structure=kuhn_structure(len(n)))
        assert R.stats(mine)[0] == K
        assert np.array_equal(mine >= 0, theirs > 0) and R.same_partition(mine, theirs)
        # the numbering: ascending smallest linear index, axis 0 fastest
        flat = mine.reshape(-1, order="F")
        first = [int(np.flatnonzero(flat == c)[0]) for c in range(K)]
        assert first == sorted(first)


def test_the_kuhn_adjacency_is_not_an_image_library_connectivity():
    """the (1, 1) diagonal joins, the (1, −1) diagonal does not"""
    a = np.ones((4, 4))
    a[1, 1] = a[2, 2] = -1.0
    assert R.count(a) == 1
    b = np.ones((4, 4))
    b[1, 2] = b[2, 1] = -1.0
    assert R.count(b) == 2


@pytest.mark.parametrize("n", GRIDS, ids=str)
def test_components_are_the_pieces_of_the_volume_mesh(n):
    lc, hc = tuple(0.0 for _ in n), tuple(1.0 for _ in n)
    for k, frac in enumerate(FRACTIONS):
        vals = R.random_field(n, frac, 200 + k)[0]
        verts, elems, _ = V.volume_mesh(vals, lc, hc)
        assert R.count(vals) == R.mesh_components(elems, len(verts)), (n, frac)


@pytest.mark.parametrize("name", ("spiral", "serpentine", "bodies", "shell", "isolated", "diagonals"))
def test_fixture_counts(name):
    vals = getattr(R, name)()[0]
    want = {"spiral": (1, 1), "serpentine": (1, None), "bodies": (3, 1), "shell": (1, 2), "isolated": (2275, 1), "diagonals": (67, None)}[name]
    assert R.count(vals) == want[0]
    if want[1] is not None:
        assert R.count(vals, side="outside") == want[1]


@pytest.mark.parametrize("delta", R.CORNER_DIRECTIONS, ids=str)
def test_corner_fixture(delta):
    assert R.count(R.corner(delta)[0]) == R.corner_count(delta)
    assert sum(R.corner_count(d) == 1 for d in R.CORNER_DIRECTIONS) == 7


def test_statistics_identities():
    for n, frac in (((23, 17), 0.5), ((11, 9, 10), 0.3)):
        vals, lc, hc = R.random_field(n, frac, 5)
        lab = R.labels(vals)
        K, nodes, sums, bbox = R.stats(lab)
        assert int(nodes.sum()) == int((vals < 0).sum()) and (nodes > 0).all()
        cent = sums / nodes[:, None]
        assert (bbox[:, 0, :] <= cent).all() and (cent <= bbox[:, 1, :]).all()
        for c in (0, K - 1):
            idx = np.argwhere(lab == c)
            assert np.array_equal(idx.sum(axis=0), sums[c]) and np.array_equal(idx.min(axis=0), bbox[c, 0]) and np.array_equal(idx.max(axis=0), bbox[c, 1])


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("level", (0.0, 0.25, 1e300 * 0))
@pytest.mark.parametrize("side", R.SIDES)
def test_flip_lands_on_the_other_side(dtype, level, side):
    rng = np.random.default_rng(11)
    vals = (rng.random((19, 14)) - 0.5 + level).astype(dtype)
    # values next to the level, where the mirror image rounds onto it or across it
    lv = dtype(level)
    near = [lv, np.nextafter(lv, dtype(np.inf)), np.nextafter(lv, dtype(-np.inf)), dtype(level + 1e-30), dtype(level - 1e-30),
            dtype(level - 1e-9), dtype(level + 1e-9)]
    vals.reshape(-1)[:len(near)] = near
    vals = np.asfortranarray(vals)
    lab = R.labels(vals, level, side)
    K = R.stats(lab)[0]
    which = np.ones(K, dtype=bool)
    which[::3] = False
    out, flipped = R.flip(vals, lab, which, level, side, dtype)
    sel = (lab >= 0) & which[np.where(lab >= 0, lab, 0)]
    assert out.dtype == np.dtype(dtype) and flipped == int(sel.sum()) > 0
    assert np.array_equal(out[~sel].view(np.uint8), vals[~sel].view(np.uint8))
    assert not R.in_set(out, level, side)[sel].any()
    # and what stays is still where it was
    assert np.array_equal(R.in_set(out, level, side)[~sel], R.in_set(vals, level, side)[~sel])


def test_abi_rows():
    """the header, the ctypes table and the built library list the four lsm_cc_* symbols"""
    from lsm_amd import _lib
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "lsm.h")).read(), flags=re.S)
    for sym in CC_SYMBOLS:
        assert re.search(rf"\b{sym}\s*\(", header), f"{sym} is not declared in include/lsm.h"
        assert sym in _lib.EXPORTS, f"{sym} is not in _lib.EXPORTS"
    lib = _lib.lib()        # loads without a device
    for sym in CC_SYMBOLS:
        assert hasattr(lib, sym), f"{sym} is not exported by the library"


def test_many_tiles_fraction():
    """the fraction the GPU test uses puts between 10 % and 90 % of the set into the largest cluster"""
    vals = R.random_field(R.MANY_TILES_SHAPE, R.MANY_TILES_FRACTION, R.MANY_TILES_SEED)[0]
    share = R.largest_share(vals)
    assert 0.1 < share < 0.9
    assert round(share, 3) == R.MANY_TILES_SHARE
