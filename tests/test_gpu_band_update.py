"""update_band! in 3-D on many tiles, on faces and under motion — every implementation (the bit-row kernels, the fused byte
kernels, the generic byte kernels, the unfused cut / dilate / tiles chain; over compact tile lists and over work flags) against
the literal restatement of the reference's algorithms (tests/_nb_ref.py), bit for bit and after every update of a sequence:
the band set and its count, the kept values and the new nodes' extrapolants, the tile flags, the halo mask, the halo list's
length and what lsm_band_prepare writes on the halo.  No tolerance anywhere.

The restatement sequences are computed once per (field, nlayers, element type) and shared by the device variants."""
import copy
import functools
import itertools

import numpy as np
import pytest

from _nb_ref import NBRef

MC = 16                      # planes per tile the cases below are laid out for
TILE = (32, 8, MC)
HALO = 3                     # LSM_GHOST: what a stencil centred on a band node reads along each axis
RESOLVED = 0x40              # BandEntry::d[3]: slope neighbours resolved — set by band_halo_bits_kernel only


@pytest.fixture(scope="module")
def lsm():
    import lsm_amd
    if lsm_amd.api.ROCNarrowBandMeshField.MC != MC:
        pytest.skip("the cases are laid out for 32 x 8 x 16 tiles")
    assert lsm_amd.api.ROCNarrowBandMeshField.MC == 16
    return lsm_amd


# ----------------------------------------------------------------------------- what the restatement says, as arrays

def _ntiles(n):
    return tuple(-(-n[d] // TILE[d]) for d in range(3))


def _tile_flags(mask):
    """flags[X, Y, M] of the 32 x 8 x MC tiles holding a node of `mask`; the device's index X + nbx (Y + nby M) is the F-order ravel"""
    nb = _ntiles(mask.shape)
    pad = np.zeros(tuple(nb[d] * TILE[d] for d in range(3)), dtype=bool)
    pad[:mask.shape[0], :mask.shape[1], :mask.shape[2]] = mask
    return pad.reshape(nb[0], TILE[0], nb[1], TILE[1], nb[2], TILE[2]).any(axis=(1, 3, 5))


def _or_shifted(out, src, off):
    """out[I] |= src[I - off] wherever both lie in the grid"""
    dst, frm = [], []
    for d, o in enumerate(off):
        n = src.shape[d]
        dst.append(slice(max(o, 0), n + min(o, 0)))
        frm.append(slice(max(-o, 0), n + min(-o, 0)))
    out[tuple(dst)] |= src[tuple(frm)]


def _halo_set(band):
    """The comment above lsm_band_halo: the in-grid nodes stencils centred on band nodes read directly — LSM_GHOST nodes along
    each axis and the 3^3 box (the band itself included)."""
    h = band.copy()
    for d in range(3):
        for k in range(1, HALO + 1):
            for s in (-k, k):
                _or_shifted(h, band, tuple(s if e == d else 0 for e in range(3)))
    for off in itertools.product((-1, 0, 1), repeat=3):
        _or_shifted(h, band, off)
    return h


def _pack(m):
    return np.packbits(m.ravel())


def _bits(a, f32):
    """the bit patterns of `a` in the field's element type"""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32) if f32 else np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


class _Step:
    """One state of a sequence: the restatement's band, values, tile flags, halo and halo extrapolants."""

    def __init__(self, ref, f32):
        self.n = ref.n
        self.snap = copy.copy(ref)                  # (the offset ring is shared)
        self.snap.d = dict(ref.d)
        band = ref.mask()
        self._band = _pack(band)
        self.count = len(ref.d)
        self.bval = ref.dense()[band]               # in the order of a boolean index
        self.tiles = _tile_flags(band)
        halo = _halo_set(band)
        self._halo = _pack(halo)
        self.f32 = f32
        self.tval = np.array([self.extrapolate(tuple(int(i) for i in I)) for I in np.argwhere(halo & ~band)])
        self.memo = {}                              # extrapolants of boundary-condition sources outside that set, as asked for

    def _unpack(self, p):
        return np.unpackbits(p, count=int(np.prod(self.n))).reshape(self.n).astype(bool)

    def band(self):
        return self._unpack(self._band)

    def halo(self):
        return self._unpack(self._halo)

    def extrapolate(self, I):
        v = self.snap.extrapolate(I)                # fp64 arithmetic, rounded once on store
        return float(np.float32(v)) if self.f32 else v

    def extrapolate_memo(self, I):
        if I not in self.memo:
            try:
                self.memo[I] = self.extrapolate(I)
            except ValueError:
                self.memo[I] = None
        return self.memo[I]


def _round_f32(ref):
    ref.d = {I: float(np.float32(v)) for I, v in ref.d.items()}


# ----------------------------------------------------------------------------- 1. interior band

INT_N = (192, 48, 96)                    # 6 x 6 x 6 tiles; h = 1
INT_A = (20.0, 3.6, 3.4)
INT_C = (95.3, 23.6, 39.6)
INT_V = (0.35, 0.0, 0.9)                 # motion of the centre per step
INT_STEPS = 18
# nlayers = 1: a band one node thick loses the cut cells whose corners the moved surface has left behind, and decays when the
# surface moves fast.  The largest multiple of INT_V, among k / 20, at which the restatement's band never falls below half its
# initial node count over the 18 steps, checked on the CPU: 3145 nodes at first, 1747 after step 18 at 1.25 (and 1463 < 1572.5
# after step 17 at 1.30); the band's tiles still keep two tiles from every face.
NL1_DRIFT = 1.25
NL1_COUNTS = (3145, 1747)                # the first and the smallest node count of that sequence


# Two spheres, the second moving towards the first until their bands merge.  A convex band never offers two nearest band nodes
# to choose from; the gap between these two bands narrows through every width, so that the ring's tie-breaks (lower z, then
# lower y, then lower x wins) decide the nearest node of many halo nodes and new band nodes.
GAP_R = 3.5
GAP_C1 = (86.3, 23.7, 44.2)
GAP_C2 = (106.9, 24.3, 46.3)
GAP_V = (-0.8, -0.04, -0.1)
GAP_STEPS = 14


def _interior_field(field, step, drift, f32):
    X = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in INT_N], indexing="ij", sparse=True)
    if field == "ellipsoid":
        c = [INT_C[d] + step * drift * INT_V[d] for d in range(3)]
        r = np.sqrt(sum(((X[d] - c[d]) / INT_A[d]) ** 2 for d in range(3)))
        phi = (r - 1.0) * min(INT_A)
    else:
        c2 = [GAP_C2[d] + step * drift * GAP_V[d] for d in range(3)]
        phi = np.minimum(np.sqrt(sum((X[d] - GAP_C1[d]) ** 2 for d in range(3))), np.sqrt(sum((X[d] - c2[d]) ** 2 for d in range(3)))) - GAP_R
    phi = np.asfortranarray(phi)
    return np.asfortranarray(phi.astype(np.float32).astype(np.float64)) if f32 else phi


def _nearest_ties(band, lo, hi):
    """Among the halo nodes of the box [lo, hi]: how many have several band nodes at the smallest distance, and how many of those
    have two of them on one x-line."""
    box = tuple(slice(lo[d] - 3, hi[d] + 4) for d in range(3))
    b = band[box]
    best = np.full(b.shape, 1 << 20)
    cnt = np.zeros(b.shape, dtype=np.int64)
    lines = np.zeros(b.shape, dtype=np.int64)          # distinct (o_y, o_z) lines holding a nearest node
    for oy, oz in itertools.product(range(-3, 4), repeat=2):
        lbest = np.full(b.shape, 1 << 20)
        lcnt = np.zeros(b.shape, dtype=np.int64)
        for ox in range(-3, 4):
            sh = np.zeros(b.shape, dtype=bool)
            _or_shifted(sh, b, (-ox, -oy, -oz))         # sh[I] = b[I + off]
            d2 = np.where(sh, ox * ox + oy * oy + oz * oz, 1 << 20)
            lcnt = np.where(d2 < lbest, 1, lcnt + ((d2 == lbest) & sh))
            lbest = np.minimum(lbest, d2)
        lines = np.where(lbest < best, 1, lines + ((lbest == best) & (lbest < (1 << 20))))
        cnt = np.where(lbest < best, lcnt, np.where(lbest == best, cnt + lcnt, cnt))
        best = np.minimum(best, lbest)
    tgt = _halo_set(b) & ~b
    return int((tgt & (cnt > 1)).sum()), int((tgt & (cnt > lines)).sum())


def _seed_box(vals, lo, hi):
    """Seed mask of the box [lo, hi] with the checks that make a seeded restatement equal the unseeded one: the field is positive
    outside the box and on its outermost layer, so every cut cell has all its corners inside."""
    seed = np.zeros(vals.shape, dtype=bool)
    seed[tuple(slice(lo[d], hi[d] + 1) for d in range(3))] = True
    inner = np.zeros(vals.shape, dtype=bool)
    inner[tuple(slice(lo[d] + 1, hi[d]) for d in range(3))] = True
    assert (vals[~inner] > 0).all()
    return seed, inner


@functools.lru_cache(maxsize=None)
def _interior_sequence(field, nlayers, f32, drift):
    phi = _interior_field(field, 0, drift, f32)
    if field == "ellipsoid":
        lo = [int(INT_C[d] - INT_A[d]) - 9 for d in range(3)]
        hi = [int(INT_C[d] + INT_A[d]) + 10 for d in range(3)]
    else:
        lo = [int(min(GAP_C1[d], GAP_C2[d]) - GAP_R) - 9 for d in range(3)]
        hi = [int(max(GAP_C1[d], GAP_C2[d]) + GAP_R) + 10 for d in range(3)]
    seed, inner = _seed_box(phi, lo, hi)
    ref = NBRef(phi, nlayers, seed=seed)
    assert not (ref.mask() & ~inner).any()          # no band node on the box's outermost layer
    steps = [_Step(ref, f32)]
    for s in range(1, (INT_STEPS if field == "ellipsoid" else GAP_STEPS) + 1):
        new = _interior_field(field, s, drift, f32)
        ref.d = {I: float(new[I]) for I in ref.d}
        ref.update_band()
        if f32:
            _round_f32(ref)
        steps.append(_Step(ref, f32))
    # what the cases rely on: no work tile on a face of the tile grid (the band's tiles keep two tiles from every face), the band
    # on both sides of a tile boundary in x and in y, and tiles that become active and tiles that become empty
    nb = _ntiles(INT_N)
    gained = lost = 0
    for k, st in enumerate(steps):
        T = np.argwhere(st.tiles)
        for d in range(3):
            assert T[:, d].min() >= 2 and T[:, d].max() <= nb[d] - 3, (k, d)
        assert len(np.unique(T[:, 0])) > 1 and len(np.unique(T[:, 1])) > 1
        if k:
            gained += int((st.tiles & ~steps[k - 1].tiles).sum())
            lost += int((~st.tiles & steps[k - 1].tiles).sum())
    assert 2 * min(st.count for st in steps) >= steps[0].count      # the band never decays to less than half
    if field == "ellipsoid":
        assert gained > 0 and lost > 0
    else:                                                           # nearest nodes decided by the tie-breaks, along x and across lines
        ties = [_nearest_ties(st.band(), lo, hi) for st in steps]
        assert sum(t[1] for t in ties) > 100 and sum(t[0] - t[1] for t in ties) > 100
    return tuple(steps)


# ----------------------------------------------------------------------------- 3. bands on faces and partial tiles

FACE_N = (70, 20, 36)                    # 2 full tiles and a partial one along every axis: 6, 4 and 4 nodes
FACE_SHIFTS = (-0.9, 1.7, -0.8) * 3      # in units of h = min(meshsize)
FACE_H = 2.0 / 69.0


def _face_field(which, f32):
    """the sphere of test_band_stage_reads_reference_values_at_the_grid_boundary ("low") and its mirror image in x ("high")"""
    ax = [np.linspace(-1.0, 1.0, n) for n in FACE_N]
    X = np.meshgrid(*ax, indexing="ij", sparse=True)
    ctr = (-0.85 if which == "low" else 0.85, -0.7, 0.75)
    phi = np.asfortranarray(np.sqrt(sum((X[d] - ctr[d]) ** 2 for d in range(3))) - 0.62)
    return np.asfortranarray(phi.astype(np.float32).astype(np.float64)) if f32 else phi


def _face_shift(step, f32):
    s = FACE_SHIFTS[step - 1] * FACE_H
    return float(np.float32(s)) if f32 else s


def _shifted(vals, step, f32):
    """the stored values after the step's constant shift, in the field's element type"""
    s = _face_shift(step, f32)
    return (vals.astype(np.float32) + np.float32(s)) if f32 else vals + s


@functools.lru_cache(maxsize=None)
def _face_sequence(which, nlayers, f32):
    ref = NBRef(_face_field(which, f32), nlayers)
    band = ref.mask()
    assert band[0].any() if which == "low" else band[64:].any()      # on the x face; "high": in the 6-node tile (the hi < 8 loads)
    assert band[:, 0].any() and band[:, :, -1].any()
    steps = [_Step(ref, f32)]
    for s in range(1, len(FACE_SHIFTS) + 1):
        ref.d = dict(zip(ref.d.keys(), _shifted(np.array(list(ref.d.values())), s, f32).tolist()))
        ref.update_band()
        if f32:
            _round_f32(ref)
        steps.append(_Step(ref, f32))
    return tuple(steps)


# ----------------------------------------------------------------------------- the device against a sequence

def _list_flags(st):
    """BandEntry::d[3] of the halo list's entries (int64 pairs: the second word's top byte)"""
    n = int(st._hcount.item())
    words = st._hlist[:2 * n].cpu().numpy()[1::2]
    return (words >> 56) & 0xff


def _check(st, rec, interior, resolved):
    b, f32 = st.backend, rec.f32
    band = rec.band()
    assert np.array_equal(st.active_mask(), band)
    assert st.active_count() == rec.count
    assert np.array_equal(_bits(b.download(st.buf)[band], f32), _bits(rec.bval, f32))        # kept values and new nodes' extrapolants
    assert np.array_equal(st.tiles.cpu().numpy() != 0, rec.tiles.ravel(order="F"))
    halo, want_halo = b.mask_to_host(st.halo), rec.halo()
    if interior:
        assert np.array_equal(halo, want_halo)
    else:
        assert not (want_halo & ~halo).any()                     # + the boundary-condition sources
    nh = int(halo.sum() - band.sum())
    assert int(st._hcount.item()) == nh
    assert b.band_status(st._hcount) == (nh, False)              # nothing farther than the search radius
    if resolved is not None:
        flags = _list_flags(st)
        assert len(flags) == nh > 0
        assert ((flags & RESOLVED) != 0).all() if resolved else ((flags & RESOLVED) == 0).all()
    st.prepare(st.buf)
    dense = b.download(st.buf)
    assert np.array_equal(_bits(dense[band], f32), _bits(rec.bval, f32))
    assert np.array_equal(_bits(dense[want_halo & ~band], f32), _bits(rec.tval, f32))
    left_out = 0
    for I in np.argwhere(halo & ~want_halo):                     # boundary-condition sources: empty in the interior sequences
        I = tuple(int(i) for i in I)
        want = rec.extrapolate_memo(I)
        if want is None:                                         # more than 6 nodes from the band: the reference throws
            left_out += 1
            continue
        assert _bits(dense[I], f32) == _bits(want, f32), I
    assert left_out < 0.01 * halo.sum()
    return nh - left_out


def _equation(lsm, vals, n, box, nlayers, f32, bc, tuning):
    grid = lsm.CartesianGrid(box[0], box[1], n)
    phi = lsm.MeshField(vals, grid, dtype=np.float32 if f32 else np.float64)
    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.NarrowBandMeshField(phi, nlayers=nlayers), bc=bc,
                              tuning=tuning)
    for k, v in (tuning or {}).items():
        assert eq.backend.get_tuning(k) == v
    return eq


def _run_interior(lsm, field, nlayers, f32, drift, bc, tuning, resolved):
    seq = _interior_sequence(field, nlayers, f32, drift)
    eq = _equation(lsm, _interior_field(field, 0, drift, f32), INT_N, ((0.0,) * 3, tuple(float(n - 1) for n in INT_N)), nlayers, f32, bc, tuning)
    st = eq.current_state()
    assert min(st.mesh.meshsize()) == max(st.mesh.meshsize()) == 1.0
    compared = _check(st, seq[0], True, None)
    for s in range(1, len(seq)):
        st.backend.upload(st.buf, _interior_field(field, s, drift, f32))
        st.rebuild(from_dense=False)
        compared += _check(st, seq[s], True, resolved)           # from the first update on: which kernel wrote the list
    return compared


def _run_face(lsm, which, nlayers, f32, bc, tuning):
    seq = _face_sequence(which, nlayers, f32)
    eq = _equation(lsm, _face_field(which, f32), FACE_N, ((-1.0,) * 3, (1.0,) * 3), nlayers, f32, bc, tuning)
    st = eq.current_state()
    assert min(st.mesh.meshsize()) == FACE_H
    compared = _check(st, seq[0], False, None)
    for s in range(1, len(seq)):
        st.backend.upload(st.buf, _shifted(st.backend.download(st.buf), s, f32))
        st.rebuild(from_dense=False)
        compared += _check(st, seq[s], False, None)
    return compared


# ----------------------------------------------------------------------------- CPU: the seed option, the sequences' premises

def test_seeded_restatement_equals_the_unseeded_one():
    """NBRef(vals, nl, seed=box) holds the dict of NBRef(vals, nl) when the surface lies inside the box."""
    phi = _face_field("low", False)
    lo, hi = (0, 0, 12), (36, 16, 35)
    seed = np.zeros(FACE_N, dtype=bool)
    seed[tuple(slice(lo[d], hi[d] + 1) for d in range(3))] = True
    inner = np.zeros(FACE_N, dtype=bool)                  # the box without its outermost layer, except where that is the grid's face
    inner[tuple(slice(lo[d] + (lo[d] > 0), hi[d] + 1 - (hi[d] < FACE_N[d] - 1)) for d in range(3))] = True
    assert (phi[~inner] > 0).all()
    a, b = NBRef(phi, 3, seed=seed), NBRef(phi, 3)
    assert len(a.d) > 1000 and a.d == b.d
    assert not (a.mask() & ~inner).any()
    a.d = {I: v - 0.9 * FACE_H for I, v in a.d.items()}
    b.d = {I: v - 0.9 * FACE_H for I, v in b.d.items()}
    a.update_band()
    b.update_band()
    assert a.d == b.d


def test_the_sequences_leave_no_boundary_source_beyond_the_search_radius():
    """The face cases leave out halo nodes the restatement cannot extrapolate (boundary-condition sources more than 6 nodes from
    the band) and cap them at 1 % of the halo.  The restatement alone against that cap, with the sources of the widest
    boundary condition of the cases (ExtrapolationBC(5) beside the thinnest band, nlayers = 3) restated here, generously: nodes
    0..5 of every line through a face node that is read, the last dimension resolved first as _getindexbc does."""
    for which in ("low", "high"):
        extra = 0
        for rec in _face_sequence(which, 3, False):
            halo = rec.halo()
            src = halo.copy()
            for d in (2, 1, 0):
                s = np.moveaxis(src, d, 0)
                lo, hi = s[0].copy(), s[-1].copy()
                s[:6] |= lo
                s[-6:] |= hi
            far = 0
            for I in np.argwhere(src & ~halo):
                if rec.extrapolate_memo(tuple(int(i) for i in I)) is None:
                    far += 1
            extra += int((src & ~halo).sum())
            assert far < 0.01 * src.sum()
        assert extra > 0


# ----------------------------------------------------------------------------- GPU

def _bcs(lsm):
    return {"neumann": lsm.NeumannBC(), "ext2": lsm.ExtrapolationBC(2), "ext4": lsm.ExtrapolationBC(4),
            "ext5x": (lsm.ExtrapolationBC(5), lsm.ExtrapolationBC(2), lsm.ExtrapolationBC(2))}


@pytest.mark.gpu
@pytest.mark.parametrize("nlayers,dtype,bc", [(3, "float64", "neumann"), (2, "float32", "ext2"), (1, "float64", "neumann")])
def test_interior_band_on_the_bit_row_path_matches_the_restatement_bitwise(lsm, nlayers, dtype, bc):
    """1. An ellipsoid's band on 6 x 6 x 6 tiles, two tiles from every face, across the tile boundaries x = 96 and y = 24, moved 18
    times with tiles becoming active and empty: band_bits / band_grow_bits / band_halo_bits (every list entry says so: 0x40)."""
    drift = NL1_DRIFT if nlayers == 1 else 1.0
    if nlayers == 1:
        counts = [st.count for st in _interior_sequence("ellipsoid", 1, False, drift)]
        assert (counts[0], min(counts)) == NL1_COUNTS
    assert _run_interior(lsm, "ellipsoid", nlayers, dtype == "float32", drift, _bcs(lsm)[bc], None, True) > 50000


@pytest.mark.gpu
@pytest.mark.parametrize("nlayers,dtype,bc,tuning", [(3, "float64", "neumann", {"LSM_BAND_BITS": 0}), (2, "float32", "ext2", {"LSM_BAND_BITS": 0}),
                                                    (3, "float64", "neumann", {"LSM_BAND_BYTES": 1}), (3, "float64", "neumann", {"LSM_BAND_NO_LISTS": 1})])
def test_interior_band_on_the_other_paths_matches_the_restatement_bitwise(lsm, nlayers, dtype, bc, tuning):
    """2. The same sequences through the fused byte kernels (band_grow3 / band_search3), the generic byte kernels (band_grow /
    band_extrapolate) and the bit-row update over work flags instead of tile lists: none of them writes a resolved entry."""
    assert _run_interior(lsm, "ellipsoid", nlayers, dtype == "float32", 1.0, _bcs(lsm)[bc], tuning, False) > 50000


@pytest.mark.gpu
@pytest.mark.parametrize("nlayers,dtype,bc,tuning", [(3, "float64", "neumann", None), (2, "float32", "ext2", None),
                                                    (3, "float64", "neumann", {"LSM_BAND_BITS": 0})])
def test_two_bands_closing_a_gap_match_the_restatement_bitwise(lsm, nlayers, dtype, bc, tuning):
    """Not a case of the convex sequences: halo nodes and new band nodes with two nearest band nodes on one x-line, in the gap
    between the bands of two spheres that approach each other until they merge — the nearest-node tie-break along x (the
    lower x wins) of the bit-row search tables and of band_search3_kernel's."""
    assert _run_interior(lsm, "gap", nlayers, dtype == "float32", 1.0, _bcs(lsm)[bc], tuning, tuning is None) > 40000


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["low", "high"])
@pytest.mark.parametrize("nlayers,dtype,bc,tuning", [
    (3, "float64", "ext2", None), (3, "float32", "ext2", None),
    (3, "float64", "ext2", {"LSM_BAND_BITS": 0}), (3, "float64", "ext2", {"LSM_BAND_NO_LISTS": 1}),
    (3, "float64", "ext5x", None),                       # reach 5: 3 + 5 <= 8, still local
    (4, "float64", "ext2", None), (5, "float64", "ext2", None),   # local, fused byte kernels
    (5, "float64", "ext4", None),                        # 5 + 4 > 8: every tile is visited
    (8, "float64", "ext2", {"LSM_BAND_BYTES": 1}),       # tile + apron 9 = 50·26·34 bytes > LSM_BAND_LDS: band_cut / band_dilate / band_tiles
])
def test_band_on_faces_and_partial_tiles_matches_the_restatement_bitwise(lsm, which, nlayers, dtype, bc, tuning):
    """3. A sphere's band in a corner of a (70, 20, 36) grid — partial last tiles of 6, 4 and 4 nodes; "high": the band inside the
    6-node tile — under nine constant shifts of the stored values."""
    assert _run_face(lsm, which, nlayers, dtype == "float32", _bcs(lsm)[bc], tuning) > 20000
