"""components / remove_components_ / prune_ on the device (csrc/lsm_cc.hip through the Python API) against the restatement
(tests/_cc_ref.py).  Labels, K, nodes, index_sums, bbox and stats[0:2] are integers and the flipped values are defined operation
by operation: every comparison is for equality.  The tiles are 8×8×8 in 3-D and 32×8 in 2-D; the fixtures are the smallest
shapes at which each kernel can go wrong: inside one tile, partial tiles, clusters sprawling over tiles at the percolation
threshold (the merge), more one-node components than two numbering chunks of 4096 nodes hold rows for, diagonals, a spiral and
a serpentine (long paths), the 13 directions across a tile corner, bodies, a shell, all and none inside, many tiles."""
import functools

import numpy as np
import pytest

import _cc_ref as R

pytestmark = pytest.mark.gpu


def _lsm():
    import lsm_amd
    return lsm_amd


def _field(lsm, vals, lc, hc, dtype=None, bc=None):
    mf = lsm.MeshField(vals, lsm.CartesianGrid(lc, hc, vals.shape), dtype=dtype)
    return lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=mf, bc=bc or lsm.NeumannBC()).current_state()


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


FIXTURES = {
    "one_tile_2d-0": lambda: R.random_field((29, 7), 0.5, 0), "one_tile_2d-1": lambda: R.random_field((29, 7), 0.5, 1),
    "one_tile_2d-2": lambda: R.random_field((29, 7), 0.5, 2),
    "partial_2d-0": lambda: R.random_field((45, 19), 0.5, 0), "partial_2d-1": lambda: R.random_field((45, 19), 0.5, 1),
    "partial_2d-2": lambda: R.random_field((45, 19), 0.5, 2),
    "percolation-0": lambda: R.random_field((100, 90), 0.5, 0), "percolation-1": lambda: R.random_field((100, 90), 0.5, 1),
    "percolation-2": lambda: R.random_field((100, 90), 0.5, 2),
    "isolated": R.isolated, "diagonals": R.diagonals, "spiral": R.spiral,
    "one_tile_3d": lambda: R.random_field((5, 7, 6), 0.3, 3),
    "partial_3d-0.15": lambda: R.random_field((13, 12, 11), 0.15, 4), "partial_3d-0.25": lambda: R.random_field((13, 12, 11), 0.25, 5),
    "partial_3d-0.4": lambda: R.random_field((13, 12, 11), 0.4, 6),
    "serpentine": R.serpentine, "bodies": R.bodies, "shell": R.shell,
    "all_inside": lambda: R.from_mask(np.ones((17, 9, 10), dtype=bool)), "none_inside": lambda: R.from_mask(np.zeros((17, 9, 10), dtype=bool)),
    "many_tiles": lambda: R.random_field(R.MANY_TILES_SHAPE, R.MANY_TILES_FRACTION, R.MANY_TILES_SEED),
}


@functools.lru_cache(maxsize=None)
def fixture(name):
    vals, lc, hc = FIXTURES[name]()
    vals.setflags(write=False)
    return vals, lc, hc


@functools.lru_cache(maxsize=None)
def reference(name, level=0.0, side="inside", f32=False):
    """(labels, K, nodes, index_sums, bbox) of the restatement, computed once per case and left unchanged"""
    vals = fixture(name)[0]
    lab = R.labels(vals.astype(np.float32) if f32 else vals, level, side)
    lab.setflags(write=False)
    return (lab,) + R.stats(lab)


def _check(c, ref, vals_in_set):
    lab, K, nodes, sums, bbox = ref
    got = c.labels()
    print(f"K {c.count} (restatement {K}), stats {c.stats}, {int((got != lab).sum())} labels differ")
    assert c.count == K and c.stats[0] == K and c.stats[1] == int(vals_in_set.sum()) and c.stats[3] == 0
    assert got.dtype == np.int32 and got.shape == lab.shape and np.array_equal(got, lab)
    assert c.nodes.dtype == np.int64 and np.array_equal(c.nodes, nodes)
    assert c.index_sums.dtype == np.int64 and c.index_sums.shape == sums.shape and np.array_equal(c.index_sums, sums)
    assert c.bbox.dtype == np.int32 and c.bbox.shape == bbox.shape and np.array_equal(c.bbox, bbox)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_device_matches_restatement(name):
    lsm = _lsm()
    vals, lc, hc = fixture(name)
    if name == "spiral":
        assert R.count(vals) == 1 and R.count(vals, side="outside") == 1
    phi = _field(lsm, vals, lc, hc)
    before = phi.values()
    c = lsm.components(phi)
    _check(c, reference(name), vals < 0)
    assert np.array_equal(_bits(phi.values()), _bits(before))
    want = {"isolated": 2275, "diagonals": 67, "spiral": 1, "serpentine": 1, "bodies": 3, "shell": 1, "all_inside": 1, "none_inside": 0}.get(name)
    if want is not None:
        assert c.count == want
    if name == "none_inside":
        assert (c.labels() == -1).all() and c.nodes.shape == (0,) and c.index_sums.shape == (0, 3) and c.bbox.shape == (0, 2, 3)
    if name == "all_inside":
        n = vals.shape
        assert c.stats[2] > 0 and c.nodes[0] == vals.size
        assert c.index_sums[0].tolist() == [vals.size // n[d] * (n[d] * (n[d] - 1) // 2) for d in range(3)]
        assert c.bbox[0].tolist() == [[0, 0, 0], [n[0] - 1, n[1] - 1, n[2] - 1]]
    if name in ("one_tile_2d-0", "one_tile_3d"):
        assert c.stats[2] == 0                          # no edge leaves the only tile
    if name == "many_tiles":
        share = float(c.nodes.max()) / float(c.nodes.sum())
        print(f"many_tiles: fraction {R.MANY_TILES_FRACTION}, the largest cluster holds {share:.3f} of the set")
        assert round(share, 3) == R.MANY_TILES_SHARE and 0.1 < share < 0.9


@pytest.mark.parametrize("delta", R.CORNER_DIRECTIONS, ids=str)
def test_corner(delta):
    """two nodes across the corner of eight tiles: one component along the 7 Kuhn directions, two along the other 6"""
    lsm = _lsm()
    vals, lc, hc = R.corner(delta)
    c = lsm.components(_field(lsm, vals, lc, hc))
    lab = R.labels(vals)
    assert c.count == R.corner_count(delta) and np.array_equal(c.labels(), lab)
    assert np.array_equal(c.nodes, R.stats(lab)[1]) and c.stats[2] == (1 if c.count == 1 else 0)


def test_bodies_agree_with_the_device_volume_mesh_and_have_centroids():
    lsm = _lsm()
    vals, lc, hc = fixture("bodies")
    phi = _field(lsm, vals, lc, hc)
    c = lsm.components(phi)
    m = lsm.volume_mesh(phi)
    assert c.count == 3 == R.mesh_components(m.elements, len(m.vertices))
    assert lsm.components(phi, side="outside").count == 1
    h = np.array(phi.mesh.meshsize())
    assert np.array_equal(c.centroids, np.array(lc) + h * (c.index_sums / c.nodes[:, None]))
    assert np.array_equal(c.measures, c.nodes * float(np.prod(h)))
    lo, hi = np.array(lc) + h * c.bbox[:, 0, :], np.array(lc) + h * c.bbox[:, 1, :]
    assert (lo <= c.centroids).all() and (c.centroids <= hi).all()
    assert len(c) == 3 and "3 inside components" in repr(c)


@pytest.mark.parametrize("name", ("partial_2d-0", "partial_3d-0.25", "spiral", "shell"))
def test_outside(name):
    lsm = _lsm()
    vals, lc, hc = fixture(name)
    c = lsm.components(_field(lsm, vals, lc, hc), side="outside")
    _check(c, reference(name, 0.0, "outside"), ~(vals < 0))
    if name == "shell":
        assert c.count == 2
    if name == "spiral":
        assert c.count == 1


@pytest.mark.parametrize("name", ("partial_2d-1", "partial_3d-0.4", "shell"))
@pytest.mark.parametrize("side", R.SIDES)
def test_level(name, side):
    """level = 0.25, with nodes exactly on the level: they are outside"""
    lsm = _lsm()
    vals, lc, hc = fixture(name)
    vals = np.array(vals, order="F")
    vals.reshape(-1, order="F")[::7] = 0.25
    lab = R.labels(vals, 0.25, side)
    c = lsm.components(_field(lsm, vals, lc, hc), level=0.25, side=side)
    assert c.level == 0.25 and c.side == side
    _check(c, (lab,) + R.stats(lab), R.in_set(vals, 0.25, side))


@pytest.mark.parametrize("name", ("percolation-0", "partial_3d-0.25", "bodies"))
def test_float32_storage(name):
    """equal to the restatement on the rounded values; a level between two floats"""
    lsm = _lsm()
    vals, lc, hc = fixture(name)
    v32 = vals.astype(np.float32)
    for level in (0.0, 1e-3):
        lab = R.labels(v32, level)
        c = lsm.components(_field(lsm, v32, lc, hc, dtype=np.float32), level=level)
        _check(c, (lab,) + R.stats(lab), v32.astype(np.float64) < level)


def test_equations_as_well_as_fields():
    lsm = _lsm()
    vals, lc, hc = fixture("partial_3d-0.25")
    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(vals, lsm.CartesianGrid(lc, hc, vals.shape)), bc=lsm.NeumannBC())
    _check(lsm.components(eq), reference("partial_3d-0.25"), vals < 0)
    comps, flipped = lsm.prune_(eq, keep_largest=1)
    lab, K, nodes = reference("partial_3d-0.25")[:3]
    which = np.ones(K, dtype=bool)
    which[int(np.argmax(nodes))] = False
    want, nf = R.flip(vals, lab, which)
    assert flipped == nf and np.array_equal(_bits(eq.current_state().values()), _bits(want))


@pytest.mark.parametrize("name", ("percolation-1", "many_tiles", "serpentine"))
def test_two_calls_give_identical_arrays(name):
    lsm = _lsm()
    vals, lc, hc = fixture(name)
    phi = _field(lsm, vals, lc, hc)
    a, b = lsm.components(phi), lsm.components(phi)
    assert a.stats == b.stats and np.array_equal(a.labels(), b.labels())
    assert np.array_equal(a.nodes, b.nodes) and np.array_equal(a.index_sums, b.index_sums) and np.array_equal(a.bbox, b.bbox)


def test_workspace_reuse_small_after_large():
    """the parent array of a larger call, on the same handle's workspace: one handle is one grid, so the large call and the
    small one are two levels of one field whose sets differ greatly; then a second, smaller grid on a handle of its own"""
    lsm = _lsm()
    vals, lc, hc = fixture("many_tiles")
    phi = _field(lsm, vals, lc, hc)
    big = lsm.components(phi, level=0.3)            # nearly everything in one cluster
    lab = R.labels(vals, 0.3)
    _check(big, (lab,) + R.stats(lab), vals < 0.3)
    small = lsm.components(phi, level=-0.15)        # few nodes, small clusters, on the same workspace
    lab = R.labels(vals, -0.15)
    _check(small, (lab,) + R.stats(lab), vals < -0.15)
    _check(lsm.components(phi), reference("many_tiles"), vals < 0)
    big.close()
    assert np.array_equal(small.labels(), lab)      # an object owns its labels
    vals2, lc2, hc2 = fixture("one_tile_3d")
    _check(lsm.components(_field(lsm, vals2, lc2, hc2)), reference("one_tile_3d"), vals2 < 0)


def test_root_counts_of_more_than_8192_chunks():
    """(4097, 8194) nodes, 8197 numbering chunks: the scan of the roots per chunk (csrc/scan.h with 32-bit offsets, the total
    into the counters) runs a second round, which receives a carry.  ϕ = 1 but for 90 single nodes of ϕ = −1, no two of them Kuhn
    neighbours, half in the first chunks and half in rows 8191..8193: K, the labels (ascending by node index), the sizes, the
    index sums and the bounding boxes follow from the positions.  A dropped carry numbers the roots of chunk 8192 and beyond from
    0 again, or loses them from K."""
    import _chunk_carry as CC
    lsm = _lsm()
    I, J, lin = CC.isolated_nodes()
    vals = np.ones(CC.N, dtype=np.float32, order="F")
    vals[I, J] = -1.0
    c = lsm.components(_field(lsm, vals, (0.0, 0.0), tuple(float(m - 1) for m in CC.N), dtype=np.float32))
    K = len(lin)
    print(f"K {c.count}, stats {c.stats}")
    assert c.count == K and c.stats == (K, K, 0, 0)
    lab = c.labels()
    assert lab.shape == CC.N and int(np.count_nonzero(lab != -1)) == K and np.array_equal(lab[I, J], np.arange(K))
    far = lin // CC.CHUNK >= CC.SCAN
    assert far.any() and (lab[I[far], J[far]] == np.flatnonzero(far)).all() and np.flatnonzero(far)[0] == int((~far).sum()) > 0
    pos = np.stack([I, J], axis=1)
    assert np.array_equal(c.nodes, np.ones(K, dtype=np.int64)) and np.array_equal(c.index_sums, pos)
    assert np.array_equal(c.bbox, np.stack([pos, pos], axis=1))


# ----------------------------------------------------------------------------- remove_components_ and prune_

@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("side", R.SIDES)
@pytest.mark.parametrize("name,level", (("percolation-2", 0.0), ("partial_3d-0.4", 0.25)))
def test_remove_components_matches_flip_bit_for_bit(name, level, side, dtype):
    lsm = _lsm()
    vals, lc, hc = fixture(name)
    vals = np.array(vals, order="F").astype(dtype)
    # values on the level and next to it, where the mirror image rounds onto the level or across it
    lv = dtype(level)
    near = [lv, np.nextafter(lv, dtype(np.inf)), np.nextafter(lv, dtype(-np.inf)), dtype(level + 1e-30), dtype(level - 1e-30), dtype(level - 1e-9), dtype(level + 1e-9)]
    vals.reshape(-1, order="F")[3:3 + len(near)] = near
    phi = _field(lsm, vals, lc, hc, dtype=dtype)
    assert np.array_equal(_bits(phi.values()), _bits(vals))
    c = lsm.components(phi, level=level, side=side)
    lab = R.labels(vals, level, side)
    assert np.array_equal(c.labels(), lab)
    which = np.ones(c.count, dtype=bool)
    which[1::3] = False                             # component 0 goes: at level 0.25 it holds most of partial_3d's inside
    want, nf = R.flip(vals, lab, which, level, side, dtype)
    phi.ghosts_dirty = False
    assert lsm.remove_components_(phi, c, which) == nf > 0 and phi.ghosts_dirty
    got = phi.values()
    print(f"{int((_bits(got) != _bits(want)).sum())} of {got.size} values differ from the restatement's bits")
    assert got.dtype == np.dtype(dtype) and np.array_equal(_bits(got), _bits(want))
    sel = (lab >= 0) & which[np.where(lab >= 0, lab, 0)]
    assert not R.in_set(got, level, side)[sel].any()
    # a list of ids is the same choice; the components that were left are what a second labelling finds
    after = lsm.components(phi, level=level, side=side)
    assert after.count == int((~which).sum()) and np.array_equal(after.nodes, c.nodes[~which])
    phi2 = _field(lsm, vals, lc, hc, dtype=dtype)
    c2 = lsm.components(phi2, level=level, side=side)
    assert lsm.remove_components_(phi2, c2, [int(k) for k in np.flatnonzero(which)]) == nf
    assert np.array_equal(_bits(phi2.values()), _bits(want))


def test_shell_cavity_is_filled():
    lsm = _lsm()
    vals, lc, hc = fixture("shell")
    phi = _field(lsm, vals, lc, hc)
    comps, flipped = lsm.prune_(phi, keep_largest=1, side="outside")
    assert comps.count == 2 and flipped == int(comps.nodes.min()) and comps.nodes[0] > comps.nodes[1]     # the exterior holds node 0
    lab = R.labels(vals, 0.0, "outside")
    want, _ = R.flip(vals, lab, [False, True], 0.0, "outside")
    assert np.array_equal(_bits(phi.values()), _bits(want))
    assert lsm.components(phi, side="outside").count == 1 and lsm.components(phi).count == 1


def test_bodies_min_nodes_removes_the_smaller_sphere():
    lsm = _lsm()
    vals, lc, hc = fixture("bodies")
    lab, K, nodes = reference("bodies")[:3]
    small = int(np.argmin(nodes))
    assert sorted(nodes.tolist())[0] < 100 <= sorted(nodes.tolist())[1]
    phi = _field(lsm, vals, lc, hc)
    comps, flipped = lsm.prune_(phi, min_nodes=100)
    assert comps.count == 3 and flipped == int(nodes[small])
    want, _ = R.flip(vals, lab, np.arange(K) == small)
    assert np.array_equal(_bits(phi.values()), _bits(want))
    after = lsm.components(phi)
    assert after.count == 2 and np.array_equal(after.nodes, np.delete(nodes, small))
    # both rules: a component flagged by either goes
    phi = _field(lsm, vals, lc, hc)
    comps, flipped = lsm.prune_(phi, min_nodes=int(nodes.max()), keep_largest=2)
    assert flipped == int(nodes.sum() - nodes.max()) and lsm.components(phi).count == 1


def test_keep_largest_ties_go_to_the_smaller_id():
    lsm = _lsm()
    vals, lc, hc = fixture("isolated")
    phi = _field(lsm, vals, lc, hc)
    comps, flipped = lsm.prune_(phi, keep_largest=5)
    assert comps.count == 2275 and flipped == 2270
    after = lsm.components(phi)
    assert after.count == 5 and np.array_equal(after.labels() >= 0, (comps.labels() >= 0) & (comps.labels() < 5))
    with pytest.raises(ValueError, match="min_nodes"):
        lsm.prune_(phi)


# ----------------------------------------------------------------------------- refusals: ϕ is compared bit for bit

def test_refusals_leave_phi_unchanged():
    lsm = _lsm()
    vals, lc, hc = fixture("partial_3d-0.25")
    grid = lsm.CartesianGrid(lc, hc, vals.shape)
    phi = _field(lsm, vals, lc, hc)
    before = phi.values()

    def unchanged(f=phi, b=before):
        return np.array_equal(_bits(f.values()), _bits(b))

    for bad in (float("nan"), float("inf"), -float("inf")):
        v = np.array(vals, order="F")
        v[4, 5, 6] = bad
        v[12, 11, 10] = bad
        f = _field(lsm, vals, lc, hc).copy_(v)          # an equation in the fast mode is not built from an infinite field
        b = f.values()
        assert np.array_equal(_bits(b), _bits(v))
        with pytest.raises(ValueError, match=r"phi must be finite \(2 nodes"):
            lsm.components(f)
        with pytest.raises(ValueError, match="phi must be finite"):
            lsm.prune_(f, min_nodes=3)
        assert np.array_equal(_bits(f.values()), _bits(b))
    with pytest.raises(ValueError, match="level must be finite"):
        lsm.components(phi, level=float("nan"))
    with pytest.raises(ValueError, match="side"):
        lsm.components(phi, side="both")
    with pytest.raises(TypeError):
        lsm.components(vals)
    c = lsm.components(phi)
    for which in (np.ones(c.count + 1, dtype=bool), np.ones(c.count - 1, dtype=bool), [c.count], [-1], [0.5]):
        with pytest.raises(ValueError, match="which"):
            lsm.remove_components_(phi, c, which)
    assert unchanged()
    assert lsm.remove_components_(phi, c, np.zeros(c.count, dtype=bool)) == 0 and unchanged()
    # ϕ changed under the object: a flagged node is now outside
    lab = c.labels()
    k = int(np.argmax(c.nodes))
    I = tuple(int(i) for i in np.argwhere(lab == k)[0])
    phi[I] = 1.0
    changed = phi.values()
    with pytest.raises(ValueError, match="no longer matches"):
        lsm.remove_components_(phi, c, [k])
    assert np.array_equal(_bits(phi.values()), _bits(changed))
    # ... and a component cannot be removed twice
    other = (k + 1) % c.count
    assert lsm.remove_components_(phi, c, [other]) == int(c.nodes[other])
    once = phi.values()
    with pytest.raises(ValueError, match="no longer matches"):
        lsm.remove_components_(phi, c, [other])
    assert np.array_equal(_bits(phi.values()), _bits(once))
    # another field's components
    phi_b = _field(lsm, vals, lc, hc)
    with pytest.raises(ValueError, match="another field"):
        lsm.remove_components_(phi_b, c, [0])
    c.close()
    with pytest.raises(ValueError, match="closed"):
        lsm.remove_components_(phi, c, [0])

    per = _field(lsm, vals, lc, hc, bc=(lsm.NeumannBC(), lsm.PeriodicBC(), lsm.NeumannBC()))
    b = per.values()
    with pytest.raises(ValueError, match="PeriodicBC"):
        lsm.components(per)
    with pytest.raises(ValueError, match="PeriodicBC"):
        lsm.prune_(per, keep_largest=1)
    with pytest.raises(lsm.LsmError, match="periodic dimension"):
        per.backend.cc_create(per.buf, 0.0, 0)
    assert np.array_equal(_bits(per.values()), _bits(b))
    one = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(lambda x: x[0] - 0.3, lsm.CartesianGrid((0,), (1,), (33,))), bc=lsm.NeumannBC())
    b = one.current_state().values()
    with pytest.raises(ValueError, match="1 dimensional"):
        lsm.components(one)
    with pytest.raises(lsm.LsmError, match="1-dimensional"):
        one.backend.cc_create(one.current_state().buf, 0.0, 0)
    assert np.array_equal(_bits(one.current_state().values()), _bits(b))
    fine = lsm.CartesianGrid(lc, hc, (17, 18, 16))
    band = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), bc=lsm.NeumannBC(),
                                ic=lsm.NarrowBandMeshField(lsm.MeshField(lambda x: np.sqrt((x[0] - 0.5) ** 2 + (x[1] - 0.5) ** 2 + (x[2] - 0.5) ** 2) - 0.3, fine), nlayers=2))
    b = band.current_state().values()
    with pytest.raises(ValueError, match="NarrowBandMeshField"):
        lsm.components(band)
    with pytest.raises(ValueError, match="NarrowBandMeshField"):
        lsm.prune_(band, min_nodes=2)
    assert np.array_equal(_bits(band.current_state().values()), _bits(b))
    g = lsm.LocalGroup(1)
    slab = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(vals, grid), bc=lsm.NeumannBC(), comm=g.rank(0))
    b = slab.current_state().values()
    with pytest.raises(ValueError, match="slab"):
        lsm.components(slab)
    with pytest.raises(lsm.LsmError, match="slab"):
        slab.backend.cc_create(slab.current_state().buf, 0.0, 0)
    assert np.array_equal(_bits(slab.current_state().values()), _bits(b))
    with pytest.raises(lsm.LsmError, match="side must be"):
        phi.backend.cc_create(phi.buf, 0.0, 2)
