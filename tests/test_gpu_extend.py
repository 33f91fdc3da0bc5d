"""extend_from_interface_ on the device (csrc/lsm_eikonal.hip, lsm_extend through the Python API) against the restatement
(tests/_extend_ref.py), bit for bit in every comparison — every value is computed once from final values, so nothing depends on
the tile schedule and the same bits are owed at any number of tiles: a grid inside one tile, partial tiles on every axis, fronts
that wake tiles along each axis in turn, two fronts meeting in a shock, an interface cut by a face of the grid, anisotropic and
tiny spacing, 336 and 300 tiles; K = 1, 3, 4, 5, 8; both seedings, the mask and the two side rules, source="interface", a cutoff
with a fill, planted orphans; float32 storage; determinism; non-convergence; the refusals; eikonal_(extend=…); scratch reuse.
The tile shapes are 8×8×8 and 32×8, up to 4 fields per workgroup."""
import functools

import numpy as np
import pytest

import _eikonal_ref as R
import _extend_ref as X

pytestmark = pytest.mark.gpu

INF = float("inf")


def _lsm():
    import lsm_amd
    return lsm_amd


def _field(lsm, vals, lc, hc, dtype=None, bc=None):
    mf = lsm.MeshField(vals, lsm.CartesianGrid(lc, hc, vals.shape), dtype=dtype)
    return lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=mf, bc=bc or lsm.NeumannBC()).current_state()


def _more(phi, Fs):
    """device fields on ϕ's handle holding the host arrays Fs"""
    return [phi.copy().copy_(f) for f in Fs]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _poison(Fs, frozen):
    """the inputs with NaN at every node that is not frozen: never read"""
    return [np.asfortranarray(np.where(frozen, f, np.nan)) for f in Fs]


def _inputs(phi, h, n, lc, hc, K, **kw):
    """K input fields, NaN wherever the rule never reads them: everywhere but at the frozen nodes and the orphans"""
    base = X.fields(n, lc, hc, K)
    P = X.prepare(phi, h, base, **kw)
    return _poison(base, P.frozen | P.orphan), P


@functools.lru_cache(maxsize=None)
def _case(name, seeding, source, K=3):
    """(ϕ, n, lc, hc, h, inputs, expected outputs, stats) of the restatement; computed once, read-only"""
    phi, n, lc, hc, h = X.distance(name, seeding)
    width = X.widths(h)[seeding]
    F = _poison(X.fields(n, lc, hc, K), X.frozen_nodes(phi, h, "rule", width))
    want, stats = X.extend(phi, h, F, width=width, source=source)
    for a in F + want:
        a.setflags(write=False)
    return phi, n, lc, hc, h, F, want, stats


def _check_stats(stats, ref, n):
    nt = R.ntiles(n)
    assert stats[0] == ref["frozen"] and stats[3] == ref["orphans"] and stats[4] == ref["filled"]
    if ref["frozen"] + ref["orphans"] + ref["filled"] == int(np.prod(n)):       # nothing to compute (a width beyond a small grid)
        assert stats[1] == stats[2] == 0
        return
    assert 1 <= stats[1] <= stats[2] <= stats[1] * nt
    if nt == 1:
        assert stats[1] == stats[2] == 1


NAMES = list(R.FIXTURES) + list(X.EXTRA)
CASES = [(name, s, src) for name in NAMES for s, src in ((0, "nodes"), (1, "nodes"), (0, "interface"))]


@pytest.mark.parametrize("name,seeding,source", CASES, ids=[f"{n}-{('crossing', 'width')[s]}-{src}" for n, s, src in CASES])
def test_device_matches_restatement(name, seeding, source):
    lsm = _lsm()
    phi0, n, lc, hc, h, F0, want, ref = _case(name, seeding, source)
    phi = _field(lsm, phi0, lc, hc)
    assert np.array_equal(R.meshsize(n, lc, hc), np.array(phi.mesh.meshsize()))
    F = _more(phi, F0)
    stats = phi.backend.extend([f.buf for f in F], phi.buf, "rule", None, X.widths(h)[seeding] or 0.0, source, INF, 0.0, 0)
    print(f"{name}/{seeding}/{source}: stats {stats}")
    for f, w in zip(F, want):
        got = f.values()
        assert not np.isnan(got).any()
        assert _eq(got, w), f"{int((got != w).sum())} of {got.size} nodes differ"
    assert _eq(phi.values(), np.asarray(phi0))                       # ϕ is read only
    _check_stats(stats, ref, n)
    if name.startswith(("nine_tiles", "wake_")):
        assert stats[1] >= 8                                          # the front crosses the tiles one launch after the other
    # a second call on fresh fields: the same bits
    G = _more(phi, F0)
    phi.backend.extend([g.buf for g in G], phi.buf, "rule", None, X.widths(h)[seeding] or 0.0, source, INF, 0.0, 0)
    assert all(_eq(f.values(), g.values()) for f, g in zip(F, G))


@functools.lru_cache(maxsize=None)
def _large(name):
    """the exact two-ball distance of R.LARGE (not a solve: cheap at this size); ties may leave orphans, counted alike"""
    phi, n, lc, hc, h, _ = R.fixture(name)
    F, _ = _inputs(phi, h, n, lc, hc, 2)
    want, stats = X.extend(phi, h, F)
    return phi, n, lc, hc, h, F, want, stats


@pytest.mark.parametrize("name", ("many_tiles_3d", "many_tiles_2d"))
def test_many_tiles_owe_the_same_bits(name):
    lsm = _lsm()
    phi0, n, lc, hc, h, F0, want, ref = _large(name)
    assert R.ntiles(n) in (336, 300)
    phi = _field(lsm, phi0, lc, hc)
    F = _more(phi, F0)
    stats = phi.backend.extend([f.buf for f in F], phi.buf)
    print(f"{name}: stats {stats}")
    for f, w in zip(F, want):
        assert _eq(f.values(), w)
    _check_stats(stats, ref, n)


@pytest.mark.parametrize("name", ("partial_tiles", "two_circles"))
def test_every_field_of_a_K_call_equals_its_own_call(name):
    lsm = _lsm()
    phi0, n, lc, hc, h = X.distance(name)
    F0 = _poison(X.fields(n, lc, hc, 8), X.frozen_nodes(phi0, h))
    want, ref = X.extend(phi0, h, F0)
    phi = _field(lsm, phi0, lc, hc)
    single = []
    for f0 in F0:
        (f,) = _more(phi, [f0])
        assert lsm.extend_from_interface_(f, phi) is f
        single.append(f.values())
    for got, w in zip(single, want):
        assert _eq(got, w)
    for K in (3, 4, 5, 8):
        F = _more(phi, F0[:K])
        for f in F:
            f.ghosts_dirty = False
        assert lsm.extend_from_interface_(F, phi) is F and all(f.ghosts_dirty for f in F)
        for f, s in zip(F, single):
            assert _eq(f.values(), s), K
    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(np.asarray(phi0), lsm.CartesianGrid(lc, hc, n)), bc=lsm.NeumannBC())
    (f,) = _more(eq.current_state(), F0[:1])
    lsm.extend_from_interface_((f,), eq)                                 # a LevelSetEquation stands for its current state
    assert _eq(f.values(), single[0])


@pytest.mark.parametrize("name", ("partial_tiles", "cut_by_face_2d"))
@pytest.mark.parametrize("rule", ("mask", "inside", "outside"))
def test_mask_and_side_rules(name, rule):
    lsm = _lsm()
    phi0, n, lc, hc, h = X.distance(name)
    # the mask: a band around half of the interface — the free nodes next to the other half have no smaller neighbour
    mask = np.asfortranarray((np.abs(phi0) <= 2.0 * h.max()) & (R.nodes(n, lc, hc)[1] < 0.1)) if rule == "mask" else None
    F0, _ = _inputs(phi0, h, n, lc, hc, 2, rule=rule, mask=mask)
    want, ref = X.extend(phi0, h, F0, rule=rule, mask=mask)
    if rule == "mask":
        assert ref["orphans"] > 0
    else:
        assert ref["orphans"] == 0                                       # a whole side frozen: every free node has a smaller neighbour
    phi = _field(lsm, phi0, lc, hc)
    F = _more(phi, F0)
    lsm.extend_from_interface_(F, phi, frozen=rule if rule != "mask" else mask)
    for f, w in zip(F, want):
        assert _eq(f.values(), w)
    G = _more(phi, F0)
    stats = phi.backend.extend([g.buf for g in G], phi.buf, rule, None if mask is None else mask.astype(np.uint8))
    _check_stats(stats, ref, n)
    if rule == "mask":                                                   # a 0–1 array and a host MeshField are the same mask
        for m in (mask.astype(np.float64), lsm.MeshField(mask.astype(np.float64), lsm.CartesianGrid(lc, hc, n))):
            H = _more(phi, F0)
            lsm.extend_from_interface_(H, phi, frozen=m)
            assert all(_eq(a.values(), b.values()) for a, b in zip(H, F))


@pytest.mark.parametrize("name", ("partial_tiles", "two_circles", "nine_tiles_2d"))
def test_cutoff_with_fill(name):
    lsm = _lsm()
    phi0, n, lc, hc, h = X.distance(name)
    c = 0.5 * float(np.abs(phi0).max())
    clipped = np.asfortranarray(np.copysign(np.minimum(np.abs(phi0), c), phi0))
    F0 = _poison(X.fields(n, lc, hc, 2), X.frozen_nodes(clipped, h))
    want, ref = X.extend(clipped, h, F0, cutoff=c, fill=-7.5)
    assert ref["filled"] > 0 and ref["orphans"] == 0
    phi = _field(lsm, clipped, lc, hc)
    F = _more(phi, F0)
    lsm.extend_from_interface_(F, phi, cutoff=c, fill=-7.5)
    for f, w in zip(F, want):
        assert _eq(f.values(), w)
    G = _more(phi, F0)
    _check_stats(phi.backend.extend([g.buf for g in G], phi.buf, cutoff=c, fill=-7.5), ref, n)


def test_planted_orphans_keep_their_values():
    lsm = _lsm()
    phi0, n, lc, hc, h = X.planted_orphans()
    P = X.prepare(phi0, h, X.fields(n, lc, hc, 2))
    F0 = _poison(X.fields(n, lc, hc, 2), P.frozen | P.orphan)
    want, ref = X.extend(phi0, h, F0)
    assert ref["orphans"] == 4
    phi = _field(lsm, phi0, lc, hc)
    F = _more(phi, F0)
    stats = phi.backend.extend([f.buf for f in F], phi.buf)
    assert stats[3] == 4
    _check_stats(stats, ref, n)
    for f, f0, w in zip(F, F0, want):
        assert _eq(f.values(), w) and _eq(f.values()[P.orphan], f0[P.orphan])
    bad = [f.copy(order="F") for f in F0]
    bad[1][tuple(np.argwhere(P.orphan)[0])] = np.nan                    # an orphan is a seed: a non-finite one is refused
    B = _more(phi, bad)
    with pytest.raises(ValueError, match="finite at the frozen nodes"):
        lsm.extend_from_interface_(B, phi)
    assert all(_eq(b.values(), b0) for b, b0 in zip(B, bad))


@pytest.mark.parametrize("name,source", (("partial_tiles", "nodes"), ("two_circles", "interface"), ("tiny_h", "nodes")))
def test_float32_storage(name, source):
    """the fp64 result of the float32-rounded inputs, rounded once"""
    lsm = _lsm()
    phi64, n, lc, hc, h = X.distance(name)
    phi32 = np.asfortranarray(phi64.astype(np.float32))
    up = phi32.astype(np.float64)
    F32 = [np.asfortranarray(f.astype(np.float32)) for f in X.fields(n, lc, hc, 5)]
    P = X.prepare(up, h, [f.astype(np.float64) for f in F32], source=source)
    F32 = [np.where(P.frozen | P.orphan, f, np.float32(np.nan)) for f in F32]
    want, ref = X.extend(up, h, [f.astype(np.float64) for f in F32], source=source)
    phi = _field(lsm, phi32, lc, hc, dtype=np.float32)
    F = _more(phi, F32)
    stats = phi.backend.extend([f.buf for f in F], phi.buf, source=source)
    print(f"{name} f32: stats {stats} ({ref['orphans']} orphans by ties of rounded values)")
    for f, w in zip(F, want):
        assert f.values().dtype == np.float32 and _eq(f.values(), w.astype(np.float32))
    _check_stats(stats, ref, n)
    assert _eq(phi.values(), phi32)


def test_not_converged_leaves_the_fields_untouched():
    lsm = _lsm()
    phi0, n, lc, hc, h, F0, want, ref = _case("nine_tiles_2d", 0, "nodes")
    phi = _field(lsm, phi0, lc, hc)
    F = _more(phi, F0)
    with pytest.raises(lsm.LsmNotConvergedError, match="did not empty"):
        lsm.extend_from_interface_(F, phi, max_iters=1)
    assert all(_eq(f.values(), f0) for f, f0 in zip(F, F0))
    with pytest.raises(lsm.LsmNotConvergedError):
        lsm.eikonal_(phi, extend=F, max_iters=1)
    assert all(_eq(f.values(), f0) for f, f0 in zip(F, F0)) and _eq(phi.values(), np.asarray(phi0))
    lsm.extend_from_interface_(F, phi)                                  # and the handle still works
    assert all(_eq(f.values(), w) for f, w in zip(F, want))


def test_refusals_leave_the_fields_untouched():
    lsm = _lsm()
    phi0, n, lc, hc, h = X.distance("one_tile")
    grid = lsm.CartesianGrid(lc, hc, n)
    F0 = X.fields(n, lc, hc, 2)
    phi = _field(lsm, phi0, lc, hc)
    F = _more(phi, F0)
    ext = lsm.extend_from_interface_
    with pytest.raises(TypeError, match="device field"):
        ext(F, np.asarray(phi0))
    with pytest.raises(TypeError, match="device fields"):
        ext([F[0], F0[1]], phi)
    with pytest.raises(TypeError, match="device fields"):
        ext(lsm.MeshField(F0[0], grid), phi)
    with pytest.raises(ValueError, match="1 to 8 fields"):
        ext([], phi)
    with pytest.raises(ValueError, match="1 to 8 fields"):
        ext(_more(phi, F0[:1] * 9), phi)
    with pytest.raises(ValueError, match="same field twice"):
        ext([F[0], F[1], F[0]], phi)
    with pytest.raises(ValueError, match="phi itself"):
        ext([F[0], phi], phi)
    other = _field(lsm, phi0, lc, hc)
    with pytest.raises(ValueError, match="another backend"):
        ext([F[0], other], phi)
    with pytest.raises(ValueError, match="source='interface'"):
        ext(F, phi, source="interface", frozen="inside")
    with pytest.raises(ValueError, match="source must be"):
        ext(F, phi, source="crossings")
    with pytest.raises(ValueError, match="frozen must be"):
        ext(F, phi, frozen="solid")
    with pytest.raises(ValueError, match="mask has shape"):
        ext(F, phi, frozen=np.ones((3, 3, 3)))
    for kw in ({"width": 0.0}, {"width": -1.0}, {"width": INF}, {"cutoff": 0.0}, {"cutoff": -2.0}, {"cutoff": float("nan")}):
        with pytest.raises(ValueError, match="must be positive"):
            ext(F, phi, **kw)
    for fill in (INF, float("nan")):
        with pytest.raises(ValueError, match="fill must be finite"):
            ext(F, phi, fill=fill)
    # the C entry point's own refusals
    b, bufs = phi.backend, [f.buf for f in F]
    for kw, what in (({"width": -1.0}, "width"), ({"width": INF}, "width"), ({"cutoff": 0.0}, "cutoff"), ({"cutoff": float("nan")}, "cutoff"),
                     ({"fill": INF}, "fill"), ({"rule": "mask"}, "without a mask"), ({"rule": "inside", "source": "interface"}, "INTERFACE")):
        with pytest.raises(lsm.LsmError, match=f"lsm_extend: .*{what}"):
            b.extend(bufs, phi.buf, **kw)
    with pytest.raises(lsm.LsmError, match="nfields"):
        b.extend([], phi.buf)
    with pytest.raises(lsm.LsmError, match="nfields"):
        b.extend(bufs[:1] * 9, phi.buf)
    with pytest.raises(lsm.LsmError, match="same field twice"):
        b.extend([bufs[0], bufs[1], bufs[0]], phi.buf)
    with pytest.raises(lsm.LsmError, match="phi itself"):
        b.extend([bufs[0], phi.buf], phi.buf)
    for rule, source in ((7, 0), (-1, 0), (0, 2)):
        stats = (b.lib.lsm_extend.argtypes[11]._type_ * 5)()
        ptrs = (b.lib.lsm_extend.argtypes[2]._type_ * 2)(*[b.ptr(x) for x in bufs])
        assert b.lib.lsm_extend(b.h, b.ptr(phi.buf), ptrs, 2, rule, None, 0.0, source, INF, 0.0, 0, stats, None) == lsm._lib.ERR_INVALID
    assert all(_eq(f.values(), f0) for f, f0 in zip(F, F0))
    # the data refusals, counted by the init kernel before anything is written
    bad = np.array(phi0, order="F")
    bad[2, 3, 1] = np.nan
    bad[2, 3, 2] = np.nan
    nanphi = _field(lsm, bad, lc, hc)
    N_ = _more(nanphi, F0)
    with pytest.raises(ValueError, match=r"phi must be finite \(2 nodes\)"):
        ext(N_, nanphi)
    with pytest.raises(lsm.LsmError) as e:
        nanphi.backend.extend([f.buf for f in N_], nanphi.buf)
    assert (e.value.reason, e.value.offenders) == (1, 2)
    assert all(_eq(f.values(), f0) for f, f0 in zip(N_, F0))
    fr = X.frozen_nodes(phi0, h)
    badF = [f.copy(order="F") for f in F0]
    for I in np.argwhere(fr)[:3]:
        badF[0][tuple(I)] = np.inf
    badF[1][tuple(np.argwhere(fr)[0])] = np.nan
    B = _more(phi, badF)
    with pytest.raises(ValueError, match=r"finite at the frozen nodes \(3 nodes\)"):
        ext(B, phi)
    assert all(_eq(f.values(), f0) for f, f0 in zip(B, badF))
    same_sign = _field(lsm, np.abs(phi0) + 0.1, lc, hc)
    S = _more(same_sign, F0)
    for kw in ({}, {"frozen": "inside"}, {"frozen": np.zeros(n, dtype=bool)}):
        with pytest.raises(ValueError, match="no node is frozen"):
            ext(S, same_sign, **kw)
    assert all(_eq(f.values(), f0) for f, f0 in zip(S, F0))
    # what eikonal_ refuses of its `extend` it refuses before ϕ changes
    with pytest.raises(ValueError, match="phi itself"):
        lsm.eikonal_(phi, extend=[phi])
    with pytest.raises(ValueError, match="extend_source"):
        lsm.eikonal_(phi, extend=F, extend_source="faces")
    assert _eq(phi.values(), np.asarray(phi0))
    # the grids and fields the extension does not run on
    per = _field(lsm, phi0, lc, hc, bc=(lsm.NeumannBC(), lsm.PeriodicBC(), lsm.NeumannBC()))
    Pf = _more(per, F0)
    with pytest.raises(ValueError, match="PeriodicBC"):
        ext(Pf, per)
    with pytest.raises(lsm.LsmError, match="periodic dimension"):
        per.backend.extend([f.buf for f in Pf], per.buf)
    one = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(lambda x: x[0] - 0.4, lsm.CartesianGrid((0.0,), (1.0,), (17,))),
                               bc=lsm.NeumannBC())
    O = [one.current_state().copy()]
    with pytest.raises(ValueError, match="1 dimensional"):
        ext(O, one)
    with pytest.raises(lsm.LsmError, match="1-dimensional"):
        one.backend.extend([O[0].buf], one.current_state().buf)
    fine = lsm.CartesianGrid(lc, hc, (17, 18, 16))
    band = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), bc=lsm.NeumannBC(),
                                ic=lsm.NarrowBandMeshField(lsm.MeshField(lambda x: np.sqrt(x[0] ** 2 + x[1] ** 2 + x[2] ** 2) - 0.5, fine), nlayers=2))
    with pytest.raises(ValueError, match="NarrowBandMeshField"):
        ext([band.current_state().copy()], band)
    g = lsm.LocalGroup(1)
    slab = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(np.asarray(phi0), grid), bc=lsm.NeumannBC(), comm=g.rank(0))
    Sl = _more(slab.current_state(), F0)
    with pytest.raises(ValueError, match="slab"):
        ext(Sl, slab)
    with pytest.raises(lsm.LsmError, match="slab"):
        slab.backend.extend([f.buf for f in Sl], slab.current_state().buf)
    assert all(_eq(f.values(), f0) for f, f0 in zip(Pf + Sl, F0 + F0))
    ext(F, phi)                                                          # and the handle still works
    want, _ = X.extend(phi0, h, F0)
    assert all(_eq(f.values(), w) for f, w in zip(F, want))


@pytest.mark.parametrize("kw", ({}, {"width": "w"}, {"cutoff": "c"}, {"extend_source": "interface"}), ids=("crossing", "width", "cutoff", "interface"))
def test_eikonal_with_extend_is_the_two_calls(kw):
    lsm = _lsm()
    phi0, n, lc, hc, h, _ = R.fixture("partial_tiles")
    kw = {k: {"w": 1.5 * float(h.max()), "c": 0.6}.get(v, v) for k, v in kw.items()}
    F0 = X.fields(n, lc, hc, 2)
    a, b = _field(lsm, phi0, lc, hc), _field(lsm, phi0, lc, hc)
    Fa, Fb = _more(a, F0), _more(b, F0)
    assert lsm.eikonal_(a, extend=Fa, **kw) is a
    ek = {k: v for k, v in kw.items() if k != "extend_source"}
    lsm.eikonal_(b, **ek)
    lsm.extend_from_interface_(Fb, b, fill=0.0, source=kw.get("extend_source", "nodes"), **ek)
    assert _eq(a.values(), b.values()) and all(_eq(x.values(), y.values()) for x, y in zip(Fa, Fb))
    assert all(x.ghosts_dirty for x in Fa) and not all(_eq(x.values(), f0) for x, f0 in zip(Fa, F0))
    # against the restatement of both steps
    phi1 = R.eikonal(phi0, h, None, ek.get("width"), ek.get("cutoff"))
    want, ref = X.extend(phi1, h, F0, width=ek.get("width"), cutoff=ek.get("cutoff"), fill=0.0, source=kw.get("extend_source", "nodes"))
    assert _eq(a.values(), phi1) and all(_eq(x.values(), w) for x, w in zip(Fa, want))
    if "cutoff" in ek:
        assert ref["filled"] > 0 and ref["orphans"] == 0              # the plateau beyond the cutoff is filled, not orphaned
    one = _field(lsm, phi0, lc, hc)
    (f,) = _more(one, F0[:1])
    lsm.eikonal_(one, extend=f, **kw)                                    # a single field instead of a sequence
    assert _eq(f.values(), Fa[0].values())


def test_scratch_reuse_across_calls_of_different_K_and_grid():
    """one handle: K = 8, 1, 5 and an eikonal_ solve in between share the workspace; handles of a smaller, then a larger grid"""
    lsm = _lsm()
    for name in ("one_tile", "two_circles", "nine_tiles_3d"):
        phi0, n, lc, hc, h = X.distance(name)
        F0 = _poison(X.fields(n, lc, hc, 8), X.frozen_nodes(phi0, h))
        want, ref = X.extend(phi0, h, F0)
        phi = _field(lsm, phi0, lc, hc)
        for K in (8, 1, 5):
            F = _more(phi, F0[:K])
            _check_stats(phi.backend.extend([f.buf for f in F], phi.buf), ref, n)
            assert all(_eq(f.values(), w) for f, w in zip(F, want))
            scratch = phi.copy()
            lsm.eikonal_(scratch)                                        # T, the frozen bytes and the lists are eikonal_'s too
        F = _more(phi, F0[:2])
        lsm.extend_from_interface_(F, phi)
        assert all(_eq(f.values(), w) for f, w in zip(F, want))
