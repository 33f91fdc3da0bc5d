"""Every case of tests/_stage_geometry.py's tables lands in the launch class its comment claims (no GPU: the launch
arithmetic of stage_kernel.h mirrored in Python; profiles/stage_geometry/ holds the device trace that confirmed the mirror)."""
import pytest

import _stage_geometry as G


@pytest.mark.parametrize("name", list(G.GEOMETRY))
def test_forced_geometry_rows_land_in_their_class(name):
    shape, planes, tuning, expect = G.GEOMETRY[name]
    mb, me = planes or (0, shape[2])
    for mode in ("strict", "fast"):
        L = G.launch(shape, G.COMBO_HEADLINE, mode=mode, tuning=tuning, mb=mb, me=me)
        assert L.kernel == "tiled" and (L.tx, L.ty) == (32, 8)
        G.check(L, expect)
        # the chunks tile the plane range exactly, long chunks first; every chunk starts inside the range (a tail tile's m0 < me)
        assert L.chunks[0][0] == mb and L.chunks[-1][1] == me and len(L.chunks) == L.nb[2]
        assert all(a[1] == b[0] for a, b in zip(L.chunks, L.chunks[1:])) and all(c[0] < c[1] for c in L.chunks)
        assert [c[2] for c in L.chunks] == [False] * (len(L.chunks) - L.nb[2] + L.nbig if L.mc_tail else len(L.chunks)) + [True] * (L.nb[2] - L.nbig if L.mc_tail else 0)
        if L.tail != "dynamic":
            # TileOrder::entry hands every tile out exactly once, long tiles as long and tail tiles as tail
            ids = sorted(e for lst in L.xcd_lists() for e in lst)
            assert ids == [(i, i >= L.nbigt) for i in range(L.ntiles)]
            assert max(len(lst) for lst in L.xcd_lists()) * 8 <= L.grid
        else:
            assert L.nbigt % 8 == 0 and L.tail_wgs % 8 == 0 and L.tail_wgs >= L.ntail and L.grid == L.nbigt + L.tail_wgs
    # a launch on a caller's stream gets no ticket counter: the static tail
    if expect.get("tail") == "dynamic":
        assert G.launch(shape, G.COMBO_HEADLINE, tuning=tuning, mb=mb, me=me, own_stream=False).tail == "static"


def test_the_classes_the_issue_names_are_all_in_the_table():
    rows = {k: G.launch(s, G.COMBO_HEADLINE, tuning=t, mb=(p or (0, 0))[0], me=(p or (0, s[2]))[1]) for k, (s, p, t, _) in G.GEOMETRY.items()}
    assert {L.tail for L in rows.values()} == {"none", "static", "dynamic"}
    assert {32, 64, 1, 7, 24} <= {L.mc for L in rows.values()} and {1, 5, 7, 16} <= {L.mc_tail for L in rows.values()}
    assert any(L.tail == "dynamic" and L.spare > 0 for L in rows.values()) and any(L.tail == "dynamic" and L.spare == 0 for L in rows.values())
    uneven = [sorted({len(lst) for lst in L.xcd_lists()}) for L in rows.values() if L.tail == "static"]
    assert any(len(u) > 1 for u in uneven)                                   # XCD lists of different lengths
    assert rows["static_mc32"].xcd_lists()[7] == [(35, False)] and len(rows["static_mc32"].xcd_lists()[0]) == 8
    # chunk lengths that are and are not multiples of the 7-fold unroll
    lens = {c[1] - c[0] for L in rows.values() for c in L.chunks}
    assert {7, 14, 21} & lens and {1, 2, 3, 5, 6, 12, 16, 24, 32, 64} <= lens
    # without the switch every one of these grids ends at mc = 8 and no tail: what the suite covered before
    for s, p, _, _ in G.GEOMETRY.values():
        L = G.launch(s, G.COMBO_HEADLINE)
        assert L.mc == 8 and L.tail == "none"


@pytest.mark.parametrize("key", list(G.PAIR_GEOMETRY), ids=str)
def test_pair_kernels_take_the_forced_chunk(key):
    shape, mc = key
    for combo in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 0, 1), (0, 0, 0, 2)):
        L = G.launch(shape, combo, tuning={"LSM_STAGE_MC": mc})
        assert L.kernel == "pairs" and L.mc == mc and L.tail == "none"
        G.check(L, G.PAIR_GEOMETRY[key])
        assert G.launch(shape, combo).mc == 8                                 # the default shrinks to 8 on these grids
        one = G.launch(shape, combo, tuning={"LSM_STAGE_MC": mc, "LSM_PAIRS": 0})
        assert one.kernel == "wide" and one.tx == 64 and one.mc == mc
        assert G.launch(shape, combo, mode="strict", tuning={"LSM_STAGE_MC": mc}).kernel == "tiled"
    assert G.launch((131, 20, 150), (0, 1, 0, 0)).kernel == "wide"           # odd n1: no pairs


@pytest.mark.parametrize("key", list(G.GEOMETRY_2D), ids=str)
def test_2d_rows_per_chunk(key):
    shape, mc2 = key
    L = G.launch(shape, G.COMBO_HEADLINE, tuning={"LSM_STAGE_MC2": mc2})
    assert L.kernel == "tiled" and L.tx == 256 and L.mc == mc2 and L.tail == "none"
    G.check(L, G.GEOMETRY_2D[key])


@pytest.mark.parametrize("key", list(G.DEFAULT_GEOMETRY), ids=str)
def test_default_tuning_turns_the_paths_on_at_size(key):
    shape, combo = key
    G.check(G.launch(shape, combo), G.DEFAULT_GEOMETRY[key])


def test_planner_passes():
    adv = ("adv", ("rot", 1.0, 0.0, 0.0), "weno5")
    four = [adv, ("eik", None), ("nm", ("const", (0.3,))), ("curv", ("const", (-0.05,)))]
    assert G.passes(four) == [((2, 0, 0, 2), False, True), ((0, 1, 1, 0), True, True)]
    assert G.passes([("eik", None), ("adv", ("const", (1.0, 0.0, 0.0)), "weno5")]) == [((2, 0, 0, 2), True, False)]
    assert G.passes([("nm", ("const", (0.1,))), ("curv", ("const", (-0.1,)))]) == [((0, 1, 1, 0), True, True)]
    assert [p[0] for p in G.passes([adv, ("adv", ("const", (1.0, 0.0, 0.0)), "upwind")])] == [(2, 0, 0, 0), (1, 0, 0, 0)]
    # a FIELD speed keeps a single term off the pair kernels but not off the wide tile
    assert [L.kernel for L in G.launches((256, 16, 64), [("nm", ("field", None))])] == ["wide"]
    assert [L.kernel for L in G.launches((256, 16, 64), [("nm", ("const", (0.5,)))])] == ["pairs"]
    assert [L.kernel for L in G.launches((256, 16, 64), [("nm", ("const", (0.5,)))], out2=True)] == ["tiled"]
