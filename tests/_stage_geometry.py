"""The launch arithmetic of the stage kernels in plain Python — a mirror of `launch_one`, `launch_tiled` and `launch_pairs`
(levelsetmethods.jl_amd/csrc/stage_kernel.h) and of `stage_impl`'s planner (lsm_api.hip) for DENSE launches (no band mask, no
tile list) — and the table of forced geometries that tests/test_gpu_stage_geometry.py runs against the oracle.

Results are identical by design whichever path a launch takes, so a parity test cannot see that path.  The table therefore
states, per case, the class it is meant to land in; tests/test_stage_geometry_table.py asserts the claim with this mirror
(no GPU), and profiles/stage_geometry/ holds one kernel trace that confirmed the mirror's workgroup counts on the device.
"""
from dataclasses import dataclass, field

MC3, MC2, TX2 = 64, 8, 256                 # TileCfg<3>::MC, TileCfg<2>::MC, TileCfg<2>::TX
DEFAULT_TUNING = {"LSM_STAGE_TAIL": 16, "LSM_STAGE_TAIL_DYN": 25, "LSM_STAGE_MC": 0, "LSM_STAGE_MC2": 0, "LSM_PAIRS": 1,
                  "LSM_STAGE_GENERIC": 0}
# LSM_FOR_EACH_COMBO: (ADV, NM, CURV, EIK); ADV 1 = upwind, 2 = WENO5; EIK 1 = frozen sign, 2 = current sign
COMBOS = {(1, 0, 0, 0), (2, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (0, 0, 0, 2), (2, 0, 0, 2), (2, 0, 0, 1),
          (0, 1, 1, 0), (2, 0, 1, 0), (2, 1, 0, 0)}
_SLOT = {"adv": 0, "nm": 1, "curv": 2, "eik": 3}


def _cdiv(a, b):
    return (a + b - 1) // b


def passes(specs):
    """stage_impl's planner: the terms of a stage in fused passes.  specs as tests/_hip.py's Case.terms takes them.
    Returns [(combo, consts, natural)] — consts: every coefficient of the pass is a constant."""
    out, i = [], 0
    while i < len(specs):
        c, slots, consts = [0, 0, 0, 0], [], True
        while i < len(specs):
            s = specs[i]
            k = _SLOT[s[0]]
            if c[k]:
                break
            trial = list(c)
            trial[k] = {"adv": lambda: 2 if s[2] == "weno5" else 1, "nm": lambda: 1, "curv": lambda: 1,
                        "eik": lambda: 2 if s[1] is None else 1}[s[0]]()
            if tuple(trial) not in COMBOS:
                break
            c = trial
            slots.append(k)
            if s[0] != "eik" and s[1][0] != "const":
                consts = False
            i += 1
        assert slots, "no fused combination starts with this term"
        out.append((tuple(c), consts, all(b > a for a, b in zip(slots, slots[1:]))))
    return out


@dataclass
class Launch:
    kernel: str                 # "pairs" (stage_kernel2) | "wide" (64×8 tile) | "tiled" (32×8; 256×1 in 2-D)
    tx: int                     # nodes per tile along x (128 for the pair kernels)
    ty: int
    mc: int                     # planes (rows in 2-D) per long chunk
    nb: tuple                   # tiles along x, y; chunks along the march axis (long + tail)
    nbig: int = 0               # long chunk layers in front of a graded tail (0: no tail)
    mc_tail: int = 0
    tail: str = "none"          # "none" | "static" | "dynamic"
    tail_wgs: int = 0           # workgroups that draw a ticket (dynamic tail)
    grid: int = 0               # workgroups launched
    chunks: list = field(default_factory=list)      # [(m0, m1, is_tail)] along the march axis

    @property
    def per_layer(self):
        return self.nb[0] * self.nb[1]

    @property
    def ntiles(self):
        return self.per_layer * self.nb[2]

    @property
    def nbigt(self):
        return self.per_layer * self.nbig if self.mc_tail else self.ntiles

    @property
    def ntail(self):
        return self.ntiles - self.nbigt

    @property
    def spare(self):            # workgroups of a dynamic tail that draw a ticket beyond the last tail tile and return
        return self.tail_wgs - self.ntail if self.tail == "dynamic" else 0

    def chunk_of(self, m):
        return next((k, c) for k, c in enumerate(self.chunks) if c[0] <= m < c[1])

    def xcd_lists(self):
        """TileOrder::entry for every workgroup of a launch without a dynamic tail: per XCD, the (tile id, is_tail) list."""
        big_per, small_per = _cdiv(self.nbigt, 8), _cdiv(self.ntail, 8)
        lists = []
        for x in range(8):
            nb = min(max(self.nbigt - x * big_per, 0), big_per)
            so = self.nbigt + x * small_per
            lists.append([(x * big_per + j, False) for j in range(nb)] +
                         [(so + j, True) for j in range(small_per) if so + j < self.ntiles])
        return lists


def launch(n, combo, mode="fast", tuning=None, mb=0, me=None, consts=True, natural=True, out2=False, own_stream=True):
    """One dense launch of the fused combination `combo` on a grid of n nodes (2-D or 3-D), plane range [mb, me)."""
    t = dict(DEFAULT_TUNING, **(tuning or {}))
    nd = len(n)
    me = n[-1] if me is None else me
    adv, nm, curv, eik = combo
    assert combo in COMBOS and nd in (2, 3) and 0 <= mb < me <= n[-1]
    span = me - mb
    single = (adv != 0) + (nm != 0) + (eik != 0) == 1 and not curv and adv != 2
    fast3 = mode == "fast" and nd == 3
    if fast3 and single and t["LSM_PAIRS"] and not out2 and natural and consts and n[0] % 2 == 0 and n[0] >= 128 \
            and not t["LSM_STAGE_GENERIC"]:                                                  # launch_pairs
        nb0, nb1 = _cdiv(n[0], 128), _cdiv(n[1], 8)
        mc = MC3
        if t["LSM_STAGE_MC"] > 0:
            mc = t["LSM_STAGE_MC"]
        else:
            while mc > 8 and nb0 * nb1 * _cdiv(span, mc) < 2048:
                mc //= 2
        nb2 = _cdiv(span, mc)
        L = Launch("pairs", 128, 8, mc, (nb0, nb1, nb2))
        L.grid = 8 * _cdiv(L.ntiles, 8)
        L.chunks = [(mb + k * mc, min(mb + (k + 1) * mc, me), False) for k in range(nb2)]
        return L
    if nd == 2:
        mc = t["LSM_STAGE_MC2"] if t["LSM_STAGE_MC2"] > 0 else MC2
        nb = (_cdiv(n[0], TX2), 1, _cdiv(span, mc))
        L = Launch("tiled", TX2, 1, mc, nb)
        L.grid = 8 * _cdiv(L.ntiles, 8)
        L.chunks = [(mb + k * mc, min(mb + (k + 1) * mc, me), False) for k in range(nb[2])]
        return L
    wide = fast3 and single and n[0] >= 64 and not out2                                      # wide_tile_combo + launch_one
    tx = 64 if wide else 32
    nb0, nb1 = _cdiv(n[0], tx), _cdiv(n[1], 8)
    mc = MC3
    if t["LSM_STAGE_MC"] > 0:
        mc = t["LSM_STAGE_MC"]
    else:
        while mc > 8 and nb0 * nb1 * _cdiv(span, mc) < 2048:
            mc //= 2
    nb2 = _cdiv(span, mc)
    L = Launch("wide" if wide else "tiled", tx, 8, mc, (nb0, nb1, nb2))
    tail = t["LSM_STAGE_TAIL"]
    if nb2 >= 4 and 0 < tail < mc:                                                           # the graded tail
        L.nbig, L.mc_tail = nb2 - 1, tail
        left = span - L.nbig * mc
        L.nb = (nb0, nb1, L.nbig + _cdiv(left, tail))
    L.grid = 8 * _cdiv(L.ntiles, 8)
    if L.mc_tail:
        L.tail = "static"
        L.grid = 8 * (_cdiv(L.nbigt, 8) + _cdiv(L.ntail, 8))
        dyn = t["LSM_STAGE_TAIL_DYN"]
        if dyn > 0 and own_stream and L.nbigt % 8 == 0:
            L.tail = "dynamic"
            L.tail_wgs = _cdiv(L.ntail + L.ntail * dyn // 100, 8) * 8
            L.grid = L.nbigt + L.tail_wgs
    nlong = L.nbig if L.mc_tail else nb2
    L.chunks = [(mb + k * mc, min(mb + (k + 1) * mc, me), False) for k in range(nlong)]
    m = mb + nlong * mc
    while L.mc_tail and m < me:
        L.chunks.append((m, min(m + L.mc_tail, me), True))
        m += L.mc_tail
    return L


def launches(n, specs, **kw):
    """The launches of one lsm_stage call (one per fused pass; a later pass is the same geometry with another combo)."""
    out2 = kw.pop("out2", False)
    return [launch(n, c, consts=consts, natural=nat, out2=out2, **kw) for c, consts, nat in passes(specs)]


# ---- the forced geometries -------------------------------------------------------------------------------------------
# Every row: id -> (shape, (mb, me) or None, tuning, expected class of the 32×8-tile launch).  `expect` names the fields of Launch the
# row is there for; tests/test_stage_geometry_table.py asserts them, the GPU module runs the row.  T = LSM_STAGE_TAIL,
# D = LSM_STAGE_TAIL_DYN, MC = LSM_STAGE_MC.
def _t(mc, tail=16, dyn=25):
    return {"LSM_STAGE_MC": mc, "LSM_STAGE_TAIL": tail, "LSM_STAGE_TAIL_DYN": dyn}


GEOMETRY = {
    # 2×2 tiles per layer, 4 long layers of 32 + tail 16 + 6: nbigt = 16 is a multiple of 8 -> dynamic tail, 8 tail tiles
    "dyn25_mc32":  ((64, 16, 150), None, _t(32, 16, 25),  dict(mc=32, nbig=4, nbigt=16, ntail=8, tail="dynamic", tail_wgs=16, spare=8, grid=32)),
    "dyn100_mc32": ((64, 16, 150), None, _t(32, 16, 100), dict(mc=32, nbigt=16, ntail=8, tail="dynamic", tail_wgs=16, spare=8, grid=32)),
    "dyn1_mc32":   ((64, 16, 150), None, _t(32, 16, 1),   dict(mc=32, nbigt=16, ntail=8, tail="dynamic", tail_wgs=8, spare=0, grid=24)),   # no spare workgroup
    "dyn0_mc32":   ((64, 16, 150), None, _t(32, 16, 0),   dict(mc=32, nbigt=16, ntail=8, tail="static", grid=24)),
    # 3×3 tiles per layer (partial in x and y), nbigt = 36: static tail, XCD lists of 5,5,5,5,5,5,5,1 long + 3,3,3,3,3,3,0,0 short tiles
    "static_mc32": ((70, 21, 150), None, _t(32, 16, 25),  dict(mc=32, nbig=4, nbigt=36, ntail=18, tail="static", grid=64, last=6)),
    # 2×3 tiles, 4 long layers of 64 + tail 16 + 16 + 12
    "dyn_mc64":    ((37, 21, 300), None, _t(64, 16, 25),  dict(mc=64, nbig=4, nbigt=24, ntail=18, tail="dynamic", tail_wgs=24, spare=6, grid=48, last=12)),
    "static_mc64": ((37, 21, 300), None, _t(64, 16, 0),   dict(mc=64, nbig=4, nbigt=24, ntail=18, tail="static", grid=48, last=12)),
    # exactly 3 chunk layers: the tail must stay off; exactly 4: it is on (3 long layers, nbigt = 12: static)
    "layers3":     ((64, 16, 96),  None, _t(32, 16, 25),  dict(mc=32, nbig=0, ntail=0, tail="none", nchunks=3, grid=16)),
    "layers4":     ((64, 16, 128), None, _t(32, 16, 25),  dict(mc=32, nbig=3, nbigt=12, ntail=8, tail="static", nchunks=5, grid=24)),
    # edge values of the tail length: shorter than, and equal to, the WENO5 register ring's 7-fold unroll
    "tail1":       ((64, 16, 140), None, _t(32, 1, 25),   dict(mc=32, nbig=4, ntail=48, tail="dynamic", tail_wgs=64, last=1)),
    "tail5":       ((64, 16, 150), None, _t(32, 5, 25),   dict(mc=32, nbig=4, ntail=20, tail="dynamic", tail_wgs=32, last=2)),
    "tail7":       ((70, 21, 150), None, _t(32, 7, 25),   dict(mc=32, nbig=4, ntail=36, tail="static", last=1)),
    "tail7_x3":    ((64, 16, 149), None, _t(32, 7, 25),   dict(mc=32, nbig=4, ntail=12, tail="dynamic", last=7)),                         # 21 = 3 × 7 planes left
    # edge values of the chunk length: one plane, the unroll itself, not a power of two; a tail needs tail < mc
    "mc1":         ((37, 21, 40),  None, _t(1, 16, 25),   dict(mc=1, tail="none", nchunks=40)),
    "mc7":         ((64, 16, 100), None, _t(7, 5, 25),    dict(mc=7, nbig=14, ntail=4, tail="dynamic", last=2)),                          # 98 = 14 × 7, then one chunk of 2
    "mc7_static":  ((70, 21, 75),  None, _t(7, 3, 25),    dict(mc=7, nbig=10, nbigt=90, ntail=18, tail="static", last=2)),
    "mc24":        ((64, 16, 150), None, _t(24, 16, 25),  dict(mc=24, nbig=6, nbigt=24, ntail=4, tail="dynamic", last=6)),
    "mc14":        ((70, 21, 150), None, _t(14, 7, 25),   dict(mc=14, nbig=10, ntail=18, tail="static", last=3)),                         # chunks of 2 × 7 planes, tail of 7
    # plane ranges that do not start at 0 and engage the tail
    "planes_dyn":    ((64, 16, 170), (5, 155),  _t(32, 16, 25), dict(mc=32, nbig=4, nbigt=16, ntail=8, tail="dynamic", tail_wgs=16, last=6)),
    "planes_dyn8":   ((64, 16, 170), (30, 165), _t(32, 16, 25), dict(mc=32, nbig=4, nbigt=16, ntail=4, tail="dynamic", tail_wgs=8, last=7)),
    "planes_static": ((70, 21, 170), (7, 170),  _t(32, 16, 25), dict(mc=32, nbig=5, nbigt=45, ntail=9, tail="static", last=3)),
}
COMBO_HEADLINE = (2, 0, 0, 2)

# the pair kernels under LSM_STAGE_MC (FAST, a single upwind / NormalMotion / Eikonal term): shape, mc -> chunks, last chunk's planes
PAIR_GEOMETRY = {
    ((256, 11, 150), 64): dict(nb=(2, 2, 3), last=22, grid=16),
    ((256, 11, 150), 32): dict(nb=(2, 2, 5), last=22, grid=24),
    ((256, 11, 150), 7):  dict(nb=(2, 2, 22), last=3, grid=88),
    ((130, 20, 150), 64): dict(nb=(2, 3, 3), last=22, grid=24),
    ((130, 20, 150), 32): dict(nb=(2, 3, 5), last=22, grid=32),
    ((130, 20, 150), 7):  dict(nb=(2, 3, 22), last=3, grid=136),
}

# 2-D: LSM_STAGE_MC2 rows per chunk on rows longer than one 256-node tile
GEOMETRY_2D = {
    ((270, 100), 1): dict(nb=(2, 1, 100), grid=200), ((270, 100), 8): dict(nb=(2, 1, 13), grid=32), ((270, 100), 64): dict(nb=(2, 1, 2), grid=8),
    ((300, 50), 1): dict(nb=(2, 1, 50), grid=104), ((300, 50), 8): dict(nb=(2, 1, 7), grid=16), ((300, 50), 64): dict(nb=(2, 1, 1), grid=8),
}

# default tuning at sizes where the defaults themselves turn the paths on
DEFAULT_GEOMETRY = {
    # 8 × 32 tiles per layer, mc 32 (64 would give 1024 tiles), 7 long layers + 16 + 10, nbigt = 1792: dynamic
    ((250, 253, 250), (2, 0, 0, 2)): dict(kernel="tiled", mc=32, nbig=7, nbigt=1792, ntail=512, tail="dynamic", tail_wgs=640, last=10),
    ((250, 253, 250), (0, 1, 1, 0)): dict(kernel="tiled", mc=32, nbig=7, nbigt=1792, ntail=512, tail="dynamic", tail_wgs=640, last=10),
    # the headline grid: 16 × 64 tiles per layer, mc 64, 7 long layers + 4 × 16
    ((512, 512, 512), (2, 0, 0, 2)): dict(kernel="tiled", mc=64, nbig=7, nbigt=7168, ntail=4096, tail="dynamic", tail_wgs=5120, last=16),
    # single terms: the pair kernels at their default chunk of 64 planes (4 × 64 tiles × 8 layers = 2048)
    ((512, 512, 512), (1, 0, 0, 0)): dict(kernel="pairs", mc=64, nb=(4, 64, 8), grid=2048),
    ((512, 512, 512), (0, 1, 0, 0)): dict(kernel="pairs", mc=64, nb=(4, 64, 8), grid=2048),
    ((512, 512, 512), (0, 0, 0, 2)): dict(kernel="pairs", mc=64, nb=(4, 64, 8), grid=2048),
    ((512, 512, 256), (1, 0, 0, 0)): dict(kernel="pairs", mc=32, nb=(4, 64, 8), grid=2048),
}


def check(L, expect):
    """Assert that launch L has every property `expect` names ("last" = planes of the last chunk, "nchunks" = chunks along the march axis)."""
    for k, v in expect.items():
        got = {"last": lambda: L.chunks[-1][1] - L.chunks[-1][0], "nchunks": lambda: len(L.chunks)}.get(k, lambda: getattr(L, k))()
        assert got == v, (k, got, v)
