"""The restatement of volume_mesh (tests/_vol_ref.py, the contract of csrc/lsm_vol.hip) against facts that do not come from it:
the vertex count, conformity (every face in at most two elements), the boundary of the mesh being exactly isosurface's mesh with
its normal pointing out, positive volumes summing to the volume the interface encloses, the Euler characteristic, the orientation
table derived again from random fields, second-order convergence, exact half spaces, nodes on the level, full and empty fields;
and the Medit writer of export_volume_mesh on plain numpy input."""
import functools
import itertools
import math

import numpy as np
import pytest

import _iso_ref as R
import _vol_ref as V
from test_isosurface_host import DISK_R, PLANES, SPHERE_R, case, count_sign_changes, grid_vals

CLOSED = ["sphere9", "sphere17", "sphere33", "torus", "disk17", "disk33"]
EULER = {"torus": 0}


@functools.lru_cache(maxsize=None)
def vcase(name):
    """(values, lc, hc, vertices, elements, interface) of a named case: computed once, shared, never modified"""
    vals, lc, hc, _, _ = case(name)
    out = V.volume_mesh(vals, lc, hc)
    for a in out:
        a.setflags(write=False)
    return (vals, lc, hc) + out


# ----------------------------------------------------------------------------- checks that do not come from the restatement

def _canonical(f):
    """rows rotated (an even permutation) so that the smallest vertex comes first; segments stay as they are"""
    if f.shape[1] == 2 or not len(f):
        return f
    k = np.argmin(f, axis=1)
    return np.take_along_axis(f, (k[:, None] + np.arange(3)[None, :]) % 3, axis=1)


def boundary_faces(elems):
    """(all faces sorted by vertex, the faces that occur once oriented as the boundary of their element: normal pointing out of
    an element of positive volume, the vertex opposite each of them).  The face opposite vertex i of (v0 … vN) is
    (−1)^i (v0 … v̂i … vN); a transposition of its first two vertices stands for the minus sign."""
    N1 = elems.shape[1]
    faces, opp = [], []
    for i in range(N1):
        f = np.delete(elems, i, axis=1)
        if i % 2 == 1:
            f = f[:, [1, 0] + list(range(2, N1 - 1))]
        faces.append(f)
        opp.append(elems[:, i])
    faces, opp = np.concatenate(faces), np.concatenate(opp)
    srt = np.sort(faces, axis=1)
    _, inv, cnt = np.unique(srt, axis=0, return_inverse=True, return_counts=True)
    once = cnt[inv.reshape(-1)] == 1
    return srt, cnt, faces[once], opp[once]


def assert_boundary_is(verts, elems, interface, other=None):
    """every face in at most two elements; the faces occurring once are exactly `interface`, as oriented elements (up to an even
    permutation), and the interface's normal points away from the vertex opposite it; `other(points)`: a predicate the
    remaining once-faces must satisfy (None: there are none)"""
    srt, cnt, once, opp = boundary_faces(elems)
    assert cnt.max() <= 2, "a face occurs in more than two elements"
    key = lambda f: {tuple(r) for r in _canonical(f).tolist()}
    got, want = key(once), key(interface)
    assert len(want) == len(interface), "an interface element occurs twice"
    assert want <= got, "an interface element is no boundary face of the mesh (or is oriented into it)"
    rest = np.array([r for r in _canonical(once).tolist() if tuple(r) not in want], dtype=np.int64).reshape(-1, elems.shape[1] - 1)
    if other is None:
        assert not len(rest), f"{len(rest)} boundary faces are no interface elements"
    else:
        assert len(rest) and all(other(verts[r]) for r in rest)
    # the normal, by isosurface's convention, points out of the element
    N = verts.shape[1]
    p, q = verts[once], verts[opp]
    if N == 2:
        d = p[:, 1] - p[:, 0]
        nrm = np.stack([d[:, 1], -d[:, 0]], axis=1)
    else:
        nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert ((nrm * (q - p[:, 0])).sum(axis=1) <= 0).all()


def euler_characteristic(nv, elems):
    """V − E + F (− T): the sub-simplices of every dimension, counted once"""
    N1 = elems.shape[1]
    chi = nv
    for k in range(2, N1 + 1):
        sub = np.concatenate([np.sort(elems[:, list(c)], axis=1) for c in itertools.combinations(range(N1), k)])
        chi += (-1) ** (k - 1) * len(np.unique(sub, axis=0))
    return chi


# ----------------------------------------------------------------------------- closed cases

@pytest.mark.parametrize("name", CLOSED)
def test_closed_cases(name):
    vals, lc, hc, v, e, f = vcase(name)
    _, _, _, iv, ie = case(name)
    N = vals.ndim
    assert v.shape[1] == N and e.shape[1] == N + 1 and f.shape[1] == N and e.dtype == np.int64 and f.dtype == np.int64
    assert len(v) == int(np.count_nonzero(vals < 0)) + count_sign_changes(vals)
    assert np.array_equal(np.unique(e), np.arange(len(v))), "an unreferenced vertex"
    assert np.array_equal(v[f], iv[ie]), "the interface is not isosurface's mesh"
    assert_boundary_is(v, e, f)
    vol = V.signed_volumes(v, e)
    assert (vol > 0).all()
    assert vol.sum() == pytest.approx(R.enclosed(v, f), rel=1e-13)
    assert euler_characteristic(len(v), e) == EULER.get(name, 1)


# ----------------------------------------------------------------------------- the orientation table

@pytest.mark.parametrize("N", [2, 3])
def test_swap_table_rederived_from_random_fields(N):
    """without the table an element is swapped on odd permutations only: then the sign of its volume depends on (sign pattern,
    sub-element) alone, never on the values, and the keys of negative volume are the table"""
    rng = np.random.default_rng(11)
    neg, pos = set(), set()
    for trial in range(4):
        n = (7, 6, 5)[:N]
        vals = np.asfortranarray(rng.standard_normal(n))
        h = rng.uniform(0.5, 2.0, size=N)
        v, e, _, key = V.volume_mesh(vals, (0.0,) * N, tuple(h * (np.array(n) - 1)), swap=V.NO_SWAP, keys=True)
        vol = V.signed_volumes(v, e)
        assert (vol != 0).all()
        for (p, s, t), x in zip(key.tolist(), vol.tolist()):
            (neg if x < 0 else pos).add((s, t))
    keys = {(s, t) for s in range(1, 1 << (N + 1)) for t in range(len(V.pattern_subelements(N, s)))}
    assert len(keys) == (10 if N == 2 else 35)
    assert not (neg & pos), "the sign depends on the values"
    assert neg | pos == keys, "a key never occurred"
    assert neg == set(V.SWAP[N])


# ----------------------------------------------------------------------------- convergence

def test_second_order_3d():
    exact = 4 / 3 * math.pi * SPHERE_R ** 3
    err = [abs(V.measure(*vcase(k)[3:5]) / exact - 1) for k in ("sphere17", "sphere33")]
    assert 3 <= err[0] / err[1] <= 5, err


def test_second_order_2d():
    exact = math.pi * DISK_R ** 2
    err = []
    for k in ("disk33", "disk65"):
        vals, lc, hc, _, _ = case(k)
        v, e, _ = V.volume_mesh(vals, lc, hc)
        err.append(abs(V.measure(v, e) / exact - 1))
    assert 3 <= err[0] / err[1] <= 5, err


# ----------------------------------------------------------------------------- exact planes

PLANE_VOLUME = {"z": 0.3, "diag147": 1.47 ** 3 / 6 - 3 * 0.47 ** 3 / 6, "diag15": 0.5}


def _on_one_box_face(p):
    return any((p[:, a] == x).all() for a in range(p.shape[1]) for x in (0.0, 1.0))


@pytest.mark.parametrize("name", sorted(PLANES))
def test_planes_are_exact(name):
    n, f, _ = PLANES[name]
    vals = grid_vals(n, f, (0.0,) * 3, (1.0,) * 3)
    v, e, i = V.volume_mesh(vals, (0.0,) * 3, (1.0,) * 3)
    vol = V.signed_volumes(v, e)
    assert (vol >= 0).all()
    assert vol.sum() == pytest.approx(PLANE_VOLUME[name], rel=1e-13)
    assert_boundary_is(v, e, i, other=_on_one_box_face)


# ----------------------------------------------------------------------------- nodes on the level

@pytest.mark.parametrize("N", [2, 3])
def test_nodes_on_the_level(N):
    """x + y (+ z) = 1.5 on a dyadic grid passes through nodes: they are outside, elements of zero volume appear and are oriented
    by the table; moving those nodes off the level by the smallest amount, either way, leaves the volume unchanged"""
    n = (17,) * N
    f = lambda X: sum(X) - 1.5
    vals = grid_vals(n, f, (0.0,) * N, (1.0,) * N)
    assert (vals == 0).any()
    v, e, _ = V.volume_mesh(vals, (0.0,) * N, (1.0,) * N)
    vol = V.signed_volumes(v, e)
    assert (vol >= 0).all() and (vol == 0).any()
    for sign in (1.0, -1.0):
        nudged = np.where(vals == 0, -1e-300 * sign, vals)
        vn, en, _ = V.volume_mesh(np.asfortranarray(nudged), (0.0,) * N, (1.0,) * N)
        voln = V.signed_volumes(vn, en)
        assert (voln >= 0).all()
        assert voln.sum() == pytest.approx(vol.sum(), rel=1e-13)


# ----------------------------------------------------------------------------- full and empty fields

@pytest.mark.parametrize("n", [(5, 4, 3), (5, 4)])
def test_all_inside_and_all_outside(n):
    N = len(n)
    lc, hc = (0.0, -1.0, 2.0)[:N], (2.0, 0.5, 2.75)[:N]
    v, e, i = V.volume_mesh(np.full(n, -1.0, order="F"), lc, hc)
    cells = int(np.prod([k - 1 for k in n]))
    assert len(v) == int(np.prod(n)) and len(e) == math.factorial(N) * cells and i.shape == (0, N)
    vol = V.signed_volumes(v, e)
    assert (vol > 0).all() and vol.sum() == pytest.approx(float(np.prod(np.array(hc) - np.array(lc))), rel=1e-13)
    assert_boundary_is(v, e, i, other=lambda p: any((p[:, a] == x).all() for a in range(N) for x in (lc[a], hc[a])))
    v, e, i = V.volume_mesh(np.full(n, 1.0, order="F"), lc, hc)
    assert v.shape == (0, N) and e.shape == (0, N + 1) and i.shape == (0, N)
    assert v.dtype == np.float64 and e.dtype == np.int64 and i.dtype == np.int64
    v, e, i = V.volume_mesh(np.zeros(n, order="F"), lc, hc)             # ϕ == level is outside
    assert len(v) == 0 and len(e) == 0 and len(i) == 0


def test_levels_and_float32():
    vals, lc, hc, _, _ = case("sphere9")
    for level in (0.1, -0.07):
        v, e, i = V.volume_mesh(vals, lc, hc, level=level)
        assert len(v) == int(np.count_nonzero(vals < level)) + count_sign_changes(vals, level)
        assert_boundary_is(v, e, i)
        assert V.measure(v, e) == pytest.approx(R.enclosed(v, i), rel=1e-13)
    a = V.volume_mesh(vals.astype(np.float32), lc, hc)
    b = V.volume_mesh(vals.astype(np.float32).astype(np.float64), lc, hc)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ----------------------------------------------------------------------------- DomainMesh and the Medit writer

_V3 = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [0.0, 1.0e-5, -0.25], [1.0e6, 1.0, 1.0 / 3.0], [0.0, 0.0, 2.0]])
_T3 = np.array([[0, 1, 2, 4], [1, 3, 2, 4]])
_F3 = np.array([[0, 2, 1]])
_EXPECTED_3D = """MeshVersionFormatted 1
Dimension 3

Vertices
5
0.0 0.0 0.0 1
1.0 0.0 0.5 1
0.0 1.0e-5 -0.25 1
1.0e6 1.0 0.3333333333333333 1
0.0 0.0 2.0 1

Tetrahedra
2
1 2 3 5 3
2 4 3 5 3

Triangles
1
1 3 2 10

End
"""
_V2 = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0e-5], [1.0e6, 1.0 / 3.0]])
_T2 = np.array([[0, 1, 2], [1, 3, 2]])
_F2 = np.array([[1, 3], [3, 2]])
_EXPECTED_2D = """MeshVersionFormatted 1
Dimension 2

Vertices
4
0.0 0.0 1
1.0 0.0 1
0.0 1.0e-5 1
1.0e6 0.3333333333333333 1

Triangles
2
1 2 3 3
2 4 3 3

Edges
2
2 4 10
4 3 10

End
"""


@pytest.mark.parametrize("N", [2, 3])
def test_export_volume_mesh_writes_the_file(tmp_path, N):
    import lsm_amd
    vs, ts, fs, expected = (_V2, _T2, _F2, _EXPECTED_2D) if N == 2 else (_V3, _T3, _F3, _EXPECTED_3D)
    m = lsm_amd.DomainMesh(vs, ts, fs)
    assert len(m) == 2 and m.ndim == N and m.level == 0.0 and m.mesh is None
    assert m.vertices.dtype == np.float64 and m.elements.dtype == np.int64 and m.interface.dtype == np.int64
    assert "DomainMesh" in repr(m) and ("tetrahedra" if N == 3 else "triangles") in repr(m)
    out = str(tmp_path / "domain.mesh")
    assert lsm_amd.export_volume_mesh(m, out) == out
    assert open(out).read() == expected


def test_export_volume_mesh_refusals(tmp_path):
    import lsm_amd
    out = str(tmp_path / "domain.mesh")
    m = lsm_amd.DomainMesh(_V3, _T3, _F3)
    for kw in ("hgrad", "hmin", "hmax", "hausd"):
        with pytest.raises(NotImplementedError, match="mmg2d_O3 / mmg3d_O3"):
            lsm_amd.export_volume_mesh(m, out, **{kw: 0.1})
    m1 = lsm_amd.DomainMesh(np.zeros((2, 1)), np.array([[0, 1]]), np.zeros((0, 1), dtype=np.int64))
    with pytest.raises(ValueError, match="export_mesh of 1 dimensional level-set not supported."):
        lsm_amd.export_volume_mesh(m1, out)
    with pytest.raises(TypeError):
        lsm_amd.export_volume_mesh(np.zeros((3, 3, 3)), out)
    with pytest.raises(TypeError, match="device field"):
        lsm_amd.volume_mesh(np.zeros((3, 3, 3)))


def test_domain_mesh_measure():
    import lsm_amd
    for name in ("sphere9", "disk17"):
        _, _, _, v, e, f = vcase(name)
        m = lsm_amd.DomainMesh(v, e, f)
        assert m.measure() == pytest.approx(V.measure(v, e), rel=1e-15)
    N = 3
    empty = lsm_amd.DomainMesh(np.zeros((0, N)), np.zeros((0, N + 1), dtype=np.int64), np.zeros((0, N), dtype=np.int64))
    assert empty.measure() == 0.0 and len(empty) == 0
