"""Host-side mirror of the reference's operator interface for the grid-update path:
CartesianGrid / MeshField / boundary conditions / terms / integrators / LevelSetEquation /
integrate! (Python spelling: ``integrate_``), with the same names, argument meaning and error
behaviour, driving the HIP kernels through the C ABI (include/lsm.h).

The step loop, hooks, Δt arithmetic and error raising stay on the host exactly as in
src/timestepping.jl:101-122; only `_advance!` and `compute_cfl` cross into the library.
"""
import ctypes as C
import math
import os

import numpy as np

from . import _lib as L

# ----------------------------------------------------------------------------- meshes.jl


class CartesianGrid:
    """CartesianGrid(lc, hc, n) — src/meshes.jl:1-5,34-42 — or CartesianGrid(lc, hc, meshsize=h) — src/meshes.jl:69-83:
    the cell count of each dimension is rounded UP, so the realised spacing is never coarser than `meshsize`."""

    def __init__(self, lc, hc, n=None, *, meshsize=None):
        lc, hc = tuple(lc), tuple(hc)
        if (n is None) == (meshsize is None):
            raise ValueError("pass either the node counts n or meshsize")
        if n is None:
            if len(lc) != len(hc):
                raise ValueError("lc and hc must have the same length")
            h = (meshsize,) * len(lc) if isinstance(meshsize, (int, float)) else tuple(meshsize)
            if len(h) != len(lc):
                raise ValueError("meshsize must be a scalar or have one entry per dimension")
            if not all(x > 0 for x in h):
                raise ValueError("meshsize must be positive in every dimension")
            if not all(b > a for a, b in zip(lc, hc)):
                raise ValueError("hc must be strictly greater than lc in every dimension")
            n = tuple(int(math.ceil((b - a) / x)) + 1 for a, b, x in zip(lc, hc, h))
        n = tuple(n)
        if not (len(lc) == len(hc) == len(n)):
            raise ValueError("all arguments must have the same length")
        self.lc = tuple(float(x) for x in lc)
        self.hc = tuple(float(x) for x in hc)
        self.n = tuple(int(x) for x in n)

    @property
    def ndim(self):
        return len(self.n)

    def size(self):
        return self.n

    def meshsize(self, dim=None):
        """(hc - lc) / (n - 1) — src/meshes.jl:109-110 (dim is 0-based)."""
        h = tuple((self.hc[d] - self.lc[d]) / (self.n[d] - 1) for d in range(self.ndim))
        return h if dim is None else h[dim]

    def getnode(self, I):
        """lc + (I-1)*h for a 0-based index tuple I — src/meshes.jl:114-130."""
        I = tuple(I)
        if not all(0 <= I[d] < self.n[d] for d in range(self.ndim)):
            raise ValueError(f"{I} is not a valid node index for this grid")
        h = self.meshsize()
        return tuple(self.lc[d] + float(I[d]) * h[d] for d in range(self.ndim))

    def coords(self):
        h = self.meshsize()
        return [self.lc[d] + np.arange(self.n[d], dtype=np.float64) * h[d] for d in range(self.ndim)]

    def __len__(self):
        return int(np.prod(self.n))

    def nodeindices(self):
        """All node indices (0-based tuples), first index fastest like CartesianIndices — src/meshes.jl:138."""
        return _cartesian_indices(self.n)

    def cellindices(self):
        """All cell indices: cell I is bounded by nodes I and I+1, n[d]-1 cells per dimension — src/meshes.jl:147."""
        return _cartesian_indices(tuple(k - 1 for k in self.n))

    def compute_index(self, x):
        """Index of the cell containing x, clamped to the grid — src/meshes.jl:155-169."""
        h = self.meshsize()
        return tuple(min(max(int(math.floor((x[d] - self.lc[d]) / h[d])), 0), self.n[d] - 2) for d in range(self.ndim))

    def getcell(self, I):
        """CartesianCell of cell I: lc = node I, hc = lc + h — src/meshes.jl:183-197 (unpacks as `lc, hc = cell`)."""
        I = tuple(I)
        if not all(0 <= I[d] < self.n[d] - 1 for d in range(self.ndim)):
            raise ValueError(f"{I} is not a valid cell index for this grid")
        h = self.meshsize()
        lc = tuple(self.lc[d] + float(I[d]) * h[d] for d in range(self.ndim))
        return CartesianCell(lc, tuple(lc[d] + h[d] for d in range(self.ndim)))

    def grid1d(self, dim=None):
        """Node coordinates along `dim` as LinRange(lc, hc, n) does — src/meshes.jl:90-91."""
        ax = [np.linspace(self.lc[d], self.hc[d], self.n[d]) for d in range(self.ndim)]
        return tuple(ax) if dim is None else ax[dim]

    def _c(self):
        g = L.LsmGrid()
        g.ndim = self.ndim
        for d in range(3):
            g.n[d] = self.n[d] if d < self.ndim else 1
            g.lc[d] = self.lc[d] if d < self.ndim else 0.0
            g.hc[d] = self.hc[d] if d < self.ndim else 1.0
        return g

    def _show(self):
        """src/meshes.jl:226-242."""
        return "\n".join([f"CartesianGrid in ℝ{_superscript(self.ndim)}"] + _grid_fields(self))

    __repr__ = _show


class CartesianCell:
    """A cell of a CartesianGrid: the box between the nodes at `lc` and `hc` — src/meshes.jl:171-181."""

    def __init__(self, lc, hc):
        self.lc, self.hc = tuple(lc), tuple(hc)

    def __iter__(self):
        return iter((self.lc, self.hc))

    def _show(self):
        """src/meshes.jl:243-250"""
        f = lambda c: "(" + ", ".join(_sig4(x) for x in c) + ")"
        return f"CartesianCell in ℝ{_superscript(len(self.lc))}\n  ├─ lower corner: {f(self.lc)}\n  └─ upper corner: {f(self.hc)}"

    __repr__ = _show


def _cartesian_indices(shape):
    """index tuples of an array of `shape`, first index fastest (Julia's CartesianIndices order)"""
    import itertools
    return [tuple(reversed(t)) for t in itertools.product(*[range(k) for k in reversed(shape)])]


def nodeindices(g):
    return g.nodeindices()


def cellindices(g):
    return g.cellindices()


def getnode(g, *I):
    return g.getnode(I[0] if len(I) == 1 and not isinstance(I[0], int) else I)


def getcell(g, *I):
    return g.getcell(I[0] if len(I) == 1 and not isinstance(I[0], int) else I)


def active_nodeindices(phi):
    """active_nodeindices(ϕ) — src/meshfield.jl:134 (dense: every node) / :462 (band: the stored nodes)."""
    return phi.active_nodeindices() if hasattr(phi, "active_nodeindices") else phi.mesh.nodeindices()


def active_cellindices(phi):
    return phi.active_cellindices() if hasattr(phi, "active_cellindices") else phi.mesh.cellindices()


def update_band_(phi):
    """update_band!(ϕ) — src/meshfield.jl:553 (dense: no-op) / :555-588 (band)."""
    if isinstance(phi, LevelSetEquation):
        return phi.update_band()
    return phi.rebuild() if hasattr(phi, "rebuild") else phi


# ----------------------------------------------------------------------------- boundaryconditions.jl

class BoundaryCondition:
    pass


class PeriodicBC(BoundaryCondition):
    kind, degree = L.BC_PERIODIC, 0

    def __repr__(self):
        return "Periodic"


class ExtrapolationBC(BoundaryCondition):
    """ExtrapolationBC{P} — src/boundaryconditions.jl:40-46."""
    kind = L.BC_EXTRAPOLATION

    def __init__(self, P=0):
        if P < 0:
            raise ValueError("extrapolation order P must be at least 0")
        self.degree = int(P)

    def __repr__(self):
        return {0: "Neumann", 1: "Linear extrapolation"}.get(self.degree, f"Degree {self.degree} extrapolation")


def NeumannBC():
    return ExtrapolationBC(0)


def LinearExtrapolationBC():
    return ExtrapolationBC(1)


class SymmetryBC(BoundaryCondition):
    kind, degree = L.BC_SYMMETRY, 0

    def __repr__(self):
        return "Symmetry"


def _same_bc(a, b):
    return a.kind == b.kind and a.degree == b.degree


def _normalize_bc(bc, dim):
    """src/boundaryconditions.jl:166-188."""
    if isinstance(bc, BoundaryCondition):
        return tuple((bc, bc) for _ in range(dim))
    if len(bc) != dim:
        raise ValueError("invalid number of boundary conditions")
    out = []
    for i, b in enumerate(bc):
        if isinstance(b, BoundaryCondition):
            out.append((b, b))
            continue
        if not (len(b) == 2 and all(isinstance(x, BoundaryCondition) for x in b)):
            raise ValueError(f"invalid boundary condition for dimension {i + 1}")
        left, right = b
        if isinstance(left, PeriodicBC) != isinstance(right, PeriodicBC):
            raise ValueError(f"periodic boundary conditions cannot be mixed with others in dimension {i + 1}")
        out.append((left, right))
    return tuple(out)


def _bc_c(bcs, ndim, slab_faces=(False, False)):
    arr = L.BcArray()
    for d in range(3):
        for s in range(2):
            if d < ndim:
                arr[d][s].kind, arr[d][s].degree = bcs[d][s].kind, bcs[d][s].degree
                if d == ndim - 1 and slab_faces[s]:
                    arr[d][s].kind, arr[d][s].degree = L.BC_NONE, 0
            else:
                arr[d][s].kind, arr[d][s].degree = L.BC_EXTRAPOLATION, 0
    return arr


# ----------------------------------------------------------------------------- show (text/plain) helpers
# The reference prints trees (src/meshes.jl:226-242, src/meshfield.jl:294-312,395-414, src/levelsetequation.jl:91-116,
# src/boundaryconditions.jl:197-211, src/timestepping.jl:94-97; checked by test/test-show.jl): `show(x)` returns the
# same text, `repr(x)` of an equation the compact one-line form.

def _superscript(n):
    return "".join("⁰¹²³⁴⁵⁶⁷⁸⁹"[int(d)] for d in str(int(n)))


def _jl_float(x):
    """A Float64 as Julia prints it: shortest round-trip digits, exponent form below 1e-4 and from 1e6 on."""
    x = float(x)
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "Inf" if x > 0 else "-Inf"
    if x == 0.0:
        return "-0.0" if math.copysign(1.0, x) < 0 else "0.0"
    r = repr(x)
    mant, _, ex = r.partition("e")
    if "e" in r:
        e = int(ex)
        digits = mant.replace("-", "").replace(".", "")
        point = (mant.replace("-", "").index(".") if "." in mant else len(mant.replace("-", ""))) + e
    else:
        digits = mant.replace("-", "").replace(".", "")
        point = mant.replace("-", "").index(".") if "." in mant else len(digits)
    lead = len(digits) - len(digits.lstrip("0"))
    digits, point = digits[lead:].rstrip("0") or "0", point - lead
    sign = "-" if x < 0 else ""
    e10 = point - 1                                  # decimal exponent of the leading digit
    if -5 < e10 < 6:                                 # Julia: plain notation for 1e-4 <= |x| < 1e6
        if point <= 0:
            return f"{sign}0.{'0' * (-point)}{digits}"
        if point >= len(digits):
            return f"{sign}{digits}{'0' * (point - len(digits))}.0"
        return f"{sign}{digits[:point]}.{digits[point:]}"
    return f"{sign}{digits[0]}.{digits[1:] or '0'}e{e10}"


def _sig4(x):
    """round(x; sigdigits = 4) printed as Julia prints the result."""
    x = float(x)
    if x == 0.0 or math.isnan(x) or math.isinf(x):
        return _jl_float(x)
    return _jl_float(float(f"{x:.3e}"))


def _bc_str(bcs):
    """src/boundaryconditions.jl:197-211."""
    allb = [b for pair in bcs for b in pair]
    if all(_same_bc(b, allb[0]) for b in allb):
        return f"{allb[0]!r} (all)"
    names = ("x", "y", "z") if len(bcs) <= 3 else tuple(f"d{i + 1}" for i in range(len(bcs)))
    return ", ".join(f"{names[d]}: " + (repr(l) if _same_bc(l, r) else f"{l!r} ↔ {r!r}") for d, (l, r) in enumerate(bcs))


def _grid_fields(g, prefix="  ", last=True):
    dom = " × ".join(f"[{_jl_float(a)}, {_jl_float(b)}]" for a, b in zip(g.lc, g.hc))
    h = "(" + ", ".join(_sig4(x) for x in g.meshsize()) + ")"
    return [f"{prefix}├─ domain:  {dom}", f"{prefix}├─ nodes:   {' × '.join(map(str, g.n))}",
            f"{prefix}{'└─' if last else '├─'} spacing: h = {h}"]


def _field_fields(mesh, bcs, valtype, extrema, prefix="  ", active=None):
    lines = _grid_fields(mesh, prefix, last=False)
    if bcs is not None:
        lines.append(f"{prefix}├─ bc:     {_bc_str(bcs)}")
    if active is not None:
        lines.append(f"{prefix}├─ active:  {active[0]} nodes ({active[1]}-layer halo)")
    if extrema is None:
        lines.append(f"{prefix}└─ valtype: {valtype}")
    else:
        lines.append(f"{prefix}├─ valtype: {valtype}")
        lines.append(f"{prefix}└─ values:  min = {_sig4(extrema[0])},  max = {_sig4(extrema[1])}")
    return lines


def _embed_show(label, text, indent="  "):
    """src/levelsetequation.jl:91-99."""
    parts = text.split("\n")
    return [f"{indent}├─ {label}: {parts[0]}"] + [f"{indent}│{line}" for line in parts[1:]]


def show(x):
    """The text/plain `show` of the reference for grids, fields, integrators and equations (test/test-show.jl)."""
    return x._show() if hasattr(x, "_show") else repr(x)


# ----------------------------------------------------------------------------- meshfield.jl

class MeshField:
    """Host-resident dense field (src/meshfield.jl:51-55): `vals` is a numpy array of shape
    grid.n in Fortran order (the reference's column-major Array), or shape (ncomp, *grid.n) for
    vector-valued coefficient fields."""

    def __init__(self, vals_or_f, grid, bc=None, dtype=None):
        # element type as in the reference (the eltype of `vals`): float64, or float32 storage when asked for / given
        if dtype is None:
            dtype = np.float32 if getattr(vals_or_f, "dtype", None) == np.float32 else np.float64
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError(f"unsupported element type {dtype}: float64 or float32")
        if callable(vals_or_f):
            xs = np.meshgrid(*grid.coords(), indexing="ij", sparse=True)
            v = vals_or_f(tuple(xs))
            if isinstance(v, (tuple, list)):
                v = np.stack([np.broadcast_to(np.asarray(c, dtype=np.float64), grid.n) for c in v])
            else:
                v = np.broadcast_to(np.asarray(v, dtype=np.float64), grid.n)
            vals = np.array(v, dtype=dtype)
        else:
            vals = np.array(vals_or_f, dtype=dtype)
        if vals.shape[-grid.ndim:] != grid.n:
            raise ValueError(f"values of shape {vals.shape} do not match the grid {grid.n}")
        self.vals = np.asfortranarray(vals) if vals.ndim == grid.ndim else vals
        self.mesh = grid
        self.bcs = None if bc is None else _normalize_bc(bc, grid.ndim)

    def has_boundary_conditions(self):
        return self.bcs is not None

    def values(self):
        return self.vals

    def copy(self):
        m = MeshField(self.vals.copy(order="K"), self.mesh, dtype=self.vals.dtype)
        m.bcs = self.bcs
        return m

    def copy_(self, src):
        """copy!(dest, src) — src/meshfield.jl:282-292: the values of `src`; dest keeps its mesh and boundary conditions."""
        v = src.values() if hasattr(src, "values") else np.asarray(src)
        if v.shape != self.vals.shape:
            raise ValueError("copy!: the fields have different sizes")
        self.vals[...] = v
        return self

    def with_bc(self, bc):
        """_add_boundary_conditions(ϕ, bc) — src/meshfield.jl:104-113: a field over the SAME values array with boundary conditions."""
        m = MeshField.__new__(MeshField)
        m.vals, m.mesh, m.bcs = self.vals, self.mesh, _normalize_bc(bc, self.mesh.ndim)
        return m

    @property
    def ndim(self):
        return self.mesh.ndim

    def meshsize(self, dim=None):
        return self.mesh.meshsize(dim)

    def __getitem__(self, I):
        """ϕ[I] with 0-based I; out-of-grid indices go through the boundary conditions
        (_getindexbc, src/meshfield.jl:213-260)."""
        I = tuple(I) if not isinstance(I, int) else (I,)
        n = self.mesh.n
        if all(0 <= I[d] < n[d] for d in range(len(n))):
            return float(self.vals[I])
        if self.bcs is None:
            raise ValueError(f"index {I} lies outside the grid, but the field has no boundary conditions to resolve it.")
        return self._getindexbc(I, len(n))

    def _getindexbc(self, I, dim):
        if dim == 0:
            return float(self.vals[I])
        d = dim - 1
        n = self.mesh.n[d]
        if 0 <= I[d] < n:
            return self._getindexbc(I, dim - 1)
        left = I[d] < 0
        bc = self.bcs[d][0 if left else 1]
        k = -I[d] if left else I[d] - (n - 1)
        b, sgn = (0, 1) if left else (n - 1, -1)
        acc = 0.0
        if bc.kind == L.BC_PERIODIC:
            J = I[:d] + (((n - 1) - k) if left else k,) + I[d + 1:]
            acc += 1.0 * self._getindexbc(J, dim - 1)
        elif bc.kind == L.BC_EXTRAPOLATION:
            P = bc.degree
            for j in range(P + 1):
                w = 1.0
                for m in range(P + 1):
                    if m != j:
                        w *= (-k - m) / (j - m)
                acc += w * self._getindexbc(I[:d] + (b + sgn * j,) + I[d + 1:], dim - 1)
        else:
            acc += 1.0 * self._getindexbc(I[:d] + (b + sgn * k,) + I[d + 1:], dim - 1)
        return acc

    # ---- set operations on level sets (src/levelsetops.jl:246-325): union = min, intersection = max,
    #      complement = negation, difference = max(ϕ₁, -ϕ₂); the in-place forms return self, as the reference's `!` forms
    def _other(self, o):
        if not isinstance(o, MeshField) or o.mesh.n != self.mesh.n:
            raise ValueError("set operations need two MeshFields on the same grid")
        return o.vals

    def union_(self, o):
        np.minimum(self.vals, self._other(o), out=self.vals)
        return self

    def intersect_(self, o):
        np.maximum(self.vals, self._other(o), out=self.vals)
        return self

    def complement_(self):
        np.negative(self.vals, out=self.vals)
        return self

    def setdiff_(self, o):
        np.maximum(self.vals, -self._other(o), out=self.vals)
        return self

    def union(self, o):
        return self.copy().union_(o)

    def intersect(self, o):
        return self.copy().intersect_(o)

    def complement(self):
        return self.copy().complement_()

    def setdiff(self, o):
        return self.copy().setdiff_(o)

    __or__, __and__, __sub__, __neg__ = union, intersect, setdiff, complement     # ϕ₁ ∪ ϕ₂, ϕ₁ ∩ ϕ₂, setdiff, complement

    def _show(self):
        """src/meshfield.jl:294-312."""
        scalar = self.vals.ndim == self.mesh.ndim
        et = "Float32" if self.vals.dtype == np.float32 else "Float64"
        vt = et if scalar else f"SVector{{{self.vals.shape[0]}, {et}}}"
        ext = (self.vals.min(), self.vals.max()) if scalar else None
        return "\n".join([f"MeshField on CartesianGrid in ℝ{_superscript(self.mesh.ndim)}"] + _field_fields(self.mesh, self.bcs, vt, ext))

    __repr__ = _show


class LazyMeshField:
    """MeshField(f, grid) whose samples are only ever materialised slab by slab (large grids,
    multi-GPU): `f` receives a tuple of broadcastable coordinate arrays like MeshField's."""

    def __init__(self, f, grid, bc=None, dtype=np.float64):
        self.f, self.mesh = f, grid
        self.dtype = np.dtype(dtype)
        self.bcs = None if bc is None else _normalize_bc(bc, grid.ndim)

    def has_boundary_conditions(self):
        return self.bcs is not None

    def local_values(self, slab):
        cs = self.mesh.coords()
        if slab is not None:
            cs[-1] = cs[-1][slab[0]:slab[0] + slab[1]]
        xs = np.meshgrid(*cs, indexing="ij", sparse=True)
        shape = tuple(len(c) for c in cs)
        return np.asfortranarray(np.broadcast_to(np.asarray(self.f(tuple(xs)), dtype=np.float64), shape))


class ROCMeshField:
    """Device-resident field: a padded HBM buffer (layout from lsm_layout) + the grid + the
    normalised boundary conditions + the backend handle.  Plays the role of the
    `ROCMeshField <: AbstractMeshField` of SURVEY.md §8b."""

    def __init__(self, backend, mesh, bcs, buf=None):
        self.backend, self.mesh, self.bcs = backend, mesh, bcs
        self.buf = backend.alloc() if buf is None else buf
        self.ghosts_dirty = True    # set whenever the interior is rewritten from outside a step

    @classmethod
    def from_host(cls, backend, mf, bcs=None, local=None):
        f = cls(backend, mf.mesh, bcs if bcs is not None else mf.bcs)
        v = mf.vals if local is None else mf.vals[(Ellipsis, local)]
        backend.upload(f.buf, v)
        return f

    def values(self):
        """Host copy of the (local) interior, Fortran order."""
        return self.backend.download(self.buf)

    def to_host(self):
        m = MeshField(self.values(), self.mesh)
        m.bcs = self.bcs
        return m

    def copy(self):
        return ROCMeshField(self.backend, self.mesh, self.bcs, self.backend.clone(self.buf))

    def copy_(self, src):
        """copy!(dest, src) — src/meshfield.jl:289-292; accepts a device or a host field."""
        if isinstance(src, ROCMeshField):
            self.backend.copy_(self.buf, src.buf)
        else:
            self.backend.upload(self.buf, src.vals if isinstance(src, MeshField) else src)
        self.ghosts_dirty = True
        return self

    def extrema(self):
        return self.backend.extrema(self.buf)

    def _offset(self, I):
        I = tuple(I) if not isinstance(I, int) else (I,)
        lay = self.backend.lay
        if not all(0 <= I[d] < int(lay.n[d]) for d in range(len(I))):
            raise IndexError(f"index {I} is outside the (local) grid; ghost values are resolved inside the kernels")
        return int(lay.origin) + sum(int(I[d]) * int(lay.stride[d]) for d in range(len(I)))

    def __getitem__(self, I):
        """ϕ[I] (0-based, in-grid): scalar device read — slow, for tests and hooks (src/meshfield.jl:213-217)."""
        return float(self.buf[self._offset(I)].item())

    def __setitem__(self, I, val):
        """ϕ[I] = v (src/meshfield.jl:263-266): scalar device write; marks the ghost layers stale."""
        self.buf[self._offset(I)] = float(val)
        self.ghosts_dirty = True

    def _valtype(self):
        return "Float32" if np.dtype(getattr(self.backend, "dtype", np.float64)) == np.float32 else "Float64"

    def _show(self):
        """src/meshfield.jl:294-312 — the device field prints as the reference's MeshField does (extrema by lsm_extrema)."""
        return "\n".join([f"MeshField on CartesianGrid in ℝ{_superscript(self.mesh.ndim)}"] +
                         _field_fields(self.mesh, self.bcs, self._valtype(), self.extrema()))

    __repr__ = _show


class NarrowBandMeshField:
    """NarrowBandMeshField(ϕ::MeshField; nlayers = 3) / NarrowBandMeshField(f, grid; bc, nlayers)
    (src/meshfield.jl:411-440): host-side description of a field restricted to the topological band
    of `nlayers` nodes around the cut cells.  Passing it as `ic` makes the equation evolve the band only."""

    def __init__(self, phi_or_f, grid=None, bc=None, nlayers=3):
        base = phi_or_f if isinstance(phi_or_f, MeshField) else MeshField(phi_or_f, grid, bc=bc)
        if base.bcs is not None and any(b.kind == L.BC_PERIODIC for pair in base.bcs for b in pair):
            raise ValueError("PeriodicBC is not supported on a NarrowBandMeshField")   # src/meshfield.jl:339-340
        self.base, self.mesh, self.bcs, self.nlayers = base, base.mesh, base.bcs, int(nlayers)
        self.vals = base.vals

    def has_boundary_conditions(self):
        return self.bcs is not None


class ROCNarrowBandMeshField(ROCMeshField):
    """Device narrow band: dense padded values + a byte mask of active nodes (+ the halo mask and
    tile flags derived from it).  Non-band entries of the value array are scratch: before every
    stage they are refilled, within 3 nodes of the band, with the reference's affine extrapolant."""
    MC = int(os.environ.get("LSM_BAND_MC", "16"))   # planes per brick in band mode (tile = 32 x 8 x MC in 3-D; 16 measured best at 768^3: tools/band_probe.py)
    HALO = 3

    def __init__(self, backend, mesh, bcs, nlayers, buf=None):
        super().__init__(backend, mesh, bcs, buf)
        self.nlayers = int(nlayers)
        self.mask = backend.alloc_mask()
        self.halo = backend.alloc_mask()
        self.tiles = backend.alloc_tiles(self.MC)
        self._scratch = (backend.alloc_mask(), backend.alloc_mask())   # reused by every rebuild
        self._hlist = self._hcount = None

    def rebuild(self, from_dense=False):
        """update_band! (src/meshfield.jl:555-588) + what is derived from the new band: tile flags, the
        halo mask and the (halo node -> nearest band node) list every stage input is filled from."""
        b = self.backend
        if self._hlist is None:
            self._hlist, self._hcount = b.alloc_halo_list(1 << 16)
        b.band_update(self.buf, self.mask, from_dense, self.nlayers, self._scratch[0], self._scratch[1], self.halo,
                      self.tiles, self.MC, self._hlist, self._hcount)
        self._check_halo()
        self.ghosts_dirty = True

    def _check_halo(self):
        b = self.backend
        want, missed = b.band_status(self._hcount)
        if want > self._hlist.numel() // 2:          # list too short: grow it and search again
            self._hlist, self._hcount = b.alloc_halo_list(2 * want)
            b.band_halo(self.buf, self.mask, self.halo, self.tiles, self.MC, self._hlist, self._hcount)
            want, missed = b.band_status(self._hcount)
        if missed:                                   # src/meshfield.jl:499-500
            raise ValueError("a stencil of the band reads a node more than 6 nodes away from every band node")

    def prepare(self, buf):
        """Make `buf` readable by stencils: band halo (extrapolation) then out-of-grid ghosts (BCs)."""
        self.backend.band_prepare(buf, self.mask, self._hlist, self._hcount, self.tiles, self.MC)

    def active_mask(self):
        return self.backend.mask_to_host(self.mask)

    def active_count(self):
        return self.backend.band_count(self.mask)

    def _show(self):
        """src/meshfield.jl:395-414: the extrema are those of the band's values (off-band entries are scratch)."""
        vals = self.values()[self.active_mask()]
        ext = (vals.min(), vals.max()) if vals.size else (float("nan"), float("nan"))
        return "\n".join([f"NarrowBandMeshField on CartesianGrid in ℝ{_superscript(self.mesh.ndim)}"] +
                         _field_fields(self.mesh, self.bcs, self._valtype(), ext, active=(self.active_count(), self.nlayers)))

    __repr__ = _show

    def active_nodeindices(self):
        return [tuple(int(i) for i in I) for I in np.argwhere(self.active_mask())]

    def active_cellindices(self):
        """Cells whose 2^N corners are all band nodes (src/meshfield.jl:364-369), by their lower corner (0-based)."""
        m = self.active_mask()
        N = m.ndim
        ok = np.ones(tuple(k - 1 for k in m.shape), dtype=bool)
        for off in np.ndindex(*(2,) * N):
            ok &= m[tuple(slice(o, m.shape[d] - 1 + o) for d, o in enumerate(off))]
        return [tuple(int(i) for i in I) for I in np.argwhere(ok)]

    def values(self):
        """Host copy: stored values on the band, NaN elsewhere."""
        v = self.backend.download(self.buf)
        v[~self.active_mask()] = np.nan
        return v

    def copy(self):
        c = ROCNarrowBandMeshField(self.backend, self.mesh, self.bcs, self.nlayers, self.backend.clone(self.buf))
        c.mask.copy_(self.mask)
        c.halo.copy_(self.halo)
        c.tiles.copy_(self.tiles)
        if self._hlist is not None:
            c._hlist, c._hcount = self._hlist.clone(), self._hcount.clone()
        return c

    def copy_(self, src):
        """copy!(dest, src) (src/meshfield.jl:282-292): the values AND the active set of `src` (the Dict copy! syncs keys);
        dest keeps its own mesh, boundary conditions and nlayers."""
        if not isinstance(src, ROCNarrowBandMeshField):
            raise ValueError("copy! into a narrow-band field takes a narrow-band field")
        self.backend.copy_(self.buf, src.buf)
        self.mask.copy_(src.mask)
        self.halo.copy_(src.halo)
        self.tiles.copy_(src.tiles)
        if src._hlist is not None:
            self._hlist, self._hcount = src._hlist.clone(), src._hcount.clone()
        # the handle's compact tile lists (and a prefetched Δt) describe the band this buffer held before: rebuild them
        self.backend.band_retile(self.mask, self.tiles, self.MC)
        if self._hcount is not None:
            self.backend.band_status(self._hcount)
        self.ghosts_dirty = True
        return self

    def __getitem__(self, I):
        """ϕ[I] (src/meshfield.jl:441-445,475-511): stored value on the band, affine extrapolant from the
        nearest band node elsewhere in the grid, boundary conditions outside the grid.  Slow scalar path."""
        I = tuple(I) if not isinstance(I, int) else (I,)
        n = self.mesh.n
        if all(0 <= I[d] < n[d] for d in range(len(n))):
            off = self._offset(I)
            if not bool(self.mask[off].item()):
                t = self.backend.alloc_mask()
                t[off] = 1
                self.backend.band_fill(self.buf, self.mask, t, None, self.MC)   # whole grid: the node may be far from the band
                if self.backend.band_missed():
                    raise ValueError(f"index {I} is more than 6 nodes from the band")
            return float(self.buf[off].item())
        if self.bcs is None:
            raise ValueError(f"index {I} lies outside the grid, but the field has no boundary conditions to resolve it.")
        return self._bc_resolve(I, len(n))

    def _bc_resolve(self, I, dim):   # _getindexbc (src/meshfield.jl:248-260) over this field's own getindex
        if dim == 0:
            return self[I]
        d = dim - 1
        n = self.mesh.n[d]
        if 0 <= I[d] < n:
            return self._bc_resolve(I, dim - 1)
        left = I[d] < 0
        bc = self.bcs[d][0 if left else 1]
        k = -I[d] if left else I[d] - (n - 1)
        b, sgn = (0, 1) if left else (n - 1, -1)
        acc = 0.0
        if bc.kind == L.BC_EXTRAPOLATION:
            P = bc.degree
            for j in range(P + 1):
                w = 1.0
                for m in range(P + 1):
                    if m != j:
                        w *= (-k - m) / (j - m)
                acc += w * self._bc_resolve(I[:d] + (b + sgn * j,) + I[d + 1:], dim - 1)
        else:
            acc += 1.0 * self._bc_resolve(I[:d] + (b + sgn * k,) + I[d + 1:], dim - 1)
        return acc


# ----------------------------------------------------------------------------- derivatives.jl schemes

class SpatialScheme:
    pass


class Upwind(SpatialScheme):
    code = L.SCHEME_UPWIND


class WENO5(SpatialScheme):
    code = L.SCHEME_WENO5


# ----------------------------------------------------------------------------- coefficient catalogue
# Julia closures f(x,t) cannot run on the device (SURVEY.md §7 hard part 2).  Coefficients are:
#   numbers / tuples            -> CONST
#   RigidRotation               -> ROTATION   (the (x,t)->(-x₂,x₁) of the reference's tests/docs)
#   SeparableCoefficient        -> SEPARABLE  (per-axis tables × g(t), e.g. vortex deformation)
#   MeshField                   -> FIELD      (device arrays, SoA per component)
#   python callable f(x,t)      -> FIELD re-sampled on the host before the CFL and each stage (slow path)

class RigidRotation:
    """u = ω·(-(x₂-c₂), x₁-c₁ [, 0])."""

    def __init__(self, omega=1.0, center=(0.0, 0.0)):
        self.omega, self.center = float(omega), (float(center[0]), float(center[1]))


class SeparableCoefficient:
    """u_c(x,t) = ((T_c1[i1]·T_c2[i2])·T_c3[i3])·g(t); tables[c][axis] are 1-D arrays over the
    GLOBAL grid; time is None (g=1) or ('cos', T) for g = cos(πt/T)."""

    def __init__(self, tables, time=None):
        self.tables = [[np.asarray(t, dtype=np.float64) for t in comp] for comp in tables]
        self.time = time


def vortex_deformation(grid, period=3.0):
    """LeVeque's 3-D deformation field:
    u = 2 sin²(πx) sin(2πy) sin(2πz) g, v = -sin(2πx) sin²(πy) sin(2πz) g, w = -sin(2πx) sin(2πy) sin²(πz) g,
    g = cos(πt/period).  Tables are evaluated with the host libm at the node coordinates."""
    x, y, z = grid.coords()
    s2 = lambda a: np.sin(np.pi * a) * np.sin(np.pi * a)
    s = lambda a: np.sin(2 * np.pi * a)
    return SeparableCoefficient([[2 * s2(x), s(y), s(z)], [-s(x), s2(y), s(z)], [-s(x), s(y), s2(z)]], time=("cos", period))


class _Coeff:
    """Resolved coefficient bound to a backend: owns device buffers, fills an LsmCoeff."""

    def __init__(self, spec, ncomp, grid, backend, slab):
        self.spec, self.ncomp, self.grid, self.backend, self.slab = spec, ncomp, grid, backend, slab
        self.c = L.LsmCoeff()
        self._keep = []
        self.callable = None
        self.fields = None
        if isinstance(spec, RigidRotation):
            self.c.kind = L.COEFF_ROTATION
            self.c.value[0], self.c.value[1], self.c.value[2] = spec.omega, spec.center[0], spec.center[1]
        elif isinstance(spec, SeparableCoefficient):
            self.c.kind = L.COEFF_SEPARABLE
            if spec.time is not None:
                self.c.time_kind, self.c.time_param = L.TIME_COS, float(spec.time[1])
            for k in range(ncomp):
                t = backend.table(np.concatenate(spec.tables[k]))
                self._keep.append(t)
                self.c.sep[k] = t.data_ptr()
        elif isinstance(spec, (MeshField, ROCMeshField)) or callable(spec) or self._device_components(spec):
            self.c.kind = L.COEFF_FIELD
            self.fields = [getattr(backend, "alloc_side", backend.alloc)() for _ in range(ncomp)]
            for k, t in enumerate(self.fields):
                self.c.field[k] = t.data_ptr()
            if callable(spec):
                self.callable = spec
            else:
                self.set_values(spec)
        else:
            vals = spec if isinstance(spec, (tuple, list, np.ndarray)) else (spec,)
            if len(vals) != ncomp:
                raise ValueError(f"expected {ncomp} coefficient component(s), got {len(vals)}")
            self.c.kind = L.COEFF_CONST
            for k, v in enumerate(vals):
                self.c.value[k] = float(v)

    def _local(self, a):
        if self.slab is None:
            return a
        return a[..., self.slab[0]:self.slab[0] + self.slab[1]]

    @staticmethod
    def _device_components(spec):
        return isinstance(spec, (tuple, list)) and len(spec) > 0 and all(isinstance(x, ROCMeshField) for x in spec)

    def set_values(self, vals):
        """New values of a FIELD coefficient: a host array of shape grid.n or (ncomp, *grid.n) / a host MeshField
        (uploaded), or device fields — a ROCMeshField (scalar speed / b) or one per component (velocity) — copied
        device to device into the coefficient's float64 side arrays (a float32 field widens exactly)."""
        if isinstance(vals, ROCMeshField) or self._device_components(vals):
            comps = [vals] if isinstance(vals, ROCMeshField) else list(vals)
            if len(comps) != self.ncomp:
                raise ValueError(f"expected {self.ncomp} coefficient component(s), got {len(comps)}")
            for k, src in enumerate(comps):
                if src.buf.numel() == self.fields[k].numel() and src.buf.device == self.fields[k].device:
                    self.fields[k].copy_(src.buf)                      # same padded layout: HBM to HBM
                else:
                    v = src.values().astype(np.float64)                # another handle's layout (e.g. a whole-grid field on a slab)
                    getattr(self.backend, "upload_side", self.backend.upload)(self.fields[k], v if v.shape == tuple(self.backend.local_shape()) else self._local(v))
            return
        if isinstance(vals, MeshField):
            vals = vals.vals
        vals = np.asarray(vals, dtype=np.float64)
        if vals.ndim == self.grid.ndim:
            vals = vals[None]
        for k in range(self.ncomp):
            getattr(self.backend, "upload_side", self.backend.upload)(self.fields[k], self._local(vals[k]))

    def refresh(self, t):
        """Slow path: re-sample a python callable f(x, t) on the host."""
        if self.callable is None:
            return
        xs = tuple(np.meshgrid(*self.grid.coords(), indexing="ij", sparse=True))
        v = self.callable(xs, t)
        if not isinstance(v, (tuple, list)):
            v = (v,)
        self.set_values(np.stack([np.broadcast_to(np.asarray(c, dtype=np.float64), self.grid.n) for c in v]))


# ----------------------------------------------------------------------------- levelsetterms.jl

class LevelSetTerm:
    update_func = None
    coeff = None

    def _bind(self, grid, backend, slab):
        pass


class AdvectionTerm(LevelSetTerm):
    """AdvectionTerm(𝐮[, scheme = WENO5(), update_func]) — 𝐮 ⋅ ∇ϕ (src/levelsetterms.jl:45-63)."""
    kind = L.TERM_ADVECTION

    def __init__(self, velocity, scheme=None, update_func=None):
        self.velocity, self.scheme, self.update_func = velocity, scheme or WENO5(), update_func

    def _bind(self, grid, backend, slab):
        self.coeff = _Coeff(self.velocity, grid.ndim, grid, backend, slab)

    def __repr__(self):
        return "𝐮 ⋅ ∇ ϕ"


class CurvatureTerm(LevelSetTerm):
    """CurvatureTerm(b) — b κ|∇ϕ| (src/levelsetterms.jl:104-107)."""
    kind = L.TERM_CURVATURE

    def __init__(self, b):
        self.b = b

    def _bind(self, grid, backend, slab):
        self.coeff = _Coeff(self.b, 1, grid, backend, slab)

    def __repr__(self):
        return "b κ|∇ϕ|"


class NormalMotionTerm(LevelSetTerm):
    """NormalMotionTerm(v[, update_func]) — v|∇ϕ| (src/levelsetterms.jl:139-146)."""
    kind = L.TERM_NORMAL_MOTION

    def __init__(self, speed, update_func=None):
        self.speed, self.update_func = speed, update_func

    def _bind(self, grid, backend, slab):
        self.coeff = _Coeff(self.speed, 1, grid, backend, slab)

    def __repr__(self):
        return "v|∇ϕ|"


class EikonalReinitializationTerm(LevelSetTerm):
    """EikonalReinitializationTerm([ϕ₀]) — sign(ϕ)(|∇ϕ| - 1) (src/levelsetterms.jl:211-222).
    With ϕ₀ (host MeshField or device field) the smoothed sign S₀ = ϕ₀/√(ϕ₀²+Δx²) is frozen."""
    kind = L.TERM_EIKONAL

    def __init__(self, phi0=None):
        self.phi0 = phi0
        self.s0 = None

    def _bind(self, grid, backend, slab):
        if self.phi0 is None:
            return
        if isinstance(self.phi0, ROCMeshField):
            src = self.phi0.buf
        else:
            src = backend.alloc()
            v = self.phi0.vals if isinstance(self.phi0, MeshField) else np.asarray(self.phi0)
            backend.upload(src, v if slab is None else v[..., slab[0]:slab[0] + slab[1]])
        self.s0 = getattr(backend, "alloc_side", backend.alloc)()
        backend.eikonal_sign(src, self.s0)

    def __repr__(self):
        return "sign(ϕ) (|∇ϕ| - 1)" if self.phi0 is None else "sign(ϕ₀) (|∇ϕ| - 1)"


def _terms_c(terms):
    arr = (L.LsmTerm * max(1, len(terms)))()
    for i, t in enumerate(terms):
        arr[i].kind = t.kind
        arr[i].scheme = t.scheme.code if isinstance(t, AdvectionTerm) else 0
        if t.coeff is not None:
            C.memmove(C.byref(arr[i].coeff), C.byref(t.coeff.c), C.sizeof(L.LsmCoeff))
        if isinstance(t, EikonalReinitializationTerm) and t.s0 is not None:
            arr[i].s0 = t.s0.data_ptr()
    return arr


# ----------------------------------------------------------------------------- timestepping.jl

class TimeIntegrator:
    def __init__(self, cfl=0.5):
        self.cfl = float(cfl)

    def _show(self):
        """src/timestepping.jl:94-97."""
        return f"{self._describe}\n  └─ cfl: {_jl_float(self.cfl)}"

    __repr__ = _show


class ForwardEuler(TimeIntegrator):
    name, _describe = "fe", "ForwardEuler (1st order explicit)"


class RK2(TimeIntegrator):
    name, _describe = "rk2", "RK2 (2nd order TVD Runge-Kutta, Heun's method)"


class RK3(TimeIntegrator):
    name, _describe = "rk3", "RK3 (3rd order TVD Runge-Kutta)"


class SemiImplicitI2OE(TimeIntegrator):
    """SemiImplicitI2OE(cfl = 2.0) — the semi-implicit I2OE scheme for one AdvectionTerm (src/timestepping.jl:68-92,204-426).
    Every step solves the reference's global linear system on the device (lsm_advance_i2oe: matrix-free BiCGSTAB) instead of
    the reference's sparse direct solve.  Extra keywords of this implementation, not part of `show`: `rtol`, the tolerance on
    ‖r‖₂/‖rhs‖₂, and `max_iters`, the iterations a step may take before it fails with LsmNotConvergedError."""
    name, _describe = "i2oe", "SemiImplicitI2OE (semi-implicit advection, Mikula et al.)"

    def __init__(self, cfl=2.0, *, rtol=1e-13, max_iters=500):
        super().__init__(cfl)
        self.rtol, self.max_iters = float(rtol), int(max_iters)
        if not self.rtol > 0 or self.max_iters < 1:
            raise ValueError("SemiImplicitI2OE: rtol must be positive and max_iters at least 1")


class SemiLagrangian(TimeIntegrator):
    """SemiLagrangian(cfl = 4.0; order = 3, trace = 2, limiter = true) — large advection steps by backward characteristics for one
    AdvectionTerm on a dense field of a single device (not part of the reference).  Every node is traced back
    along the velocity for Δt (trace 1: one Euler step; 2: the midpoint rule) and ϕⁿ is read there by the tensor-product Lagrange
    interpolant of degree `order` (1, 3 or 5), clamped to the departure cell's extrema with `limiter`.  One gather pass per step
    (lsm_advance_semilag), stable at any cfl; the term's scheme is ignored.  `stats` (an extra of this implementation): read the
    step's counters into `ls.semilag_last` after every step — a record per workgroup, a reduction and a host wait; False leaves
    them out and `ls.semilag_last` None."""
    name, _describe = "semilag", "SemiLagrangian (backward characteristics, Lagrange interpolation)"

    def __init__(self, cfl=4.0, *, order=3, trace=2, limiter=True, stats=True):
        super().__init__(cfl)
        self.order, self.trace, self.limiter, self.stats = order, trace, bool(limiter), bool(stats)


def _jl_min(*xs):
    m = xs[0]
    for x in xs[1:]:
        m = float("nan") if (math.isnan(m) or math.isnan(x)) else (x if x < m else m)
    return m


def _eps(x):
    return float(np.spacing(abs(float(x))))


# ----------------------------------------------------------------------------- slab groups inside one process

class LocalGroup:
    """Every rank of a slab decomposition as a handle of THIS process (include/lsm.h: LSM_COMM_LOCAL; any devices):
    `g = LocalGroup(world)`, then `LevelSetEquation(..., comm=g.rank(r), device=...)` on one host thread per rank.
    Ghost planes move by peer copies inside the library; no torch.distributed, no RCCL."""

    def __init__(self, world):
        import threading
        self.world = int(world)
        self._barrier = threading.Barrier(self.world)
        self._slots = [None] * self.world
        self._backends = []

    def rank(self, r):
        if not 0 <= r < self.world:
            raise ValueError("rank out of range")
        return _LocalRank(self, int(r))

    def abort(self):
        """A rank has failed: nobody may keep waiting for it — neither at this object's barrier nor inside the library
        (lsm_comm_abort: the exchanges and the Δt all-reduce of the other ranks return LSM_ERR_COMM)."""
        self._barrier.abort()
        for b in self._backends:
            b.comm_abort()

    def exchange(self, r, v):
        """all_gather_object among the ranks' threads."""
        self._slots[r] = v
        self._barrier.wait()
        out = list(self._slots)
        self._barrier.wait()
        return out


class _LocalRank:
    def __init__(self, group, r):
        self.group, self.r = group, r


# ----------------------------------------------------------------------------- levelsetequation.jl

class LevelSetEquation:
    BAND_OVERLAP = 10   # least number of planes of each neighbour a slab of a band keeps: nearest-band-node radius 6 + slope 1 + stencil 3

    """LevelSetEquation(; terms, integrator = RK2(), ic, bc = nothing, t = 0) — src/levelsetequation.jl:59-78.

    Extra keywords of this implementation: mode ('fast' | 'strict' arithmetic), device, and
    `comm` (a torch.distributed process group, or a rank of an in-process LocalGroup: the grid is then split into
    slabs of the last dimension, one per rank, with the ghost-plane exchange inside the library — RCCL or peer copies)."""

    def __init__(self, *, terms, ic, integrator=None, bc=None, t=0, mode="fast", device=0, comm=None, backend_factory=None, tuning=None):
        if isinstance(terms, LevelSetTerm):
            terms = (terms,)
        if not (isinstance(terms, tuple) and all(isinstance(x, LevelSetTerm) for x in terms)):
            raise ValueError(f"terms must be a LevelSetTerm or a tuple of them, got {type(terms)}")
        if len(terms) == 0 or len(terms) > L.MAX_TERMS:
            raise ValueError(f"between 1 and {L.MAX_TERMS} terms are supported")
        self.terms = terms
        self.integrator = integrator or RK2()
        if bc is None:
            if not ic.has_boundary_conditions():
                raise ValueError("no boundary conditions: pass `bc` or build `ic` with one")
            bcs = ic.bcs
        else:
            bcs = _normalize_bc(bc, ic.mesh.ndim)
        self.mesh_ = ic.mesh
        self.bcs = bcs
        self.t = t
        self.comm = comm
        grid = ic.mesh
        N = grid.ndim
        # slab decomposition of the last dimension
        self.rank, self.world = 0, 1
        self.slab = None
        slab_faces = (False, False)
        if comm is not None:
            if isinstance(comm, _LocalRank):
                self.rank, self.world = comm.r, comm.group.world
            else:
                import torch.distributed as dist
                self.rank, self.world = dist.get_rank(comm), dist.get_world_size(comm)
            nl = grid.n[N - 1]
            base, rem = divmod(nl, self.world)
            counts = [base + (1 if r < rem else 0) for r in range(self.world)]
            lo = sum(counts[:self.rank])
            self.slab = (lo, counts[self.rank])
            self.counts = counts
            self.own = (0, counts[self.rank])      # local plane range of the planes this rank owns
            if self.world > 1 and min(counts) < L.GHOST + 1:
                # every rank raises the same error (a rank failing alone would leave the others in their next collective):
                # the periodic wrap sends planes shifted by one node, and a SymmetryBC end face reads LSM_GHOST planes inwards
                raise ValueError(f"a slab needs at least {L.GHOST + 1} planes: {nl} planes over {self.world} ranks leave {min(counts)}")
            if isinstance(ic, NarrowBandMeshField) and self.world > 1:
                # a band needs its neighbours' mask AND values up to 7 planes deep (nearest band node within 6, its
                # slope neighbour) plus the stencil reach: every rank keeps BAND_OVERLAP planes of its neighbours as
                # ordinary planes of its own (extended) slab, computes everything on them redundantly — results are
                # right at least BAND_OVERLAP planes away from the cut faces, i.e. on the owned planes — and refreshes
                # them from their owners after every stage and every band update.
                # reinitialize! measures physical distances: a band node lies up to (nlayers + 2)·max(h) from the interface,
                # and the ball it searches for nearer samples must stay clear of the cut faces (2 planes of wrong patches)
                hs = grid.meshsize()
                W = max(self.BAND_OVERLAP, int(math.ceil((ic.nlayers + 2) * max(hs) / hs[N - 1])) + 3)
                self.BAND_OVERLAP = W
                if min(counts) < W or ic.nlayers + 1 > W:
                    raise ValueError(f"a slab-decomposed band needs at least {W} planes per rank and nlayers < {W}")
                wlo = W if self.rank > 0 else 0
                whi = W if self.rank < self.world - 1 else 0
                self.own = (wlo, counts[self.rank])
                self.slab = (lo - wlo, counts[self.rank] + wlo + whi)
            periodic = bcs[N - 1][0].kind == L.BC_PERIODIC
            slab_faces = (self.rank > 0 or (periodic and self.world > 1), self.rank < self.world - 1 or (periodic and self.world > 1))
            self.periodic_last = periodic
        # storage type of the state = element type of `ic` (side arrays and all arithmetic stay float64)
        if isinstance(ic, ROCMeshField):
            self.dtype = ic.backend.dtype if hasattr(ic.backend, "dtype") else np.dtype(np.float64)
        elif isinstance(ic, LazyMeshField):
            self.dtype = ic.dtype
        else:
            self.dtype = np.dtype(ic.vals.dtype)
        factory = backend_factory
        if factory is None:
            from .backend import HipBackend
            factory = lambda g, b, s: HipBackend(g, b, slab=s, mode=mode, device=device, dtype=self.dtype, tuning=tuning)   # tuning: {"LSM_...": value} (include/lsm.h)
        elif self.dtype != np.float64:
            raise ValueError("float32 fields need the HIP backend")
        self.backend = factory(grid._c(), _bc_c(bcs, N, slab_faces), self.slab)
        # dense slabs on the HIP backend: the plane exchange and the Δt all-reduce run inside the library
        # (lsm_comm_attach_rccl / _local); torch.distributed only carries the RCCL unique id to the ranks
        self.lib_comm = False
        import os as _os
        band_slab = isinstance(ic, NarrowBandMeshField) and comm is not None and self.world > 1
        if (comm is not None and self.world > 1 and hasattr(self.backend, "comm_attach_rccl")
                and (band_slab or _os.environ.get("LSM_LIB_COMM", "1") != "0")):
            self._attach_library_comm()
        if band_slab:
            # the overlap planes of a band travel inside the library only (lsm_band_overlap_mask / _values)
            if not self.lib_comm:
                raise ValueError("a slab-decomposed NarrowBandMeshField needs the library's communicator (lsm_comm_attach_rccl / _local)")
            self.backend.band_overlap_config(self.BAND_OVERLAP)
        # copy `ic` so the equation owns its state (src/levelsetequation.jl:67-76)
        self.band = isinstance(ic, NarrowBandMeshField)
        if self.band:
            self.state = ROCNarrowBandMeshField(self.backend, grid, bcs, ic.nlayers)
            v = ic.vals
            self.backend.upload(self.state.buf, v if self.slab is None else v[..., self.slab[0]:self.slab[0] + self.slab[1]])
            self.state.rebuild(from_dense=True)   # NarrowBandMeshField(ϕ; nlayers): seed every node, then update_band!
            if self.comm is not None and self.world > 1:
                self._band_sync_after_update()
        else:
            self.state = ROCMeshField(self.backend, grid, bcs)
        if self.band:
            pass
        elif isinstance(ic, ROCMeshField):
            self.backend.copy_(self.state.buf, ic.buf)
        elif isinstance(ic, LazyMeshField):
            self.backend.upload(self.state.buf, ic.local_values(self.slab))
        else:
            v = ic.vals
            self.backend.upload(self.state.buf, v if self.slab is None else v[..., self.slab[0]:self.slab[0] + self.slab[1]])
        for term in terms:
            term._bind(grid, self.backend, self.slab)
        self._range_checked_at = 0
        self._check_range()
        self._bufs = None
        self._hook_keep = None
        import os as _os
        self.overlap = _os.environ.get("LSM_SLAB_OVERLAP", "1") != "0"   # boundary-first stages overlapping the halo exchange
        if any(t.update_func is not None for t in terms) and hasattr(self.backend, "cfl_cache"):
            self.backend.cfl_cache(False)   # hooks may mutate coefficients in place

    # accessors (src/levelsetequation.jl:124-162)
    def current_state(self):
        return self.state

    def current_time(self):
        return self.t

    def mesh(self):
        return self.mesh_

    def time_integrator(self):
        return self.integrator

    def _pde(self):
        return "ϕₜ + " + " + ".join(repr(t) for t in self.terms) + " = 0"

    def _show(self):
        """src/levelsetequation.jl:101-110 (text/plain)."""
        lines = ["LevelSetEquation", f"  ├─ equation: {self._pde()}", f"  ├─ time:     {_jl_float(self.t)}"]
        lines += _embed_show("integrator", show(self.integrator)) + _embed_show("state", show(self.state))
        return "\n".join(lines + ["  ╰─"])

    def __repr__(self):
        """src/levelsetequation.jl:113-117 (compact form)."""
        return f"LevelSetEquation({self._pde()}, t={_jl_float(self.t)})"

    def _check_range(self):
        """FAST arithmetic has a domain (include/lsm.h, LSM_MODE_FAST): refuse to run outside it instead of returning
        Inf/NaN silently.  Checked when the equation is built and every 64 steps (one reduction pass)."""
        if not hasattr(self.backend, "check_range"):
            return
        ok, m = self.backend.check_range(self.state.buf)
        if self.comm is not None and self.world > 1:
            # every rank raises or none does: a rank failing alone would leave the others in their next exchange
            parts = self._all_gather_object((ok, m))
            ok, m = all(p[0] for p in parts), max(p[1] for p in parts)
        if not ok:
            raise ValueError(f"max|ϕ| = {m:.3g} is outside the domain of the FAST arithmetic mode (differences between neighbouring nodes "
                             f"must stay below 1e35: max|ϕ| <= {L.FAST_MAX_ABS:g}); rescale the field or build the equation with mode=\"strict\"")

    # ---- update_term! (src/levelsetterms.jl:14,65-69,148-152) + slow-path coefficient sampling
    def _needs_hook(self):
        return any(t.update_func is not None or (t.coeff is not None and t.coeff.callable is not None) for t in self.terms)

    def _update_terms(self, field, t):
        for term in self.terms:
            if term.coeff is not None:
                term.coeff.refresh(t)
            if term.update_func is not None:
                term.update_func(term.coeff, field, t)

    # ---- compute_cfl (src/levelsetterms.jl:22-28)
    def compute_cfl(self, t=None):
        t = self.t if t is None else t
        arr = _terms_c(self.terms)
        if self.band:   # minimum over active_nodeindices (src/levelsetterms.jl:31-38)
            dt = self.backend.compute_cfl_band(arr, len(self.terms), self.state.buf, self.state.mask, t, self.state.tiles, self.state.MC)
        else:
            dt = self.backend.compute_cfl_local(arr, len(self.terms), self.state.buf, t)
        if self.comm is not None and self.world > 1:
            dt = self._allreduce_min(dt)
        if not dt > 0:
            raise ValueError(f"invalid time-step based on CFL condition: Δt = {dt} (check for NaN/Inf in velocity or speed)")
        return dt

    def _attach_library_comm(self):
        b = self.backend
        if isinstance(self.comm, _LocalRank):
            g = self.comm.group
            backs = g.exchange(self.rank, b)
            if self.rank == 0:
                type(b).comm_attach_local(backs)
                g._backends = list(backs)
            g.exchange(self.rank, None)            # nobody runs ahead of the attachment
        else:
            import torch.distributed as dist
            # a rank whose library cannot open RCCL (or whose communicator does not come up) must not leave the others
            # exchanging with nobody: the ranks agree, and the group as a whole falls back to the stage-by-stage exchange
            # over torch.distributed (same planes, same order, same results — DESIGN.md §6) with a warning
            err = None
            try:
                box = [b.comm_unique_id() if self.rank == 0 else None]
            except L.LsmError as e:
                box, err = [None], e
            dist.broadcast_object_list(box, src=dist.get_global_rank(self.comm, 0), group=self.comm)
            if box[0] is not None:
                try:
                    b.comm_attach_rccl(box[0], self.rank, self.world)
                except L.LsmError as e:
                    err = e
            else:
                err = err or L.LsmError("rank 0 could not create an RCCL unique id")
            oks = self._all_gather_object(err is None)
            if not all(oks):
                if err is None:
                    b.comm_detach()
                import warnings
                warnings.warn(f"libhiplsm's RCCL communicator is unavailable ({err or 'on another rank'}); "
                              "exchanging ghost planes through torch.distributed instead")
                return
        self.lib_comm = True

    def _all_gather_object(self, v):
        if isinstance(self.comm, _LocalRank):
            return self.comm.group.exchange(self.rank, v)
        import torch.distributed as dist
        parts = [None] * self.world
        dist.all_gather_object(parts, v, group=self.comm)
        return parts

    def _allreduce_min(self, dt):
        if self.lib_comm:
            return self.backend.allreduce_dt(dt)   # lsm_allreduce_dt: MIN over the ranks, NaN wins
        import torch
        import torch.distributed as dist
        dev = self.state.buf.device
        # on the current stream, behind the stages of the previous step: one collective in flight at a time per rank (the
        # local Δt may come early from the library's CFL stream, but overlapping this all-reduce with the plane exchange
        # of the previous step would run two communicators concurrently — not worth the 8 bytes)
        x = torch.tensor([-1.0 if math.isnan(dt) else dt], dtype=torch.float64, device=dev)   # NaN must win
        dist.all_reduce(x, op=dist.ReduceOp.MIN, group=self.comm)
        v = float(x.item())
        return float("nan") if v < 0 else v

    # ---- _advance! (src/timestepping.jl:126-202)
    def _advance(self, tc, dt):
        b = self.backend
        if self._bufs is None:
            self._bufs = (b.alloc(), b.alloc())   # cached across integrate! calls (the reference reallocates)
        b1, b2 = self._bufs
        arr = _terms_c(self.terms)
        n = len(self.terms)
        phi = self.state.buf
        name = self.integrator.name
        if self.band:
            return self._advance_band(tc, dt, b1, b2)
        if self.comm is None or self.lib_comm:
            if self.lib_comm and self.state.ghosts_dirty:   # a slab's lsm_advance_* expects valid ghosts on entry
                b.fill_ghosts(phi, 7)
                b.halo_exchange(phi)
                self.state.ghosts_dirty = False
            hook = None
            if self._needs_hook():
                def cb(_user, stage, field_ptr, t_stage):
                    try:
                        fld = self.state if stage == 0 else ROCMeshField(b, self.mesh_, self.bcs, b1 if stage == 1 else b2)
                        self._update_terms(fld, t_stage)
                        return 0
                    except Exception as e:   # surface python errors as an aborted step
                        self._hook_error = e
                        return 1
                hook = L.StageHook(cb)
                self._hook_keep = hook
            self._hook_error = None
            try:
                b.advance_single(name, arr, n, phi, b1, b2, tc, dt, hook)
            except L.LsmError:
                if self.lib_comm:
                    b.comm_abort()      # the other ranks get LSM_ERR_COMM instead of waiting for this one
                if self._hook_error is not None:
                    raise self._hook_error
                raise
            if not self.lib_comm:
                self.state.ghosts_dirty = True      # a whole-grid lsm_advance_* leaves ϕ's ghost layers stale (include/lsm.h)
            return
        # slab mode: stage by stage with ghost-plane exchange between stages
        fld = lambda buf: ROCMeshField(b, self.mesh_, self.bcs, buf)
        if self.state.ghosts_dirty:
            self._halo(phi)
            self.state.ghosts_dirty = False
        T = lambda: _terms_c(self.terms)
        if name == "fe":
            self._update_terms(self.state, tc)
            self._stage_slab(T(), n, phi, None, b1, None, L.BASE_PSI, dt, 0.0, tc)
            b.copy_(phi, b1)                       # copy!(ϕ, dst): ghosts travel with the padded buffer
        elif name == "rk2":
            self._update_terms(self.state, tc)
            self._stage_slab(T(), n, phi, None, b1, b2, L.BASE_PSI, dt, 0.5 * dt, tc)
            self._update_terms(fld(b1), tc + dt)
            self._stage_slab(T(), n, b1, b2, phi, None, L.BASE_OTHER, 0.5 * dt, 0.0, tc + dt)
        else:
            self._update_terms(self.state, tc)
            self._stage_slab(T(), n, phi, None, b1, None, L.BASE_PSI, dt, 0.0, tc)
            self._update_terms(fld(b1), tc + dt)
            self._stage_slab(T(), n, b1, phi, b2, None, L.BASE_RK3_S2, 0.25 * dt, 0.0, tc + dt)
            self._update_terms(fld(b2), tc + 0.5 * dt)
            self._stage_slab(T(), n, b2, phi, phi, None, L.BASE_RK3_S3, (2.0 / 3) * dt, 0.0, tc + 0.5 * dt)

    def _advance_band(self, tc, dt, b1, b2):
        """_advance! on a NarrowBandMeshField: lsm_advance_band_fe/rk2/rk3 (include/lsm.h) — the same stages, looping over
        active nodes only (src/timestepping.jl:128-202 with active_nodeindices = the band); every stage input is made
        readable first (band halo by affine extrapolation, then the boundary-condition ghosts) and, on a slab, the overlap
        planes of every stage result come from their owners."""
        b, st = self.backend, self.state
        if os.environ.get("LSM_BAND_PY") == "1":      # the stage-by-stage sequence through lsm_band_prepare / lsm_stage_band (tests)
            return self._advance_band_py(tc, dt, b1, b2)
        hook = None
        if self._needs_hook():
            def cb(_user, stage, field_ptr, t_stage):
                try:
                    fld = st if stage == 0 else ROCMeshField(b, self.mesh_, self.bcs, b1 if stage == 1 else b2)
                    self._update_terms(fld, t_stage)
                    return 0
                except Exception as e:   # surface python errors as an aborted step
                    self._hook_error = e
                    return 1
            hook = L.StageHook(cb)
            self._hook_keep = hook
        self._hook_error = None
        band_c = b.band_c(st.mask, st.tiles, st.MC, st._hlist, st._hcount)
        try:
            b.advance_band(self.integrator.name, _terms_c(self.terms), len(self.terms), band_c, st.buf, b1, b2, tc, dt, hook)
        except L.LsmError:
            if self.lib_comm:
                b.comm_abort()
            if self._hook_error is not None:
                raise self._hook_error
            raise
        st.ghosts_dirty = True

    def _advance_band_py(self, tc, dt, b1, b2):
        """The same step driven stage by stage from here (what lsm_advance_band_* does inside the library)."""
        b, st = self.backend, self.state
        n = len(self.terms)
        phi = st.buf
        name = self.integrator.name
        T = lambda: _terms_c(self.terms)
        sb = lambda psi, phin, out, out2, mode, c1, c2, t: b.stage_band(T(), n, psi, phin, out, out2, mode, c1, c2, t,
                                                                      st.mask, st.tiles, st.MC)
        fld = lambda buf: ROCMeshField(b, self.mesh_, self.bcs, buf)
        slabbed = self.comm is not None and self.world > 1
        sync = (lambda buf: b.band_overlap_values(buf)) if slabbed else (lambda buf: None)   # stencil inputs: owners' values
        st.prepare(phi)
        self._update_terms(st, tc)
        if name == "fe":
            b.copy_(b1, phi)                     # copy!(dst, ϕ): non-band entries keep ϕ's (scratch) values
            sb(phi, None, b1, None, L.BASE_PSI, dt, 0.0, tc)
            b.copy_(phi, b1)
        elif name == "rk2":
            sb(phi, None, b1, b2, L.BASE_PSI, dt, 0.5 * dt, tc)
            sync(b1)
            st.prepare(b1)
            self._update_terms(fld(b1), tc + dt)
            sb(b1, b2, phi, None, L.BASE_OTHER, 0.5 * dt, 0.0, tc + dt)
        else:
            sb(phi, None, b1, None, L.BASE_PSI, dt, 0.0, tc)
            sync(b1)
            st.prepare(b1)
            self._update_terms(fld(b1), tc + dt)
            sb(b1, phi, b2, None, L.BASE_RK3_S2, 0.25 * dt, 0.0, tc + dt)
            sync(b2)
            st.prepare(b2)
            self._update_terms(fld(b2), tc + 0.5 * dt)
            sb(b2, phi, phi, None, L.BASE_RK3_S3, (2.0 / 3) * dt, 0.0, tc + 0.5 * dt)
        sync(phi)
        st.ghosts_dirty = True

    def update_band(self):
        """update_band!(ϕ) after an accepted step (src/timestepping.jl:115): no-op on a dense field."""
        if self.band:
            self.state.rebuild(from_dense=False)
            if self.comm is not None and self.world > 1:
                self._band_sync_after_update()

    def _band_sync_after_update(self):
        """Slab of a band: the band set and the values of newly active nodes are only right away from the cut faces;
        take both from the owners on the overlap planes (lsm_band_overlap_mask: whole planes of mask bytes, after which
        only the band nodes' values travel), then re-derive tiles, lists and the halo from the full mask."""
        st, b = self.state, self.backend
        b.band_overlap_mask(st.mask)
        b.band_overlap_values(st.buf)
        b.band_retile(st.mask, st.tiles, st.MC)
        b.band_status(st._hcount)
        b.band_halo(st.buf, st.mask, st.halo, st.tiles, st.MC, st._hlist, st._hcount)
        st._check_halo()

    def _stage_slab(self, arr, n, psi, phin, out, out2, mode, cdt, cdt2, t):
        """One stage of a slab followed by its ghost resolution.  With overlap, the G+1 planes next to
        each slab interface are updated and ghost-filled first, their exchange is started, and the
        interior is updated while the planes travel over xGMI (the results are identical: every node is
        computed by the same kernel from the same inputs)."""
        b = self.backend
        N = self.mesh_.ndim
        nloc = int(b.lay.n[N - 1])
        B = L.GHOST + 1                      # +1: the periodic wrap sends planes shifted by one node
        if not (self.overlap and (self.world > 1 or getattr(self, "_force_overlap", False)) and N >= 2 and nloc >= 2 * B + 1
                and hasattr(b, "stage_planes")):
            b.stage(arr, n, psi, phin, out, out2, mode, cdt, cdt2, t)
            self._halo(out)
            return
        for m0, m1 in ((0, B), (nloc - B, nloc)):
            b.stage_planes(arr, n, psi, phin, out, out2, mode, cdt, cdt2, t, m0, m1)
            b.fill_ghosts_planes(out, m0, m1)
        reqs = self._exchange_start(out)
        b.stage_planes(arr, n, psi, phin, out, out2, mode, cdt, cdt2, t, B, nloc - B)
        b.fill_ghosts_planes(out, B, nloc - B)
        for w in reqs:
            w.wait()
        b.fill_ghosts(out, 1 << (N - 1))     # physical BC ghost planes of the end ranks (slab interfaces are skipped)

    def _halo(self, buf):
        """Ghost resolution for a slab: BC fill of every dimension (slab interfaces are skipped by
        the library), then exchange of LSM_GHOST full padded planes with the neighbouring ranks.
        Because the exchanged planes carry their own dim-1..N-1 ghosts, the corner composition of
        _getindexbc (src/meshfield.jl:248-260) is preserved."""
        self.backend.fill_ghosts(buf, 7)
        for w in self._exchange_start(buf):
            w.wait()

    def _exchange_start(self, buf):
        """Post the ghost-plane sends/receives of one field; returns the pending works."""
        import torch.distributed as dist
        if self.world == 1:
            return []
        b = self.backend
        N = self.mesh_.ndim
        G = L.GHOST
        sl = int(b.lay.stride[N - 1])          # elements per padded plane
        nloc = int(b.lay.n[N - 1])
        flat = b.flat(buf)
        plane = lambda k0, k1: flat[(k0 + G) * sl:(k1 + G) * sl]   # local plane range [k0, k1)
        up = self.rank + 1 if self.rank < self.world - 1 else (0 if self.periodic_last else None)
        dn = self.rank - 1 if self.rank > 0 else (self.world - 1 if self.periodic_last else None)
        # periodic wrap has period n-1 (nodes 1 and n coincide, src/boundaryconditions.jl:107-119):
        # across the wrap the sender skips its duplicate end node.
        wrap_up = self.rank == self.world - 1
        wrap_dn = self.rank == 0
        # op order [send up, recv dn, send dn, recv up]: messages between one pair of ranks match in
        # posting order (RCCL and gloo alike), which matters when up == dn (2 ranks, periodic ring).
        ops = []
        if up is not None:
            s0 = nloc - G - (1 if wrap_up else 0)
            ops.append(dist.P2POp(dist.isend, plane(s0, s0 + G), up, group=self.comm))
        if dn is not None:
            ops.append(dist.P2POp(dist.irecv, plane(-G, 0), dn, group=self.comm))
            s0 = 1 if wrap_dn else 0
            ops.append(dist.P2POp(dist.isend, plane(s0, s0 + G), dn, group=self.comm))
        if up is not None:
            ops.append(dist.P2POp(dist.irecv, plane(nloc, nloc + G), up, group=self.comm))
        return dist.batch_isend_irecv(ops) if ops else []

    def gather_state(self):
        """Full-grid host copy of the state on every rank (tests / diagnostics)."""
        v = self.state.values()
        if self.comm is None or self.world == 1:
            return v
        v = v[..., self.own[0]:self.own[0] + self.own[1]]       # a band slab also holds copies of its neighbours' planes
        N = self.mesh_.ndim
        return np.asfortranarray(np.concatenate(self._all_gather_object(v), axis=N - 1))


def integrate_(ls, tf, dt=float("inf"), prehook=None, posthook=None):
    """integrate!(ls, tf, Δt = Inf; prehook, posthook) — src/levelsetequation.jl:194-203 and the
    step loop _integrate! of src/timestepping.jl:101-122, on the host."""
    tc = ls.current_time()
    if not tf >= tc:
        raise ValueError(f"final time {tf} must be ≥ initial time {tc}: the level-set equation cannot be solved back in time")
    if isinstance(ls.integrator, SemiImplicitI2OE):
        return _integrate_i2oe(ls, tc, tf, dt, prehook, posthook)
    if isinstance(ls.integrator, SemiLagrangian):
        return _integrate_semilag(ls, tc, tf, dt, prehook, posthook)
    alpha = ls.integrator.cfl
    while tc <= tf - _eps(tc):
        if prehook is not None:
            prehook(ls)
        ls._update_terms(ls.state, tc)
        step = _jl_min(dt, alpha * ls.compute_cfl(tc), tf - tc)
        ls._advance(tc, step)
        tc += step
        ls.t = tc
        ls._range_checked_at += 1
        if ls._range_checked_at % 64 == 0:
            ls._check_range()
        ls.update_band()   # re-tube before the posthook (no-op on a full grid) — src/timestepping.jl:115
        if posthook is not None:
            posthook(ls)
    ls.t = tf
    return ls


def _bc_jl(bc):
    if isinstance(bc, SymmetryBC):
        return "SymmetryBC()"
    if isinstance(bc, PeriodicBC):
        return "PeriodicBC()"
    return f"ExtrapolationBC{{{bc.degree}}}()"


def _validate_i2oe(ls):
    """The reference's checks (src/timestepping.jl:204-205,236-244,366-369), made on the host before any step."""
    if ls.band:
        raise ValueError("SemiImplicitI2OE requires a full-grid MeshField, got ROCNarrowBandMeshField")
    if not (len(ls.terms) == 1 and isinstance(ls.terms[0], AdvectionTerm)):
        raise ValueError("SemiImplicitI2OE requires exactly one AdvectionTerm")
    if not all(n >= 3 for n in ls.mesh_.n):
        raise ValueError("SemiImplicitI2OE requires at least 3 grid nodes along each dimension")
    for sides in ls.bcs:
        for bc in sides:
            if not (isinstance(bc, PeriodicBC) or (isinstance(bc, ExtrapolationBC) and bc.degree <= 1)):
                raise ValueError(f"boundary condition {_bc_jl(bc)} is not supported by SemiImplicitI2OE")
    if ls.comm is not None and ls.world > 1:
        raise ValueError("SemiImplicitI2OE runs on a single device: a slab decomposition (comm) is not supported")


def _integrate_i2oe(ls, tc, tf, dt, prehook, posthook):
    """_integrate!(ls, ϕ::MeshField, ::SemiImplicitI2OE, ...) — src/timestepping.jl:207-233: one device solve per step
    (lsm_advance_i2oe); no update_band!.  The iterations and the relative residual of the last step are kept in
    ls.i2oe_last, the iterations of all steps in ls.i2oe_iters."""
    _validate_i2oe(ls)
    integ = ls.integrator
    ls.i2oe_iters = 0
    while tc <= tf - _eps(tc):
        if prehook is not None:
            prehook(ls)
        ls._update_terms(ls.state, tc)
        step = _jl_min(dt, integ.cfl * ls.compute_cfl(tc), tf - tc)
        ls.i2oe_last = ls.backend.advance_i2oe(_terms_c(ls.terms), ls.state.buf, tc, step, integ.rtol, integ.max_iters)
        ls.i2oe_iters += ls.i2oe_last[0]
        ls.state.ghosts_dirty = True
        tc += step
        ls.t = tc
        ls._range_checked_at += 1
        if ls._range_checked_at % 64 == 0:
            ls._check_range()
        if posthook is not None:
            posthook(ls)
    ls.t = tf
    return ls


def _validate_semilag(ls):
    """What SemiLagrangian can run, checked on the host before any step."""
    integ = ls.integrator
    if ls.band:
        raise ValueError("SemiLagrangian requires a full-grid MeshField, got ROCNarrowBandMeshField")
    if not (len(ls.terms) == 1 and isinstance(ls.terms[0], AdvectionTerm)):
        raise ValueError("SemiLagrangian requires exactly one AdvectionTerm")
    if ls.comm is not None and ls.world > 1:
        raise ValueError("SemiLagrangian runs on a single device: a slab decomposition (comm) is not supported")
    if isinstance(integ.order, bool) or integ.order not in (1, 3, 5):
        raise ValueError(f"SemiLagrangian: order must be 1, 3 or 5, got {integ.order!r}")
    if isinstance(integ.trace, bool) or integ.trace not in (1, 2):
        raise ValueError(f"SemiLagrangian: trace must be 1 or 2, got {integ.trace!r}")


def _integrate_semilag(ls, tc, tf, dt, prehook, posthook):
    """The step loop of _integrate_i2oe with one gather pass per step (lsm_advance_semilag); no update_band!.  The step is out of
    place: the new state is written to a stage buffer, which then changes places with the state's buffer (nothing on the handle
    keeps ϕ's pointer between calls: the Δt caches are keyed by the term alone, and a Renderer re-attaches to a changed buffer).
    The counters of the last step — (staged workgroups, fallback workgroups, largest displacement in cells) — are kept in
    ls.semilag_last: every step therefore ends in one small reduction and a host wait, unless the integrator was built with
    stats=False."""
    _validate_semilag(ls)
    integ = ls.integrator
    while tc <= tf - _eps(tc):
        if prehook is not None:
            prehook(ls)
        ls._update_terms(ls.state, tc)
        step = _jl_min(dt, integ.cfl * ls.compute_cfl(tc), tf - tc)
        if getattr(ls, "_semilag_buf", None) is None:
            ls._semilag_buf = ls.backend.alloc()   # the one stage buffer of this integrator, kept across integrate! calls
        out = ls._semilag_buf
        ls.semilag_last = ls.backend.advance_semilag(_terms_c(ls.terms), ls.state.buf, out, tc, step, integ.order, integ.trace, integ.limiter,
                                                     want_stats=integ.stats)
        ls.state.buf, ls._semilag_buf = out, ls.state.buf
        ls.state.ghosts_dirty = True
        tc += step
        ls.t = tc
        ls._range_checked_at += 1
        if ls._range_checked_at % 64 == 0:
            ls._check_range()
        if posthook is not None:
            posthook(ls)
    ls.t = tf
    return ls


def _sum_over_ranks(ls, x):
    if ls.comm is None or ls.world == 1:
        return x
    if isinstance(ls.comm, _LocalRank):
        return float(sum(ls._all_gather_object(float(x))))   # rank order: the same sum on every rank
    import torch
    import torch.distributed as dist
    t = torch.tensor([x], dtype=torch.float64, device=ls.state.buf.device)
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=ls.comm)
    return float(t.item())


def _band_single_device(ls, what):
    if ls.comm is not None and ls.world > 1:
        raise ValueError(f"{what} of a slab-decomposed NarrowBandMeshField is not built (the band-free grid lines are "
                         "classified by the nearest band node of the whole band)")


def volume(ls):
    """volume(eq) — measure of {ϕ ≤ 0} with the smoothed Heaviside (src/levelsetops.jl:27-33,
    src/levelsetequation.jl:165); the standard posthook diagnostic (docs/src/levelset-equation.md:142-149).
    NarrowBandMeshField states: from the band alone (src/levelsetops.jl:34-116)."""
    if getattr(ls, "band", False):
        _band_single_device(ls, "volume")
        return ls.backend.band_volume(ls.state.buf, ls.state.mask)
    return _sum_over_ranks(ls, ls.backend.volume_local(ls.state.buf))


def perimeter(ls):
    """perimeter(eq) — measure of {ϕ = 0} with the smoothed Dirac delta (src/levelsetops.jl:139-149); for a
    NarrowBandMeshField state the sum over the active nodes (:150-166)."""
    if getattr(ls, "band", False):
        _band_single_device(ls, "perimeter")
        ls.state.prepare(ls.state.buf)      # ϕ[I] off the band (extrapolation) and outside the grid (BCs) for the centred gradient
        return ls.backend.band_perimeter(ls.state.buf, ls.state.mask)
    if ls.comm is not None and ls.world > 1:
        # slab interfaces: the centred gradient needs the neighbours' planes
        if ls.lib_comm:                 # the library's own communicator (RCCL or peer copies), as in _advance
            ls.backend.fill_ghosts(ls.state.buf, 7)
            ls.backend.halo_exchange(ls.state.buf)
            ls.state.ghosts_dirty = False
        else:
            ls._halo(ls.state.buf)      # torch.distributed fallback
    return _sum_over_ranks(ls, ls.backend.perimeter_local(ls.state.buf))


def extend_along_normals_(F, phi, nb_iters=50, cfl=0.45, frozen=None, interface_band=1.5, min_norm=1.0e-14):
    """extend_along_normals!(F, ϕ; nb_iters, cfl, frozen, interface_band, min_norm) —
    src/velocityextension.jl:20-76.  `F` and `phi` are device fields (ROCMeshField) on the same mesh;
    `frozen` is None (band rule) or a boolean/0-1 host array or device field.  F is updated in place."""
    if not (isinstance(F, ROCMeshField) and isinstance(phi, ROCMeshField)):
        raise ValueError("F and ϕ must be device fields (ROCMeshField) of the same equation/backend")
    if F.mesh.n != phi.mesh.n:
        raise ValueError("F and ϕ must be defined on the same mesh")
    if nb_iters < 0:
        raise ValueError("nb_iters must be non-negative")
    if not cfl > 0:
        raise ValueError("cfl must be strictly positive")
    if not interface_band >= 0:
        raise ValueError("interface_band must be non-negative")
    if not min_norm >= 0:
        raise ValueError("min_norm must be non-negative")
    b = phi.backend
    fz = None
    if frozen is not None:
        if isinstance(frozen, (ROCMeshField, SideField)):
            fz = frozen.buf if str(frozen.buf.dtype) == "torch.float64" else frozen.buf.double()   # side arrays are float64
        else:
            a = np.asarray(frozen.vals if isinstance(frozen, MeshField) else frozen)
            if a.shape != phi.mesh.n:
                raise ValueError("frozen mask must have the same size as ϕ")
            fz = getattr(b, "alloc_side", b.alloc)()
            getattr(b, "upload_side", b.upload)(fz, a.astype(np.float64))
    b.extend_along_normals(F.buf, phi.buf, fz, int(nb_iters), float(cfl), float(interface_band), float(min_norm))
    F.ghosts_dirty = True
    return F


class SideField:
    """A float64 device array in the padded layout of a backend (coefficient fields, frozen masks, the outputs of
    curvature_field / gradient_field / normal_field)."""

    def __init__(self, backend, mesh, buf=None):
        self.backend, self.mesh = backend, mesh
        self.buf = backend.alloc_side() if buf is None else buf

    def values(self):
        return self.backend.download_side(self.buf)


def _geometry(phi, what, ncomp, scale, band, fill, out, frozen_out):
    if not isinstance(phi, ROCMeshField):
        raise ValueError("ϕ must be a device field (ROCMeshField)")
    b = phi.backend
    mask = None
    if isinstance(phi, ROCNarrowBandMeshField):     # the queries work on both field types (docs/src/geometry-queries.md)
        phi.prepare(phi.buf)                        # ϕ[I] off the band (extrapolation) and outside the grid (BCs)
        mask = phi.mask
    outs = out if out is not None else [SideField(b, phi.mesh) for _ in range(ncomp)]
    if len(outs) != ncomp:
        raise ValueError(f"expected {ncomp} output field(s)")
    b.geometry(what, phi.buf, [o.buf if isinstance(o, SideField) else o for o in outs], scale=scale,
               band_width=-1.0 if band is None else float(band), fill=fill,
               frozen_out=None if frozen_out is None else (frozen_out.buf if isinstance(frozen_out, SideField) else frozen_out), mask=mask)
    phi.ghosts_dirty = False
    return outs


def curvature_field(phi, scale=1.0, band=None, fill=0.0, out=None, frozen_out=None):
    """scale·curvature(ϕ, I) (src/levelsetops.jl:197-205) at every node, on the device.  `band`: only nodes with
    |ϕ[I]| <= band are evaluated (the others get `fill`) and `frozen_out` (a SideField) marks them with 1.0 — the
    seed-and-freeze loop of the reference's speed update functions (test/test-velocityextension.jl:118-131)."""
    return _geometry(phi, L.GEOM_CURVATURE, 1, scale, band, fill, None if out is None else [out], frozen_out)[0]


def gradient_field(phi, scale=1.0):
    """gradient(ϕ, I) (src/levelsetops.jl:212-215) at every node: one SideField per dimension."""
    return _geometry(phi, L.GEOM_GRADIENT, phi.mesh.ndim, scale, None, 0.0, None, None)


def normal_field(phi, scale=1.0):
    """normal(ϕ, I) = ∇ϕ/‖∇ϕ‖ (src/levelsetops.jl:222-226) at every node: one SideField per dimension."""
    return _geometry(phi, L.GEOM_NORMAL, phi.mesh.ndim, scale, None, 0.0, None, None)


def curvature(phi, I):
    """curvature(ϕ, I) — scalar convenience (slow: evaluates the field); 0-based I."""
    return float(curvature_field(phi).values()[tuple(I)])


def gradient(phi, I):
    return np.array([float(g.values()[tuple(I)]) for g in gradient_field(phi)])


def normal(phi, I):
    return np.array([float(g.values()[tuple(I)]) for g in normal_field(phi)])


class InterpolatedField:
    """InterpolatedField(ϕ, order) (src/interpolation.jl:117-151): the piecewise polynomial interpolant of a device field
    (dense, or a narrow band near its active nodes), evaluated on the device.  `itp(x)` for one point or an (npts, ndim) array; `gradient`, `hessian`,
    `value_and_gradient`, `value_gradient_hessian` as in the reference (:228-260)."""

    def __init__(self, phi, order=3):
        if not isinstance(phi, ROCMeshField):
            raise ValueError("InterpolatedField wraps a device field (ROCMeshField / ROCNarrowBandMeshField)")
        if not 1 <= int(order) <= 5:
            raise ValueError("interpolation order must be in 1..5")
        self.phi, self.order = phi, int(order)

    def _eval(self, x, grad, hess):
        x = np.asarray(x, dtype=np.float64)
        single = x.ndim == 1
        pts = x[None, :] if single else x
        if pts.ndim != 2 or pts.shape[1] != self.phi.mesh.ndim:
            raise ValueError(f"points must have {self.phi.mesh.ndim} coordinates")
        if isinstance(self.phi, ROCNarrowBandMeshField):
            # a band field interpolates wherever the patch's stencil stays on band or halo nodes (test/test-narrow-band.jl:91-103):
            # the halo holds the extrapolated values, exactly what the reference's nb[I] returns there
            self.phi.prepare(self.phi.buf)
        v, g, H = self.phi.backend.interpolate(self.phi.buf, self.order, pts, grad, hess)
        self.phi.ghosts_dirty = False
        if single:
            return float(v[0]), (g[0] if grad else None), (H[0] if hess else None)
        return v, g, H

    def __call__(self, x):
        return self._eval(x, False, False)[0]

    def gradient(self, x):
        return self._eval(x, True, False)[1]

    def hessian(self, x):
        return self._eval(x, False, True)[2]

    def value_and_gradient(self, x):
        return self._eval(x, True, False)[:2]

    def value_gradient_hessian(self, x):
        return self._eval(x, True, True)


class NewtonSDF:
    """NewtonSDF(ϕ; order = 3, upsample = 2, maxiters = 10, xtol, ftol) (src/sdf.jl:57-78) on the device: samples the
    interface of a private copy of ϕ once; `sdf(x)` is the signed distance at a point or an (npts, ndim) array of
    points (src/sdf.jl:80-84); `get_sample_points()`; `closest_point(x)`.  ϕ: a dense or narrow-band device field."""

    def __init__(self, phi, order=3, upsample=2, maxiters=10, xtol=None, ftol=None):
        if not isinstance(phi, ROCMeshField):
            raise ValueError("NewtonSDF takes a device field (ROCMeshField / ROCNarrowBandMeshField)")
        eps = float(np.sqrt(np.finfo(np.float64).eps))
        b = phi.backend
        mask = None
        if isinstance(phi, ROCNarrowBandMeshField):
            phi.prepare(phi.buf)
            mask = phi.mask
        else:
            b.fill_ghosts(phi.buf)
            phi.ghosts_dirty = False
        self.backend, self.ndim = b, phi.mesh.ndim
        self._h, self.nsamples = b.sdf_create(phi.buf, mask, order, upsample, maxiters, eps if xtol is None else xtol, eps if ftol is None else ftol)

    def _eval(self, x, want_cp):
        x = np.asarray(x, dtype=np.float64)
        single = x.ndim == 1
        pts = x[None, :] if single else x
        if pts.ndim != 2 or pts.shape[1] != self.ndim:
            raise ValueError(f"points must have {self.ndim} coordinates")
        d, cp, nfail = self.backend.sdf_eval(self._h, pts, want_cp)
        if single:
            return float(d[0]), (cp[0] if want_cp else None), nfail
        return d, cp, nfail

    def __call__(self, x):
        return self._eval(x, False)[0]

    def closest_point(self, x):
        """(closest point(s), number of non-converged solves) — _closest_point_on_interface, src/sdf.jl:113-127"""
        _, cp, nfail = self._eval(x, True)
        return cp, nfail

    def get_sample_points(self):
        return self.backend.sdf_samples(self._h, self.nsamples)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            try:
                self.backend.sdf_destroy(h)
            except Exception:
                pass


def hausdorff_distance(sdf1, sdf2):
    """hausdorff_distance(sdf₁, sdf₂) (src/sdf.jl:129-150): the larger of the two one-sided maxima over the sample points of
    one interface of the distance to the other."""
    def one_sided(a, b):
        pts = a.get_sample_points()
        cp, _ = b.closest_point(pts)
        return float(np.sqrt(((pts - cp) ** 2).sum(axis=1)).max())
    return max(one_sided(sdf1, sdf2), one_sided(sdf2, sdf1))


def reinitialize_(phi, order=3, upsample=2, maxiters=20, xtol=None, ftol=None):
    """reinitialize!(ϕ; order = 3, upsample = 2, maxiters = 20, xtol = nothing, ftol = nothing)
    (src/reinitializer.jl:12-42): overwrite every active node of ϕ with its signed distance to the interface,
    by the Newton closest-point method on the piecewise-polynomial interpolant of ϕ (NewtonSDF, src/sdf.jl).
    `phi` is a device field (or an equation: its current state).  Returns ϕ; warns, like the reference, when
    the closest-point solver did not converge at some nodes."""
    import warnings
    eq = phi if isinstance(phi, LevelSetEquation) else None
    if eq is not None:
        phi = eq.current_state()
    if not isinstance(phi, ROCMeshField):
        raise TypeError("reinitialize_ expects a device field (ROCMeshField / ROCNarrowBandMeshField) or a LevelSetEquation")
    if phi.bcs is None:
        raise ValueError("the field needs boundary conditions: the interpolation stencils reach outside the grid")
    b = phi.backend
    eps = float(np.finfo(getattr(b, "dtype", np.dtype(np.float64))).eps)
    xtol = math.sqrt(eps) if xtol is None else float(xtol)      # sqrt(eps(T)), T = float(valtype(ϕ)) — src/sdf.jl:66-67
    ftol = math.sqrt(eps) if ftol is None else float(ftol)
    band = isinstance(phi, ROCNarrowBandMeshField)
    if band:
        phi.prepare(phi.buf)              # stencil nodes off the band: the affine extrapolant, then the BC ghosts
    else:
        b.fill_ghosts(phi.buf, 7)
    ncand, nfail, nfar = b.reinitialize(phi.buf, phi.mask if band else None, order, upsample, maxiters, xtol, ftol)
    phi.ghosts_dirty = True
    if eq is not None and eq.comm is not None and eq.world > 1:
        if not band:
            raise ValueError("reinitialize! of a slab-decomposed dense field is not supported")
        eq.backend.band_overlap_values(phi.buf)     # the neighbours' planes: their owners' values
        nfail = nfar = 0                 # counted on the extended slab, cut faces included: not meaningful per rank
    if nfar:
        warnings.warn(f"reinitialize!: no interface sample was found ({nfar} nodes left unchanged)")
    if nfail:
        n_active = phi.active_count() if band else int(np.prod(phi.mesh.n))
        warnings.warn(f"reinitialize!: closest-point solver did not converge for {nfail} / {n_active} points")
    return phi


def current_state(ls):
    return ls.current_state()


def current_time(ls):
    return ls.current_time()


# ----------------------------------------------------------------------------- quadrature (ext/ImplicitIntegrationExt.jl)

_BAND_VOLUME_MSG = ("volume integrals (surface=false) are not supported on NarrowBandMeshField. "
                    "Use a full MeshField for volume integrals, or pass surface=true for surface integrals.")


class Quadrature:
    """ImplicitIntegration.Quadrature: nodes `coords` (m, N) and `weights` (m,)."""

    def __init__(self, coords, weights):
        self.coords, self.weights = coords, weights

    def __len__(self):
        return len(self.weights)

    def __repr__(self):
        return f"Quadrature with {len(self)} nodes in ℝ{_superscript(self.coords.shape[1])}"


class CellQuadratures:
    """quadrature(…)'s result: a mapping from 0-based cell tuples to their `Quadrature`, as the reference's `Dict`.  Cut cells
    in bulk: `cells` (ncut, N), `offsets` (ncut + 1; the nodes of cut cell i are offsets[i]:offsets[i+1]), `coords`, `weights`.
    Full cells (volume: every coefficient < 0): `full_cells` (nfull, N) and `rule`, the tensor rule on the unit cell; their
    nodes are made on request.  `total()`: the sum of every weight, on the device; `nfallback`: boxes that reached the
    subdivision limit and got the low-order rule."""

    def __init__(self, backend, mesh, handle, counts, q, surface):
        self.mesh, self.quadrature_order, self.surface = mesh, int(q), bool(surface)
        self._backend, self._h = backend, handle
        self.ncut, self.nnodes, self.nfull, self.nfallback = counts
        cells, offsets, coords, weights, full, rx, rw = backend.quad_read(handle, counts, q)
        self._dims = np.array([k - 1 for k in mesh.n], dtype=np.int64)
        self._cut_lin, self._full_lin = cells.cpu().numpy(), full.cpu().numpy()
        self.offsets = offsets.cpu().numpy()
        self.coords, self.weights = coords.cpu().numpy(), weights.cpu().numpy()
        self.rule = Quadrature(rx.cpu().numpy(), rw.cpu().numpy())
        self.cells, self.full_cells = self._unlin(self._cut_lin), self._unlin(self._full_lin)
        self._h_vec = np.array(mesh.meshsize(), dtype=np.float64)
        self._lc = np.array(mesh.lc, dtype=np.float64)

    def _unlin(self, lin):
        out, r = np.empty((len(lin), len(self._dims)), dtype=np.int64), np.asarray(lin, dtype=np.int64)
        for d, k in enumerate(self._dims):
            out[:, d] = r % k
            r = r // k
        return out

    def _lin(self, I):
        I = (I,) if isinstance(I, (int, np.integer)) else tuple(I)
        if len(I) != len(self._dims) or not all(0 <= int(I[d]) < self._dims[d] for d in range(len(I))):
            raise KeyError(I)
        lin, s = 0, 1
        for d, k in enumerate(self._dims):
            lin += int(I[d]) * s
            s *= int(k)
        return lin

    def _full_nodes(self, cells):
        """nodes and weights of full cells (rows of `full_cells`): the unit rule mapped to each cell"""
        lo = self._lc + cells.astype(np.float64) * self._h_vec                    # (c, N)
        x = lo[:, None, :] + self.rule.coords[None, :, :] * self._h_vec         # (c, m, N)
        w = np.broadcast_to(self.rule.weights * float(np.prod(self._h_vec)), x.shape[:2])
        return x.reshape(-1, x.shape[-1]), w.reshape(-1)

    def __getitem__(self, I):
        lin = self._lin(I)
        i = int(np.searchsorted(self._cut_lin, lin))
        if i < self.ncut and self._cut_lin[i] == lin:
            a, b = int(self.offsets[i]), int(self.offsets[i + 1])
            return Quadrature(self.coords[a:b], self.weights[a:b])
        j = int(np.searchsorted(self._full_lin, lin))
        if j < self.nfull and self._full_lin[j] == lin:
            return Quadrature(*self._full_nodes(self.full_cells[j:j + 1]))
        raise KeyError(I)

    def __contains__(self, I):
        try:
            self[I]
        except KeyError:
            return False
        return True

    def __len__(self):
        return self.ncut + self.nfull

    def keys(self):
        lin = np.concatenate([self._cut_lin, self._full_lin])
        return [tuple(int(v) for v in I) for I in self._unlin(np.sort(lin))]

    def __iter__(self):
        return iter(self.keys())

    def values(self):
        return [self[I] for I in self.keys()]

    def items(self):
        return [(I, self[I]) for I in self.keys()]

    def total(self):
        """Σ of every weight, full cells included (computed on the device)"""
        return self._backend.quad_total(self._h)

    def __repr__(self):
        return (f"CellQuadratures: {self.ncut} cut cells ({self.nnodes} nodes), {self.nfull} full cells, "
                f"quadrature_order = {self.quadrature_order}, surface = {str(self.surface).lower()}")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            try:
                self._backend.quad_destroy(h)
            except Exception:
                pass


def quadrature(phi, *, interpolation_order=None, quadrature_order, surface=False):
    """quadrature(ϕ; interpolation_order, quadrature_order, surface = false) / quadrature(itp::InterpolatedField; quadrature_order,
    surface = false) (src/LevelSetMethods.jl:103-126, ext/ImplicitIntegrationExt.jl): nodes and weights integrating over ϕ < 0, or
    over ϕ = 0 with surface = True, of the piecewise interpolant of degree interpolation_order, quadrature_order Gauss–Legendre
    points per direction, computed on the device.  ϕ: a device field (dense or narrow band: surface only) or an
    InterpolatedField.  Returns a CellQuadratures; warns when some boxes got the low-order fallback."""
    import warnings
    if isinstance(phi, InterpolatedField):
        if interpolation_order is not None:
            raise TypeError("quadrature(::InterpolatedField) takes no keyword interpolation_order: the field fixes it")
        field, order = phi.phi, phi.order
    elif isinstance(phi, ROCMeshField):
        if interpolation_order is None:
            raise TypeError("quadrature(ϕ) needs the keyword interpolation_order (or pass an InterpolatedField)")
        field, order = phi, interpolation_order
    else:
        raise TypeError("quadrature takes a device field (ROCMeshField / ROCNarrowBandMeshField) or an InterpolatedField")
    band = isinstance(field, ROCNarrowBandMeshField)
    if band and not surface:
        raise ValueError(_BAND_VOLUME_MSG)
    if int(order) != order or not 1 <= int(order) <= 5:
        raise ValueError("interpolation_order must be in 1..5")
    if int(quadrature_order) != quadrature_order or not 1 <= int(quadrature_order) <= 20:
        raise ValueError("quadrature_order must be in 1..20")
    b = field.backend
    if getattr(b, "slab", None) is not None:
        raise ValueError("quadrature of a slab-decomposed field (a field with a comm) is not supported")
    if field.bcs is None:
        raise ValueError("the field needs boundary conditions: the interpolation stencils reach outside the grid")
    mask = None
    if band:
        field.prepare(field.buf)
        mask = field.mask
    h, counts = b.quad_create(field.buf, mask, int(order), int(quadrature_order), surface)
    field.ghosts_dirty = False
    q = CellQuadratures(b, field.mesh, h, counts, int(quadrature_order), surface)
    if q.nfallback:
        warnings.warn(f"quadrature: {q.nfallback} boxes reached the subdivision limit and got the low-order rule")
    return q


def integrate(f, q, chunk=1 << 16):
    """Σ f(x)·w over the nodes of one Quadrature, or of every cell of a CellQuadratures (full cells `chunk` at a time).
    f maps an (m, N) array of points to (m,) values."""
    if isinstance(q, Quadrature):
        return float(np.dot(np.asarray(f(q.coords), dtype=np.float64), q.weights)) if len(q) else 0.0
    if not isinstance(q, CellQuadratures):
        raise TypeError("integrate(f, q): q is a Quadrature or a CellQuadratures")
    s = float(np.dot(np.asarray(f(q.coords), dtype=np.float64), q.weights)) if q.nnodes else 0.0
    for a in range(0, q.nfull, chunk):
        x, w = q._full_nodes(q.full_cells[a:a + chunk])
        s += float(np.dot(np.asarray(f(x), dtype=np.float64), w))
    return s


# ----------------------------------------------------------------------------- interface meshes (ext/MMGSurfaceExt.jl, ext/MakieExt.jl)

_REMESH_MSG = ("export_surface_mesh(…; {name}): the mmgs remeshing pass (mmgs_O3 of ext/MMGSurfaceExt.jl) is not part of this library; "
               "the file written without these keywords is its input")


class InterfaceMesh:
    """isosurface(…)'s result: the interface {ϕ = level} as an indexed mesh.  `vertices` (nv, N) float64, `elements` (ne, N)
    int64, 0-based: segments in 2-D, triangles in 3-D, oriented so that a triangle's (v1 − v0) × (v2 − v0), a segment's
    (Δy, −Δx), points from ϕ < level to ϕ >= level.  `mesh`: the grid; `level`; len() = ne."""

    def __init__(self, vertices, elements, mesh=None, level=0.0):
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float64)
        self.elements = np.ascontiguousarray(elements, dtype=np.int64)
        self.mesh, self.level = mesh, float(level)

    @property
    def ndim(self):
        return int(self.vertices.shape[1])

    def __len__(self):
        return int(self.elements.shape[0])

    def measure(self):
        """total length (2-D) or area (3-D) of the elements, computed on the host"""
        if not len(self):
            return 0.0
        p = self.vertices[self.elements]
        if self.ndim == 2:
            return float(np.hypot(*(p[:, 1] - p[:, 0]).T).sum())
        return float(0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1).sum())

    def __repr__(self):
        kind = "segments" if self.ndim == 2 else "triangles"
        return f"InterfaceMesh in ℝ{_superscript(self.ndim)}: {len(self.vertices)} vertices, {len(self)} {kind}, level = {_jl_float(self.level)}"


def isosurface(phi, level=0.0):
    """The interface {ϕ = level} of a device field as an indexed mesh, extracted on the device: marching
    simplices on the Freudenthal subdivision of every cell — watertight, consistently oriented, shared vertices.  What
    export_surface_mesh gets from marching cubes (ext/MMGSurfaceExt.jl:48-50) and ext/MakieExt.jl draws.  ϕ: a ROCMeshField, a
    ROCNarrowBandMeshField (the cells whose corners are all band nodes) or a LevelSetEquation (its current_state()).  Only the
    interior is read.  Returns an InterfaceMesh."""
    if isinstance(phi, LevelSetEquation):
        phi = phi.current_state()
    if not isinstance(phi, ROCMeshField):
        raise TypeError("isosurface takes a device field (ROCMeshField / ROCNarrowBandMeshField) or a LevelSetEquation, "
                        f"not {type(phi).__name__}")
    N = phi.mesh.ndim
    if N == 1:
        raise ValueError("isosurface of a 1 dimensional level-set is not supported: 2-D and 3-D fields only")
    b = phi.backend
    if getattr(b, "slab", None) is not None:
        raise ValueError("isosurface of a slab-decomposed field (a field with a comm) is not supported")
    level = float(level)
    if not math.isfinite(level):
        raise ValueError("isosurface: level must be finite")
    mask = phi.mask if isinstance(phi, ROCNarrowBandMeshField) else None
    h, counts = b.iso_create(phi.buf, mask, level)
    try:
        verts, elems = b.iso_read(h, counts)
        return InterfaceMesh(verts.cpu().numpy(), elems.cpu().numpy(), phi.mesh, level)
    finally:
        b.iso_destroy(h)


def _write_3D_triangular_mesh(path, vertices, triangles):
    """ext/MMGSurfaceExt.jl:82-102: a Medit .mesh file of 0-based triangles (written 1-based), every reference 1"""
    with open(path, "w") as f:
        f.write("MeshVersionFormatted 1\nDimension 3\n\nVertices\n")
        f.write(f"{len(vertices)}\n")
        f.writelines(f"{_jl_float(x)} {_jl_float(y)} {_jl_float(z)} 1\n" for x, y, z in np.asarray(vertices, dtype=np.float64).tolist())
        f.write("\nTriangles\n")
        f.write(f"{len(triangles)}\n")
        f.writelines(f"{i + 1} {j + 1} {k + 1} 1\n" for i, j, k in np.asarray(triangles, dtype=np.int64).tolist())
        f.write("\nEnd\n")


def export_surface_mesh(phi_or_eq, output, level=0.0, hgrad=None, hmin=None, hmax=None, hausd=None):
    """export_surface_mesh(ϕ, output; hgrad, hmin, hmax, hausd) (ext/MMGSurfaceExt.jl:35-80) up to the remesher: the zero
    contour of a 3-D field (a device field or a LevelSetEquation; beyond the reference, also an InterfaceMesh already extracted,
    which makes the writer usable without a device) written as the Medit
    .mesh file the reference hands to mmgs.  The remeshing keywords raise NotImplementedError.  Returns `output`."""
    if isinstance(phi_or_eq, LevelSetEquation):
        phi_or_eq = phi_or_eq.current_state()
    N = phi_or_eq.ndim if isinstance(phi_or_eq, InterfaceMesh) else getattr(getattr(phi_or_eq, "mesh", None), "ndim", None)
    if N is not None and N != 3:
        raise ValueError(f"export_mesh of {N} dimensional level-set not supported.")
    for name, value in (("hgrad", hgrad), ("hmin", hmin), ("hmax", hmax), ("hausd", hausd)):
        if value is not None:
            raise NotImplementedError(_REMESH_MSG.format(name=name))
    m = phi_or_eq if isinstance(phi_or_eq, InterfaceMesh) else isosurface(phi_or_eq, level)
    _write_3D_triangular_mesh(output, m.vertices, m.elements)
    return output


# ----------------------------------------------------------------------------- from a mesh back to a level set

def read_mesh(path):
    """The interface mesh of a Medit .mesh file, as an InterfaceMesh: the subset of the format this library writes
    (export_surface_mesh, export_volume_mesh) — `Dimension`, `Vertices`, then `Triangles` (3-D) or `Edges` (2-D); numbers are
    1-based in the file, references are ignored, other sections (the `Triangles` / `Tetrahedra` of a volume file) are skipped.
    Runs on the host: no device is needed."""
    with open(path) as f:
        tok = f.read().split()
    rows = {"Vertices": None, "Edges": 3, "Triangles": 4, "Quadrilaterals": 5, "Tetrahedra": 5, "Hexahedra": 9, "Corners": 1,
            "RequiredVertices": 1, "Ridges": 1, "RequiredEdges": 1}
    N, verts, found, i = None, None, {}, 0
    while i < len(tok):
        key = tok[i]
        i += 1
        if key == "End":
            break
        if key == "MeshVersionFormatted":
            i += 1
        elif key == "Dimension":
            N = int(tok[i])
            i += 1
            if N not in (2, 3):
                raise ValueError(f"read_mesh: Dimension {N} is not supported: 2-D and 3-D meshes only")
        elif key in rows:
            if N is None:
                raise ValueError(f"read_mesh: {key} before Dimension")
            count, width = int(tok[i]), rows[key] or N + 1
            i += 1
            body = tok[i:i + count * width]
            if len(body) != count * width:
                raise ValueError(f"read_mesh: the {key} section ends early")
            i += count * width
            if key == "Vertices":
                verts = np.array([float(x) for x in body], dtype=np.float64).reshape(count, width)[:, :N]
            else:
                found[key] = np.array([int(x) for x in body], dtype=np.int64).reshape(count, width)[:, :width - 1]
        else:
            raise ValueError(f"read_mesh: unexpected keyword {key!r}")
    if N is None:
        raise ValueError("read_mesh: no Dimension")
    if verts is None:
        raise ValueError("read_mesh: no Vertices section")
    kind = "Triangles" if N == 3 else "Edges"
    elems = found.get(kind, np.zeros((0, N), dtype=np.int64)) - 1
    if elems.size and (elems.min() < 0 or elems.max() >= len(verts)):
        raise ValueError(f"read_mesh: a vertex number of the {kind} section lies outside 1..{len(verts)}")
    return InterfaceMesh(verts, elems)


def _mesh_arrays(mesh, what):
    """(vertices (nv, N) float64, elements (ne, N) int64) of an InterfaceMesh or a (vertices, elements) pair"""
    if isinstance(mesh, InterfaceMesh):
        v, e = mesh.vertices, mesh.elements
    else:
        try:
            v, e = mesh
        except (TypeError, ValueError):
            raise TypeError(f"{what}: mesh must be an InterfaceMesh or a (vertices, elements) pair, not {type(mesh).__name__}") from None
        v, e = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(e, dtype=np.int64)
    if v.ndim != 2 or e.ndim != 2 or v.shape[1] not in (2, 3) or e.shape[1] != v.shape[1]:
        raise ValueError(f"{what}: vertices (nv, N) and elements (ne, N) with N = 2 (segments) or 3 (triangles) are expected, "
                         f"got shapes {v.shape} and {e.shape}")
    return v, e


def mesh_distance_(phi, mesh, cutoff=None):
    """Overwrite a device field with the signed distance to a closed, consistently oriented mesh, computed on the device
    (DESIGN.md §7.14): ϕ[I] = s·min(d, cutoff), d the exact Euclidean distance from node I to the nearest element (segments in
    2-D, triangles in 3-D), s = −1 where the mesh winds around the node and +1 elsewhere — the inverse of isosurface.  `phi`: a
    dense ROCMeshField or a LevelSetEquation (its current state), changed in place; `mesh`: an InterfaceMesh or a (vertices,
    elements) pair, oriented as InterfaceMesh documents (normals pointing out of the region that becomes ϕ < 0); cutoff = None
    means +inf.  Raises ValueError when the mesh is open or inconsistently oriented as seen from some grid line.  Returns ϕ."""
    eq = phi if isinstance(phi, LevelSetEquation) else None
    if eq is not None:
        phi = eq.current_state()
    if not isinstance(phi, ROCMeshField):
        raise TypeError(f"mesh_distance_ takes a device field (ROCMeshField) or a LevelSetEquation, not {type(phi).__name__}")
    if isinstance(phi, ROCNarrowBandMeshField):
        raise ValueError("mesh_distance_ is not supported on NarrowBandMeshField: the band is where the interface was, not where the "
                         "mesh is. Use a full MeshField, then build the band from it.")
    N = phi.mesh.ndim
    if N == 1:
        raise ValueError("mesh_distance_ of a 1 dimensional level-set is not supported: 2-D and 3-D fields only")
    b = phi.backend
    if getattr(b, "slab", None) is not None:
        raise ValueError("mesh_distance_ of a slab-decomposed field (a field with a comm) is not supported")
    v, e = _mesh_arrays(mesh, "mesh_distance_")
    if v.shape[1] != N:
        raise ValueError(f"mesh_distance_: a mesh in {v.shape[1]} dimensions cannot be measured on a {N} dimensional grid")
    c = float("inf") if cutoff is None else float(cutoff)
    if not c > 0:
        raise ValueError("mesh_distance_: cutoff must be positive (None or inf: no cutoff)")
    _, unbalanced, _ = b.mesh_distance(phi.buf, v, e, c)
    phi.ghosts_dirty = True
    if unbalanced:
        raise ValueError(f"mesh_distance: the mesh is not closed or not consistently oriented ({unbalanced} grid rows see unbalanced crossings)")
    return phi


def mesh_distance(mesh, grid, cutoff=None, dtype=None, mode="fast", device=0, far=None):
    """The signed distance to a closed mesh on `grid` as a host MeshField, usable as `ic=`: mesh_distance_ on a throwaway device
    field.  `mesh`: an InterfaceMesh (read_mesh's, isosurface's) or a (vertices, elements) pair; dtype: float64 (default) or
    float32 storage (the distance is computed in fp64 and rounded once).  far=None: nodes beyond the cutoff carry ±cutoff;
    far="eikonal": they are filled in by eikonal_ from the nodes within the cutoff minus one cell diagonal, which hold exact
    distances (exact near the mesh, first-order far from it, at the cost of a narrow exact pass).  Without a finite cutoff every
    node already holds its exact distance and `far` changes nothing."""
    if far not in (None, "eikonal"):
        raise ValueError(f"mesh_distance: far must be None or 'eikonal', not {far!r}")
    ic = MeshField(np.zeros(grid.n, dtype=np.float64 if dtype is None else dtype, order="F"), grid, dtype=dtype)
    eq = LevelSetEquation(terms=(NormalMotionTerm(0.0),), ic=ic, bc=NeumannBC(), mode=mode, device=device)
    try:
        mesh_distance_(eq, mesh, cutoff)
        if far == "eikonal" and cutoff is not None and math.isfinite(float(cutoff)):
            width = float(cutoff) - math.sqrt(sum(float(h) ** 2 for h in grid.meshsize()))
            if not width > 0:
                raise ValueError("mesh_distance: far='eikonal' needs a cutoff larger than one cell diagonal")
            eikonal_(eq, width=width)
        vals = eq.current_state().values()
    finally:
        eq.backend.close()
    return MeshField(vals, grid, dtype=dtype)


# ----------------------------------------------------------------------------- far-field distance and travel times

def eikonal_(phi, speed=None, width=None, cutoff=None, max_iters=None, extend=None, extend_source="nodes"):
    """Overwrite a device field with sign(ϕ)·min(T, cutoff), T the first-order Godunov solution of |∇T| = 1/speed over the whole
    grid, solved on the device by the block-based fast iterative method.  speed=None: T is the distance to
    the interface {ϕ = 0} — a redistancing of the whole grid in O(nodes), first-order accurate; where the exact distance of a
    band matters, run reinitialize_ or mesh_distance_ first and pass `width`.  `speed`: a positive scalar, an array of the
    grid's shape or a host MeshField on the same grid: T is then the travel time of a front of that speed.  width=None: the
    nodes next to a sign change are seeded from the crossings along the grid lines (any ϕ); width = w > 0: the nodes with
    |ϕ| <= w keep |ϕ| (ϕ already holds distances or times there).  cutoff=None means +inf: nodes with T <= cutoff hold the
    values they hold without one, the others ±cutoff.  `max_iters` bounds the outer iterations (default 2·Σ n_d); exceeding it
    raises a RuntimeError (LsmNotConvergedError) with ϕ unchanged.  `phi`: a dense ROCMeshField or a LevelSetEquation (its current
    state), changed in place.  `extend`: a field or a sequence of 1…8 fields that extend_from_interface_ carries along the new
    distance right after the solve, with the same `width` and `cutoff`, fill=0.0 and source=`extend_source`: redistance and
    extend in one call.  Returns ϕ."""
    if extend is not None:
        _extend_fields(extend, phi.current_state() if isinstance(phi, LevelSetEquation) else phi, "eikonal_")    # refused before ϕ changes
        if extend_source not in ("nodes", "interface"):
            raise ValueError(f"eikonal_: extend_source must be 'nodes' or 'interface', not {extend_source!r}")
    eq = phi if isinstance(phi, LevelSetEquation) else None
    if eq is not None:
        phi = eq.current_state()
    if not isinstance(phi, ROCMeshField):
        raise TypeError(f"eikonal_ takes a device field (ROCMeshField) or a LevelSetEquation, not {type(phi).__name__}")
    if isinstance(phi, ROCNarrowBandMeshField):
        raise ValueError("eikonal_ is not supported on NarrowBandMeshField: the solve runs over the whole grid. "
                         "Use a full MeshField, then build the band from it.")
    N = phi.mesh.ndim
    if N == 1:
        raise ValueError("eikonal_ of a 1 dimensional level-set is not supported: 2-D and 3-D fields only")
    b = phi.backend
    if getattr(b, "slab", None) is not None:
        raise ValueError("eikonal_ of a slab-decomposed field (a field with a comm) is not supported")
    if phi.bcs is not None and any(bc.kind == L.BC_PERIODIC for pair in phi.bcs for bc in pair):
        raise ValueError("eikonal_ with a PeriodicBC dimension is not supported: the front does not wrap around")
    w = 0.0 if width is None else float(width)
    if not (w > 0 and math.isfinite(w)) and width is not None:
        raise ValueError("eikonal_: width must be positive and finite (None: seed from the crossings)")
    c = float("inf") if cutoff is None else float(cutoff)
    if not c > 0:
        raise ValueError("eikonal_: cutoff must be positive (None or inf: no cutoff)")
    sp = None
    if speed is not None:
        if isinstance(speed, MeshField):
            if tuple(speed.mesh.n) != tuple(phi.mesh.n):
                raise ValueError("eikonal_: the speed is a MeshField on another grid")
            speed = speed.vals
        if np.ndim(speed) == 0:
            F = float(speed)
            if not (F > 0 and math.isfinite(F)):
                raise ValueError("eikonal_: the speed must be finite and positive")
            sp = b.torch.full((int(np.prod(phi.mesh.n)),), F, dtype=b.torch.float64, device=b.device)     # filled on the device
        else:
            sp = np.asarray(speed, dtype=np.float64)
            if sp.shape != tuple(phi.mesh.n):
                raise ValueError(f"eikonal_: the speed has shape {sp.shape}, the grid has {tuple(phi.mesh.n)} nodes")
    try:
        b.eikonal(phi.buf, sp, w, c, 0 if max_iters is None else max(1, int(max_iters)))
    except L.LsmNotConvergedError:
        raise
    except L.LsmError as e:
        # what the seed kernel found in the data is the caller's argument error, as the refusals above are
        why = {1: "phi must be finite", 2: "the speed must be finite and positive at every node",
               3: "phi has no interface (no node is zero or next to a change of sign)"}.get(getattr(e, "reason", 0))
        if why is None:
            raise
        raise ValueError(f"eikonal_: {why}") from None
    phi.ghosts_dirty = True
    if extend is not None:
        extend_from_interface_(extend, phi, width=width, source=extend_source, cutoff=cutoff, fill=0.0, max_iters=max_iters)
    return phi


# ----------------------------------------------------------------------------- extension velocities over the whole grid

def _extend_fields(F, phi, who):
    """the list of device fields F names, checked against ϕ: the refusals of extend_from_interface_ that need no data"""
    fields = [F] if isinstance(F, (ROCMeshField, MeshField)) or not isinstance(F, (list, tuple)) else list(F)
    if not isinstance(phi, ROCMeshField):
        raise TypeError(f"{who} takes a device field (ROCMeshField) or a LevelSetEquation as phi, not {type(phi).__name__}")
    for f in fields:
        if not isinstance(f, ROCMeshField):
            raise TypeError(f"{who} extends device fields (ROCMeshField), not {type(f).__name__}")
    for f in fields + [phi]:
        if isinstance(f, ROCNarrowBandMeshField):
            raise ValueError(f"{who} is not supported on NarrowBandMeshField: the extension runs over the whole grid")
    if not 1 <= len(fields) <= 8:
        raise ValueError(f"{who}: 1 to 8 fields, not {len(fields)}")
    for k, f in enumerate(fields):
        if f is phi or f.buf is phi.buf:
            raise ValueError(f"{who}: a field to extend is phi itself")
        if any(f is o or f.buf is o.buf for o in fields[:k]):
            raise ValueError(f"{who}: the same field twice")
        if f.backend is not phi.backend:
            raise ValueError(f"{who}: a field lives on another backend than phi (fields of one equation share one)")
        if f.mesh is not phi.mesh and (tuple(f.mesh.n) != tuple(phi.mesh.n) or tuple(f.mesh.lc) != tuple(phi.mesh.lc) or tuple(f.mesh.hc) != tuple(phi.mesh.hc)):
            raise ValueError(f"{who}: a field lives on another mesh than phi")
    return fields


def extend_from_interface_(F, phi, *, width=None, frozen=None, source="nodes", cutoff=None, fill=0.0, max_iters=None):
    """Carry the values of F off the interface of ϕ over the whole grid, constant along the characteristics of |ϕ|
    (∇F·∇|ϕ| = 0, first-order upwind), on the device in O(nodes): the extension velocity an optimisation loop
    needs before every advection, where extend_along_normals_ moves the information about `cfl` of a cell per sweep.  ϕ should
    be distance-like (eikonal_, reinitialize_); every node is reached whatever ϕ holds.  `F`: a ROCMeshField or a sequence of
    1…8 of them on ϕ's backend, changed in place; `phi`: a dense ROCMeshField or a LevelSetEquation (its current state), read only.
    The frozen nodes keep their F.  frozen=None: eikonal_'s seeding set for the same `width` — the nodes next to a sign change
    and the zeros of ϕ, with width = w > 0 also every node with |ϕ| <= w; "inside": ϕ <= 0; "outside": ϕ >= 0; a boolean or
    0–1 array of the grid's shape or a host MeshField on the same grid: where it is non-zero.  source="interface" (with
    frozen=None): the nodes next to a sign change first take the value F has at their crossings, interpolated along the grid
    lines.  Nodes that are not frozen and have |ϕ| >= cutoff take `fill`.  Every value lies within the range of the seeds; the
    result is the same bits in every run.  `max_iters` bounds the outer iterations (default 2·Σ n_d); exceeding it raises a
    RuntimeError (LsmNotConvergedError) with F unchanged.  Returns F."""
    eq = phi if isinstance(phi, LevelSetEquation) else None
    if eq is not None:
        phi = eq.current_state()
    fields = _extend_fields(F, phi, "extend_from_interface_")
    N = phi.mesh.ndim
    if N == 1:
        raise ValueError("extend_from_interface_ of a 1 dimensional level-set is not supported: 2-D and 3-D fields only")
    b = phi.backend
    if getattr(b, "slab", None) is not None:
        raise ValueError("extend_from_interface_ of a slab-decomposed field (a field with a comm) is not supported")
    if phi.bcs is not None and any(bc.kind == L.BC_PERIODIC for pair in phi.bcs for bc in pair):
        raise ValueError("extend_from_interface_ with a PeriodicBC dimension is not supported: the characteristics do not wrap around")
    w = 0.0 if width is None else float(width)
    if not (w > 0 and math.isfinite(w)) and width is not None:
        raise ValueError("extend_from_interface_: width must be positive and finite (None: the crossing seed)")
    c = float("inf") if cutoff is None else float(cutoff)
    if not c > 0:
        raise ValueError("extend_from_interface_: cutoff must be positive (None or inf: no cutoff)")
    fill = float(fill)
    if not math.isfinite(fill):
        raise ValueError("extend_from_interface_: fill must be finite")
    if source not in ("nodes", "interface"):
        raise ValueError(f"extend_from_interface_: source must be 'nodes' or 'interface', not {source!r}")
    if source == "interface" and frozen is not None:
        raise ValueError("extend_from_interface_: source='interface' takes the values at the crossings of phi and goes with frozen=None only")
    rule, mask = "rule", None
    if isinstance(frozen, str):
        if frozen not in ("inside", "outside"):
            raise ValueError(f"extend_from_interface_: frozen must be None, 'inside', 'outside' or a mask, not {frozen!r}")
        rule = frozen
    elif frozen is not None:
        if isinstance(frozen, MeshField):
            if tuple(frozen.mesh.n) != tuple(phi.mesh.n):
                raise ValueError("extend_from_interface_: the frozen mask is a MeshField on another grid")
            frozen = frozen.vals
        mask = np.asarray(frozen)
        if mask.shape != tuple(phi.mesh.n):
            raise ValueError(f"extend_from_interface_: the frozen mask has shape {mask.shape}, the grid has {tuple(phi.mesh.n)} nodes")
        rule = "mask"
    try:
        b.extend([f.buf for f in fields], phi.buf, rule, mask, w, source, c, fill, 0 if max_iters is None else max(1, int(max_iters)))
    except L.LsmNotConvergedError:
        raise
    except L.LsmError as e:
        why = {1: "phi must be finite", 2: "every field must be finite at the frozen nodes",
               3: "no node is frozen (phi has no interface, or the mask is empty)"}.get(getattr(e, "reason", 0))
        if why is None:
            raise
        raise ValueError(f"extend_from_interface_: {why} ({getattr(e, 'offenders', 0)} nodes)") from None
    for f in fields:
        f.ghosts_dirty = True
    return F


def eikonal(phi, speed=None, width=None, cutoff=None, max_iters=None, mode="fast", device=0):
    """eikonal_ of a host MeshField on a throwaway device field: returns a new host MeshField, usable as `ic=`."""
    if not isinstance(phi, MeshField):
        raise TypeError(f"eikonal takes a host MeshField, not {type(phi).__name__}; eikonal_ works on device fields in place")
    dtype = np.asarray(phi.vals).dtype
    eq = LevelSetEquation(terms=(NormalMotionTerm(0.0),), ic=MeshField(phi.vals, phi.mesh, dtype=dtype), bc=NeumannBC(), mode=mode, device=device)
    try:
        vals = eikonal_(eq, speed, width, cutoff, max_iters).values()
    finally:
        eq.backend.close()
    return MeshField(vals, phi.mesh, dtype=dtype)


# ----------------------------------------------------------------------------- connected components

class Components:
    """components(…)'s result: the K connected pieces of {ϕ < level} (side "inside") or of its complement ("outside") over the
    Kuhn edges, numbered by their smallest linear node index (axis 0 fastest).  `count` = K; `labels()`: int32 of the grid's
    shape, −1 off the set (`labels_device`: the same on the device, flat, axis 0 fastest); `nodes` int64 (K); `index_sums` int64
    (K, N): the sums of the 0-based node indices per axis; `bbox` int32 (K, 2, N): the smallest and the largest index per axis;
    `centroids` (K, N) = lc + h·index_sums/nodes; `measures` (K) = nodes·∏h, a first-order estimate of a piece's size (every
    node counts as one cell; the cut cells at the interface are not weighed: use quadrature for that); `stats` = (K, nodes in
    the set, Kuhn edges between set nodes in different tiles, non-finite nodes).  The object keeps the labels on the device for
    remove_components_; close() releases them."""

    def __init__(self, backend, mesh, level, side, handle, stats):
        self.backend, self.mesh, self.level, self.side, self._h, self.stats = backend, mesh, float(level), side, handle, stats
        self.count = int(stats[0])
        labels, nodes, sums, bbox = backend.cc_read(handle, self.count)
        self.labels_device = labels
        self.nodes, self.index_sums, self.bbox = nodes.cpu().numpy(), sums.cpu().numpy(), bbox.cpu().numpy()

    def labels(self):
        return self.labels_device.cpu().numpy().reshape(self.mesh.n, order="F")

    @property
    def centroids(self):
        lc, h = np.asarray(self.mesh.lc, dtype=np.float64), np.asarray(self.mesh.meshsize(), dtype=np.float64)
        return lc + h * (self.index_sums.astype(np.float64) / self.nodes.astype(np.float64)[:, None])

    @property
    def measures(self):
        return self.nodes.astype(np.float64) * float(np.prod(np.asarray(self.mesh.meshsize(), dtype=np.float64)))

    def __len__(self):
        return self.count

    def __repr__(self):
        return (f"Components of a {self.mesh.ndim}-dimensional level-set: {self.count} {self.side} "
                f"{'component' if self.count == 1 else 'components'}, {int(self.stats[1])} nodes, level = {_jl_float(self.level)}")

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            try:
                self.backend.cc_destroy(h)
            except Exception:
                pass

    __del__ = close


_SIDES = {"inside": 0, "outside": 1}


def _cc_field(phi, what):
    """the dense single-device 2-D / 3-D field behind components / remove_components_ / prune_, or the refusal"""
    if isinstance(phi, LevelSetEquation):
        phi = phi.current_state()
    if not isinstance(phi, ROCMeshField):
        raise TypeError(f"{what} takes a device field (ROCMeshField) or a LevelSetEquation, not {type(phi).__name__}")
    if isinstance(phi, ROCNarrowBandMeshField):
        raise ValueError(f"{what} is not supported on NarrowBandMeshField: a band does not hold the whole set. Use a full MeshField.")
    if phi.mesh.ndim == 1:
        raise ValueError(f"{what} of a 1 dimensional level-set is not supported: 2-D and 3-D fields only")
    if getattr(phi.backend, "slab", None) is not None:
        raise ValueError(f"{what} of a slab-decomposed field (a field with a comm) is not supported")
    if phi.bcs is not None and any(bc.kind == L.BC_PERIODIC for pair in phi.bcs for bc in pair):
        raise ValueError(f"{what} with a PeriodicBC dimension is not supported: components are not joined across the wrap")
    if int(np.prod([int(n) for n in phi.mesh.n], dtype=object)) >= 2 ** 31 - 1:
        raise ValueError(f"{what}: the grid has 2^31 - 1 nodes or more")
    return phi


def components(phi_or_eq, level=0.0, side="inside"):
    """The connected components of {ϕ < level} (side="inside"; ϕ == level is outside, as for isosurface) or of its complement
    (side="outside"), labelled on the device by block-based union–find.  Two nodes of the set are adjacent iff
    they differ by ±d, d ∈ {0,1}^N \\ {0}: the edges of the Kuhn subdivision behind isosurface and volume_mesh (6 neighbours in
    2-D, 14 in 3-D), so the inside components are exactly the connected pieces of volume_mesh(ϕ, level) — not those of the 4/8-
    or 6/26-connectivity of image libraries.  ϕ: a dense ROCMeshField or a LevelSetEquation (its current state), 2-D or 3-D, no
    PeriodicBC dimension, finite.  Returns a Components; an empty set gives count 0."""
    phi = _cc_field(phi_or_eq, "components")
    if side not in _SIDES:
        raise ValueError('components: side must be "inside" or "outside"')
    level = float(level)
    if not math.isfinite(level):
        raise ValueError("components: level must be finite")
    b = phi.backend
    try:
        h, stats = b.cc_create(phi.buf, level, _SIDES[side])
    except L.LsmError as e:
        if getattr(e, "nonfinite", 0):
            raise ValueError(f"components: phi must be finite ({e.nonfinite} nodes are not)") from None
        raise
    return Components(b, phi.mesh, level, side, h, stats)


def _cc_which(comps, which, what):
    w = np.asarray(which)
    if w.dtype == np.bool_:
        if w.shape != (comps.count,):
            raise ValueError(f"{what}: `which` has {w.size} entries, there are {comps.count} components")
        return w
    ids = w.astype(np.int64).reshape(-1) if w.size else np.zeros(0, dtype=np.int64)
    if w.size and (not np.issubdtype(w.dtype, np.integer) or ids.min() < 0 or ids.max() >= comps.count):
        raise ValueError(f"{what}: `which` must be a boolean array of length {comps.count} or a list of component ids below it")
    out = np.zeros(comps.count, dtype=np.bool_)
    out[ids] = True
    return out


def remove_components_(phi, comps, which):
    """Move every node of the components flagged in `which` (a boolean array of length comps.count, or a list of ids) to the
    other side of comps.level, in place, on the device: v' = level + (level − v), mirrored at the level; an outside node that
    does not land below the level takes the value just below it.  Returns the number of nodes flipped and sets
    ϕ.ghosts_dirty.  The result is NOT a distance function near what was removed: the mirrored values meet their neighbours
    with a kink, and the removed piece's interface is gone while the values around it still point at it.  Follow with
    reinitialize_ (near the interface) or eikonal_ (the whole grid) before anything that relies on |∇ϕ| = 1.  Raises a
    ValueError, with ϕ unchanged, when ϕ no longer matches `comps` (it was changed, or these components were removed before)."""
    phi = _cc_field(phi, "remove_components_")
    if not isinstance(comps, Components):
        raise TypeError(f"remove_components_ takes the Components of this field, not {type(comps).__name__}")
    if comps._h is None:
        raise ValueError("remove_components_: the Components object is closed")
    if comps.backend is not phi.backend:
        raise ValueError("remove_components_: the Components belong to another field's backend")
    w = _cc_which(comps, which, "remove_components_")
    if not w.any():
        return 0
    b = phi.backend
    flags = b.torch.from_numpy(w.astype(np.uint8)).to(b.device)
    try:
        flipped = b.cc_flip(comps._h, phi.buf, flags)
    except L.LsmError as e:
        if "phi has changed" in str(e):
            raise ValueError("remove_components_: phi no longer matches the Components (a flagged node is on the other side of level); "
                             "call components again") from None
        raise
    phi.ghosts_dirty = True
    return flipped


def prune_(phi_or_eq, min_nodes=None, keep_largest=None, level=0.0, side="inside"):
    """components, a choice on the host, remove_components_: flags the components with fewer than `min_nodes` nodes, and all
    but the `keep_largest` largest (ties go to the smaller id); with both, a component flagged by either rule goes.  Returns
    (Components, flipped); the Components describe ϕ BEFORE pruning.  side="outside", keep_largest=1 fills cavities;
    min_nodes removes the islands an advection leaves behind.  As for remove_components_, reinitialize_ or eikonal_ afterwards."""
    if min_nodes is None and keep_largest is None:
        raise ValueError("prune_: give min_nodes, keep_largest or both")
    if keep_largest is not None and int(keep_largest) < 0:
        raise ValueError("prune_: keep_largest must not be negative")
    phi = _cc_field(phi_or_eq, "prune_")
    comps = components(phi, level, side)
    which = np.zeros(comps.count, dtype=np.bool_)
    if min_nodes is not None:
        which |= comps.nodes < int(min_nodes)
    if keep_largest is not None:
        order = np.lexsort((np.arange(comps.count), -comps.nodes))      # by size, descending; ties: the smaller id first
        which[order[int(keep_largest):]] = True
    return comps, remove_components_(phi, comps, which)


# ----------------------------------------------------------------------------- hole nucleation

class Nucleation:
    """nucleate_ / find_nucleation_sites' result: `centres` int64 (K, N), the multi-indices of the chosen nodes sorted by
    (value, linear index); `indices` int64 (K), their linear indices (axis 0 fastest); `values` float64 (K), the criterion at them;
    `found`, the number of centres before the cut to max_holes; `changed`, the number of nodes the punch changed (0 without one)."""

    def __init__(self, mesh, indices, values, found, changed=0):
        self.mesh, self.indices, self.values, self.found, self.changed = mesh, indices, values, int(found), int(changed)
        n = [int(m) for m in mesh.n]
        self.centres = (np.stack(np.unravel_index(indices, n, order="F"), axis=1).astype(np.int64) if indices.size
                        else np.zeros((0, len(n)), dtype=np.int64))

    def __len__(self):
        return int(self.indices.size)

    def __repr__(self):
        return (f"Nucleation on a {self.mesh.ndim}-dimensional grid: {len(self)} of {self.found} "
                f"{'centre' if self.found == 1 else 'centres'}, {self.changed} nodes changed")


def _nucleation_field(x, what, name):
    """the dense single-device 2-D / 3-D field behind nucleate_ / find_nucleation_sites, or the refusal"""
    if isinstance(x, LevelSetEquation):
        x = x.current_state()
    if not isinstance(x, ROCMeshField):
        raise TypeError(f"{what} takes device fields (ROCMeshField), not {type(x).__name__} for {name}")
    if isinstance(x, ROCNarrowBandMeshField):
        raise ValueError(f"{what} is not supported on NarrowBandMeshField: a band does not hold the whole set. Use a full MeshField.")
    if x.mesh.ndim == 1:
        raise ValueError(f"{what} of a 1 dimensional level-set is not supported: 2-D and 3-D fields only")
    if getattr(x.backend, "slab", None) is not None:
        raise ValueError(f"{what} of a slab-decomposed field (a field with a comm) is not supported")
    if x.bcs is not None and any(bc.kind == L.BC_PERIODIC for pair in x.bcs for bc in pair):
        raise ValueError(f"{what} with a PeriodicBC dimension is not supported: the window and the balls do not wrap")
    if int(np.prod([int(n) for n in x.mesh.n], dtype=object)) >= 2 ** 31 - 1:
        raise ValueError(f"{what}: the grid has 2^31 - 1 nodes or more")
    return x


def _nucleation_args(phi, t, what, threshold, radius, spacing, clearance, max_holes, level):
    """(ϕ, t, threshold, radius, spacing, clearance, max_holes, level) checked: the refusals need no device call"""
    threshold, radius, level = float(threshold), float(radius), float(level)
    if not (math.isfinite(radius) and radius > 0.0):
        raise ValueError(f"{what}: radius must be finite and positive")
    spacing = 2.0 * radius if spacing is None else float(spacing)
    clearance = radius if clearance is None else float(clearance)
    if not (math.isfinite(threshold) and math.isfinite(level) and math.isfinite(clearance)):
        raise ValueError(f"{what}: threshold, level and clearance must be finite")
    if not math.isfinite(spacing):
        raise ValueError(f"{what}: spacing must be finite")
    if max_holes is not None:
        max_holes = int(max_holes)
        if max_holes < 0:
            raise ValueError(f"{what}: max_holes must not be negative")
    phi, t = _nucleation_field(phi, what, "phi"), _nucleation_field(t, what, "t")
    if t.backend is not phi.backend:
        raise ValueError(f"{what}: t must be a field of phi's backend (the same grid and layout)")
    w = [math.ceil(spacing / float(h)) for h in phi.mesh.meshsize()]
    if min(w) < 1 or max(w) > 32:
        raise ValueError(f"{what}: the window ceil(spacing/h) = {tuple(w)} nodes must lie in [1, 32] along every axis")
    return phi, t, threshold, radius, spacing, clearance, max_holes, level


def _nucleation_sites(phi, t, threshold, spacing, clearance, max_holes, level):
    idx, val = phi.backend.nucleate_find(phi.buf, t.buf, threshold, level, clearance, spacing)
    order = np.lexsort((idx, val))      # by (value, index); −0 and +0 compare equal, as on the device
    found = int(idx.size)
    if max_holes is not None:
        order = order[:max_holes]
    return idx[order], val[order], found


def find_nucleation_sites(phi, t, *, threshold, radius, spacing=None, clearance=None, max_holes=None, level=0.0):
    """nucleate_ without the punch: the centres the criterion field t selects, as a Nucleation with changed = 0; ϕ is not written."""
    phi, t, threshold, radius, spacing, clearance, max_holes, level = _nucleation_args(phi, t, "find_nucleation_sites", threshold, radius, spacing, clearance,
                                                                                         max_holes, level)
    idx, val, found = _nucleation_sites(phi, t, threshold, spacing, clearance, max_holes, level)
    return Nucleation(phi.mesh, idx, val, found)


def nucleate_(phi, t, *, threshold, radius, spacing=None, clearance=None, max_holes=None, level=0.0):
    """Punch holes into ϕ where the criterion field t is lowest, on the device: the step by which a level-set
    optimisation changes topology.  t: a dense ROCMeshField on ϕ's backend — ElasticitySolution.topological_derivative(), or any
    criterion of the caller's.  A node is a candidate where t < threshold and ϕ ≤ level − clearance (inside the material, away from
    the boundary; ϕ is taken for a signed distance); a candidate is a centre iff its (value, index) is the smallest among the
    candidates within ceil(spacing/h) nodes of it along every axis, so two centres are more than `spacing` apart.  The centres
    are sorted by (value, index), cut to the `max_holes` lowest, and a ball of `radius` is removed around each:
    ϕ ← max(ϕ, level + radius − |x − c|) over the ball's bounding box.  spacing defaults to 2·radius (disjoint balls), clearance
    to radius.  Returns a Nucleation and sets ϕ.ghosts_dirty; follow with reinitialize_ before anything that relies on |∇ϕ| = 1."""
    phi, t, threshold, radius, spacing, clearance, max_holes, level = _nucleation_args(phi, t, "nucleate_", threshold, radius, spacing, clearance, max_holes,
                                                                                         level)
    idx, val, found = _nucleation_sites(phi, t, threshold, spacing, clearance, max_holes, level)
    changed = phi.backend.nucleate_punch(phi.buf, idx, level, radius) if idx.size else 0
    phi.ghosts_dirty = True
    return Nucleation(phi.mesh, idx, val, found, changed)


# ----------------------------------------------------------------------------- elliptic solves (the state equation of a shape optimisation)

_PRECONDS = {"mg": L.PRECOND_MG, "jacobi": L.PRECOND_JACOBI}
_ELLIPTIC_REFUSALS = {1: "phi must be finite", 2: "the cell coefficients `a` must be finite and positive", 3: "c must be finite and not negative",
                      4: "no fixed node and c = 0 everywhere: the problem is singular", 5: "every node is fixed"}


def face_mask(grid, d, side):
    """The boolean node mask (shape grid.n) of a face of the box: dimension d (0-based), side 0 (lower) or 1 (upper); for `dirichlet=`."""
    n = tuple(int(m) for m in grid.n)
    if not 0 <= int(d) < len(n) or side not in (0, 1):
        raise ValueError("face_mask: d must be a dimension of the grid and side 0 or 1")
    m = np.zeros(n, dtype=np.bool_, order="F")
    m[tuple(slice(None) if e != d else (0 if side == 0 else n[d] - 1) for e in range(len(n)))] = True
    return m


def _finite_positive(x):
    return bool(np.all(np.isfinite(x)) and np.all(np.asarray(x) > 0))


def _elliptic_field(phi, what):
    """the dense single-device 2-D / 3-D field behind an elliptic solve, or the refusal"""
    if isinstance(phi, LevelSetEquation):
        phi = phi.current_state()
    if not isinstance(phi, ROCMeshField):
        raise TypeError(f"{what} takes a device field (ROCMeshField) or a LevelSetEquation, not {type(phi).__name__}")
    if isinstance(phi, ROCNarrowBandMeshField):
        raise ValueError(f"{what} is not supported on NarrowBandMeshField: the equation is solved over the whole box. Use a full MeshField.")
    if phi.mesh.ndim == 1:
        raise ValueError(f"{what} of a 1 dimensional level-set is not supported: 2-D and 3-D fields only")
    if getattr(phi.backend, "slab", None) is not None:
        raise ValueError(f"{what} of a slab-decomposed field (a field with a comm) is not supported")
    if phi.bcs is not None and any(bc.kind == L.BC_PERIODIC for pair in phi.bcs for bc in pair):
        raise ValueError(f"{what} with a PeriodicBC dimension is not supported: the faces of the box are natural (zero-flux)")
    if any(int(m) < 3 for m in phi.mesh.n):
        raise ValueError(f"{what} needs at least 3 nodes in every dimension")
    return phi


def _host_values(v):
    """the host array behind a scalar / array / MeshField argument, or None for a device field"""
    if isinstance(v, ROCMeshField):
        return None
    return np.asarray(v.vals if isinstance(v, MeshField) else v, dtype=np.float64)


class EllipticSolution:
    """elliptic_solve's result: `u` (a ROCMeshField on ϕ's backend: coeff.set_values takes it device to device), `iterations`,
    `relres` (the recursive ‖r‖₂/‖b_free‖₂), `levels` of the hierarchy; energy_density(): the ROCMeshField of
    e_I = Σ_d mean over the existing sides of k̄·((u_J − u_I)/h_d)² — a|∇u|² at the nodes, the normal speed of a compliance
    descent; compliance() = ∏h·Σ m f u, reduced on the device."""

    def __init__(self, op, u, f, iterations, relres):
        self.operator, self.u, self._f, self.iterations, self.relres, self.levels = op, u, f, int(iterations), float(relres), op.levels

    def energy_density(self):
        op = self.operator
        e = ROCMeshField(op.backend, self.u.mesh, self.u.bcs)
        op.backend.elliptic_energy(op._handle(), self.u.buf, e.buf)
        return e

    def mutual_energy_density(self, other):
        """the ROCMeshField of m_I = energy_density()'s sums with g·g replaced by g_u·g_v, v = other.u: a∇u·∇v at the nodes, the integrand
        of the shape derivative of l·u for this state and the adjoint `other` (A v = l) of the same operator.  The c·u·v
        term is not in it.  With other = self it is energy_density() bit for bit, and it is symmetric bit for bit."""
        op = self.operator
        if not isinstance(other, EllipticSolution) or other.operator is not op:
            raise ValueError("mutual_energy_density: the other solution belongs to another operator")
        e = ROCMeshField(op.backend, self.u.mesh, self.u.bcs)
        op.backend.elliptic_energy_mutual(op._handle(), self.u.buf, other.u.buf, e.buf)
        return e

    def compliance(self):
        op = self.operator
        return op.backend.elliptic_compliance(op._handle(), self._f, self.u.buf)


class EllipticMultiSolution:
    """solve_many's result: a sequence of K EllipticSolutions of one operator (len, indexing, iteration), each with its own u, iterations,
    relres and source.  `iterations` and `relres` are tuples, `operator` and `levels` as on a single solution.  compliances() → the K
    values; compliance(weights=None) = Σ w_k·c_k (weights default to 1); cross_compliance(i, j) = ∏h·Σ (m·f_i)·u_j; energy_density(weights=None)
    → the ROCMeshField of Σ_k w_k·e_k in one pass over the grid; mutual_energy_density(i, j) → that of columns i and j."""

    def __init__(self, op, columns):
        self.operator, self._columns, self.levels = op, tuple(columns), op.levels
        self.iterations = tuple(c.iterations for c in self._columns)
        self.relres = tuple(c.relres for c in self._columns)

    def __len__(self):
        return len(self._columns)

    def __getitem__(self, k):
        return self._columns[k]

    def __iter__(self):
        return iter(self._columns)

    def _weights(self, weights, what):
        K = len(self._columns)
        w = [1.0] * K if weights is None else [float(v) for v in weights]
        if len(w) != K:
            raise ValueError(f"{what}: {len(w)} weights for {K} columns")
        if not all(math.isfinite(v) for v in w):
            raise ValueError(f"{what}: the weights must be finite")
        return w

    def compliances(self):
        return tuple(c.compliance() for c in self._columns)

    def compliance(self, weights=None):
        w = self._weights(weights, "compliance")
        total = 0.0
        for wk, ck in zip(w, self.compliances()):
            total = total + wk * ck
        return total

    def cross_compliance(self, i, j):
        op = self.operator
        return op.backend.elliptic_compliance(op._handle(), self._columns[i]._f, self._columns[j].u.buf)

    def energy_density(self, weights=None):
        op = self.operator
        w = self._weights(weights, "energy_density")
        u0 = self._columns[0].u
        e = ROCMeshField(op.backend, u0.mesh, u0.bcs)
        op.backend.elliptic_energy_many(op._handle(), [c.u.buf for c in self._columns], w, e.buf)
        return e

    def mutual_energy_density(self, i, j):
        return self._columns[i].mutual_energy_density(self._columns[j])


class EllipticOperator:
    """The discrete operator of −∇·(a∇u) + c·u on ϕ's grid and its multigrid hierarchy, kept on the device for repeated solves
    with new right-hand sides and guesses: solve(f, u0=None, rtol=1e-8, max_iters=500) → EllipticSolution.  The arguments are
    elliptic_solve's.  ϕ is read once, here: after ϕ has moved, build a new operator.  close() releases the device memory."""

    def __init__(self, phi_or_eq, *, a_in=1.0, a_out=1e-3, a=None, c=0.0, dirichlet=None, level=0.0, precond="mg"):
        what = "elliptic_solve"
        self._h = None
        if precond not in _PRECONDS:
            raise ValueError(f'{what}: precond must be "mg" or "jacobi", not {precond!r}')
        a_host = None if a is None or (hasattr(a, "is_cuda")) else np.asarray(a, dtype=np.float64)
        if a is None:
            if not (_finite_positive(float(a_in)) and _finite_positive(float(a_out))):
                raise ValueError(f"{what}: a_in and a_out must be finite and positive")
            if not math.isfinite(float(level)):
                raise ValueError(f"{what}: level must be finite")
        elif a_host is not None and not _finite_positive(a_host):
            raise ValueError(f"{what}: the cell coefficients `a` must be finite and positive")
        c_host = _host_values(c)
        if c_host is not None and not (np.all(np.isfinite(c_host)) and np.all(c_host >= 0)):
            raise ValueError(f"{what}: c must be finite and not negative")
        mask = values = None
        if dirichlet is not None:
            if not (isinstance(dirichlet, (tuple, list)) and len(dirichlet) == 2):
                raise TypeError(f"{what}: dirichlet must be a pair (mask, values)")
            mask = np.asarray(dirichlet[0])
            if mask.dtype != np.bool_:
                raise TypeError(f"{what}: the Dirichlet mask must be a boolean array")
            values = np.asarray(dirichlet[1], dtype=np.float64)
            if not np.all(np.isfinite(values)):
                raise ValueError(f"{what}: the Dirichlet values must be finite")
        if c_host is not None and not np.any(c_host > 0) and (mask is None or not mask.any()):
            raise ValueError(f"{what}: no fixed node and c = 0 everywhere: the problem is singular")
        phi = _elliptic_field(phi_or_eq, what)
        n = tuple(int(m) for m in phi.mesh.n)
        if mask is not None and mask.shape != n:
            raise ValueError(f"{what}: the Dirichlet mask has shape {mask.shape}, the grid has {n} nodes")
        if values is not None and values.ndim and values.shape != n:
            raise ValueError(f"{what}: the Dirichlet values have shape {values.shape}, the grid has {n} nodes")
        if mask is not None and mask.all():
            raise ValueError(f"{what}: every node is fixed")
        cells = tuple(m - 1 for m in n)
        if a_host is not None and a_host.ndim and a_host.shape != cells:
            raise ValueError(f"{what}: `a` has shape {a_host.shape}, the grid has {cells} cells")
        if c_host is not None and c_host.ndim and c_host.shape != n:
            raise ValueError(f"{what}: c has shape {c_host.shape}, the grid has {n} nodes")
        b = self.backend = phi.backend
        self.mesh, self.bcs, self.precond = phi.mesh, phi.bcs, precond
        self._phi, self._level = (None if a is not None else phi), float(level)      # the density of modes() is read from the same ϕ
        t = b.torch
        a_dev = None if a is None else b.node_array(a if a_host is None else a_host, "a", cells)
        c_dev = None
        if c_host is None:
            c_dev = b.interior(c.buf).to(t.float64).contiguous().reshape(-1)
        elif c_host.ndim:
            c_dev = b.node_array(c_host, "c")
        self._mask = self._values = fixed = None
        if mask is not None and mask.any():
            self._mask = t.from_numpy(np.ascontiguousarray(mask.T)).to(b.device)                      # the interior view's axis order
            self._values = t.from_numpy(np.ascontiguousarray(np.broadcast_to(values, n).T)).to(b.device)
            fixed = self._mask.to(t.uint8).contiguous().reshape(-1)
        try:
            self._h, stats = b.elliptic_create(None if a is not None else phi.buf, level, a_in, a_out, a_dev, 0.0 if c_dev is not None else float(c_host),
                                               c_dev, fixed, _PRECONDS[precond])
        except L.LsmError as e:
            why = _ELLIPTIC_REFUSALS.get(getattr(e, "reason", 0))
            if why is None:
                raise
            raise ValueError(f"{what}: {why}") from None
        self.levels, self.free_nodes, self.fixed_nodes = stats[0], stats[1], stats[2]

    def _handle(self):
        if self._h is None:
            raise ValueError("the EllipticOperator is closed")
        return self._h

    def _field(self, u0, homogeneous=False):
        """a new field holding the guess (zero without one) and, on the Dirichlet nodes, their values — or zero (homogeneous: an adjoint
        column)"""
        b = self.backend
        u = ROCMeshField(b, self.mesh, self.bcs)
        if isinstance(u0, ROCMeshField):
            if u0.backend is not b:
                raise ValueError("elliptic_solve: u0 belongs to another field's backend")
            u.copy_(u0)
        elif u0 is not None:
            v = _host_values(u0)
            u.copy_(np.broadcast_to(v, tuple(int(m) for m in self.mesh.n)))
        if self._mask is not None:
            iv = b.interior(u.buf)
            iv.copy_(b.torch.where(self._mask, b.torch.zeros_like(iv) if homogeneous else self._values.to(iv.dtype), iv))
        return u

    def _source(self, f):
        """f as one flat float64 device array"""
        b = self.backend
        if isinstance(f, ROCMeshField):
            return b.interior(f.buf).to(b.torch.float64).contiguous().reshape(-1)
        return b.node_array(f if b.torch.is_tensor(f) else _host_values(f), "f")       # a flat float64 device tensor is taken as it is

    def solve(self, f, u0=None, rtol=1e-8, max_iters=500):
        b = self.backend
        h = self._handle()
        rtol = float(rtol)
        if not (rtol > 0 and math.isfinite(rtol)) or int(max_iters) < 1:
            raise ValueError("elliptic_solve: rtol must be positive and finite, max_iters at least 1")
        fd = self._source(f)
        u = self._field(u0)
        try:
            it, rel = b.elliptic_solve(h, fd, u.buf, rtol, int(max_iters))
        except L.LsmNotConvergedError:
            raise
        except L.LsmError as e:
            if "must be finite" in str(e):
                raise ValueError("elliptic_solve: f, u0 and the Dirichlet values must be finite") from None
            raise
        return EllipticSolution(self, u, fd, it, rel)

    def solve_many(self, fs, u0=None, homogeneous=None, rtol=1e-8, max_iters=500):
        """K = len(fs) ≤ 8 sources of this operator in one batched solve → EllipticMultiSolution.  Column k is solve(fs[k], u0[k]) bit for
        bit: u, iterations and relres.  `fs`: a sequence of sources, each in any form solve takes; `u0`: None or a
        sequence of guesses (an entry may be None); `homogeneous`: a sequence of booleans — a true column takes zero on the Dirichlet
        nodes instead of their values (an adjoint column).  Unless every column converges nothing is kept: LsmNotConvergedError carries
        .iterations, .relres and .status (1 converged, 2 out of iterations, −2 / −3 breakdown) tuples; ValueError for what is refused
        and for non-finite data, naming the column."""
        what = "elliptic_solve_many"
        rtol = float(rtol)
        if not (rtol > 0 and math.isfinite(rtol)) or int(max_iters) < 1:
            raise ValueError(f"{what}: rtol must be positive and finite, max_iters at least 1")
        if not isinstance(fs, (tuple, list)):
            raise TypeError(f"{what}: fs must be a sequence of sources")
        b = self.backend
        K = len(fs)
        if not 1 <= K <= b.ELLIPTIC_MAXCOLS:
            raise ValueError(f"{what}: {K} sources (1 to {b.ELLIPTIC_MAXCOLS} are solved together)")
        if u0 is not None and not isinstance(u0, (tuple, list)):
            raise TypeError(f"{what}: u0 must be None or a sequence of guesses, one per source")
        if homogeneous is not None and not isinstance(homogeneous, (tuple, list)):
            raise TypeError(f"{what}: homogeneous must be None or a sequence of booleans, one per source")
        u0 = [None] * K if u0 is None else list(u0)
        homogeneous = [False] * K if homogeneous is None else [bool(v) for v in homogeneous]
        if len(u0) != K or len(homogeneous) != K:
            raise ValueError(f"{what}: u0 and homogeneous must have one entry per source ({K})")
        h = self._handle()
        fds = [self._source(f) for f in fs]
        us = [self._field(u0[k], homogeneous[k]) for k in range(K)]
        try:
            its, rels, _ = b.elliptic_solve_many(h, b.torch.cat(fds), [u.buf for u in us], rtol, int(max_iters))
        except L.LsmNotConvergedError:
            raise
        except L.LsmError as e:
            if "must be finite" in str(e):
                col = [k for k, v in enumerate(getattr(e, "status", ())) if v == -1]
                raise ValueError(f"{what}: f, u0 and the Dirichlet values must be finite (column {col[0] if col else '?'})") from None
            raise
        return EllipticMultiSolution(self, [EllipticSolution(self, us[k], fds[k], its[k], rels[k]) for k in range(K)])

    def apply(self, x):
        """A x on all nodes, no elimination: x a host array of the grid's shape; returns one (for tests and diagnostics)"""
        b = self.backend
        n = tuple(int(m) for m in self.mesh.n)
        y = b.elliptic_apply(self._handle(), b.node_array(np.asarray(x, dtype=np.float64), "x"))
        return y.cpu().numpy().reshape(n, order="F")

    def cells(self):
        """the level-0 cell coefficients, a host array of shape n − 1"""
        n = tuple(int(m) - 1 for m in self.mesh.n)
        return self.backend.elliptic_cells(self._handle()).cpu().numpy().reshape(n, order="F")

    def modes(self, m, *, rho_in=1.0, rho_out=1e-6, rho=None, x0=None, rtol=1e-6, max_iters=300):
        """the m smallest eigenpairs of A u = λ M u for this operator (the fixed nodes zero): an EllipticModes.  See elliptic_modes."""
        return EllipticModes(self, m, rho_in=rho_in, rho_out=rho_out, rho=rho, x0=x0, rtol=rtol, max_iters=max_iters)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            try:
                self.backend.elliptic_destroy(h)
            except Exception:
                pass

    __del__ = close


def elliptic_solve(phi_or_eq, f, *, a_in=1.0, a_out=1e-3, a=None, c=0.0, dirichlet=None, u0=None, level=0.0, rtol=1e-8, max_iters=500, precond="mg"):
    """Solve −∇·(a∇u) + c·u = f on the box of ϕ's grid, on the device: the state equation of a level-set shape optimisation with
    an ersatz material.  Unknowns at the nodes, zero-flux conditions on every face, u fixed on the nodes of
    `dirichlet=(mask, values)` (a boolean array of the grid's shape — face_mask builds a face's — and a scalar or an array).
    The coefficient of a cell is a_out + (a_in − a_out)·θ, θ = clamp(½ − (mean of ϕ's corner values − level)/min h, 0, 1): a_in
    where ϕ < level, a_out outside, the exact fill fraction in between for a distance function with an axis-aligned interface.
    `a` (a scalar or an array of shape n − 1) gives the cell coefficients directly and ϕ is not read.  `f` and `c` (≥ 0): a
    scalar, a host array or MeshField, or a ROCMeshField.  Conjugate gradients from `u0` (zero without one) until
    ‖r‖₂ ≤ rtol·‖b_free‖₂, preconditioned by one multigrid V-cycle (precond="mg") or by the diagonal ("jacobi").  Returns an
    EllipticSolution.  Raises ValueError / TypeError for what is refused (1-D, a band field, a slab or a field with a comm, a
    PeriodicBC dimension, fewer than 3 nodes in a dimension, coefficients that are not finite and positive, c < 0, no fixed node
    with c ≡ 0, non-finite data) and LsmNotConvergedError when max_iters does not suffice.  For repeated solves keep an
    EllipticOperator."""
    op = EllipticOperator(phi_or_eq, a_in=a_in, a_out=a_out, a=a, c=c, dirichlet=dirichlet, level=level, precond=precond)
    try:
        return op.solve(f, u0=u0, rtol=rtol, max_iters=max_iters)
    except BaseException:
        op.close()
        raise


def elliptic_solve_many(phi_or_eq, fs, *, a_in=1.0, a_out=1e-3, a=None, c=0.0, dirichlet=None, u0=None, homogeneous=None, level=0.0, rtol=1e-8, max_iters=500,
                        precond="mg"):
    """elliptic_solve for K ≤ 8 sources `fs` of the one structure, solved together on the device (EllipticOperator.solve_many): several
    load cases of a thermal compliance design, or a state and its adjoint (homogeneous=(False, True)) whose mutual_energy_density is the
    speed of an objective l·u — a sensor temperature, a mean over a region.  Returns an EllipticMultiSolution; the other arguments are
    elliptic_solve's."""
    op = EllipticOperator(phi_or_eq, a_in=a_in, a_out=a_out, a=a, c=c, dirichlet=dirichlet, level=level, precond=precond)
    try:
        return op.solve_many(fs, u0=u0, homogeneous=homogeneous, rtol=rtol, max_iters=max_iters)
    except BaseException:
        op.close()
        raise


def regularize_(g, alpha, rtol=1e-8, max_iters=500):
    """Replace the device field g by the solution V of (I − α²Δ)V = g with zero-flux faces, in place: the H¹ regularisation of a
    shape gradient (a velocity that is smooth over the length α).  One elliptic_solve with a = α², c = 1, f = g, from the guess
    g.  Returns the EllipticSolution (its u is a new field; g holds the same values)."""
    alpha = float(alpha)
    if not (alpha > 0 and math.isfinite(alpha)):
        raise ValueError("regularize_: alpha must be positive and finite")
    g = _elliptic_field(g, "regularize_")
    sol = elliptic_solve(g, g, a=alpha * alpha, c=1.0, u0=g, rtol=rtol, max_iters=max_iters)
    g.copy_(sol.u)
    sol.operator.close()
    return sol


# ----------------------------------------------------------------------------- elasticity solves (the state equation of a structural optimisation)

_PLANES = {"stress": L.PLANE_STRESS, "strain": L.PLANE_STRAIN}
_ELASTIC_REFUSALS = {1: "phi must be finite", 2: "the cell moduli must be finite and positive",
                     4: "component {detail} has no fixed bit anywhere (its translation is in the null space)", 5: "every component of every node is fixed"}


def _component_values(v, N, n, what):
    """the (N,)+n host array behind a scalar, an N-tuple of scalars / arrays, or an array of shape (N,)+n"""
    if isinstance(v, (tuple, list)):
        if len(v) != N:
            raise ValueError(f"{what} has {len(v)} components, the grid has {N} dimensions")
        return np.stack([np.broadcast_to(np.asarray(c.vals if isinstance(c, MeshField) else c, dtype=np.float64), n) for c in v])
    a = np.asarray(v, dtype=np.float64)
    if a.ndim == 0:
        return np.broadcast_to(a, (N,) + n)
    if a.shape != (N,) + n:
        raise ValueError(f"{what} has shape {a.shape}, expected {(N,) + n} (or {N} components)")
    return a


class ElasticitySolution:
    """elasticity_solve's result: `u` (a tuple of N ROCMeshFields on ϕ's backend), `iterations`, `relres` (the recursive
    ‖r‖₂/‖b_free‖₂), `levels` of the hierarchy; energy_density(): the ROCMeshField of e_I = the mean over the cells around I of
    E_C·(C₀ε:ε averaged over the cell) — the integrand of the compliance shape derivative, the normal speed of a compliance
    descent (coeff.set_values takes it device to device); compliance() = ∏h·Σ b·u, reduced on the device.  Stress recovery
    (DESIGN.md §7.20): strain(), stress() (tuples of ROCMeshFields in Voigt order), von_mises(), stress_max(), stress_norm(p, sref),
    stress_sensitivity(p, sref, rtol, max_iters) → StressSensitivity.  topological_derivative(): the ROCMeshField T that nucleate_ takes
    (DESIGN.md §7.21)."""

    def __init__(self, op, u, f, iterations, relres):
        self.operator, self.u, self._f, self.iterations, self.relres, self.levels = op, tuple(u), f, int(iterations), float(relres), op.levels

    def energy_density(self):
        op = self.operator
        e = ROCMeshField(op.backend, self.u[0].mesh, self.u[0].bcs)
        op.backend.elastic_energy(op._handle(), [c.buf for c in self.u], e.buf)
        return e

    def mutual_energy_density(self, other):
        """the ROCMeshField of m_I = the mean over the cells around I of E_C·(C₀ε(u):ε(v) averaged over the cell), v = other.u: the
        integrand of the shape derivative of l·u for this state and the adjoint `other` (K v = l) of the same operator (DESIGN.md
        §7.25).  With other = self it is energy_density() bit for bit."""
        op = self.operator
        if not isinstance(other, ElasticitySolution) or other.operator is not op:
            raise ValueError("mutual_energy_density: the other solution belongs to another operator")
        e = ROCMeshField(op.backend, self.u[0].mesh, self.u[0].bcs)
        op.backend.elastic_energy_mutual(op._handle(), [c.buf for c in self.u], [c.buf for c in other.u], e.buf)
        return e

    def compliance(self):
        op = self.operator
        if self._f is None:
            raise ValueError("elasticity_solve: this displacement came without a load (with_displacement): it has no compliance")
        return op.backend.elastic_compliance(op._handle(), self._f, [c.buf for c in self.u])

    # ---- stress recovery: cell-mean values at the centroids, node fields their means over the cells around a node
    def _stress_fields(self, what, count):
        op = self.operator
        h = op._handle()
        out = tuple(ROCMeshField(op.backend, self.u[0].mesh, self.u[0].bcs) for _ in range(count))
        op.backend.elastic_stress(h, [c.buf for c in self.u], what, [c.buf for c in out])
        return out

    def strain(self):
        """the strain as N(N+1)/2 ROCMeshFields in Voigt order — 2-D (00, 11, 01), 3-D (00, 11, 22, 12, 02, 01) — with engineering shears"""
        N = self.operator.ndim
        return self._stress_fields(L.STRESS_STRAIN, N * (N + 1) // 2)

    def stress(self):
        """the stress E_C·C₀:ε as N(N+1)/2 ROCMeshFields in Voigt order; the ersatz modulus relaxes it in the void"""
        N = self.operator.ndim
        return self._stress_fields(L.STRESS_STRESS, N * (N + 1) // 2)

    def von_mises(self):
        """the von Mises stress (with the out-of-plane normal stress in plane strain) as one ROCMeshField"""
        return self._stress_fields(L.STRESS_VON_MISES, 1)[0]

    def topological_derivative(self):
        """the topological derivative of the compliance as one ROCMeshField: a small traction-free hole of volume
        v around x raises compliance() by about T(x)·v.  T ≥ 0; nucleate_ punches holes where it is lowest."""
        op = self.operator
        h = op._handle()
        out = ROCMeshField(op.backend, self.u[0].mesh, self.u[0].bcs)
        op.backend.elastic_topo(h, [c.buf for c in self.u], out.buf)
        return out

    def stress_max(self):
        """the largest von Mises stress of a cell"""
        op = self.operator
        h = op._handle()
        return op.backend.elastic_stress_norm(h, [c.buf for c in self.u], 2.0, 1.0)[1]

    def _stress_norm(self, p, sref):
        """(G_p, J′, sref) after the refusals; a zero state gives (0, 0, sref) and no aggregate is formed"""
        op = self.operator
        p, sref = _stress_args(p, sref)
        h = op._handle()
        if sref is None:
            sref = self.stress_max()
            if sref == 0.0:
                return 0.0, 0.0, sref
            if not math.isfinite(sref):
                raise ValueError("stress_norm: the displacement must be finite")
        J, _ = op.backend.elastic_stress_norm(h, [c.buf for c in self.u], p, sref)
        vol = float(np.prod(self.u[0].mesh.meshsize()))
        return sref * (vol * J) ** (1.0 / p), J, sref

    def stress_norm(self, p=8.0, sref=None):
        """the p-norm of the von Mises stress, G_p = sref·(∏h·Σ_C (s_C/sref)^p)^(1/p), 2 ≤ p ≤ 64, reduced on the device; sref (the
        largest cell stress without one) only scales the powers"""
        return self._stress_norm(p, sref)[0]

    def stress_sensitivity(self, p=8.0, sref=None, rtol=1e-8, max_iters=500):
        """G_p and its sensitivity: one adjoint solve A λ = ∂J′/∂u with the same operator and zero values on the fixed components, then
        the node field E_C·∂G_p/∂E_C averaged over the cells around a node — energy_density()'s convention, positive where more
        material raises G_p; a NormalMotionTerm speed through coeff.set_values.  Returns a StressSensitivity."""
        op = self.operator
        rtol = float(rtol)
        if not (rtol > 0 and math.isfinite(rtol)) or int(max_iters) < 1:
            raise ValueError("stress_sensitivity: rtol must be positive and finite, max_iters at least 1")
        value, J, sref_used = self._stress_norm(p, sref)
        b = op.backend
        h = op._handle()
        p = float(p)
        field = ROCMeshField(b, self.u[0].mesh, self.u[0].bcs)
        if J == 0.0:      # no stress anywhere: nothing to differentiate
            return StressSensitivity(0.0, field, None, 0, p, sref_used)
        if not math.isfinite(J):
            raise ValueError("stress_sensitivity: the aggregate is not finite (a non-finite displacement, or sref too small for p)")
        ubufs = [c.buf for c in self.u]
        load = b.elastic_stress_load(h, ubufs, p, sref_used)
        lam = op._fields(None, fixed="zero")
        it, rel = b.elastic_solve(h, load, [c.buf for c in lam], rtol, int(max_iters))
        adjoint = ElasticitySolution(op, lam, load, it, rel)
        b.elastic_stress_sensitivity(h, ubufs, [c.buf for c in lam], p, sref_used, value / (p * J), field.buf)
        return StressSensitivity(value, field, adjoint, it, p, sref_used)


class ElasticityMultiSolution:
    """solve_many's result: a sequence of K ElasticitySolutions of one operator (len, indexing, iteration), each with its own u,
    iterations, relres and load, so that compliance(), the stress recovery, topological_derivative() and stress_sensitivity() work on
    a column.  `iterations` and `relres` are tuples, `operator` and `levels` as on a single solution.  compliances() → the K values;
    compliance(weights=None) = Σ w_k·c_k (weights default to 1); cross_compliance(i, j) = ∏h·Σ (m·f_i)·u_j; energy_density(weights=None)
    → the ROCMeshField of Σ_k w_k·e_k in one pass over the grid; mutual_energy_density(i, j) → that of columns i and j."""

    def __init__(self, op, columns):
        self.operator, self._columns, self.levels = op, tuple(columns), op.levels
        self.iterations = tuple(c.iterations for c in self._columns)
        self.relres = tuple(c.relres for c in self._columns)

    def __len__(self):
        return len(self._columns)

    def __getitem__(self, k):
        return self._columns[k]

    def __iter__(self):
        return iter(self._columns)

    def _weights(self, weights, what):
        K = len(self._columns)
        w = [1.0] * K if weights is None else [float(v) for v in weights]
        if len(w) != K:
            raise ValueError(f"{what}: {len(w)} weights for {K} columns")
        if not all(math.isfinite(v) for v in w):
            raise ValueError(f"{what}: the weights must be finite")
        return w

    def compliances(self):
        return tuple(c.compliance() for c in self._columns)

    def compliance(self, weights=None):
        w = self._weights(weights, "compliance")
        total = 0.0
        for wk, ck in zip(w, self.compliances()):
            total = total + wk * ck
        return total

    def cross_compliance(self, i, j):
        op = self.operator
        return op.backend.elastic_compliance(op._handle(), self._columns[i]._f, [c.buf for c in self._columns[j].u])

    def energy_density(self, weights=None):
        op = self.operator
        w = self._weights(weights, "energy_density")
        u0 = self._columns[0].u[0]
        e = ROCMeshField(op.backend, u0.mesh, u0.bcs)
        op.backend.elastic_energy_many(op._handle(), [[c.buf for c in col.u] for col in self._columns], w, e.buf)
        return e

    def mutual_energy_density(self, i, j):
        return self._columns[i].mutual_energy_density(self._columns[j])


def _stress_args(p, sref):
    """the refusals of the stress aggregate that need no device"""
    p = float(p)
    if not (math.isfinite(p) and 2.0 <= p <= 64.0):
        raise ValueError(f"stress_norm: p must be finite with 2 <= p <= 64, not {p}")
    if sref is not None:
        sref = float(sref)
        if not _finite_positive(sref):
            raise ValueError("stress_norm: sref must be finite and positive")
    return p, sref


class StressSensitivity:
    """stress_sensitivity's result: `value` (G_p), `field` (the ROCMeshField of E_C·∂G_p/∂E_C averaged over the cells around a node),
    `adjoint` (the ElasticitySolution of the adjoint solve; None for a zero state), `iterations` of that solve, `p`, `sref`."""

    def __init__(self, value, field, adjoint, iterations, p, sref):
        self.value, self.field, self.adjoint, self.iterations, self.p, self.sref = float(value), field, adjoint, int(iterations), float(p), float(sref)


class ElasticityOperator:
    """The discrete Q1 elasticity operator of ϕ's grid and its multigrid hierarchy, kept on the device for repeated solves with
    new loads and guesses: solve(f, u0=None, rtol=1e-8, max_iters=500) → ElasticitySolution.  The arguments are
    elasticity_solve's.  ϕ is read once, here: after ϕ has moved, build a new operator.  `levels`, `free_dofs`, `fixed_dofs`;
    apply(x), cells(), stiffness(level) show the operator; modes(m, …) → ElasticityModes, its lowest vibration modes;
    with_displacement(u) → an ElasticitySolution around a given u, for the stress recovery; close() releases the device memory."""

    def __init__(self, phi_or_eq, *, E_in=1.0, E_out=1e-3, E=None, nu=0.3, plane="stress", dirichlet=None, level=0.0, precond="mg"):
        what = "elasticity_solve"
        self._h = None
        if precond not in _PRECONDS:
            raise ValueError(f'{what}: precond must be "mg" or "jacobi", not {precond!r}')
        if plane not in _PLANES:
            raise ValueError(f'{what}: plane must be "stress" or "strain", not {plane!r}')
        nu = float(nu)
        if not (math.isfinite(nu) and -1.0 < nu < 0.5):
            raise ValueError(f"{what}: nu must be finite with -1 < nu < 0.5")
        E_host = None if E is None or hasattr(E, "is_cuda") else np.asarray(E, dtype=np.float64)
        if E is None:
            if not (_finite_positive(float(E_in)) and _finite_positive(float(E_out))):
                raise ValueError(f"{what}: E_in and E_out must be finite and positive")
            if not math.isfinite(float(level)):
                raise ValueError(f"{what}: level must be finite")
        elif E_host is not None and not _finite_positive(E_host):
            raise ValueError(f"{what}: the cell moduli `E` must be finite and positive")
        mask = values = None
        if dirichlet is not None:
            if not (isinstance(dirichlet, (tuple, list)) and len(dirichlet) == 2):
                raise TypeError(f"{what}: dirichlet must be a pair (mask, values)")
            mask = np.asarray(dirichlet[0])
            if mask.dtype != np.bool_:
                raise TypeError(f"{what}: the Dirichlet mask must be a boolean array")
        phi = _elliptic_field(phi_or_eq, what)
        n = tuple(int(m) for m in phi.mesh.n)
        N = len(n)
        if mask is not None:
            if mask.shape == n:
                mask = np.broadcast_to(mask[..., None], n + (N,))
            elif mask.shape != n + (N,):
                raise ValueError(f"{what}: the Dirichlet mask has shape {mask.shape}, expected {n} or {n + (N,)}")
            values = _component_values(dirichlet[1], N, n, f"{what}: the Dirichlet values")
            if not np.all(np.isfinite(values)):
                raise ValueError(f"{what}: the Dirichlet values must be finite")
        for i in range(N):
            if mask is None or not mask[..., i].any():
                raise ValueError(f"{what}: component {i} has no fixed bit anywhere: its translation is in the null space")
        if mask.all():
            raise ValueError(f"{what}: every component of every node is fixed")
        cells = tuple(m - 1 for m in n)
        if E_host is not None and E_host.ndim and E_host.shape != cells:
            raise ValueError(f"{what}: `E` has shape {E_host.shape}, the grid has {cells} cells")
        b = self.backend = phi.backend
        self.mesh, self.bcs, self.precond, self.ndim = phi.mesh, phi.bcs, precond, N
        t = b.torch
        E_dev = None if E is None else b.node_array(E if E_host is None else E_host, "E", cells)
        bits = np.zeros(n, dtype=np.uint8)
        for i in range(N):
            bits |= mask[..., i].astype(np.uint8) << np.uint8(i)
        self._mask = [t.from_numpy(np.array(mask[..., i].T, order="C")).to(b.device) for i in range(N)]      # the interior view's axis order
        self._values = [t.from_numpy(np.array(values[i].T, order="C")).to(b.device) for i in range(N)]
        fixed = t.from_numpy(np.array(bits.reshape(-1, order="F"))).to(b.device)
        try:
            self._h, stats = b.elastic_create(None if E is not None else phi.buf, level, E_in, E_out, E_dev, nu, _PLANES[plane], fixed, _PRECONDS[precond])
        except L.LsmError as e:
            why = _ELASTIC_REFUSALS.get(getattr(e, "reason", 0))
            if why is None:
                raise
            raise ValueError(f"{what}: " + why.format(detail=getattr(e, "detail", 0))) from None
        self.levels, self.free_dofs, self.fixed_dofs = stats[0], stats[1], stats[2]
        self._phi, self._level = (None if E is not None else phi), float(level)      # the density of modes() is read from the same ϕ

    def modes(self, m, *, rho_in=1.0, rho_out=1e-6, rho=None, x0=None, rtol=1e-6, max_iters=300):
        """the m smallest eigenpairs of K u = λ M u for this operator (the fixed components zero): an ElasticityModes.  See elasticity_modes."""
        return ElasticityModes(self, m, rho_in=rho_in, rho_out=rho_out, rho=rho, x0=x0, rtol=rtol, max_iters=max_iters)

    def _handle(self):
        if self._h is None:
            raise ValueError("the ElasticityOperator is closed")
        return self._h

    def _fields(self, u0, fixed="prescribed", what="elasticity_solve: u0"):
        """N new fields holding the guess (zero without one) and, on the fixed components, the prescribed values
        (fixed="prescribed"), zero ("zero": an adjoint solve) or the guess's own values ("keep": with_displacement)"""
        b, N = self.backend, self.ndim
        n = tuple(int(m) for m in self.mesh.n)
        if u0 is not None and not (isinstance(u0, (tuple, list)) and all(isinstance(c, ROCMeshField) for c in u0)):
            u0 = list(_component_values(u0, N, n, what))
        if u0 is not None and len(u0) != N:
            raise ValueError(f"{what} has {len(u0)} components, the grid has {N} dimensions")
        out = []
        for i in range(N):
            u = ROCMeshField(b, self.mesh, self.bcs)
            if u0 is not None:
                if isinstance(u0[i], ROCMeshField) and u0[i].backend is not b:
                    raise ValueError(f"{what} belongs to another field's backend")
                u.copy_(u0[i])
            if fixed != "keep":
                iv = b.interior(u.buf)
                vals = self._values[i].to(iv.dtype) if fixed == "prescribed" else b.torch.zeros_like(iv)
                iv.copy_(b.torch.where(self._mask[i], vals, iv))
            out.append(u)
        return out

    def with_displacement(self, u):
        """An ElasticitySolution around displacements from elsewhere, without a solve: the entry to strain(), stress(), von_mises(),
        stress_norm() and stress_sensitivity() for a given u — N host arrays, an array of shape (N,)+n, or N ROCMeshFields (copied).
        It has no load, so compliance() raises."""
        self._handle()
        if u is None:
            raise ValueError("with_displacement: u must be given")
        return ElasticitySolution(self, self._fields(u, fixed="keep", what="with_displacement: u"), None, 0, 0.0)

    def _load(self, f):
        """f as one flat float64 device array, component-major"""
        b, N = self.backend, self.ndim
        t = b.torch
        n = tuple(int(m) for m in self.mesh.n)
        if t.is_tensor(f):
            return b.node_array(f, "f", (N,) + n)
        if isinstance(f, (tuple, list)) and len(f) == N and all(isinstance(c, ROCMeshField) for c in f):
            return t.cat([b.interior(c.buf).to(t.float64).contiguous().reshape(-1) for c in f])
        v = _component_values(f, N, n, "elasticity_solve: f")
        return t.from_numpy(np.concatenate([v[i].reshape(-1, order="F") for i in range(N)])).to(b.device)

    def solve(self, f, u0=None, rtol=1e-8, max_iters=500):
        b = self.backend
        h = self._handle()
        rtol = float(rtol)
        if not (rtol > 0 and math.isfinite(rtol)) or int(max_iters) < 1:
            raise ValueError("elasticity_solve: rtol must be positive and finite, max_iters at least 1")
        fd = self._load(f)
        u = self._fields(u0)
        try:
            it, rel = b.elastic_solve(h, fd, [c.buf for c in u], rtol, int(max_iters))
        except L.LsmNotConvergedError:
            raise
        except L.LsmError as e:
            if "must be finite" in str(e):
                raise ValueError("elasticity_solve: f, u0 and the Dirichlet values must be finite") from None
            raise
        return ElasticitySolution(self, u, fd, it, rel)

    def solve_many(self, fs, u0=None, homogeneous=None, rtol=1e-8, max_iters=500):
        """K = len(fs) ≤ 8 load cases of this operator in one batched solve → ElasticityMultiSolution.  Column k is solve(fs[k], u0[k]) bit
        for bit: u, iterations and relres.  `fs`: a sequence of loads, each in any form solve takes; `u0`: None or a
        sequence of guesses (an entry may be None); `homogeneous`: a sequence of booleans — a true column takes zero on the fixed
        components instead of the prescribed values (an adjoint column).  Unless every column converges nothing is kept:
        LsmNotConvergedError carries .iterations, .relres and .status (1 converged, 2 out of iterations, −2 / −3 breakdown) tuples;
        ValueError for what is refused and for non-finite data, naming the column."""
        b = self.backend
        h = self._handle()
        what = "elasticity_solve_many"
        rtol = float(rtol)
        if not (rtol > 0 and math.isfinite(rtol)) or int(max_iters) < 1:
            raise ValueError(f"{what}: rtol must be positive and finite, max_iters at least 1")
        if not isinstance(fs, (tuple, list)):
            raise TypeError(f"{what}: fs must be a sequence of loads")
        K = len(fs)
        if not 1 <= K <= b.ELASTIC_MAXCOLS:
            raise ValueError(f"{what}: {K} load cases (1 to {b.ELASTIC_MAXCOLS} are solved together)")
        u0 = [None] * K if u0 is None else list(u0)
        homogeneous = [False] * K if homogeneous is None else [bool(v) for v in homogeneous]
        if len(u0) != K or len(homogeneous) != K:
            raise ValueError(f"{what}: u0 and homogeneous must have one entry per load case ({K})")
        fds = [self._load(f) for f in fs]
        us = [self._fields(u0[k], fixed="zero" if homogeneous[k] else "prescribed", what=f"{what}: u0[{k}]") for k in range(K)]
        try:
            its, rels, _ = b.elastic_solve_many(h, b.torch.cat(fds), [[c.buf for c in u] for u in us], rtol, int(max_iters))
        except L.LsmNotConvergedError:
            raise
        except L.LsmError as e:
            if "must be finite" in str(e):
                col = [k for k, v in enumerate(getattr(e, "status", ())) if v == -1]
                raise ValueError(f"{what}: f, u0 and the Dirichlet values must be finite (column {col[0] if col else '?'})") from None
            raise
        return ElasticityMultiSolution(self, [ElasticitySolution(self, us[k], fds[k], its[k], rels[k]) for k in range(K)])

    def apply(self, x):
        """A x on all components, no elimination: x a host array of shape (N,)+n; returns one (for tests and diagnostics)"""
        b, N = self.backend, self.ndim
        n = tuple(int(m) for m in self.mesh.n)
        nn = int(np.prod(n))
        y = b.elastic_apply(self._handle(), self._load(np.asarray(x, dtype=np.float64))).cpu().numpy()
        return np.stack([y[i * nn:(i + 1) * nn].reshape(n, order="F") for i in range(N)])

    def cells(self):
        """the level-0 cell moduli, a host array of shape n − 1"""
        n = tuple(int(m) - 1 for m in self.mesh.n)
        return self.backend.elastic_cells(self._handle()).cpu().numpy().reshape(n, order="F")

    def stiffness(self, level=0):
        """the unit element matrix K0 of a level as the device holds it: (2^N·N)², row a·N + i"""
        return self.backend.elastic_stiffness(self._handle(), level)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            try:
                self.backend.elastic_destroy(h)
            except Exception:
                pass

    __del__ = close


def elasticity_solve(phi_or_eq, f, *, E_in=1.0, E_out=1e-3, E=None, nu=0.3, plane="stress", dirichlet=None, u0=None, level=0.0, rtol=1e-8, max_iters=500,
                     precond="mg"):
    """Solve −∇·σ(u) = f, σ = E(x)·C₀(ν):ε(u), on the box of ϕ's grid, on the device: the state equation of a structural level-set
    shape optimisation with an ersatz material.  Q1 elements, the N displacement components at the nodes,
    traction-free faces.  The modulus of a cell is E_out + (E_in − E_out)·θ with elliptic_solve's fill fraction θ; `E` (a scalar
    or an array of shape n − 1) gives the cell moduli directly and ϕ is not read.  `plane` ("stress" or "strain") matters in 2-D
    only.  `dirichlet=(mask, g)` fixes displacement components: the mask is a boolean array of the grid's shape (all components
    of those nodes) or of shape n + (N,) (component by component: rollers, symmetry planes); g a scalar, an N-tuple or an array of
    shape (N,) + n.  Every component needs a fixed bit somewhere, and the set must not leave a rotation free.  `f`: N host arrays
    (or scalars), an array of shape (N,) + n, or N ROCMeshFields; a uniform traction t on a face normal to d is f = 2t/h_d on that
    face's nodes.  Conjugate gradients from `u0` (zero without one) until ‖r‖₂ ≤ rtol·‖b_free‖₂, preconditioned by one multigrid
    V-cycle (precond="mg") or by the diagonal ("jacobi").  Returns an ElasticitySolution.  Raises ValueError / TypeError for
    what is refused (1-D, a band field, a slab, a PeriodicBC dimension, fewer than 3 nodes in a dimension, moduli that are not
    finite and positive, ν outside (−1, 0.5), an unknown plane, a component that is fixed nowhere, everything fixed, non-finite
    data) and LsmNotConvergedError when max_iters does not suffice.  For repeated solves keep an ElasticityOperator."""
    op = ElasticityOperator(phi_or_eq, E_in=E_in, E_out=E_out, E=E, nu=nu, plane=plane, dirichlet=dirichlet, level=level, precond=precond)
    try:
        return op.solve(f, u0=u0, rtol=rtol, max_iters=max_iters)
    except BaseException:
        op.close()
        raise


def elasticity_solve_many(phi_or_eq, fs, *, E_in=1.0, E_out=1e-3, E=None, nu=0.3, plane="stress", dirichlet=None, u0=None, homogeneous=None, level=0.0,
                          rtol=1e-8, max_iters=500, precond="mg"):
    """elasticity_solve for K ≤ 8 load cases `fs` of the one structure, solved together on the device (ElasticityOperator.solve_many):
    several load cases of a compliance design, or a state and its adjoint (homogeneous=(False, True)) whose mutual_energy_density is
    the speed of a displacement objective.  Returns an ElasticityMultiSolution; the other arguments are elasticity_solve's."""
    op = ElasticityOperator(phi_or_eq, E_in=E_in, E_out=E_out, E=E, nu=nu, plane=plane, dirichlet=dirichlet, level=level, precond=precond)
    try:
        return op.solve_many(fs, u0=u0, homogeneous=homogeneous, rtol=rtol, max_iters=max_iters)
    except BaseException:
        op.close()
        raise


# ----------------------------------------------------------------------------- thermoelastic coupling (heat state → thermal load → structure)

class ThermoelasticSensitivity:
    """ThermoelasticSolution.sensitivity's result: `value` (∏h·Σ b_l·u, compliance()'s scaling), `field` (the ROCMeshField d: the integrand
    of the shape derivative of l·u in energy_density()'s convention), `adjoint` (the ElasticitySolution of A v = b_l), `heat_adjoint`
    (the EllipticSolution w of the heat adjoint; None when T was given), `iterations` and `heat_iterations` of the two adjoint solves."""

    def __init__(self, value, field, adjoint, heat_adjoint, iterations, heat_iterations):
        self.value, self.field, self.adjoint, self.heat_adjoint = float(value), field, adjoint, heat_adjoint
        self.iterations, self.heat_iterations = int(iterations), int(heat_iterations)


class ThermoelasticSolution:
    """Thermoelastic.solve's result: `temperature` (the EllipticSolution of the heat state; None when T was given), `T` (the temperature
    ROCMeshField), `displacement` (the ElasticitySolution of A u = b_m + b_th(T)), `coupling` (the Thermoelastic).  stress() and
    von_mises() are ElasticitySolution's with the thermal strain taken off: every normal stress loses E_C·α_C·β·θ_C (β = 1/(1−2ν), or
    1/(1−ν) in plane stress), the out-of-plane one of plane strain included; the shears and the strain are the displacement's.  The
    von Mises stress therefore differs from displacement.von_mises() in plane stress only.  sensitivity(l) → ThermoelasticSensitivity."""

    def __init__(self, coupling, temperature, T, displacement):
        self.coupling, self.temperature, self.T, self.displacement = coupling, temperature, T, displacement

    def _stress_fields(self, what, count):
        c, u = self.coupling, self.displacement.u
        op = c.elastic
        out = tuple(ROCMeshField(op.backend, u[0].mesh, u[0].bcs) for _ in range(count))
        op.backend.elastic_thermal_stress(op._handle(), [x.buf for x in u], self.T.buf, c.T_ref, c._alpha, what, [x.buf for x in out])
        return out

    def stress(self):
        """the stress E_C·(C₀:ε − α_C·β·θ_C·I) as N(N+1)/2 ROCMeshFields in Voigt order"""
        N = self.coupling.elastic.ndim
        return self._stress_fields(L.STRESS_STRESS, N * (N + 1) // 2)

    def von_mises(self):
        """the von Mises stress of stress() (with the out-of-plane normal stress in plane strain) as one ROCMeshField"""
        return self._stress_fields(L.STRESS_VON_MISES, 1)[0]

    def sensitivity(self, l, rtol=1e-8, max_iters=500):
        """The objective l·u (l in any form ElasticityOperator.solve takes a load) and its sensitivity for the coupled problem in which one
        ϕ gives both the conductivity and the modulus: the elastic adjoint A v = b_l (zero on the fixed components),
        the heat adjoint w whose source is ∂(v·b_th)/∂T (zero on the Dirichlet nodes), then one fused pass:
        d = mean over the cells around a node of E_C·(t_C·tr_C(v) − q_C(u, v)) − a∇T·∇w — energy_density()'s convention, a
        NormalMotionTerm speed through coeff.set_values.  When T was given the temperature does not depend on the design: no heat
        adjoint is run and nothing is subtracted.  Returns a ThermoelasticSensitivity."""
        c = self.coupling
        eop, hop = c.elastic, c.heat
        rtol = float(rtol)
        if not (rtol > 0 and math.isfinite(rtol)) or int(max_iters) < 1:
            raise ValueError("thermoelastic sensitivity: rtol must be positive and finite, max_iters at least 1")
        b, h = eop.backend, eop._handle()
        ubufs = [x.buf for x in self.displacement.u]
        ld = eop._load(l)
        v = eop._fields(None, fixed="zero")
        vbufs = [x.buf for x in v]
        it, rel = b.elastic_solve(h, ld, vbufs, rtol, int(max_iters))
        adjoint = ElasticitySolution(eop, v, ld, it, rel)
        value = b.elastic_compliance(h, ld, ubufs)
        heat_adjoint, minus, itw = None, None, 0
        if self.temperature is not None:
            src = b.elastic_thermal_source(h, vbufs, c._alpha)
            w = hop._field(None, homogeneous=True)
            itw, relw = b.elliptic_solve(hop._handle(), src, w.buf, rtol, int(max_iters))
            heat_adjoint = EllipticSolution(hop, w, src, itw, relw)
            minus = self.temperature.mutual_energy_density(heat_adjoint)
        field = ROCMeshField(b, self.T.mesh, self.T.bcs)
        b.elastic_thermal_sensitivity(h, ubufs, vbufs, self.T.buf, c.T_ref, c._alpha, None if minus is None else minus.buf, field.buf)
        return ThermoelasticSensitivity(value, field, adjoint, heat_adjoint, it, itw)


class Thermoelastic:
    """The coupling of a heat problem and a structure on one grid: `heat` an EllipticOperator, `elastic` an
    ElasticityOperator of the same backend and mesh (both built from the one ϕ), `alpha` the expansion coefficient (a scalar or a
    cell array of shape n − 1), `T_ref` the stress-free temperature.  thermal_load(T) → the load of the eigenstress E·C₀:(α(T − T_ref)I)
    as ElasticityOperator.solve takes it; solve(q, f) → ThermoelasticSolution.  The operators are borrowed; close() closes both."""

    def __init__(self, heat_op, elastic_op, *, alpha, T_ref=0.0):
        what = "Thermoelastic"
        if not isinstance(heat_op, EllipticOperator) or not isinstance(elastic_op, ElasticityOperator):
            raise TypeError(f"{what} takes an EllipticOperator and an ElasticityOperator")
        if heat_op.backend is not elastic_op.backend:
            raise ValueError(f"{what}: the two operators must share a backend (build both from the same ϕ)")
        if tuple(int(m) for m in heat_op.mesh.n) != tuple(int(m) for m in elastic_op.mesh.n) or \
                tuple(heat_op.mesh.meshsize()) != tuple(elastic_op.mesh.meshsize()):
            raise ValueError(f"{what}: the two operators must share a mesh")
        T_ref = float(T_ref)
        if not math.isfinite(T_ref):
            raise ValueError(f"{what}: T_ref must be finite")
        b = elastic_op.backend
        cells = tuple(int(m) - 1 for m in elastic_op.mesh.n)
        if b.torch.is_tensor(alpha):
            self._alpha = b.node_array(alpha, "alpha", cells)
        else:
            a = np.asarray(alpha, dtype=np.float64)
            if not np.all(np.isfinite(a)):
                raise ValueError(f"{what}: alpha must be finite")
            if a.ndim and a.shape != cells:
                raise ValueError(f"{what}: alpha has shape {a.shape}, the grid has {cells} cells")
            self._alpha = b.node_array(a, "alpha", cells) if a.ndim else float(a)
        self.heat, self.elastic, self.T_ref, self.backend = heat_op, elastic_op, T_ref, b

    def _temperature(self, T):
        """T as a ROCMeshField of the operators' backend: one is taken as it is, a scalar / host array / MeshField is uploaded"""
        b = self.backend
        if isinstance(T, EllipticSolution):
            T = T.u
        if isinstance(T, ROCMeshField):
            if T.backend is not b or isinstance(T, ROCNarrowBandMeshField):
                raise ValueError("Thermoelastic: T must be a dense field of the operators' backend")
            return T
        out = ROCMeshField(b, self.elastic.mesh, self.elastic.bcs)
        out.copy_(np.broadcast_to(_host_values(T), tuple(int(m) for m in self.elastic.mesh.n)))
        return out

    def thermal_load(self, T):
        """f_th as a flat float64 device tensor, component-major: elastic.solve(f_th) is the structure under the thermal load alone"""
        return self.backend.elastic_thermal_load(self.elastic._handle(), self._temperature(T).buf, self.T_ref, self._alpha)

    def solve(self, q=None, f=None, *, T=None, rtol=1e-8, max_iters=500):
        """The heat state heat.solve(q) (or the given temperature T: a ROCMeshField, a scalar or a host array), its thermal load added
        to the mechanical load f (none without one) on the device, then the structure: bit for bit
        elastic.solve(f + thermal_load(T)).  Returns a ThermoelasticSolution."""
        if (q is None) == (T is None):
            raise ValueError("Thermoelastic.solve takes either the heat source q or the temperature T")
        temperature = None if T is not None else self.heat.solve(q, rtol=rtol, max_iters=max_iters)
        Tf = self._temperature(T if T is not None else temperature.u)
        fth = self.thermal_load(Tf)
        load = fth if f is None else self.elastic._load(f) + fth
        return ThermoelasticSolution(self, temperature, Tf, self.elastic.solve(load, rtol=rtol, max_iters=max_iters))

    def close(self):
        self.heat.close()
        self.elastic.close()


def thermoelastic_solve(phi_or_eq, q, f=None, *, alpha, T_ref=0.0, heat=None, elastic=None, rtol=1e-8, max_iters=500):
    """Thermoelastic.solve in one call: `heat` and `elastic` are the keyword arguments of EllipticOperator and ElasticityOperator
    (dirichlet=, a_in=, E_in=, nu=, plane=, …) for the one ϕ; q the heat source, f the mechanical load (or None), alpha the expansion
    coefficient, T_ref the stress-free temperature.  Returns a ThermoelasticSolution; its .coupling.close() releases both operators."""
    hop = EllipticOperator(phi_or_eq, **(heat or {}))
    eop = None
    try:
        eop = ElasticityOperator(phi_or_eq, **(elastic or {}))
        return Thermoelastic(hop, eop, alpha=alpha, T_ref=T_ref).solve(q, f, rtol=rtol, max_iters=max_iters)
    except BaseException:
        hop.close()
        if eop is not None:
            eop.close()
        raise


# ----------------------------------------------------------------------------- homogenisation (ϕ as one cell of a periodic material)

class _CellProblem:
    """What Homogenization and ConductivityHomogenization share: an operator on the torus of the grid's m = n − 1 cells per axis, its
    K cell problems and their correctors kept on the device (csrc/cell_problem.h).  A subclass gives
      _what, _prefix   its name in messages and the backend's method prefix
      _cells, _unit    what messages call the cell array and a cell problem's index
      _host_finite     solve_rhs and apply refuse non-finite host input here (or pass it to the device)
      _material, _lead its own construction checks (what they return goes to the backend's create) and the lead shape of all correctors"""

    def __init__(self, phi_or_eq, v_in, v_out, v, names, level, precond, **material):
        what, (n_in, n_out, n_v) = self._what, names
        self._h = None
        if precond not in _PRECONDS:
            raise ValueError(f'{what}: precond must be "mg" or "jacobi", not {precond!r}')
        material = self._material(**material)
        v_host = None if v is None or hasattr(v, "is_cuda") else np.asarray(v, dtype=np.float64)
        if v is None:
            if not (_finite_positive(float(v_in)) and _finite_positive(float(v_out))):
                raise ValueError(f"{what}: {n_in} and {n_out} must be finite and positive")
            if not math.isfinite(float(level)):
                raise ValueError(f"{what}: level must be finite")
        elif v_host is not None and not _finite_positive(v_host):
            raise ValueError(f"{what}: the {self._cells} `{n_v}` must be finite and positive")
        phi = phi_or_eq.current_state() if isinstance(phi_or_eq, LevelSetEquation) else phi_or_eq
        if not isinstance(phi, ROCMeshField):
            raise TypeError(f"{what} takes a device field (ROCMeshField) or a LevelSetEquation, not {type(phi).__name__}")
        if isinstance(phi, ROCNarrowBandMeshField):
            raise ValueError(f"{what} is not supported on NarrowBandMeshField: the cell problems are solved over the whole box. Use a full MeshField.")
        if phi.mesh.ndim == 1:
            raise ValueError(f"{what} of a 1 dimensional level-set is not supported: 2-D and 3-D fields only")
        if getattr(phi.backend, "slab", None) is not None:
            raise ValueError(f"{what} of a slab-decomposed field (a field with a comm) is not supported")
        n = tuple(int(m) for m in phi.mesh.n)
        if any(m < 3 for m in n):
            raise ValueError(f"{what} needs at least 2 cells (3 nodes) in every dimension")
        self.cells_shape = cells = tuple(m - 1 for m in n)
        if v_host is not None and v_host.ndim and v_host.shape != cells:
            raise ValueError(f"{what}: `{n_v}` has shape {v_host.shape}, the grid has {cells} cells")
        b = self.backend = phi.backend
        self.mesh, self.bcs, self.precond, self.ndim = phi.mesh, phi.bcs, precond, len(n)
        v_dev = None if v is None else b.node_array(v if v_host is None else v_host, n_v, cells)
        try:
            self._h, stats = getattr(b, f"{self._prefix}_create")(None if v is not None else phi.buf, level, v_in, v_out, v_dev, *material, _PRECONDS[precond])
        except L.LsmError as e:
            why = {1: "phi must be finite", 2: f"the {self._cells} must be finite and positive"}.get(getattr(e, "reason", 0))
            if why is None:
                raise
            raise ValueError(f"{what}: {why} ({getattr(e, 'detail', 0)} entries are not)") from None
        self.levels, self.free_dofs = stats[0], stats[1]
        K = self._lead()[0]
        self.iterations, self.relres, self._tensor = [0] * K, [0.0] * K, None

    def _material(self):
        return ()

    def _handle(self):
        if self._h is None:
            raise ValueError(f"the {type(self).__name__} is closed")
        return self._h

    def _call(self, name, *args):
        return getattr(self.backend, f"{self._prefix}_{name}")(self._handle(), *args)

    def _dev(self, v, lead, what, finite=True):
        """lead + m host values (or a device tensor of as many) as one flat float64 device array"""
        b = self.backend
        shape = tuple(lead) + self.cells_shape
        if b.torch.is_tensor(v):
            return b.node_array(v, what, shape)
        a = np.asarray(v, dtype=np.float64)
        if a.shape != shape:
            raise ValueError(f"{what} has shape {a.shape}, expected {shape}")
        if finite and not np.all(np.isfinite(a)):
            raise ValueError(f"{what} must be finite")
        flat = np.concatenate([r.reshape(-1, order="F") for r in a.reshape((-1,) + self.cells_shape)])
        return b.torch.from_numpy(flat).to(b.device)

    def _unflat(self, t, lead):
        """a flat device tensor as a host array of shape lead + m"""
        m = self.cells_shape
        v = t.cpu().numpy().reshape((-1, int(np.prod(m))))
        return np.stack([r.reshape(m, order="F") for r in v]).reshape(tuple(lead) + m)

    def _index(self, k, what=None):
        what = what or self._unit
        K = self._lead()[0]
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError(f"{self._what}: {what} must be an integer, not {type(k).__name__}")
        if not 0 <= int(k) < K:
            raise ValueError(f"{self._what}: {what} {k} of {K}")
        return int(k)

    def solve(self, chi0=None, rtol=1e-8, max_iters=500):
        """all correctors by PCG from chi0 (the shape of correctors(); zero without one).  A failure raises and leaves the stored
        correctors as they were."""
        self._handle()
        rtol = float(rtol)
        if not (rtol > 0 and math.isfinite(rtol)) or int(max_iters) < 1:
            raise ValueError(f"{self._what}: rtol must be positive and finite, max_iters at least 1")
        guess = None if chi0 is None else self._dev(chi0, self._lead(), f"{self._what}: chi0")
        self.iterations, self.relres = self._call("solve", guess, rtol, int(max_iters))
        self._tensor = None
        return self

    def solve_rhs(self, f, x0=None, rtol=1e-8, max_iters=500):
        """the same PCG for a right-hand side of the caller's, A x = f away from the pinned node 0: f and x0 host arrays of the shape
        of one corrector.  Returns (x, iterations, relres); the correctors are not touched (for diagnostics and tests of the V-cycle)."""
        lead = self._lead()[1:]
        fd = self._dev(f, lead, f"{self._what}: f", self._host_finite)
        xd = self._dev(np.zeros(lead + self.cells_shape) if x0 is None else x0, lead, f"{self._what}: x0", self._host_finite)
        it, rel = self._call("solve_rhs", fd, xd, float(rtol), int(max_iters))
        return self._unflat(xd, lead), it, rel

    def with_correctors(self, chi):
        """take correctors from elsewhere (the shape of correctors()), without a solve"""
        self._handle()
        self._call("set_correctors", self._dev(chi, self._lead(), "with_correctors: chi"))
        self._tensor = None
        return self

    @property
    def tensor(self):
        if self._tensor is None:
            self._tensor = self._call("tensor")
        return self._tensor

    def correctors(self):
        return self._unflat(self._call("correctors"), self._lead())

    def sensitivity(self, W):
        W = np.asarray(W, dtype=np.float64)
        K = self._lead()[0]
        if W.shape != (K, K) or not np.all(np.isfinite(W)) or not np.array_equal(W, W.T):
            raise ValueError(f"{self._what}: W must be a finite symmetric {K}×{K} matrix")
        g = ROCMeshField(self.backend, self.mesh, self.bcs)
        self._call("sensitivity", W, g.buf)
        return g

    def cells(self):
        return self._unflat(self._call("cells"), ())

    def apply(self, x):
        """A x on all components, no pin: x a host array of the shape of one corrector; returns one"""
        lead = self._lead()[1:]
        return self._unflat(self._call("apply", self._dev(x, lead, f"{self._what}: x", self._host_finite)), lead)

    def load(self, k):
        return self._unflat(self._call("load", self._index(k)), self._lead()[1:])

    def energy_cells(self, p, q):
        return self._unflat(self._call("energy_cells", self._index(p), self._index(q)), ())

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            try:
                getattr(self.backend, f"{self._prefix}_destroy")(h)
            except Exception:
                pass

    __del__ = close


class Homogenization(_CellProblem):
    """homogenize's result and its operator, kept on the device.  The torus has m = n − 1 nodes (and cells) per axis;
    M = N(N+1)/2 unit strains in Voigt order: 2-D (00, 11, 01), 3-D (00, 11, 22, 12, 02, 01), engineering shears.
    `tensor` ((M, M) numpy, exactly symmetric), `iterations` and `relres` (one entry per corrector), `levels`, `free_dofs`;
    corrector(k) → N ROCMeshFields (image nodes n − 1 from node 0); correctors() → host (M, N) + m; sensitivity(W) → the ROCMeshField
    of the integrand of d(W:C^H)/dΩ, a normal speed (coeff.set_values takes it device to device); cells(), apply(x), load(k),
    energy_cells(p, q), stiffness(level) show the operator; solve(chi0=None, rtol, max_iters) solves again (a warm start);
    with_correctors(chi) sets the correctors without a solve; close() releases the device memory.  ϕ is read once, at construction:
    after ϕ has moved, build a new object and pass the old correctors() as chi0."""
    _what, _prefix, _cells, _unit, _host_finite = "homogenize", "homog", "cell moduli", "the unit strain", False

    def __init__(self, phi_or_eq, *, E_in=1.0, E_out=1e-3, E=None, nu=0.3, plane="stress", level=0.0, precond="mg"):
        super().__init__(phi_or_eq, E_in, E_out, E, ("E_in", "E_out", "E"), level, precond, nu=nu, plane=plane)

    def _material(self, nu, plane):
        if plane not in _PLANES:
            raise ValueError(f'{self._what}: plane must be "stress" or "strain", not {plane!r}')
        nu = float(nu)
        if not (math.isfinite(nu) and -1.0 < nu < 0.5):
            raise ValueError(f"{self._what}: nu must be finite with -1 < nu < 0.5")
        return nu, _PLANES[plane]

    @property
    def nstrains(self):
        return self.ndim * (self.ndim + 1) // 2

    def _lead(self):
        return (self.nstrains, self.ndim)

    def corrector(self, k):
        u = [ROCMeshField(self.backend, self.mesh, self.bcs) for _ in range(self.ndim)]
        self._call("corrector", self._index(k), [c.buf for c in u])
        return tuple(u)

    def stiffness(self, level=0):
        return self._call("stiffness", level)



def homogenize(phi_or_eq, *, E_in=1.0, E_out=1e-3, E=None, nu=0.3, plane="stress", level=0.0, rtol=1e-8, max_iters=500, precond="mg", chi0=None):
    """The effective elasticity tensor C^H of the periodic material whose cell is the box of ϕ's grid, on the device:
    elasticity_solve's Q1 discretisation, cell moduli, material and `plane`, on the torus of the grid's n − 1 cells per axis (node n − 1
    is node 0; ϕ needs no PeriodicBC, only its cells are read).  For each of the M = N(N+1)/2 unit strains a periodic corrector χ^k
    (zero at node 0) is found by conjugate gradients, from `chi0` ((M, N) + (n − 1); zero without one) until ‖r‖₂ ≤ rtol·‖f^k‖₂,
    preconditioned by one wrapping multigrid V-cycle (precond="mg") or the diagonal ("jacobi").  Returns a Homogenization: `tensor`,
    `sensitivity(W)` and the rest.  Raises ValueError / TypeError for what is refused (1-D, a band field, a slab, fewer than 2 cells in
    a dimension, moduli that are not finite and positive, ν outside (−1, 0.5), an unknown plane, non-finite data) and
    LsmNotConvergedError when max_iters does not suffice."""
    hom = Homogenization(phi_or_eq, E_in=E_in, E_out=E_out, E=E, nu=nu, plane=plane, level=level, precond=precond)
    try:
        return hom.solve(chi0=chi0, rtol=rtol, max_iters=max_iters)
    except BaseException:
        hom.close()
        raise


class ConductivityHomogenization(_CellProblem):
    """homogenize_conductivity's result and its operator, kept on the device.  The torus has m = n − 1 nodes (and
    cells) per axis; there are N unit gradients e_0 … e_{N−1}.  `tensor` ((N, N) numpy, exactly symmetric), `iterations` and `relres`
    (one entry per corrector), `levels`, `free_dofs`, `cells_shape`; corrector(k) → a ROCMeshField (image nodes n − 1 from node 0);
    correctors() → host (N,) + m; sensitivity(W) → the ROCMeshField of the integrand of d(W:K^H)/dΩ, a normal speed (coeff.set_values
    takes it device to device); cells(), apply(x), load(k), energy_cells(p, q) show the operator; solve(chi0=None, rtol, max_iters)
    solves again (a warm start); solve_rhs(f, x0) runs the same PCG on a right-hand side of the caller's; with_correctors(chi) sets
    the correctors without a solve; close() releases the device memory.  ϕ is read once, at construction: after ϕ has moved, build
    a new object and pass the old correctors() as chi0."""
    _what, _prefix, _cells, _unit, _host_finite = "homogenize_conductivity", "hcond", "cell coefficients", "the unit gradient", True

    def __init__(self, phi_or_eq, *, a_in=1.0, a_out=1e-3, a=None, level=0.0, precond="mg"):
        super().__init__(phi_or_eq, a_in, a_out, a, ("a_in", "a_out", "a"), level, precond)

    def _lead(self):
        return (self.ndim,)

    def corrector(self, k):
        u = ROCMeshField(self.backend, self.mesh, self.bcs)
        self._call("corrector", self._index(k), u.buf)
        return u



def homogenize_conductivity(phi_or_eq, *, a_in=1.0, a_out=1e-3, a=None, level=0.0, rtol=1e-8, max_iters=500, precond="mg", chi0=None):
    """The effective conductivity tensor K^H of −∇·(a∇u) — thermal, electrical or diffusive — for the periodic material whose cell is the
    box of ϕ's grid, on the device: elliptic_solve's edge discretisation and cell coefficients (a_out + (a_in −
    a_out)·θ, or the cell array `a` of shape n − 1) with c = 0, on the torus of the grid's n − 1 cells per axis (node n − 1 is node 0; ϕ
    needs no PeriodicBC, only its cells are read).  For each of the N unit gradients a periodic corrector χ^p (zero at node 0) is found
    by conjugate gradients, from `chi0` ((N,) + (n − 1); zero without one) until ‖r‖₂ ≤ rtol·‖f^p‖₂, preconditioned by one wrapping
    multigrid V-cycle (precond="mg") or the diagonal ("jacobi").  Returns a ConductivityHomogenization: `tensor`, `sensitivity(W)` and
    the rest.  Raises ValueError / TypeError for what is refused (1-D, a band field, a slab, fewer than 2 cells in a dimension,
    coefficients that are not finite and positive, non-finite data) and LsmNotConvergedError when max_iters does not suffice."""
    hom = ConductivityHomogenization(phi_or_eq, a_in=a_in, a_out=a_out, a=a, level=level, precond=precond)
    try:
        return hom.solve(chi0=chi0, rtol=rtol, max_iters=max_iters)
    except BaseException:
        hom.close()
        raise


# ----------------------------------------------------------------------------- vibration modes (the eigenfrequency objective of a structural optimisation)

def _modes_args(m, rho_in, rho_out, rho, rtol, max_iters, from_phi, what="elasticity_modes", cells="cell moduli `E`"):
    """the refusals of elasticity_modes (or of `what`) that need neither a field nor a device; returns ρ as a host array, a device tensor
    or None"""
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)):
        raise TypeError(f"{what}: m must be an integer, not {type(m).__name__}")
    if not 1 <= int(m) <= 8:
        raise ValueError(f"{what}: m must be between 1 and 8, not {m}")
    rtol = float(rtol)
    if not (rtol > 0 and math.isfinite(rtol)) or int(max_iters) < 1:
        raise ValueError(f"{what}: rtol must be positive and finite, max_iters at least 1")
    if rho is None:
        if not from_phi:
            raise ValueError(f"{what}: the operator was built from {cells}, not from ϕ: give the cell densities `rho`")
        if not (_finite_positive(float(rho_in)) and _finite_positive(float(rho_out))):
            raise ValueError(f"{what}: rho_in and rho_out must be finite and positive")
        return None
    if hasattr(rho, "is_cuda"):
        return rho
    rho = np.asarray(rho, dtype=np.float64)
    if not _finite_positive(rho):
        raise ValueError(f"{what}: the cell densities `rho` must be finite and positive")
    return rho


class ElasticityModes:
    """elasticity_modes' result: `eigenvalues` (λ_k = ω_k², ascending), `frequencies` (√λ/2π), `iterations` (block iterations),
    `relres` (per mode, the recursive ‖A x − λ M x‖₂/(λ‖M x‖₂)), `operator`; mode(k) → N ROCMeshFields normalised to ∫ρ|u|² = 1, exact
    zeros on the fixed components, the sign unspecified; sensitivity(k) → the ROCMeshField g = e − λ_k·ρ̄·|u|², the integrand of
    dλ_k/dΩ that a NormalMotionTerm takes as its speed; vectors() → a host array (m, N) + n, the next design's `x0`; mass() → the
    lumped node mass, n-shaped; solve(x0=None, rtol=…, max_iters=…) runs again; close() releases the device memory.  The object
    borrows its operator: after operator.close() every use is a ValueError."""

    def __init__(self, op, m, *, rho_in=1.0, rho_out=1e-6, rho=None, x0=None, rtol=1e-6, max_iters=300):
        self._h = None
        rho = _modes_args(m, rho_in, rho_out, rho, rtol, max_iters, getattr(op, "_phi", None) is not None)
        self.operator, self.m = op, int(m)
        b = self.backend = op.backend
        n = tuple(int(k) for k in op.mesh.n)
        if 3 * self.m > op.free_dofs:
            raise ValueError(f"elasticity_modes: 3·m = {3 * self.m} exceeds the {op.free_dofs} free components")
        cells = tuple(k - 1 for k in n)
        if rho is not None and not hasattr(rho, "is_cuda") and rho.ndim and rho.shape != cells:
            raise ValueError(f"elasticity_modes: `rho` has shape {rho.shape}, the grid has {cells} cells")
        rho_dev = None if rho is None else b.node_array(rho, "rho", cells)
        try:
            self._h = b.modes_create(op._handle(), None if rho is not None else op._phi.buf, op._level, rho_in, rho_out, rho_dev, self.m)
        except L.LsmError as e:
            if "must be finite" in str(e):
                raise ValueError("elasticity_modes: " + str(e).split(": ", 2)[-1]) from None
            raise
        self.eigenvalues = self.relres = None
        self.iterations = 0
        self.solve(x0=x0, rtol=rtol, max_iters=max_iters)

    def _handle(self):
        if self._h is None:
            raise ValueError("the ElasticityModes object is closed")
        self.operator._handle()     # ValueError once the operator is closed: the modes object borrows it
        return self._h

    def solve(self, x0=None, rtol=1e-6, max_iters=300):
        h = self._handle()
        b, op, m = self.backend, self.operator, self.m
        rtol = float(rtol)
        if not (rtol > 0 and math.isfinite(rtol)) or int(max_iters) < 1:
            raise ValueError("elasticity_modes: rtol must be positive and finite, max_iters at least 1")
        n = tuple(int(k) for k in op.mesh.n)
        xd = None
        if x0 is not None:
            if b.torch.is_tensor(x0):
                xd = b.node_array(x0, "x0", (m, op.ndim) + n)
            else:
                a = np.asarray(x0, dtype=np.float64)
                if a.shape != (m, op.ndim) + n:
                    raise ValueError(f"elasticity_modes: x0 has shape {a.shape}, expected {(m, op.ndim) + n}")
                if not np.all(np.isfinite(a)):
                    raise ValueError("elasticity_modes: x0 must be finite")
                xd = b.torch.from_numpy(np.concatenate([a[k, i].reshape(-1, order="F") for k in range(m) for i in range(op.ndim)])).to(b.device)
        try:
            code, lam, rel, it, stats = b.modes_solve(h, m, xd, rtol, int(max_iters))
        except L.LsmError as e:
            if "must be finite" in str(e):
                raise ValueError("elasticity_modes: x0 must be finite") from None
            raise
        self.eigenvalues, self.relres, self.iterations, self.stats = lam, rel, it, stats
        if code != L.OK:
            msg = b.lib.lsm_last_error(b.h)
            err = L.LsmNotConvergedError(f"lsm_elastic_modes_solve failed ({code}): {msg.decode() if msg else ''}")
            err.eigenvalues, err.relres, err.iterations, err.modes = lam, rel, it, self
            raise err
        return self

    @property
    def frequencies(self):
        return np.sqrt(self.eigenvalues) / (2.0 * math.pi)

    def _k(self, k):
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError(f"elasticity_modes: the mode index must be an integer, not {type(k).__name__}")
        if not 0 <= int(k) < self.m:
            raise ValueError(f"elasticity_modes: mode {k} of {self.m}")
        return int(k)

    def mode(self, k):
        h, k, op = self._handle(), self._k(k), self.operator
        u = [ROCMeshField(self.backend, op.mesh, op.bcs) for _ in range(op.ndim)]
        self.backend.modes_store(h, k, [c.buf for c in u])
        return tuple(u)

    def sensitivity(self, k):
        h, k, op = self._handle(), self._k(k), self.operator
        g = ROCMeshField(self.backend, op.mesh, op.bcs)
        self.backend.modes_sensitivity(h, k, g.buf)
        return g

    def vectors(self):
        h, op, m = self._handle(), self.operator, self.m
        n = tuple(int(k) for k in op.mesh.n)
        nn = int(np.prod(n))
        x = self.backend.modes_vectors(h, m * op.ndim * nn).cpu().numpy()
        return np.stack([np.stack([x[(k * op.ndim + i) * nn:(k * op.ndim + i + 1) * nn].reshape(n, order="F") for i in range(op.ndim)]) for k in range(m)])

    def mass(self):
        h = self._handle()
        n = tuple(int(k) for k in self.operator.mesh.n)
        return self.backend.modes_mass(h).cpu().numpy().reshape(n, order="F")

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            try:
                self.backend.modes_destroy(h)
            except Exception:
                pass

    __del__ = close


def elasticity_modes(phi_or_eq, m, *, E_in=1.0, E_out=1e-3, E=None, nu=0.3, plane="stress", dirichlet=None, level=0.0, precond="mg", rho_in=1.0, rho_out=1e-6,
                     rho=None, x0=None, rtol=1e-6, max_iters=300):
    """The m (1 … 8) lowest vibration modes of the ersatz-material structure of ϕ: the smallest eigenpairs of K u = λ M u, λ = ω², on
    the device.  K is elasticity_solve's operator with its arguments (`E_in` … `precond`), the fixed components of
    `dirichlet` are zero for the modes whatever values it prescribes, and a structure needs enough of them to hold every rigid-body
    motion.  M is a lumped mass: the density of a cell is rho_out + (rho_in − rho_out)·θ with the modulus' fill fraction θ, or
    `rho` (a scalar or an array of shape n − 1), which is required when `E` gave the moduli.  Keep rho_out/rho_in far below
    E_out/E_in (the defaults: 1e-6 against 1e-3): with equal densities the ersatz material is as heavy as the structure and a
    thousand times softer, and the lowest "modes" are spurious ones that live in the void, below the structure's first frequency.
    A locally optimal block preconditioned CG (LOBPCG) from `x0` (a host array (m, N) + n, such as the last design's vectors();
    a fixed pseudo-random start without one) until ‖K x − λ M x‖₂ ≤ rtol·λ·‖M x‖₂ for every mode.  Returns an ElasticityModes, whose
    `operator` the caller closes.  Raises ValueError / TypeError for what is refused (elasticity_solve's refusals, m outside 1 … 8,
    3·m above the free components, densities not finite and positive, `E` without `rho`, a non-finite x0) and LsmNotConvergedError,
    which carries `eigenvalues`, `relres`, `iterations` and `modes`, when max_iters does not suffice."""
    rho = _modes_args(m, rho_in, rho_out, rho, rtol, max_iters, E is None)
    op = ElasticityOperator(phi_or_eq, E_in=E_in, E_out=E_out, E=E, nu=nu, plane=plane, dirichlet=dirichlet, level=level, precond=precond)
    try:
        return op.modes(m, rho_in=rho_in, rho_out=rho_out, rho=rho, x0=x0, rtol=rtol, max_iters=max_iters)
    except BaseException as e:
        if not isinstance(e, L.LsmNotConvergedError):     # the partial results of a failed solve still need their operator
            op.close()
        raise


# ----------------------------------------------------------------------------- scalar eigenmodes (cavities, membranes, the λ₁ objective)

class EllipticModes:
    """elliptic_modes' result: `eigenvalues` (λ_k, ascending), `frequencies` (√λ/2π), `iterations` (block iterations), `relres` (per
    mode, the recursive ‖A x − λ M x‖₂/(λ‖M x‖₂)), `stats` (iterations, preconditioner applications, directions dropped, unconverged
    columns), `operator`; mode(k) → one ROCMeshField normalised to ∫ρu² = 1, exact zeros on the fixed nodes, the sign unspecified;
    sensitivity(k) → the ROCMeshField g = e − λ_k·ρ̄·u², e the energy density a|∇u|² of the mode: the integrand of dλ_k/dΩ that a
    NormalMotionTerm takes as its speed (c does not move with the shape and gives no term; for a membrane whose outside nodes are
    fixed the derivative is a boundary flux, not this field); vectors() → a host array (m,) + n, the next design's `x0`; mass() → the
    lumped node mass, n-shaped; solve(x0=None, rtol=…, max_iters=…) runs again; close() releases the device memory.  The object
    borrows its operator: after operator.close() every use is a ValueError."""

    def __init__(self, op, m, *, rho_in=1.0, rho_out=1e-6, rho=None, x0=None, rtol=1e-6, max_iters=300):
        self._h = None
        rho = _modes_args(m, rho_in, rho_out, rho, rtol, max_iters, getattr(op, "_phi", None) is not None, "elliptic_modes", "cell coefficients `a`")
        self.operator, self.m = op, int(m)
        b = self.backend = op.backend
        n = tuple(int(k) for k in op.mesh.n)
        if 3 * self.m > op.free_nodes:
            raise ValueError(f"elliptic_modes: 3·m = {3 * self.m} exceeds the {op.free_nodes} free nodes")
        cells = tuple(k - 1 for k in n)
        if rho is not None and not hasattr(rho, "is_cuda") and rho.ndim and rho.shape != cells:
            raise ValueError(f"elliptic_modes: `rho` has shape {rho.shape}, the grid has {cells} cells")
        rho_dev = None if rho is None else b.node_array(rho, "rho", cells)
        try:
            self._h = b.emodes_create(op._handle(), None if rho is not None else op._phi.buf, op._level, rho_in, rho_out, rho_dev, self.m)
        except L.LsmError as e:
            if "must be finite" in str(e):
                raise ValueError("elliptic_modes: " + str(e).split(": ", 2)[-1]) from None
            raise
        self.eigenvalues = self.relres = None
        self.iterations = 0
        self.solve(x0=x0, rtol=rtol, max_iters=max_iters)

    def _handle(self):
        if self._h is None:
            raise ValueError("the EllipticModes object is closed")
        self.operator._handle()     # ValueError once the operator is closed: the modes object borrows it
        return self._h

    def solve(self, x0=None, rtol=1e-6, max_iters=300):
        h = self._handle()
        b, op, m = self.backend, self.operator, self.m
        rtol = float(rtol)
        if not (rtol > 0 and math.isfinite(rtol)) or int(max_iters) < 1:
            raise ValueError("elliptic_modes: rtol must be positive and finite, max_iters at least 1")
        n = tuple(int(k) for k in op.mesh.n)
        xd = None
        if x0 is not None:
            if b.torch.is_tensor(x0):
                xd = b.node_array(x0, "x0", (m,) + n)
            else:
                a = np.asarray(x0, dtype=np.float64)
                if a.shape != (m,) + n:
                    raise ValueError(f"elliptic_modes: x0 has shape {a.shape}, expected {(m,) + n}")
                if not np.all(np.isfinite(a)):
                    raise ValueError("elliptic_modes: x0 must be finite")
                xd = b.torch.from_numpy(np.concatenate([a[k].reshape(-1, order="F") for k in range(m)])).to(b.device)
        try:
            code, lam, rel, it, stats = b.emodes_solve(h, m, xd, rtol, int(max_iters))
        except L.LsmError as e:
            if "must be finite" in str(e):
                raise ValueError("elliptic_modes: x0 must be finite") from None
            raise
        self.eigenvalues, self.relres, self.iterations, self.stats = lam, rel, it, stats
        if code != L.OK:
            msg = b.lib.lsm_last_error(b.h)
            err = L.LsmNotConvergedError(f"lsm_elliptic_modes_solve failed ({code}): {msg.decode() if msg else ''}")
            err.eigenvalues, err.relres, err.iterations, err.modes = lam, rel, it, self
            raise err
        return self

    @property
    def frequencies(self):
        return np.sqrt(self.eigenvalues) / (2.0 * math.pi)

    def _k(self, k):
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError(f"elliptic_modes: the mode index must be an integer, not {type(k).__name__}")
        if not 0 <= int(k) < self.m:
            raise ValueError(f"elliptic_modes: mode {k} of {self.m}")
        return int(k)

    def mode(self, k):
        h, k, op = self._handle(), self._k(k), self.operator
        u = ROCMeshField(self.backend, op.mesh, op.bcs)
        self.backend.emodes_store(h, k, u.buf)
        return u

    def sensitivity(self, k):
        h, k, op = self._handle(), self._k(k), self.operator
        g = ROCMeshField(self.backend, op.mesh, op.bcs)
        self.backend.emodes_sensitivity(h, k, g.buf)
        return g

    def vectors(self):
        h, op, m = self._handle(), self.operator, self.m
        n = tuple(int(k) for k in op.mesh.n)
        nn = int(np.prod(n))
        x = self.backend.emodes_vectors(h, m * nn).cpu().numpy()
        return np.stack([x[k * nn:(k + 1) * nn].reshape(n, order="F") for k in range(m)])

    def mass(self):
        h = self._handle()
        n = tuple(int(k) for k in self.operator.mesh.n)
        return self.backend.emodes_mass(h).cpu().numpy().reshape(n, order="F")

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            try:
                self.backend.emodes_destroy(h)
            except Exception:
                pass

    __del__ = close


def elliptic_modes(phi_or_eq, m, *, a_in=1.0, a_out=1e-3, a=None, c=0.0, dirichlet=None, level=0.0, precond="mg", rho_in=1.0, rho_out=1e-6, rho=None, x0=None,
                   rtol=1e-6, max_iters=300):
    """The m (1 … 8) lowest eigenmodes of −∇·(a∇u) + c·u = λ ρ u on the box of ϕ's grid: the smallest eigenpairs of A u = λ M u on the
    device — the resonances of a cavity or the cut-off wavenumbers of a waveguide (natural walls, ersatz material in
    the void), the tones of a membrane, the principal eigenvalue of a diffusion problem, the objective of a "maximise λ₁" shape
    optimisation.  A is elliptic_solve's operator with its arguments (`a_in` … `precond`) and its c term; the nodes of `dirichlet` are
    zero in every mode whatever values it prescribes.  A must be positive definite: a cavity with natural walls only needs c > 0.
    With a constant c and ρ ≡ 1 the spectrum is that of c = 0 shifted by exactly c; in general the pencil is (K + c·m, M), and an exact
    spectral shift is not offered.  M is a lumped mass: the density of a cell is rho_out + (rho_in − rho_out)·θ with the coefficient's
    fill fraction θ, or `rho` (a scalar or an array of shape n − 1), which is required when `a` gave the coefficients.  Keep
    rho_out/rho_in far below a_out/a_in (the defaults: 1e-6 against 1e-3): with equal densities the ersatz material is as heavy as
    the domain and a thousand times softer, and the lowest "modes" are spurious ones that live in the void (a clamped two-hole plate
    on 33×33: a first "mode" of 0.26 in the holes, against 2.09 with rho_out = 1e-6).  A membrane of shape {ϕ < 0} fixes the
    nodes outside: dirichlet=(ϕ.values() >= 0, 0.0).  A locally optimal block preconditioned CG (LOBPCG) from `x0` (a host array
    (m,) + n, such as the last design's vectors(); a fixed pseudo-random start without one) until ‖A x − λ M x‖₂ ≤ rtol·λ·‖M x‖₂ for
    every mode.  Returns an EllipticModes, whose `operator` the caller closes.  Raises ValueError / TypeError for what is refused
    (elliptic_solve's refusals, m outside 1 … 8, 3·m above the free nodes, densities not finite and positive, `a` without `rho`, a
    non-finite x0) and LsmNotConvergedError, which carries `eigenvalues`, `relres`, `iterations` and `modes`, when max_iters does
    not suffice."""
    rho = _modes_args(m, rho_in, rho_out, rho, rtol, max_iters, a is None, "elliptic_modes", "cell coefficients `a`")
    op = EllipticOperator(phi_or_eq, a_in=a_in, a_out=a_out, a=a, c=c, dirichlet=dirichlet, level=level, precond=precond)
    try:
        return op.modes(m, rho_in=rho_in, rho_out=rho_out, rho=rho, x0=x0, rtol=rtol, max_iters=max_iters)
    except BaseException as e:
        if not isinstance(e, L.LsmNotConvergedError):     # the partial results of a failed solve still need their operator
            op.close()
        raise


# ----------------------------------------------------------------------------- meshes of the interior (ext/MMGVolumeExt.jl)

_BAND_MESH_MSG = ("volume_mesh is not supported on NarrowBandMeshField: a band does not hold the interior. "
                  "Use a full MeshField for the volume mesh, or isosurface for the interface.")
_REMESH_VOLUME_MSG = ("export_volume_mesh(…; {name}): the remeshing pass (mmg2d_O3 / mmg3d_O3 of ext/MMGVolumeExt.jl) is not part of this "
                      "library; the file written without these keywords is the level-set splitting it starts from")


class DomainMesh:
    """volume_mesh(…)'s result: the interior {ϕ < level} as a body-fitted simplicial mesh.  `vertices` (nv, N) float64;
    `elements` (ne, N + 1) int64, 0-based: triangles in 2-D, tetrahedra in 3-D, of non-negative signed volume
    det[v1 − v0, …]; `interface` (ni, N) int64: the elements of isosurface(ϕ, level), in its order and orientation (normals
    pointing out of the mesh), in this mesh's vertex numbers.  `mesh`: the grid; `level`; len() = ne."""

    def __init__(self, vertices, elements, interface, mesh=None, level=0.0):
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float64)
        self.elements = np.ascontiguousarray(elements, dtype=np.int64)
        self.interface = np.ascontiguousarray(interface, dtype=np.int64)
        self.mesh, self.level = mesh, float(level)

    @property
    def ndim(self):
        return int(self.vertices.shape[1])

    def __len__(self):
        return int(self.elements.shape[0])

    def measure(self):
        """Σ signed element volumes (areas in 2-D), computed on the host"""
        if not len(self):
            return 0.0
        p = self.vertices[self.elements]
        d = p[:, 1:] - p[:, :1]
        if self.ndim == 2:
            return float(0.5 * (d[:, 0, 0] * d[:, 1, 1] - d[:, 0, 1] * d[:, 1, 0]).sum())
        return float((d[:, 0] * np.cross(d[:, 1], d[:, 2])).sum() / 6.0)

    def __repr__(self):
        kind, ikind = ("triangles", "segments") if self.ndim == 2 else ("tetrahedra", "triangles")
        return (f"DomainMesh in ℝ{_superscript(self.ndim)}: {len(self.vertices)} vertices, {len(self)} {kind}, "
                f"{len(self.interface)} interface {ikind}, level = {_jl_float(self.level)}")


def volume_mesh(phi, level=0.0):
    """The interior {ϕ < level} of a dense device field as a body-fitted simplicial mesh, built on the device:
    every simplex of the Freudenthal subdivision that the level crosses is split at isosurface's cut vertices — the first
    phase of mmg2d_O3 / mmg3d_O3 -ls in export_volume_mesh (ext/MMGVolumeExt.jl), without the remesher.  Conforming, no Steiner
    points, every signed volume >= 0, and the boundary inside the box is exactly isosurface(ϕ, level).  ϕ: a ROCMeshField or a
    LevelSetEquation (its current_state()).  Only the interior of the field is read.  Returns a DomainMesh."""
    if isinstance(phi, LevelSetEquation):
        phi = phi.current_state()
    if not isinstance(phi, ROCMeshField):
        raise TypeError("volume_mesh takes a device field (ROCMeshField) or a LevelSetEquation, " f"not {type(phi).__name__}")
    if isinstance(phi, ROCNarrowBandMeshField):
        raise ValueError(_BAND_MESH_MSG)
    N = phi.mesh.ndim
    if N == 1:
        raise ValueError("volume_mesh of a 1 dimensional level-set is not supported: 2-D and 3-D fields only")
    b = phi.backend
    if getattr(b, "slab", None) is not None:
        raise ValueError("volume_mesh of a slab-decomposed field (a field with a comm) is not supported")
    level = float(level)
    if not math.isfinite(level):
        raise ValueError("volume_mesh: level must be finite")
    h, counts = b.vol_create(phi.buf, None, level)
    try:
        verts, elems, iface = b.vol_read(h, counts)
        return DomainMesh(verts.cpu().numpy(), elems.cpu().numpy(), iface.cpu().numpy(), phi.mesh, level)
    finally:
        b.vol_destroy(h)


def _write_domain_mesh(path, m):
    """a Medit .mesh file of a DomainMesh: 0-based numbers written 1-based; references 1 (vertices), 3 (elements), 10 (interface)"""
    N = m.ndim
    ekind, ikind = ("Triangles", "Edges") if N == 2 else ("Tetrahedra", "Triangles")
    with open(path, "w") as f:
        f.write(f"MeshVersionFormatted 1\nDimension {N}\n\nVertices\n{len(m.vertices)}\n")
        f.writelines(" ".join(_jl_float(x) for x in row) + " 1\n" for row in m.vertices.tolist())
        f.write(f"\n{ekind}\n{len(m.elements)}\n")
        f.writelines(" ".join(str(i + 1) for i in row) + " 3\n" for row in m.elements.tolist())
        f.write(f"\n{ikind}\n{len(m.interface)}\n")
        f.writelines(" ".join(str(i + 1) for i in row) + " 10\n" for row in m.interface.tolist())
        f.write("\nEnd\n")


def export_volume_mesh(phi_or_eq, output, level=0.0, hgrad=None, hmin=None, hmax=None, hausd=None):
    """export_volume_mesh(ϕ, output; hgrad, hmin, hmax, hausd) (ext/MMGVolumeExt.jl) up to the remesher: the interior {ϕ < level}
    of a 2-D or 3-D field (a dense device field or a LevelSetEquation; also a DomainMesh already built, which makes the writer
    usable without a device) written as a Medit .mesh file, numbers formatted as export_surface_mesh formats them.  This file's
    convention, the labels MMG's level-set mode gives its output: vertices carry reference 1; the elements (`Triangles` in 2-D,
    `Tetrahedra` in 3-D) reference 3, the ϕ < 0 subdomain; the interface (`Edges` in 2-D, `Triangles` in 3-D) reference 10.  The
    remeshing keywords raise NotImplementedError.  Returns `output`."""
    if isinstance(phi_or_eq, LevelSetEquation):
        phi_or_eq = phi_or_eq.current_state()
    N = phi_or_eq.ndim if isinstance(phi_or_eq, DomainMesh) else getattr(getattr(phi_or_eq, "mesh", None), "ndim", None)
    if N is not None and N not in (2, 3):
        raise ValueError(f"export_mesh of {N} dimensional level-set not supported.")
    for name, value in (("hgrad", hgrad), ("hmin", hmin), ("hmax", hmax), ("hausd", hausd)):
        if value is not None:
            raise NotImplementedError(_REMESH_VOLUME_MSG.format(name=name))
    m = phi_or_eq if isinstance(phi_or_eq, DomainMesh) else volume_mesh(phi_or_eq, level)
    _write_domain_mesh(output, m)
    return output


# ----------------------------------------------------------------------------- pictures (ext/MakieExt.jl:142-171)

_STYLE3 = dict(color=(70, 130, 180), background=(255, 255, 255), ambient=0.25, step=0.5, bisections=6)
_STYLE2 = dict(fill=(233, 233, 233), line=(0, 0, 0), linewidth=2.0, cell=(198, 217, 234), background=(255, 255, 255), extent=None)


def _rgb(name, c):
    c = tuple(int(x) for x in c)
    if len(c) != 3 or not all(0 <= x <= 255 for x in c):
        raise ValueError(f"render: {name} must be three integers in 0..255")
    return c


class Camera:
    """Camera(eye, lookat, up = (0, 0, 1), fov = 40.0, orthographic = None): a pinhole camera at `eye` looking at `lookat`, `fov`
    the vertical field of view in degrees; orthographic = w: parallel rays over a window w world units high.  The library sees
    only what vectors(width, height) computes in fp64: eye, forward, right·s_x, up·s_y and the orthographic flag."""

    def __init__(self, eye, lookat, up=(0.0, 0.0, 1.0), fov=40.0, orthographic=None):
        self.eye, self.lookat, self.up = (tuple(float(x) for x in a) for a in (eye, lookat, up))
        if not all(len(a) == 3 for a in (self.eye, self.lookat, self.up)):
            raise ValueError("Camera: eye, lookat and up have three components")
        self.fov = float(fov)
        self.orthographic = None if orthographic is None else float(orthographic)
        if not 0.0 < self.fov < 180.0:
            raise ValueError("Camera: fov must lie in (0, 180) degrees")
        if self.orthographic is not None and not self.orthographic > 0.0:
            raise ValueError("Camera: the orthographic window must be positive")
        self.vectors(1, 1)

    def vectors(self, width, height):
        """the 13 doubles of lsm_render_draw for an image of width × height pixels"""
        eye, lookat, up = (np.asarray(a, dtype=np.float64) for a in (self.eye, self.lookat, self.up))
        f = lookat - eye
        nf = np.sqrt(f @ f)
        if not nf > 0:
            raise ValueError("Camera: eye and lookat coincide")
        f = f / nf
        r = np.cross(f, up)
        nr = np.sqrt(r @ r)
        if not nr > 1e-12 * np.sqrt(up @ up):
            raise ValueError("Camera: up is parallel to the view direction")
        r = r / nr
        u = np.cross(r, f)
        sy = np.tan(np.radians(self.fov) / 2.0) if self.orthographic is None else 0.5 * self.orthographic
        sx = sy * (float(width) / float(height))
        return np.concatenate([eye, f, r * sx, u * sy, [0.0 if self.orthographic is None else 1.0]])

    @classmethod
    def fit(cls, grid, direction=(1.0, 1.0, 1.0), fov=40.0):
        """a perspective camera on the ray from the box's centre along `direction` that sees the whole box (its bounding sphere,
        in an image at least as wide as high)"""
        if grid.ndim != 3:
            raise ValueError("Camera.fit takes a 3-D grid")
        lc, hc, dirn = (np.asarray(a, dtype=np.float64) for a in (grid.lc, grid.hc, direction))
        if not np.sqrt(dirn @ dirn) > 0:
            raise ValueError("Camera.fit: direction must not vanish")
        c = 0.5 * (lc + hc)
        rad = 0.5 * np.sqrt(((hc - lc) ** 2).sum())
        dirn = dirn / np.sqrt(dirn @ dirn)
        dist = 1.05 * rad / np.sin(np.radians(float(fov)) / 2.0)
        return cls(c + dist * dirn, c, (0.0, 0.0, 1.0) if abs(dirn[2]) < 0.99 else (0.0, 1.0, 0.0), fov)

    def __repr__(self):
        kind = f"fov = {_jl_float(self.fov)}°" if self.orthographic is None else f"orthographic, window {_jl_float(self.orthographic)}"
        return f"Camera(eye = {self.eye}, lookat = {self.lookat}, up = {self.up}, {kind})"


def _png_bytes(rgba):
    import struct
    import zlib
    a = np.ascontiguousarray(rgba, dtype=np.uint8)
    H, W = a.shape[:2]

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    rows = np.concatenate([np.zeros((H, 1), dtype=np.uint8), a.reshape(H, W * 4)], axis=1)      # filter 0 on every row
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) +
            chunk(b"IEND", b""))


class Image:
    """render(…)'s result.  `rgba` (H, W, 4) uint8, row 0 at the top.  3-D: `depth` (H, W), the distance along the unit ray (inf
    where nothing is hit), and `normal` (H, W, 3), the unit gradient at the hit (0 where nothing is hit).  2-D: `cls` (H, W) uint8:
    0 outside, 1 inside, 2 line, 3 void, 4 / 5 active band cell outside / inside.  save(path) writes a PNG."""

    def __init__(self, rgba, depth=None, normal=None, cls=None):
        self.rgba, self.depth, self.normal, self.cls = rgba, depth, normal, cls

    @property
    def size(self):
        return int(self.rgba.shape[1]), int(self.rgba.shape[0])

    def save(self, path):
        with open(path, "wb") as f:
            f.write(_png_bytes(self.rgba))
        return path

    def __repr__(self):
        W, H = self.size
        if self.cls is not None:
            return f"Image {W}×{H} of a 2-dimensional level-set: {int((self.cls == 2).sum())} line pixels, {int((self.cls == 1).sum() + (self.cls == 5).sum())} inside"
        return f"Image {W}×{H} of a 3-dimensional level-set: {int(np.isfinite(self.depth).sum())} of {W * H} rays hit"


class Renderer:
    """Renderer(ϕ, level = 0.0): pictures of the interface {ϕ = level} of a device field, drawn on the device —
    what plot(ϕ) draws through ext/MakieExt.jl: in 3-D the first hit of a ray march through the trilinear interpolant
    (volume!(…; algorithm = :iso)), in 2-D the filled contour under its line, a band's active cells tinted.  ϕ: a ROCMeshField, a
    ROCNarrowBandMeshField or a LevelSetEquation (its current_state()); the field is referenced, not copied.  The table of bricks
    that lets rays step over uniform regions is built here, once; draw(…) may be called any number of times; after the field
    changed call refresh()."""

    def __init__(self, phi, level=0.0):
        self._h = None
        self._eq = phi if isinstance(phi, LevelSetEquation) else None
        if self._eq is not None:
            phi = self._eq.current_state()
        if not isinstance(phi, ROCMeshField):
            raise TypeError("render takes a device field (ROCMeshField / ROCNarrowBandMeshField) or a LevelSetEquation, "
                            f"not {type(phi).__name__}")
        if phi.mesh.ndim == 1:
            raise ValueError("render of a 1 dimensional level-set is not supported: 2-D and 3-D fields only")
        if getattr(phi.backend, "slab", None) is not None:
            raise ValueError("render of a slab-decomposed field (a field with a comm) is not supported")
        self.level = float(level)
        if not math.isfinite(self.level):
            raise ValueError("render: level must be finite")
        self._attach(phi)

    def _attach(self, phi):
        self.close()
        self.phi, self.backend, self.mesh = phi, phi.backend, phi.mesh
        self._buf, self._mask = phi.buf, phi.mask if isinstance(phi, ROCNarrowBandMeshField) else None
        self._h = self.backend.render_create(self._buf, self._mask, self.level)

    def refresh(self):
        """rebuild the bricks after the field changed (an equation's current state may live in another buffer after a step)"""
        if self._h is None:
            raise ValueError("Renderer: closed")
        phi = self._eq.current_state() if self._eq is not None else self.phi
        if phi is not self.phi or phi.buf is not self._buf or (phi.mask if isinstance(phi, ROCNarrowBandMeshField) else None) is not self._mask:
            self._attach(phi)
        else:
            self.backend.render_refresh(self._h)
        return self

    def bricks(self):
        """(state, uniform) per brick of 8 cells per axis: state 0 void, 1 outside, 2 inside, 3 mixed (3-D)"""
        t = self.backend.render_bricks(self._h)
        return t & 3, (t & 4) != 0

    def draw(self, camera=None, size=(640, 480), want_normal=True, **style):
        if self._h is None:
            raise ValueError("Renderer: closed")
        W, H = (int(s) for s in size)
        if W <= 0 or H <= 0:
            raise ValueError("render: size must be (width, height) with both positive")
        three = self.mesh.ndim == 3
        st = dict(_STYLE3 if three else _STYLE2)
        for k, v in style.items():
            if k not in st:
                raise TypeError(f"render: unknown style keyword {k!r} for a {self.mesh.ndim}-D field (known: {', '.join(st)})")
            st[k] = v
        if three:
            step, nb = float(st["step"]), st["bisections"]
            if not step > 0:
                raise ValueError("render: step must be positive")
            if int(nb) != nb or not 0 <= int(nb) <= 30:
                raise ValueError("render: bisections must be an integer in 0..30")
            if not 0.0 <= float(st["ambient"]) <= 1.0:
                raise ValueError("render: ambient must lie in 0..1")
            if camera is None:
                camera = Camera.fit(self.mesh)
            if not isinstance(camera, Camera):
                raise TypeError("render: camera must be a Camera")
            vec = [*_rgb("color", st["color"]), *_rgb("background", st["background"]), float(st["ambient"]), step, int(nb)]
            rgba, depth, normal = self.backend.render_draw(self._h, camera.vectors(W, H), W, H, vec, want_normal)
            return Image(rgba.cpu().numpy(), depth=depth.cpu().numpy(), normal=None if normal is None else normal.cpu().numpy())
        if camera is not None:
            raise ValueError("render: a 2-D field is drawn over `extent`, not through a camera")
        ext = st["extent"]
        x0, x1, y0, y1 = (self.mesh.lc[0], self.mesh.hc[0], self.mesh.lc[1], self.mesh.hc[1]) if ext is None else (float(e) for e in ext)
        if not (x1 > x0 and y1 > y0):
            raise ValueError("render: extent must be (x0, x1, y0, y1) with x1 > x0 and y1 > y0")
        lw = float(st["linewidth"])
        if not lw >= 0:
            raise ValueError("render: linewidth must not be negative")
        fill, line, cell, bg = (_rgb(k, st[k]) for k in ("fill", "line", "cell", "background"))
        both = tuple(int(math.floor(float(c) * float(f) / 255.0 + 0.5)) for c, f in zip(cell, fill))
        vec = [lw, x0, x1, y0, y1, *bg, *fill, *line, *bg, *cell, *both]
        rgba, cls, _ = self.backend.render_draw(self._h, None, W, H, vec)
        return Image(rgba.cpu().numpy(), cls=cls.cpu().numpy())

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            try:
                self.backend.render_destroy(h)
            except Exception:
                pass

    __del__ = close


def render(phi, camera=None, size=(640, 480), level=0.0, **style):
    """One picture of the interface {ϕ = level}: Renderer(ϕ, level).draw(camera, size, **style).  Style in 3-D: color, background,
    ambient, step (sample spacing in units of min(h)), bisections; in 2-D: fill, line, linewidth (pixels), cell, background, extent."""
    r = Renderer(phi, level)
    try:
        return r.draw(camera, size, **style)
    finally:
        r.close()


def record_(eq, tf, pattern, every=1, dt=float("inf"), **render_kw):
    """integrate_(eq, tf, dt) with a posthook that saves pattern.format(k) after every `every`-th step k = 1, 2, … from one
    Renderer (the loop behind the reference README's zalesak3d.gif).  render_kw: level and draw's arguments.  Returns the paths."""
    every = int(every)
    if every < 1:
        raise ValueError("record_: every must be at least 1")
    r = Renderer(eq, render_kw.pop("level", 0.0))
    paths, step = [], [0]

    def hook(ls):
        step[0] += 1
        if step[0] % every == 0:
            paths.append(r.refresh().draw(**render_kw).save(pattern.format(step[0])))

    try:
        integrate_(eq, tf, dt, posthook=hook)
    finally:
        r.close()
    return paths
