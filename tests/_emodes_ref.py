"""elliptic_modes restated in numpy (csrc/lsm_elliptic.hip "elliptic_modes", include/lsm.h "elliptic_modes").

The problem: the m smallest eigenpairs of A x = λ M x on the free nodes; A is _elliptic_ref's operator with its c term (scaled by
1/∏h), the fixed nodes are zero, M the lumped mass of an ersatz density, scaled by 1/∏h like A.

  density    ρ_C = ρ_out + (ρ_in − ρ_out)·θ_C: _elliptic_ref.cell_coefficients with (ρ_in, ρ_out), or a given cell array
  mass       M_I = (Σ of ρ_C over the existing cells around I, ascending, from +0)·2^−N;  ρ̄_I = that sum / (number of those cells)
  start      entry t = k·nn + id of x0: the splitmix64 value of _modes_ref.default_start with one component; zero on the fixed nodes
  iteration  _modes_ref.lobpcg, lobpcg_ld and rayleigh_ritz_jacobi themselves, driven through a one-component adapter (Op1, Hier1) over
             _elliptic_ref's Operator and Hierarchy: nothing of the iteration is written twice.  In long double the V-cycle is
             _elastic_ref._vcycle_ld's recursion on the adapter, which is _elliptic_ref._vcycle_ld's arithmetic (ω = 0.8, the same
             sweeps and transfers) on _elliptic_ref._apply_free_ld
  sensitivity  g_I = e_I − (λ·ρ̄_I)·(u_I·u_I), e = Operator.energy(u); c gives no term

What is compared bit for bit and what against bars is _modes_ref's split: the mass, the start, the block apply, the stored mode's
rounding and the sensitivity bit for bit; eigenvalues, residuals, orthonormality and iteration counts against bars.
"""
import itertools

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import _elliptic_ref as EL
import _modes_ref as R

LD = R.LD
splitmix64 = R.splitmix64
rayleigh_ritz_jacobi = R.rayleigh_ritz_jacobi


class Op1:
    """an _elliptic_ref.Operator seen as _modes_ref sees an operator: one component, vectors of shape (1,) + n"""

    def __init__(self, op):
        self.op, self.N, self.n, self.h = op, 1, op.n, op.h
        self.free, self.fixed, self.D = op.free[None], op.fixed[None], op.D[None]

    def matrix(self):
        return self.op.matrix()

    def flat(self, u):
        return np.asarray(u[0]).reshape(-1, order="F")

    def unflat(self, x):
        return x.reshape(self.n, order="F")[None]

    def apply(self, u):
        return (EL._apply_free_ld(self.op, u[0]) if u.dtype == LD else self.op.apply(u[0]))[None]


class Hier1:
    def __init__(self, hier):
        self.hier, self.ops, self.P, self.levels = hier, [Op1(o) for o in hier.ops], hier.P, hier.levels

    def omega(self, lev):
        return EL.OMEGA

    def vcycle(self, r):
        return self.hier.vcycle(r[0])[None]


def _squeeze(res):
    res["X"] = res["X"][:, 0]
    for s in res.get("steps", ()):
        s["X"] = s["X"][:, 0]
    return res


def _x0(x0):
    return None if x0 is None else np.asarray(x0)[:, None]


def lobpcg(hier, Mn, m, x0=None, rtol=1e-6, max_iters=300, precond="mg", trace=False, rr=None):
    """_modes_ref.lobpcg for an _elliptic_ref.Hierarchy; X and x0 are (m,) + n"""
    return _squeeze(R.lobpcg(Hier1(hier), Mn, m, _x0(x0), rtol, max_iters, precond, trace, rr))


def lobpcg_ld(hier, Mn, m, x0=None, rtol=1e-6, max_iters=300, precond="mg"):
    return _squeeze(R.lobpcg_ld(Hier1(hier), Mn, m, _x0(x0), rtol, max_iters, precond))


def default_start(op, m):
    """(m,) + n: entry t = k·nn + id"""
    return R.default_start(Op1(op), m)[:, 0]


def true_residual(op, Mn, x, lam):
    return R.true_residual(Op1(op), Mn, np.asarray(x)[None], lam)


def ortho_defect(op, Mn, X):
    return R.ortho_defect(Op1(op), Mn, np.asarray(X)[:, None])


def density_cells(phi, h, level, rho_in, rho_out):
    return EL.cell_coefficients(phi, h, level, rho_in, rho_out)


def _cell_sum(n, cells):
    """Σ over the 2^N cells around a node in ascending order (bit d of the cell's number: index I_d − 1 + bit), from +0; no cell: +0"""
    w = np.pad(np.asarray(cells, dtype=np.float64), 1)
    acc = np.zeros(n)
    for off in EL._offsets(len(n)):
        acc = acc + w[tuple(slice(o, o + nd) for o, nd in zip(off, n))]
    return acc


def mass(op, rho):
    return _cell_sum(op.n, rho) * 2.0 ** -op.N


def mean_density(op, rho):
    return _cell_sum(op.n, rho) / _cell_sum(op.n, np.ones(tuple(k - 1 for k in op.n)))


def cell_count(op):
    return _cell_sum(op.n, np.ones(tuple(k - 1 for k in op.n)))


def sensitivity(op, rho, u, lam):
    """g in float64 (the caller rounds to the storage type): u is the stored mode"""
    u = np.asarray(u, dtype=np.float64)
    return op.energy(u) - (lam * mean_density(op, rho)) * (u * u)


def exact(op, Mn, k):
    """the k smallest eigenvalues: dense below 3000 free nodes, shift-invert Lanczos above"""
    free = op.free.reshape(-1, order="F")
    A = op.matrix()[free][:, free]
    Mv = np.asarray(Mn).reshape(-1, order="F")[free]
    if A.shape[0] < 3000:
        return sla.eigh(A.toarray(), np.diag(Mv), eigvals_only=True, subset_by_index=(0, k - 1))
    w = spla.eigsh(A.tocsc(), k=k, M=sp.diags(Mv).tocsc(), sigma=0.0, which="LM", tol=1e-13, return_eigenvectors=False)
    return np.sort(w)


def closed_form(n, h, k, dirichlet, c=0.0):
    """the k smallest eigenvalues of the box with a ≡ 1, ρ ≡ 1: λ = c + Σ_d (4/h_d²)·sin²(k_d π/(2(n_d − 1))), k_d = 1 … n_d − 2 with
    every face fixed (dirichlet), k_d = 0 … n_d − 1 with natural faces"""
    per = [[(4.0 / (hd * hd)) * np.sin(kd * np.pi / (2.0 * (nd - 1))) ** 2 for kd in (range(1, nd - 1) if dirichlet else range(nd))] for nd, hd in zip(n, h)]
    return np.sort(np.array([c + sum(t) for t in itertools.product(*per)]))[:k]


def locked_start(op, Mn, m, locked):
    """_modes_ref.locked_start with one component: (m,) + n"""
    return R.locked_start(Op1(op), Mn, m, locked)[:, 0]


# ---- the cases shared by tests/test_emodes_host.py and tests/test_gpu_emodes.py: the smallest shapes that reach each path.  iters /
# ortho: the restatement's own iteration counts at rtol 1e-6 (and 1e-8 for TIGHT) and its max |XᵀM X − I| at 1e-6
# (tests/test_emodes_host.py asserts the counts and prints both)

def faces(n):
    m = np.zeros(n, dtype=bool)
    for d in range(len(n)):
        m |= EL.face_mask(n, d, 0) | EL.face_mask(n, d, 1)
    return m


def _ball(n, h, R0, sign):
    """a signed distance to the centred disk / ball of radius R0·min(L): sign = +1 negative inside, −1 negative outside (a void)"""
    x = np.meshgrid(*[np.arange(nd) * hd for nd, hd in zip(n, h)], indexing="ij", sparse=True)
    L = [(nd - 1) * hd for nd, hd in zip(n, h)]
    return np.asfortranarray(sign * (np.sqrt(sum((xi - 0.5 * Li) ** 2 for xi, Li in zip(x, L))) - R0 * min(L)) + np.zeros(n))


def cases():
    """name → dict(n, hc, h, phi, a (cells or None), a_in, a_out, c, fixed (mask or None), m, rho_in, rho_out, rho (cells or None), dtype,
    precond, closed (None, "dirichlet" or "natural": closed_form applies), iters, ortho)"""
    out = {}

    def add(name, n, m, phi=None, a=None, contrast=1e-3, c=0.0, fixed=None, rho_out=1e-6, rho=None, dtype=np.float64, precond="mg", closed=None):
        hc = tuple((nd - 1.0) / (max(n) - 1.0) for nd in n)
        h = tuple(x / (nd - 1) for x, nd in zip(hc, n))
        phi = EL.two_holes(n, h) if phi is None else phi(n, h)
        fx = fixed(n, phi) if callable(fixed) else fixed
        out[name] = dict(n=n, hc=hc, h=h, phi=phi, a=a, a_in=1.0, a_out=contrast, c=c, fixed=fx, m=m, rho_in=1.0, rho_out=rho_out, rho=rho, dtype=dtype,
                         precond=precond, closed=closed, iters=ITERS.get(name), ortho=ORTHO.get(name))

    def clamp(n, phi):
        return EL.face_mask(n, 0, 0)

    add("box17x13_dirichlet_m4", (17, 13), 4, contrast=1.0, rho_out=1.0, fixed=lambda n, phi: faces(n), closed="dirichlet")
    add("box17x13_natural_c_m4", (17, 13), 4, contrast=1.0, rho_out=1.0, c=0.7, closed="natural")
    add("box9x11x8_dirichlet_m3", (9, 11, 8), 3, contrast=1.0, rho_out=1.0, fixed=lambda n, phi: faces(n), closed="dirichlet")
    add("33x33_m4", (33, 33), 4, fixed=clamp)
    add("64x48_m4", (64, 48), 4, fixed=clamp)                                             # even n: the last node has no coarse partner
    add("membrane41_m4", (41, 41), 4, phi=lambda n, h: _ball(n, h, 0.4, 1.0), fixed=lambda n, phi: phi >= 0)      # an interior mask, λ₂ = λ₃
    add("17c_void_c1_m4", (17, 17, 17), 4, phi=lambda n, h: _ball(n, h, 0.3, -1.0), c=1.0)                     # no fixed node
    add("17c_void_f32_m3", (17, 17, 17), 3, phi=lambda n, h: _ball(n, h, 0.3, -1.0), fixed=lambda n, phi: EL.face_mask(n, 0, 1), dtype=np.float32)
    add("5x5_jacobi_m2", (5, 5), 2, fixed=clamp, precond="jacobi")                        # one level
    add("9x12_m8", (9, 12), 8, fixed=clamp)                                               # q = 8, 16, 24: all 21 Gram tiles
    add("20x14_m1", (20, 14), 1, fixed=clamp)
    n = (20, 14, 9)
    rng = np.random.default_rng(23)
    add("20x14x9_given_m2", n, 2, a=np.asfortranarray(0.5 + rng.random(tuple(k - 1 for k in n))), rho=np.asfortranarray(0.25 + rng.random(tuple(k - 1 for k in n))),
        c=np.asfortranarray(0.1 + rng.random(n)))
    return out


# the restatement's iteration counts (rtol 1e-6, and rtol 1e-8 for TIGHT) and max |XᵀM X − I| at 1e-6, from tests/test_emodes_host.py's print-out
ITERS = {
    "box17x13_dirichlet_m4": (23,), "box17x13_natural_c_m4": (14,), "box9x11x8_dirichlet_m3": (17,), "33x33_m4": (14, 18), "64x48_m4": (14,),
    "membrane41_m4": (27,), "17c_void_c1_m4": (12, 15), "17c_void_f32_m3": (14,), "5x5_jacobi_m2": (29, 35), "9x12_m8": (21,), "20x14_m1": (11,),
    "20x14x9_given_m2": (17,),
}
ORTHO = {
    "box17x13_dirichlet_m4": 4.4e-16, "box17x13_natural_c_m4": 1.8e-15, "box9x11x8_dirichlet_m3": 1.1e-15, "33x33_m4": 6.7e-16, "64x48_m4": 5.0e-16,
    "membrane41_m4": 1.7e-15, "17c_void_c1_m4": 1.1e-15, "17c_void_f32_m3": 4.4e-16, "5x5_jacobi_m2": 6.7e-16, "9x12_m8": 2.2e-15, "20x14_m1": 1.1e-16,
    "20x14x9_given_m2": 6.7e-16,
}
TIGHT = ("33x33_m4", "17c_void_c1_m4", "5x5_jacobi_m2")      # the cases that also run at rtol 1e-8


def build_case(cs):
    """(Hierarchy, ρ cells, node mass) of a case; an f32 case's ϕ is rounded to float32 first, as the handle stores it"""
    phi = cs["phi"].astype(cs["dtype"]).astype(np.float64)
    a = cs["a"] if cs["a"] is not None else EL.cell_coefficients(phi, cs["h"], 0.0, cs["a_in"], cs["a_out"])
    hier = EL.Hierarchy(EL.Operator(a, cs["h"], cs["c"], cs["fixed"]))
    rho = cs["rho"] if cs["rho"] is not None else density_cells(phi, cs["h"], 0.0, cs["rho_in"], cs["rho_out"])
    return hier, rho, mass(hier.ops[0], rho)


_SOLVED = {}


def base(name):
    """a case's reference data, computed once and shared: case, hier, rho, mass, exact (the m smallest eigenvalues, dense)"""
    if (name, None) not in _SOLVED:
        cs = cases()[name]
        hier, rho, Mn = build_case(cs)
        _SOLVED[(name, None)] = dict(case=cs, hier=hier, rho=rho, mass=Mn, exact=exact(hier.ops[0], Mn, cs["m"]))
    return _SOLVED[(name, None)]


def solved(name, rtol=1e-6):
    """base(name) and the restatement's own solve at rtol (lobpcg's dict), computed once"""
    key = (name, rtol)
    if key not in _SOLVED:
        res = dict(base(name))
        res.update(lobpcg(res["hier"], res["mass"], res["case"]["m"], None, rtol, 600, res["case"]["precond"]))
        _SOLVED[key] = res
    return _SOLVED[key]


# ---- single iterations (tests/test_gpu_emodes_steps.py; tests/test_emodes_host.py asserts the conditions), as _modes_ref.step_cases:
# a solve with max_iters = k returns X_k, one at rtol 1e300 X_0.  locked: the columns of locked_start that are exact eigenvectors

STEP_RTOL = 1e-6


def step_cases():
    """name → the dict of cases() with locked (a tuple, or None: the default start) and ks (the observed steps)"""
    out = {}

    def add(name, n, m, locked=None, precond="mg", ks=(0, 1, 2)):
        hc = tuple((nd - 1.0) / (max(n) - 1.0) for nd in n)
        h = tuple(x / (nd - 1) for x, nd in zip(hc, n))
        out[name] = dict(n=n, hc=hc, h=h, phi=EL.two_holes(n, h), a=None, a_in=1.0, a_out=1e-3, c=0.0, fixed=EL.face_mask(n, 0, 0), m=m, rho_in=1.0, rho_out=1e-6,
                         rho=None, dtype=np.float64, precond=precond, closed=None, iters=None, ortho=None, locked=locked, ks=tuple(ks))

    add("9x12_m4_lock02", (9, 12), 4, (0, 2))           # act (1, 3): slot j against column act[j] in the preconditioner and in P's coefficients
    add("6x5x7_m3_lock1", (6, 5, 7), 3, (1,))           # N = 3, the active set is not all columns
    add("12x9_m3", (12, 9), 3)                          # the default start, partial Gram tiles: q = 3, 6, 9
    return out


_STEPS = {}


def step_ref(name):
    """_modes_ref.step_ref for a step case: case, hier, mass, x0, and per k `ld`, `eigh`, `jacobi`, yard_x, yard_lam, scale"""
    if name in _STEPS:
        return _STEPS[name]
    cs = step_cases()[name]
    hier, _, Mn = build_case(cs)
    m, kmax = cs["m"], max(cs["ks"])
    x0 = locked_start(hier.ops[0], Mn, m, cs["locked"]) if cs["locked"] is not None else None
    runs = dict(eigh=lobpcg(hier, Mn, m, x0, STEP_RTOL, kmax, cs["precond"], trace=True)["steps"],
                jacobi=lobpcg(hier, Mn, m, x0, STEP_RTOL, kmax, cs["precond"], trace=True, rr=rayleigh_ritz_jacobi)["steps"],
                ld=lobpcg_ld(hier, Mn, m, x0, STEP_RTOL, kmax, cs["precond"])["steps"])
    steps = []
    for k in range(kmax + 1):
        if min(len(v) for v in runs.values()) <= k:
            break
        ld = runs["ld"][k]
        ax = tuple(range(1, ld["X"].ndim))
        scale = np.abs(ld["X"]).max(axis=ax)
        dx = [np.abs(R._aligned(runs[v][k]["X"].astype(LD), ld["X"]) - ld["X"]).max(axis=ax) for v in ("eigh", "jacobi")]
        dl = [np.abs(runs[v][k]["lam"].astype(LD) - ld["lam"]) for v in ("eigh", "jacobi")]
        steps.append(dict(ld=ld, eigh=runs["eigh"][k], jacobi=runs["jacobi"][k], scale=scale, yard_x=np.maximum(np.maximum(dx[0], dx[1]), LD(2.0 ** -53) * scale),
                          yard_lam=np.maximum(np.maximum(dl[0], dl[1]), LD(2.0 ** -53) * ld["lam"])))
    _STEPS[name] = dict(case=cs, hier=hier, mass=Mn, x0=x0, steps=steps)
    return _STEPS[name]
