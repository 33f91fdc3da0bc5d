"""One FAST stage of WENO5 advection + Eikonal (current sign), and of WENO5 advection alone, against the oracle on fields
that stress the WENO5 smoothness terms, the weight ratio and the Godunov clamps of csrc/stage_math.h:
exact zeros and -0.0 in the ENO pair and the second differences, w₂ = -w₃, values at both ends of FAST's range, flat data.

The spacing is 1/8 in every dimension, so node coordinates, |x - x₀| and the sawtooth are exact in binary and the zeros
are exact zeros.  The velocity is separable (the compile-time 'plain' kernel variant runs) and every component changes
sign along another axis several times: some waves see one sign of u_d and take the uniform paths, others straddle a
change and take the per-lane path; the same holds for the sign of ϕ in the Eikonal term.
"""
import numpy as np
import pytest

from test_gpu_parity import TOL_STAGE, _run_stage

pytestmark = pytest.mark.gpu

H = 0.125
SHAPES = [(40, 12, 10),    # two x tiles with a ragged one, two y tiles, one short march chunk
          (300, 9),        # 2-D path
          (70,)]           # 1-D path


def _coords(shape):
    return [np.arange(n, dtype=np.float64) * H for n in shape]


def _mesh(shape):
    return np.meshgrid(*_coords(shape), indexing="ij", sparse=True)


def _sphere(shape):
    xs = _mesh(shape)
    ctr = [(n // 2) * H + 0.03 for n in shape]
    rad = 0.3 * min((n - 1) * H for n in shape)
    return np.sqrt(sum((x - c) ** 2 for x, c in zip(xs, ctr))) - rad


def _fields(shape):
    nd = len(shape)
    xs = _mesh(shape)
    full = lambda a: np.asfortranarray(np.broadcast_to(a, shape).copy())
    out = {"sphere": full(_sphere(shape))}
    # |x - x₀| + |y - y₀| with the kink on nodes (1-D: |x - x₀|; constant along z), shifted so that ϕ changes sign
    kink = sum(np.abs(x - (n // 2) * H) for x, n in zip(xs[:2], shape[:2])) - 3 * H
    out["kink"] = full(kink)
    for a in range(nd):
        saw = np.where(np.arange(shape[a]) % 2 == 0, 1.0, -1.0).reshape([-1 if k == a else 1 for k in range(nd)])
        out[f"saw{a}"] = full(saw + 0.1 * _sphere(shape))
    out["sphere*1e-30"] = out["sphere"] * 1e-30
    out["sphere*1e+30"] = out["sphere"] * 1e30
    out["constant"] = full(np.full((1,) * nd, 0.25))
    return out


def _velocity(shape):
    """Separable tables: component d changes sign along axis (d+1) mod nd and is positive along the others."""
    nd = len(shape)
    cs = _coords(shape)
    tables = []
    for d in range(nd):
        comp = []
        for k in range(nd):
            L = (shape[k] - 1) * H
            if k == (d + 1) % nd:
                comp.append((-1.0) ** d * np.sin(2 * np.pi * 1.5 * cs[k] / L + 0.3))
            else:
                comp.append(1.0 + 0.5 * np.cos(2 * np.pi * cs[k] / L))
        tables.append(comp)
    return ("sep", tables, ("cos", 3.0))


_CASES = {}


def _case(hip, shape):
    if shape not in _CASES:
        nd = len(shape)
        _CASES[shape] = hip.Case(shape, "neumann", lc=(0.0,) * nd, hc=tuple((n - 1) * H for n in shape), mode="fast")
    return _CASES[shape]


@pytest.fixture(scope="module")
def hip():
    import _hip
    yield _hip
    _CASES.clear()


@pytest.mark.parametrize("terms", ["adv+eik", "adv"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fast_stage_on_stress_fields(hip, orc, shape, terms):
    c = _case(hip, shape)
    assert all(c.grid.meshsize(d) == H for d in range(len(shape)))
    vel = _velocity(shape)
    specs = [("adv", vel, "weno5")] + ([("eik", None)] if terms == "adv+eik" else [])
    failures = []
    for name, phi in _fields(shape).items():
        got, want, _, _ = _run_stage(c, orc, specs, phi, 0, t=0.4)
        scale = np.abs(want).max()
        err = np.abs(got - want).max()
        print(f"{'x'.join(map(str, shape)):>9s} {terms:8s} {name:13s} max|Δ| = {err:.3e} = {err / scale:.2e}·max|ϕ|")
        if not np.isfinite(got).all() or not err <= TOL_STAGE * scale:
            failures.append((name, float(err), float(scale)))
    assert not failures, failures
