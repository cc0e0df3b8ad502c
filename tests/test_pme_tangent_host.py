"""The fp64 twin of the particle-mesh Ewald tangent (tests/pme_tangent_yardstick.py) against what it must be the derivative of:
Richardson-extrapolated central differences of oracle.pme.pme_reciprocal's `phi` / `grad` along (v, t_q) with sum t_q = 0 (the
neutralising background is then a constant), and its mesh error against the exact structure-factor sum taken the same way.  CPU only.

Stencil: steps h = 2^-10 A and h / 2 (exactly representable); truncation ~ h^4 times a continuous fifth derivative (the order-8
spline is C^6) ~ 1e-12, rounding ~ 1e-16 / h ~ 1e-13: both orders below the gate of 1e-7 max|ref|.  The h against h / 2 residual is
printed.

Mesh error of the tangent against the exact sum (printed; unit prefactor, q ~ 0.4, t_q ~ 0.3, |v| ~ 1, on |t_g| ~ 0.12 - 0.19;
cells A, B and a 40-atom 14 A cell):   1e-8: t_g 1.1e-8 - 4.9e-8      1e-6: t_g 5.0e-7 - 5.8e-7   (profiles/pme_hessian.md).
Asserted: <= 1e-6 at 1e-8 - what lets the GPU cases at 1e-8 use the sweep's own gate (3.5e-4 and 6.8e-4 eV/A^2 on A and B) with
the mesh error negligible in it."""
from __future__ import annotations

import math

import numpy as np
import pytest

import pme_tangent_yardstick as Y
from oracle import pme as OP
from test_gpu_hvp_ewald import small_cell

H = 2.0 ** -10


def _case(which: str, acc: float):
    """Cell A / B (or a 40-atom 14 A cell) with one atom at fractional coordinate exactly 0, one exactly on a mesh point, and atoms
    several cells outside the box; charges, two directions and charge tangents that sum to zero."""
    c, _, cell = {"A": lambda: small_cell(5, 12, 6.0), "B": lambda: small_cell(5, 16, 7.0), "C": lambda: small_cell(9, 40, 14.0)}[which]()
    x, cell = c.astype(np.float64), cell.astype(np.float64)
    n = len(x)
    alpha, rc, mesh = OP.pme_parameters(n, cell, acc)
    x[0] = 0.0
    x[1] = (np.array([3.0, 2.0, 5.0]) / np.array(mesh)) @ cell
    x[2] += np.array([3.0, -2.0, 1.0]) @ cell
    x[3] += np.array([-4.0, 0.0, 5.0]) @ cell
    rng = np.random.default_rng(17)
    q = rng.normal(0.0, 0.4, n)
    tq = rng.normal(0.0, 0.3, (2, n))
    tq -= tq.mean(axis=1, keepdims=True)
    v = rng.standard_normal((2, n, 3))
    return x, q, tq, v, cell, alpha, mesh


def _differences(fn, x, q, tq, v):
    """(tphi, tg, residuals) of `fn(x, q) -> dict(phi, grad)` along every direction"""
    tphi, tg, res = [], [], []
    for k in range(v.shape[0]):
        a, ra = Y.richardson(lambda t, k=k: fn(x + t * v[k], q + t * tq[k])["phi"], H)
        b, rb = Y.richardson(lambda t, k=k: fn(x + t * v[k], q + t * tq[k])["grad"], H)
        tphi.append(a), tg.append(b), res.append(max(ra, rb))
    return np.array(tphi), np.array(tg), max(res)


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("acc", [1e-6, 1e-8])
def test_twin_is_the_derivative_of_the_mesh_sum(which, acc):
    x, q, tq, v, cell, alpha, mesh = _case(which, acc)
    got = Y.pme_tangent(x, q, tq, v, cell, alpha, mesh)
    ref = OP.pme_reciprocal(x, q, cell, alpha, mesh)
    phi_bg = -math.pi * q.sum() / (abs(np.linalg.det(cell)) * alpha * alpha)
    assert np.abs(got["phi"] + phi_bg - ref["phi"]).max() < 1e-12 * max(1.0, np.abs(ref["phi"]).max())
    assert np.abs(got["g"] - ref["grad"]).max() < 1e-12 * max(1.0, np.abs(ref["grad"]).max())
    assert np.abs(got["T"] - got["T"].transpose(0, 2, 1)).max() < 1e-15 * max(1.0, np.abs(got["T"]).max())  # (rounding of inv Tu inv^T)
    tphi, tg, res = _differences(lambda xx, qq: OP.pme_reciprocal(xx, qq, cell, alpha, mesh), x, q, tq, v)
    for name, a, b in (("tphi", got["tphi"], tphi), ("tg", got["tg"], tg)):
        err, gate = np.abs(a - b).max(), 1e-7 * np.abs(b).max()
        print(f"[pme-tangent host] {which} acc {acc:g} mesh {mesh}: {name} max|d| = {err:.3e} on max|ref| = {np.abs(b).max():.3e}, "
              f"gate {gate:.3e}, ratio {err / gate:.2e}; h against h/2 residual {res:.3e}")
        assert err <= gate


@pytest.mark.parametrize("which", ["A", "B", "C"])
@pytest.mark.parametrize("acc", [1e-6, 1e-8])
def test_mesh_error_of_the_tangent_against_the_exact_sum(which, acc):
    x, q, tq, v, cell, alpha, mesh = _case(which, acc)
    got = Y.pme_tangent(x, q, tq, v, cell, alpha, mesh)
    kc = math.sqrt(2.0) * math.sqrt(-2.0 * math.log(acc)) * alpha
    tphi, tg, res = _differences(lambda xx, qq: OP.exact_reciprocal(xx, qq, cell, alpha, kc), x, q, tq, v)
    e_phi, e_g = np.abs(got["tphi"] - tphi).max(), np.abs(got["tg"] - tg).max()
    print(f"[pme-tangent host] mesh error {which} acc {acc:g} mesh {mesh}: tphi {e_phi:.3e} on {np.abs(tphi).max():.3e}, "
          f"tg {e_g:.3e} on {np.abs(tg).max():.3e} (residual {res:.3e})")
    if acc == 1e-8:
        assert e_g <= 1e-6
