"""Host side of the charge response (no GPU): that the yardstick of tests/test_gpu_charge_response.py - the intermediate `_t_q1`
of the fp64 tangent sweep, oracle/aimnet2_analytic.py::evaluate_hvp - IS the derivative of the charges the oracle returns; the
unit factors and the mode algebra of aimnetcentral_amd/vibrations.py on a two-mass spring; and the null-handle contract of the two
C entry points."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

from conftest import golden


def _case(name):
    if name == "nse_b5":
        g = golden("nse")
        return g["b5_coord"], g["b5_numbers"], g["b5_charge"], g["b5_mol_idx"], g["b5_mult"]
    g = golden(name)
    n = len(g["numbers"])
    return g["coord"], g["numbers"], g["charge"], g["mol_idx"] if "mol_idx" in g.files else np.zeros(n, dtype=np.int64), None


@pytest.mark.parametrize("name", ["hvp40", "taxol", "batch5", "nse_b5"])
def test_t_q1_is_the_derivative_of_the_charges(oracle64, oracle64_nse, name):
    """Central differences of O.evaluate(...)["charges"] (and "spin_charges") at h = 1e-3 A along direction 0 against `_t_q1`;
    gate 1e-3 max|t_q|, with max|t_q| taken over direction 0 alone (measured 4.1e-4, 5.7e-4, 1.5e-4, 1.9e-4 / 1.1e-4: the floor is
    the oracle's fp32 cast of the displaced coordinates).  The tangent of the pass before, `_t_q0`, misses by 70 - 170 % of
    max|t_q|: a wrong intermediate cannot pass."""
    from oracle import aimnet2_analytic as AN
    from oracle import aimnet2_oracle as O

    coord, numbers, charge, mol, mult = _case(name)
    om = oracle64_nse if mult is not None else oracle64
    n, h = len(numbers), 1e-3
    v = np.random.default_rng(11).standard_normal((3, n, 3)).astype(np.float32)[:1]
    ref = O.evaluate(om, coord, numbers, charge, mol, return_intermediates=True, forces=False, mult=mult)
    nbl, shl = O.neighbor_list(ref["coord_wrapped"], float("inf"), mol)
    spec = AN.evaluate_hvp(om, ref["coord_wrapped"], numbers, charge, mol, ref["nbmat"], v, coulomb="simple", nbmat_lr=nbl,
                           shifts_lr=shl, mult=mult, return_intermediates=True)
    x = np.asarray(coord, dtype=np.float64)
    plus = O.evaluate(om, x + h * v[0], numbers, charge, mol, forces=False, mult=mult)
    minus = O.evaluate(om, x - h * v[0], numbers, charge, mol, forces=False, mult=mult)
    fd = [(np.asarray(plus["charges"], np.float64) - np.asarray(minus["charges"], np.float64)) / (2 * h)]
    t1, t0 = spec["_t_q1"][0], spec["_t_q0"][0]
    got, wrong = [t1.sum(-1)], [t0.sum(-1)]
    if mult is not None:
        fd.append((np.asarray(plus["spin_charges"], np.float64) - np.asarray(minus["spin_charges"], np.float64)) / (2 * h))
        got.append(t1[:, 0] - t1[:, 1])
        wrong.append(t0[:, 0] - t0[:, 1])
    top = np.abs(t1).max()
    for what, a, b, w in zip(("charges", "spin_charges"), got, fd, wrong):
        err, err0 = np.abs(a - b).max(), np.abs(w - b).max()
        print(f"{name} {what}: max|t_q1 - fd| = {err / top:.2e} max|t_q|, max|t_q0 - fd| = {err0 / top:.2e} max|t_q| (max|t_q| = {top:.3f})")
        assert err <= 1e-3 * top, f"{name} {what}: {err:.3e} > 1e-3 * {top:.3e}"
        assert err0 > 1e-3 * top


def test_two_mass_spring():
    """Masses m1 != m2 on the x axis joined by a spring k (eV/A^2), polar tensor +-q on the axis: one mode at
    521.47 sqrt(k / mu) cm^-1 with 974.88 q^2 / mu km/mol, the other five at zero wavenumber and zero intensity."""
    from aimnetcentral_amd import vibrations as vib

    assert abs(vib.WAVENUMBER_PER_ROOT - 521.47) < 0.005 and abs(vib.KM_PER_MOL - 974.88) < 0.005
    k, m1, m2, q = 31.0, 1.008, 18.998, 0.43
    mu = m1 * m2 / (m1 + m2)
    H = np.zeros((6, 6))
    H[0, 0] = H[3, 3] = k
    H[0, 3] = H[3, 0] = -k
    P = np.zeros((2, 3, 3))
    P[0, 0, 0], P[1, 0, 0] = q, -q
    nu, modes = vib.normal_modes(H.reshape(2, 3, 2, 3), [m1, m2])
    nu2, inten = vib.ir_intensities(H, P, [m1, m2])
    assert nu.shape == (6,) and modes.shape == (6, 6) and np.array_equal(nu, nu2) and inten.shape == (6,)
    assert abs(nu[-1] / (521.47 * math.sqrt(k / mu)) - 1.0) < 1e-4
    assert abs(inten[-1] / (974.88 * q * q / mu) - 1.0) < 1e-4
    assert np.abs(nu[:5]).max() < 1e-3 and np.abs(inten[:5]).max() < 1e-9 * inten[-1]
    assert np.allclose(modes.T @ modes, np.eye(6), atol=1e-12)
    nu_neg, inten_neg = vib.ir_intensities(-H, P.reshape(6, 3), [m1, m2])  # an imaginary mode: negative wavenumber, sorted first
    assert abs(nu_neg[0] / (-521.47 * math.sqrt(k / mu)) - 1.0) < 1e-4 and np.abs(nu_neg[1:]).max() < 1e-3
    assert abs(inten_neg[0] / (974.88 * q * q / mu) - 1.0) < 1e-4
    with pytest.raises(ValueError):
        vib.normal_modes(H, [m1])


def test_entry_points_with_null_handles():
    from aimnetcentral_amd import _lib

    lib = _lib.load()
    opt = _lib.EvalOptions()
    assert lib.aimnet_engine_charge_response_workspace_bytes(None, 10, 1, 1, C.byref(opt)) == 0
    inp = _lib.Inputs(n_atoms=10, n_mol=1)
    rc = lib.aimnet_engine_charge_response(None, C.byref(inp), C.byref(opt), None, 1, None, None, None, None, None, None, 0, None)
    assert rc == _lib.E_INVALID
