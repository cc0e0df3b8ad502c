"""The fp64 reference of the strain tangent (tests/strain_cases.py: 4-point central differences of the oracle's -forces and
stress x volume along x (1 + t eps) + t v on fixed lists) against what it must satisfy exactly: with eps = 0 it is evaluate_hvp's
product; an antisymmetric strain is a rotation (dG = G w, dS = S w + w^T S); and the mixed second derivative is the same from
both sides (eps : dS(v) - sum v . dG(eps) = sum (v eps) . G per system).  Bounds: the difference quotient at h = 1e-4 of values of
size 1e2 computed in float64 carries 1e-16 x 1e2 / 1e-4 = 1e-10 of rounding per evaluation and an h^4 truncation term of the same
order; 1e-7 (absolute, on |dG|, |dS| up to about 1e2) leaves room for both and is two orders below the fp32 gates of the GPU
tests.  CPU only; the two cases with more than one system."""
from __future__ import annotations

import numpy as np
import pytest

import strain_cases as SC
import tangent_cases as T

TOL = 1e-7


@pytest.mark.parametrize("name", ["tiny3-dsf8", "tiny2-flags"])
def test_reference_meets_the_identities(name, oracle64):
    ref = SC.reference(name, oracle64)
    r, V, E, hv, dS = ref["ref"], ref["V"], ref["EPS"], ref["hv"], ref["dvirial"]
    c = r.case
    assert hv.shape == (9, r.n, 3) and dS.shape == (9, r.n_mol, 3, 3) and r.n_mol > 1
    assert np.abs(hv).max() > 1.0 and np.abs(dS).max() > 1.0  # (the identities below are not about zeros)
    # pure displacement: the tangent sweep's own product
    _, spec = T.sweep(c, oracle64, V=V[7:8])
    err = np.abs(hv[7] - np.asarray(spec["hv"], np.float64)[0]).max()
    print(f"[strain-reference] {name} displacement vs evaluate_hvp: {err:.2e} of {np.abs(hv[7]).max():.2e}")
    assert err < TOL
    # rotation
    eg, es = SC.rotation_residual(ref["G"], ref["S"], hv[8], dS[8], E[8])
    print(f"[strain-reference] {name} rotation: |dG - G w| = {eg:.2e}, |dS - (S w + w^T S)| = {es:.2e}")
    assert eg < TOL and es < TOL
    # mixed derivative: displacement direction 7 against each strain direction with v = 0
    for k in range(7):
        if k == 6:  # (direction 6 carries a displacement too: its strain part alone is differenced here)
            dG_eps = r.derivative(np.zeros_like(V[6]), E[6])[0]
        else:
            dG_eps = hv[k]
        res = SC.mixed_residual(c.mol, r.n_mol, ref["G"], V[7], E[k], dS[7], dG_eps)
        print(f"[strain-reference] {name} mixed derivative, strain {k}: residual {np.abs(res).max():.2e}")
        assert np.abs(res).max() < TOL
    # step consistency of one strain direction
    dG5, dS5 = r.derivative(V[6], E[6], h=1e-5)
    assert np.abs(dG5 - hv[6]).max() < TOL and np.abs(dS5 - dS[6]).max() < TOL


def test_the_directions_are_what_the_engine_is_given():
    V, E = SC.directions("tiny3-dsf8")
    assert np.array_equal(V, V.astype(np.float32)) and np.array_equal(E, E.astype(np.float32))
    assert np.array_equal(E[8], -E[8].T) and not np.allclose(E[6], E[6].T) and not V[:6].any() and not E[7].any()
