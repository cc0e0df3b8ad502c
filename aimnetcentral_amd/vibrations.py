"""Harmonic vibrational analysis on the host: wavenumbers and normal modes from a Hessian, IR intensities from the Hessian and
the dipole derivatives (AIMNet2Calculator.eval(hessian=True) and .dipole_derivatives, or AIMNet2ASE.get_hessian and
.get_dipole_derivatives).  numpy only.

Units in: Hessian eV / A^2, masses amu, dipole derivatives e (d(e A) / dA).  Units out: cm^-1 and km / mol.
    omega   = sqrt(lambda),  lambda the eigenvalues of M^-1/2 H M^-1/2;          wavenumber = omega / (2 pi c)
    A_k     = N_A pi / (3 c^2) / (4 pi eps0) * |d mu / d Q_k|^2,                  d mu / d Q_k = sum_ia P[ia,:] L[ia,k] / sqrt(m_i)
(the double-harmonic integrated absorption coefficient).  An imaginary mode (lambda < 0) is reported as a NEGATIVE wavenumber;
all 3N modes are returned, the translations and rotations near zero among them."""
from __future__ import annotations

import math

import numpy as np

# CODATA 2018 (e, N_A and c are exact in the SI)
E_CHARGE = 1.602176634e-19       # C
AMU = 1.66053906660e-27          # kg
N_AVOGADRO = 6.02214076e23       # 1 / mol
C_LIGHT = 299792458.0            # m / s
EPS0 = 8.8541878128e-12          # F / m
ANGSTROM = 1.0e-10               # m

# sqrt(eV A^-2 amu^-1) / (2 pi c), in cm^-1: 521.47
WAVENUMBER_PER_ROOT = math.sqrt(E_CHARGE / (ANGSTROM * ANGSTROM * AMU)) / (2.0 * math.pi * C_LIGHT) / 100.0
# 1 e^2 amu^-1 * N_A pi / (3 c^2) / (4 pi eps0), in km / mol: 974.88
KM_PER_MOL = N_AVOGADRO * math.pi / (3.0 * C_LIGHT * C_LIGHT) / (4.0 * math.pi * EPS0) * E_CHARGE * E_CHARGE / AMU / 1000.0


def _mass_weights(masses, n3: int) -> np.ndarray:
    m = np.asarray(masses, dtype=np.float64).reshape(-1)
    if 3 * m.shape[0] != n3 or not (m > 0).all():
        raise ValueError(f"masses must be {n3 // 3} positive numbers")
    return np.repeat(1.0 / np.sqrt(m), 3)


def normal_modes(hessian, masses):
    """(wavenumbers_cm1 [3N], modes [3N, 3N]): ascending, column k of `modes` is the orthonormal eigenvector of the mass-weighted
    Hessian that belongs to wavenumber k.  `hessian` is (3N,3N) or (N,3,N,3)."""
    H = np.asarray(hessian, dtype=np.float64)
    n3 = int(round(math.sqrt(H.size)))
    H = H.reshape(n3, n3)
    w = _mass_weights(masses, n3)
    lam, modes = np.linalg.eigh(0.5 * (H + H.T) * w[:, None] * w[None, :])
    return np.sign(lam) * np.sqrt(np.abs(lam)) * WAVENUMBER_PER_ROOT, modes


def ir_intensities(hessian, dipole_derivatives, masses):
    """(wavenumbers_cm1 [3N], km_per_mol [3N]).  `dipole_derivatives` is (N,3,3) with P[i,a,b] = d mu_b / d x_ia, or (3N,3)."""
    nu, modes = normal_modes(hessian, masses)
    n3 = nu.shape[0]
    P = np.asarray(dipole_derivatives, dtype=np.float64).reshape(n3, 3)
    dmu_dQ = (modes * _mass_weights(masses, n3)[:, None]).T @ P  # [mode, b]
    return nu, KM_PER_MOL * (dmu_dQ * dmu_dQ).sum(axis=1)
