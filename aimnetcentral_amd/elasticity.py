"""Elastic constants on the host from the strain directions of the tangent sweep (AIMNet2Calculator.elastic_constants, or
HipEngine.hvp(..., strain=) directly).  numpy only, float64.

Conventions.  Row vectors: a strain s moves x -> x (1 + s) and cell -> cell (1 + s).  Voigt order xx, yy, zz, yz, xz, xy with
engineering shear strains: a unit Voigt strain e_I is the SYMMETRIC matrix with 1 on the diagonal (I < 3) or 1/2 in both
off-diagonal places (I >= 3), so that the energy density of a small strain is 1/2 e_I C_IJ e_J.

What the sweep returns for a direction (v = 0, strain = eps) is dS/dt, the tangent of the virial S_ab = dE / d eta_ab taken with
respect to a further MULTIPLICATIVE scaling x (1 + eta) of the configuration at t.  The second derivative of the energy with
respect to the ADDITIVE strain x -> x + x s of the one reference configuration,
    A_ab,cd = d2E / ds_ab ds_cd   at s = 0,
differs from it by the first-order term: along eps, dS = A : eps + eps^T S, so A : eps = dS - eps^T S.  Then
    born_IJ            = (1/V) e_I : A : e_J                           clamped ions
    internal_strain    L[i,c,J] = d2E / dx_ic de_J = dG_ic/dt along e_J (the sweep's hv)
    relaxed            = born - (1/V) L^T H^+ L                         ions relaxed at fixed strain
with H the Hessian and H^+ its inverse on the complement of the three uniform translations (H annihilates them, and so does L).
`born` and `relaxed` are the elastic (stress-strain) tensor only where the reference configuration has zero stress and zero
forces; under stress they are the second derivatives of the energy per volume named above, and stress-strain coefficients take
further terms in S / V that are the caller's choice of strain measure; with non-zero forces `relaxed` is not a second derivative
of a relaxed energy at all.  Units: eV / A^3 (EV_A3_TO_GPA converts)."""
from __future__ import annotations

import numpy as np

EV_A3_TO_GPA = 1.602176634e-19 / 1.0e-30 / 1.0e9  # 1 eV / A^3 = 160.2176634 GPa (e is exact in the SI)

VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))


def voigt_strains() -> np.ndarray:
    """(6, 3, 3): the symmetric matrix of each unit Voigt strain (engineering shear: 1/2 in both off-diagonal places)."""
    e = np.zeros((6, 3, 3))
    for I, (a, b) in enumerate(VOIGT):
        e[I, a, b] += 0.5
        e[I, b, a] += 0.5
    return e


def born_tensor(dvirial, virial, volume: float, strains=None) -> np.ndarray:
    """(6,6) clamped-ion tensor from dS/dt [6,3,3] along `strains` (default: voigt_strains()), the virial S [3,3] and the volume:
    (1/V) e_I : (dS_J - e_J^T S), symmetrised over (I, J) (it is symmetric up to the round-off of the sweep)."""
    e = voigt_strains() if strains is None else np.asarray(strains, dtype=np.float64)
    dS, S = np.asarray(dvirial, dtype=np.float64).reshape(6, 3, 3), np.asarray(virial, dtype=np.float64).reshape(3, 3)
    A = dS - np.einsum("jca,cb->jab", e, S)  # eps^T S
    B = np.einsum("iab,jab->ij", voigt_strains(), A) / float(volume)
    return 0.5 * (B + B.T)


def translation_complement(n: int) -> np.ndarray:
    """(3n, 3n - 3): an orthonormal basis of the displacements with no uniform translation in them."""
    T = np.tile(np.eye(3), (n, 1)) / np.sqrt(n)  # (3n, 3) orthonormal translations
    q, _ = np.linalg.qr(np.concatenate([T, np.eye(3 * n)], axis=1))
    return q[:, 3:]


def relaxed_tensor(born, internal_strain, hessian, volume: float) -> np.ndarray:
    """born - (1/V) L^T H^+ L: `internal_strain` (N,3,6) or (3N,6), `hessian` (N,3,N,3) or (3N,3N), symmetrised; H^+ is the inverse
    on the complement of the three translations (a structure with further zero modes has no relaxed tensor: LinAlgError)."""
    L = np.asarray(internal_strain, dtype=np.float64).reshape(-1, 6)
    n3 = L.shape[0]
    H = np.asarray(hessian, dtype=np.float64).reshape(n3, n3)
    H = 0.5 * (H + H.T)
    if n3 == 3:  # one atom: nothing relaxes
        return np.asarray(born, dtype=np.float64).copy()
    Q = translation_complement(n3 // 3)
    LQ = Q.T @ L
    return np.asarray(born, dtype=np.float64) - LQ.T @ np.linalg.solve(Q.T @ H @ Q, LQ) / float(volume)


def elastic_tensors(hv_displacements, hv_strains, dvirial, virial, volume: float) -> dict:
    """The results of one sweep -> `born`, `internal_strain`, `hessian`, `relaxed`.  hv_displacements [3N,3N]: row k = H e_k of the
    unit displacements; hv_strains [6,N,3] and dvirial [6,3,3]: dG/dt and dS/dt of the six Voigt strains; virial [3,3]."""
    H = np.asarray(hv_displacements, dtype=np.float64)
    n3 = H.shape[0]
    H = 0.5 * (H + H.T)
    L = np.moveaxis(np.asarray(hv_strains, dtype=np.float64).reshape(6, n3), 0, -1)  # (3N, 6)
    born = born_tensor(dvirial, virial, volume)
    n = n3 // 3
    return {"born": born, "internal_strain": L.reshape(n, 3, 6), "hessian": H.reshape(n, 3, n, 3),
            "relaxed": relaxed_tensor(born, L, H, volume)}
