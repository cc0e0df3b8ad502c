"""The directions and the fp64 reference of the strain tangent (csrc/hvp.hip armed by aimnet_engine_set_strain_tangent), shared by
tests/test_strain_reference.py (CPU: the reference against two exact identities) and tests/test_gpu_strain_tangent.py.

Reference.  Direction k = (v_k [N,3], eps_k [3,3]) is the path x(t) = x (1 + t eps_k) + t v_k, cell(t) = cell (1 + t eps_k) in the
row-vector convention of the stress.  oracle.aimnet2_analytic.evaluate(..., stress=True) keeps float64 inputs and runs on FIXED
lists with shifts, so along the path G = -forces and S = stress x volume are smooth functions of t, and their 4-point central
difference at h = 1e-4 is the derivative itself (h = 1e-4 and 1e-5 agree to 1e-8 where |dG|, |dS| are about 1e2; with eps = 0 the
difference meets evaluate_hvp's hv to 9e-9).  The path is built on the oracle's wrapped coordinates and lists (tangent_cases.lists).

Directions of a case (`directions`): the six Voigt strains with v = 0, one non-symmetric strain with a random v, one pure
displacement, one rotation (antisymmetric strain, v = 0).

Identities (exact; `rotation_residual`, `mixed_residual`):
    rotation   eps = w antisymmetric, v = 0:  dG = G w,  dS = S w + w^T S
    mixed      eps : dS(v, 0) - sum_i v_i . dG_i(0, eps) = sum_i (v_i eps) . G_i     per system"""
from __future__ import annotations

import numpy as np

import tangent_cases as T
from aimnetcentral_amd import elasticity

FD_STEP = 1e-4
CASES = ("tiny3-dsf8", "tiny3-none", "tiny1-TTF", "tiny2-flags", "nse-tiny1-TTF")
ROTATION = np.array([[0.0, 0.3, -0.2], [-0.3, 0.0, 0.1], [0.2, -0.1, 0.0]])
_REFS: dict = {}
_DIRS: dict = {}


def case(name: str):
    """tangent_cases.case, plus "tiny3-none": tiny3-dsf8 without an external Coulomb term."""
    if name == "tiny3-none":
        from types import SimpleNamespace

        c = T.case("tiny3-dsf8")
        return SimpleNamespace(**{**vars(c), "name": name, "coul": dict(coulomb="none")})
    return T.case(name)


def directions(name: str):
    """(V [9, N, 3], EPS [9, 3, 3]) float64: 0-5 Voigt strains, 6 non-symmetric strain with a random v, 7 displacement, 8 rotation."""
    if name not in _DIRS:
        n = len(case(name).numbers)
        rng = np.random.default_rng(5)
        V, E = np.zeros((9, n, 3)), np.zeros((9, 3, 3))
        E[:6] = elasticity.voigt_strains()
        E[6], V[6] = rng.standard_normal((3, 3)) * 0.5, rng.standard_normal((n, 3))
        V[7] = rng.standard_normal((n, 3))
        E[8] = ROTATION
        # what the engine is given is float32: the reference takes the same numbers
        _DIRS[name] = (V.astype(np.float32).astype(np.float64), E.astype(np.float32).astype(np.float64))
    return _DIRS[name]


class Reference:
    """G(x, cell) and S(x, cell) of a case in float64 on its fixed lists, and their derivative along a direction."""

    def __init__(self, name: str, om64):
        from oracle import aimnet2_analytic as AN

        c = self.case = case(name)
        ref, xw, nbl, shl = T.lists(c, om64)
        self.xw = np.asarray(xw, np.float64)
        self.cells = np.asarray(c.cell, np.float64).reshape(-1, 3, 3)
        self.n, self.n_mol = len(c.numbers), len(c.charge)
        kw = {k: v for k, v in c.coul.items() if k != "coulomb"}

        def gs(x, cells):
            r = AN.evaluate(om64, x, c.numbers, c.charge, c.mol, ref["nbmat"], shifts=ref.get("shifts"),
                            cell=cells if len(cells) > 1 else cells[0], coulomb=c.coul["coulomb"], nbmat_lr=nbl, shifts_lr=shl,
                            stress=True, mult=c.mult, **kw)
            vol = np.abs(np.linalg.det(cells))
            return -np.asarray(r["forces"], np.float64), np.asarray(r["stress"], np.float64).reshape(-1, 3, 3) * vol[:, None, None]

        self._gs = gs
        self.G, self.S = gs(self.xw, self.cells)
        self.volume = np.abs(np.linalg.det(self.cells))

    def derivative(self, v, eps, h: float = FD_STEP):
        """(dG/dt [N,3], dS/dt [n_mol,3,3]) at t = 0 along (v, eps): 4-point central difference."""
        def at(t):
            s = np.eye(3) + t * eps
            return self._gs(self.xw @ s + t * v, self.cells @ s)

        g = {k: at(k * h) for k in (1, -1, 2, -2)}
        return tuple((8.0 * (g[1][q] - g[-1][q]) - (g[2][q] - g[-2][q])) / (12.0 * h) for q in (0, 1))

    def per_system(self, a):
        """sum over the atoms of each system of a per-atom scalar [N]."""
        out = np.zeros(self.n_mol)
        np.add.at(out, self.case.mol, a)
        return out


def reference(name: str, om64) -> dict:
    """{"ref": Reference, "V", "EPS", "hv" [9,N,3], "dvirial" [9,n_mol,3,3], "G", "S"} once per case name; left unchanged."""
    if name not in _REFS:
        r = Reference(name, om64)
        V, E = directions(name)
        d = [r.derivative(v, e) for v, e in zip(V, E)]
        _REFS[name] = {"ref": r, "V": V, "EPS": E, "hv": np.stack([x[0] for x in d]), "dvirial": np.stack([x[1] for x in d]),
                       "G": r.G, "S": r.S}
    return _REFS[name]


def rotation_residual(G, S, dG, dS, w=ROTATION):
    """(max |dG - G w|, max |dS - (S w + w^T S)|) for the direction (v = 0, eps = w antisymmetric)."""
    return float(np.abs(dG - G @ w).max()), float(np.abs(dS - (S @ w + w.T @ S)).max())


def mixed_residual(mol, n_mol, G, v, eps, dS_v, dG_eps):
    """eps : dS(v, 0) - sum_i v_i . dG_i(0, eps) - sum_i (v_i eps) . G_i per system [n_mol]: zero."""
    def per_system(a):
        out = np.zeros(n_mol)
        np.add.at(out, mol, a)
        return out

    return np.einsum("mab,ab->m", dS_v, eps) - per_system((v * dG_eps).sum(-1)) - per_system(((v @ eps) * G).sum(-1))
