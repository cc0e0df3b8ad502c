"""fp64 yardstick of the electrostatic embedding in the analytic Hessian sweep (atoms move along v, sites are clamped), shared by
tests/test_embedding_hessian_host.py, tests/test_gpu_embedding_hessian.py and tests/golden/make_embedding_hessian.py.

The oracle has no autograd path for sum_i q_i phi_i, so the yardstick is a central difference of the embedded forces of
tests/embedding_yardstick.py (`embedded_reference`: `forces` on the atoms, `f_site` on the sites), Richardson-extrapolated:

    D(h) = -(F(x + h v) - F(x - h v)) / (2 h)        R(h, h/2) = (4 D(h/2) - D(h)) / 3        (error O(h^4))

for H v, and the same of -f_site for the mixed block ext_hv[k, A] = sum_i (d2 E / dX_A dx_i) v_i^k.  The oracle rounds the
coordinates it is given to fp32, so everything is made exactly representable: coordinates on the grid 2^-16 A, directions on the
grid 2^-4, h in {2^-10, 2^-11, 2^-12} - every displaced coordinate is then a multiple of 2^-16 below 256 A, an fp32 number, and
`_forces` asserts that before each evaluation.  `yardstick` asserts that the two extrapolants R(h, h/2) and R(h/2, h/4) agree to 1 %
of the gate they are used with (1e-5 + 3e-5 max|ref|, tests/tangent_cases.py::hv_gate, on hv and on ext_hv each) and returns the finer.

The closed-form addends of the sweep's seeds, in numpy fp64 (`addends`):  t_q g,  q T v,  J t_phi  with  t_phi_j = g_j . v_j,
J[(i,c), j] = dq_j / dx_ic and t_q = J^T v from the `_t_q1` intermediate (tests/embedding_yardstick.py::model_reference), and the
field-gradient tensor T = k_e sum_A Q_A (3 r r^T / d^5 - 1 / d^3) itself (`tensor`)."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import embedding_yardstick as Y
from conftest import golden

GRID_X, GRID_V = 2.0**-16, 2.0**-4
STEPS = (2.0**-10, 2.0**-11, 2.0**-12)
RICHARDSON_FRACTION = 0.01  # of the gate

_CASES: dict = {}
_YARD: dict = {}


def on_grid(a, step):
    return np.round(np.asarray(a, np.float64) / step) * step


def directions(n: int, k: int = 3, seed: int = 11):
    """k random directions [k, n, 3] on the grid 2^-4 (standard normal, rounded)."""
    return on_grid(np.random.default_rng(seed).standard_normal((k, n, 3)), GRID_V).astype(np.float32)


def gate(ref_values) -> float:
    """tests/tangent_cases.py::tangent_gate: 1e-5 + 3e-5 max|ref|."""
    return float(1e-5 + 3e-5 * np.abs(ref_values).max())


def _case(name, coord, numbers, charge, mol, mult, site_plan, nse=False, k=3):
    """site_plan: {molecule: (M, seed)} - the construction of embedding_yardstick.sites around that molecule."""
    x = on_grid(coord, GRID_X).astype(np.float32)
    mol = np.asarray(mol, np.int64)
    Xs, Qs, ms = [], [], []
    for m, (M, seed) in sorted(site_plan.items()):
        X, Q = Y.sites(x[mol == m], M, seed)
        Xs.append(X), Qs.append(Q), ms.append(np.full(M, m, np.int64))
    return SimpleNamespace(name=name, coord=x, numbers=np.asarray(numbers), charge=np.atleast_1d(np.asarray(charge, np.float32)), mol=mol,
                           mult=None if mult is None else np.atleast_1d(np.asarray(mult, np.float32)), X=np.concatenate(Xs),
                           Q=np.concatenate(Qs), ext_mol=np.concatenate(ms), jac_mols=tuple(sorted(site_plan)), nse=nse,
                           V=directions(len(x), k))


def _single(name):
    g = golden(name)
    return _case(name, g["coord"], g["numbers"], 0.0, np.zeros(len(g["numbers"]), np.int64), None, {0: (64, 5)})


def _one_molecule(name, g, m, prefix="", nse=False, k=1):
    at = g[prefix + "mol_idx"] == m
    return _case(name, g[prefix + "coord"][at], g[prefix + "numbers"][at], g[prefix + "charge"][m:m + 1], np.zeros(int(at.sum()), np.int64),
                 g[prefix + "mult"][m:m + 1] if nse else None, {0: (64, 5)}, nse=nse, k=k)


def _batch5():
    g = golden("batch5")  # the sites of tests/test_gpu_embedding.py::_batch_sites: molecules 2 and 4 own none, molecule 1 owns one
    return _case("batch5", g["coord"], g["numbers"], g["charge"], g["mol_idx"], None, {0: (64, 5), 1: (1, 7), 3: (64, 6)})


def _nse_b5():
    g = golden("nse")  # the sites of tests/test_gpu_embedding.py::test_two_channel_model
    return _case("nse_b5", g["b5_coord"], g["b5_numbers"], g["b5_charge"], g["b5_mol_idx"], g["b5_mult"], {1: (16, 6), 3: (16, 8)}, nse=True)


BUILDERS = {
    "cold24": lambda: _single("cold24"),
    "hvp40": lambda: _single("hvp40"),
    "batch5": _batch5,
    "nse_b5": _nse_b5,
    # the CPU cases: the smallest molecule of batch5 (11 atoms; the first of the two), and a doublet of the two-channel batch
    "batch5_mol0": lambda: _one_molecule("batch5_mol0", golden("batch5"), 0),
    "nse_b5_mol3": lambda: _one_molecule("nse_b5_mol3", golden("nse"), 3, "b5_", nse=True),
}
GPU_CASES = ("cold24", "hvp40", "batch5", "nse_b5")  # their yardsticks are committed: tests/golden/embedding_hessian.npz


def case(name: str):
    if name not in _CASES:
        _CASES[name] = BUILDERS[name]()
    return _CASES[name]


def model_at(c, om64, xx, key=None):
    """embedding_yardstick.model_reference at the coordinates xx (not kept unless `key` names it)."""
    k = ("embedding_hessian", c.name, "x0") if key is None else key
    ref = Y.model_reference(om64, k, xx, c.numbers, c.charge if len(c.charge) > 1 else float(c.charge[0]), c.mol, c.mult,
                            jac_mols=c.jac_mols)
    if key is None:
        Y._REFS.pop(k)
    return ref


def _forces(c, om64, xx, E=None):
    """The embedded forces at xx and, with the case's sites, the forces on them; with a uniform field E (V/A; phi = -E.x, grad phi =
    -E, no sites) the embedding's own part F_emb = -(q g + J phi) of the forces in their place."""
    assert (xx.astype(np.float32).astype(np.float64) == xx).all(), "a displaced coordinate is not an fp32 number"
    ref = model_at(c, om64, xx.astype(np.float32))
    if E is None:
        emb = Y.embedded_reference(ref, xx, c.X, c.Q, c.mol, c.ext_mol)
        return emb["forces"], emb["f_site"]
    n = len(xx)
    f_emb = -(ref["charges"][:, None] * (-np.asarray(E, np.float64))[None] + (ref["J"] @ (-(xx @ E))).reshape(n, 3))
    return ref["forces"] + f_emb, f_emb


def richardson(c, om64, v, E=None):
    """One direction v [N, 3] (on the grid): the extrapolants R(h, h/2) and R(h/2, h/4) of H v and of ext_hv (uniform field E: of
    H v and of H v - H_bare v)."""
    x = c.coord.astype(np.float64)
    v = np.asarray(v, np.float64)
    assert (on_grid(v, GRID_V) == v).all() and (on_grid(x, GRID_X) == x).all()
    D, S = [], []
    for h in STEPS:
        fp, sp = _forces(c, om64, x + h * v, E)
        fm, sm = _forces(c, om64, x - h * v, E)
        D.append(-(fp - fm) / (2 * h))
        S.append(-(sp - sm) / (2 * h))
    R = lambda d: ((4 * d[1] - d[0]) / 3, (4 * d[2] - d[1]) / 3)  # noqa: E731
    return R(D), R(S)


def yardstick(c, om64, V=None, E=None):
    """hv [K, N, 3] and ext_hv [K, M, 3] of the case for the directions V (default: its own, kept), with the agreement of the two
    extrapolants (`agree_hv`, `agree_ext`) - asserted to stay within 1 % of the gates.  With a uniform field E in place of the sites,
    `ext_hv` is H v - H_bare v [K, N, 3]."""
    key = (c.name, None if E is None else tuple(E)) if V is None else None
    if key is None or key not in _YARD:
        V = c.V if V is None else V
        hv, ext, a_hv, a_ext = [], [], 0.0, 0.0
        for v in V:
            (r1, r2), (s1, s2) = richardson(c, om64, v, E)
            hv.append(r2), ext.append(s2)
            a_hv, a_ext = max(a_hv, np.abs(r1 - r2).max()), max(a_ext, np.abs(s1 - s2).max())
        out = {"hv": np.stack(hv), "ext_hv": np.stack(ext), "agree_hv": a_hv, "agree_ext": a_ext}
        print(f"[embedding hessian] {c.name}: Richardson agreement hv {a_hv:.3e} (gate {gate(out['hv']):.3e}, max|Hv| "
              f"{np.abs(out['hv']).max():.3f}), ext_hv {a_ext:.3e} (gate {gate(out['ext_hv']):.3e}, max {np.abs(out['ext_hv']).max():.4f})")
        assert a_hv <= RICHARDSON_FRACTION * gate(out["hv"]), (c.name, a_hv, gate(out["hv"]))
        assert a_ext <= RICHARDSON_FRACTION * gate(out["ext_hv"]), (c.name, a_ext, gate(out["ext_hv"]))
        if key is None:
            return out
        _YARD[key] = out
    return _YARD[key]


def committed(name: str) -> dict:
    """The yardstick of a GPU case as tests/golden/make_embedding_hessian.py wrote it, checked against the case's inputs."""
    g, c = golden("embedding_hessian"), case(name)
    for k, v in (("coord", c.coord), ("V", c.V), ("X", c.X), ("Q", c.Q)):
        assert np.array_equal(g[f"{name}_{k}"], v), f"tests/golden/embedding_hessian.npz was written for another {name} {k}"
    return {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}


UNIFORM_E = np.array([0.05, -0.02, 0.03])  # V/A, the field of tests/test_gpu_embedding.py::test_uniform_field_against_the_polar_tensor


# ---- the field and the closed-form addends --------------------------------------------------------------------------------------
def tensor(x, X, Q, mol=None, ext_mol=None):
    """T [N, 3, 3] = grad grad phi (V/A^2) of the sites at the atoms and sum_A |k Q / d^3| [N], in fp64."""
    x, X, Q = np.asarray(x, np.float64), np.asarray(X, np.float64).reshape(-1, 3), np.asarray(Q, np.float64).reshape(-1)
    r = x[:, None, :] - X[None, :, :]
    d = np.linalg.norm(r, axis=-1)
    w = np.ones_like(d) if mol is None else (np.asarray(mol)[:, None] == np.asarray(ext_mol)[None, :]).astype(np.float64)
    t = w * Y.KE * Q[None, :] / d**3
    T = 3.0 * np.einsum("ia,iab,iac->ibc", t / d**2, r, r) - t.sum(1)[:, None, None] * np.eye(3)
    return T, np.abs(t).sum(1)


def six(T):
    """[N, 3, 3] -> [N, 6] in the order xx, yy, zz, xy, xz, yz of aimnet_embedding_tangent.potential_hess."""
    T = np.asarray(T)
    return np.stack([T[:, 0, 0], T[:, 1, 1], T[:, 2, 2], T[:, 0, 1], T[:, 0, 2], T[:, 1, 2]], axis=1)


def addends(c, ref, V=None, dtype=np.float64):
    """The three closed-form addends of H_emb v [K, N, 3] each, from the model reference `ref` at the case's coordinates (charges,
    J): `tq_g` = t_q g, `q_Tv` = q T v, `J_tphi` = J t_phi; and what they are built from.  `dtype` = float32 evaluates the same
    products in fp32 (the twin of the seed kernel's inputs)."""
    V = np.asarray(c.V if V is None else V, np.float64)
    K, n = V.shape[:2]
    phi, g, abs_phi, abs_g = Y.field(c.coord, c.X, c.Q, c.mol, c.ext_mol)
    T, abs_T = tensor(c.coord, c.X, c.Q, c.mol, c.ext_mol)
    J, q = ref["J"], ref["charges"]
    t_q = V.reshape(K, 3 * n) @ J  # [K, N]
    cast = lambda a: np.asarray(a, dtype)  # noqa: E731
    tq_g = cast(t_q)[:, :, None] * cast(g)[None]
    q_Tv = cast(q)[None, :, None] * np.einsum("iab,kib->kia", cast(T), cast(V))
    t_phi = np.einsum("ic,kic->ki", cast(g), cast(V))
    J_tphi = (cast(J) @ t_phi.T).T.reshape(K, n, 3)
    return {"tq_g": tq_g, "q_Tv": q_Tv, "J_tphi": J_tphi, "t_q": t_q, "t_phi": t_phi, "phi": phi, "g": g, "T": T, "abs_phi": abs_phi,
            "abs_g": abs_g, "abs_T": abs_T}
