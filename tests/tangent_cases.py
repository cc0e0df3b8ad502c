"""The inputs and the fp64 references of tests/test_gpu_tangent_branches.py, shared with tests/test_tangent_branch_fixtures.py (which
pins, without a GPU, that every case takes the branch of csrc/tangent_plan.h / csrc/hvp.hip it is named for).

A case is a namespace: coord (as given to the engine), numbers, mol, charge, mult, cell, pbc, coul (the Coulomb keywords of
HipEngine.hvp), d3 (parameters of the external DFT-D3 term, or None), V (the directions), nse (two-channel weights) and name.
`reference(case, oracle64)` is the fp64 answer, once per case name: the tangent sweep of oracle/aimnet2_analytic.py::evaluate_hvp on
the oracle's wrapped coordinates and its own lists (built with the case's own pbc flags); with D3 the product H v comes from the
autograd Hessian of oracle/aimnet2_oracle.py::evaluate with the term, and the block H_d3 v = (H_with - H_without) v is kept next to it.

Gates (none is new): hv 1e-5 + 3e-5 max|ref| (`_close` of tests/test_gpu_hvp.py), with D3 plus (2e-4 / 0.63) max|H_d3 v| - the
2e-4 eV/A^2 that test_hvp_with_external_dftd3 grants its 0.63 eV/A^2 block; dq / dspin the same 1e-5 + 3e-5 max|ref|, dmu that gate
propagated through sum_i dq_i x_i + q_i v_i (`_dmu_reference` of tests/test_gpu_charge_response.py); charges CHARGE_ATOL."""
from __future__ import annotations

import os
import re
from types import SimpleNamespace

import numpy as np
import torch

from conftest import CHARGE_ATOL, ROOT, golden

D3_RELATIVE = 2e-4 / 0.63  # of max|H_d3 v|: the allowance of test_hvp_with_external_dftd3 for its block
D3_STENCIL_H = 4e-3        # csrc/hvp.hip, Tangent::d3_block
SPLIT_GEMM_ROWS = 256      # csrc/engine.hip, mlp_gemm: the default mode takes the split GEMMs above this many stacked rows
BBOX_ATOMS_PER_MOL = 1500  # csrc/engine.h, bbox_applies (mirrored; tests/test_tangent_branch_fixtures.py holds it to the header)

_CASES: dict = {}
_REFS: dict = {}


def bbox_applies(n_atoms: int, n_mol: int) -> bool:
    return n_atoms >= BBOX_ATOMS_PER_MOL * n_mol


def bbox_constant_in_header() -> int:
    text = open(os.path.join(ROOT, "aimnetcentral_amd", "csrc", "engine.h")).read()
    m = re.search(r"bool bbox_applies\(int n_atoms, int n_mol\) \{ return \(long\)n_atoms >= (\d+)L \* n_mol; \}", text)
    assert m, "bbox_applies not found in csrc/engine.h"
    return int(m.group(1))


def d3_tables():
    t = golden("dftd3_subset")
    return {k: t[k] for k in ("c6ab", "cn_ref", "rcov", "r4r2")}


def _d3(cutoff: float) -> dict:
    g = golden("dftd3")
    return dict(s6=float(g["s6"]), s8=float(g["s8"]), a1=float(g["a1"]), a2=float(g["a2"]), cutoff=float(cutoff), smoothing_fraction=0.2)


def _random_directions(n: int, k: int = 3):
    return np.random.default_rng(11).standard_normal((k, n, 3)).astype(np.float32)


def _unit_directions(n: int):
    return np.eye(3 * n, dtype=np.float32).reshape(3 * n, n, 3)


def ragged_sizes(big: int = 40):
    return (1, 2, big, 3, 1)


def _ragged(big: int = 40):
    """(1, 2, big, 3, 1) atoms: single atoms (empty rows, NSE sums over one atom), a pair, a triple and one larger molecule."""
    from aimnetcentral_amd import workloads

    rng = np.random.Generator(np.random.PCG64(5))
    cs, zs, ms = [], [], []
    for m, n in enumerate(ragged_sizes(big)):
        c, z = workloads.random_organic(n, rng)
        cs.append(c)
        zs.append(z)
        ms.append(np.full(n, m, np.int64))
    return (np.concatenate(cs).astype(np.float32), np.concatenate(zs).astype(np.int64), np.concatenate(ms),
            np.array([0, 1, -1, 0, 0], np.float32))


def _mols(name, coul, d3=None, nse=False, k=3, big=40):
    c, z, mol, q = _ragged(big)
    mult = np.array([2, 1, 3, 2, 2], np.float32) if nse else None
    return SimpleNamespace(name=name, coord=c, numbers=z, mol=mol, charge=q, mult=mult, cell=None, pbc=None, coul=coul, d3=d3,
                           V=_random_directions(len(z), k), nse=nse)


def _tiny(name, seed, systems=None, pbc=(True, True, True), d3=None, nse=False, unit=False, rc=8.0, charge=0.0, mult=None):
    """Cells of tests/test_gpu_fuzz.py::tiny_cells (3 - 4.5 A edges, triclinic), every atom moved out of its box by up to two lattice
    vectors along the periodic axes of its own system (along an open axis that would be another geometry)."""
    import test_gpu_fuzz as F

    c, z, mol, cell, n_sys, rng = F.tiny_cells(seed)
    cells = cell.reshape(-1, 3, 3)
    if systems is not None:
        keep = np.isin(mol, systems)
        c, z, mol, cells = c[keep], z[keep], np.searchsorted(np.asarray(systems), mol[keep]), cells[list(systems)]
    n_sys = len(cells)
    flags = np.broadcast_to(np.asarray(pbc, bool).reshape(-1, 3), (n_sys, 3))
    move = rng.integers(-2, 3, size=(len(z), 3)) * flags[mol]
    c = (c.astype(np.float64) + np.einsum("na,nab->nb", move, cells[mol].astype(np.float64))).astype(np.float32)
    n = len(z)
    return SimpleNamespace(name=name, coord=c, numbers=z, mol=mol.astype(np.int64), charge=np.full(n_sys, charge, np.float32),
                           mult=None if mult is None else np.full(n_sys, mult, np.float32), cell=cells[0] if n_sys == 1 else cells,
                           pbc=np.asarray(pbc, bool), coul=dict(coulomb="dsf", dsf_rc=rc, dsf_alpha=0.25), d3=d3,
                           V=_unit_directions(n) if unit else _random_directions(n), nse=nse)


def _lone_atom(name, coul):
    return SimpleNamespace(name=name, coord=np.array([[0.3, -0.2, 0.1]], np.float32), numbers=np.array([6], np.int64),
                           mol=np.zeros(1, np.int64), charge=np.zeros(1, np.float32), mult=None, cell=None, pbc=None,
                           coul=dict(coulomb=coul), d3=None, V=_random_directions(1), nse=False)


def _cluster(name, with_far_atom=False):
    """glucose_supercell((3, 2, 3)) as one non-periodic cluster of 1 728 atoms (the bounding-box list); `with_far_atom`: a second
    molecule of one hydrogen atom 60 A away, after which the batch averages below 1 500 atoms per molecule."""
    from aimnetcentral_amd import workloads

    c, z, _ = workloads.glucose_supercell((3, 2, 3))
    c = c - c.mean(0)
    mol, q = np.zeros(len(z), np.int64), np.zeros(1, np.float32)
    V = np.random.default_rng(3).standard_normal((1, len(z), 3)).astype(np.float32)
    if with_far_atom:
        c = np.concatenate([c, c.max(0)[None] + np.array([[60.0, 0.0, 0.0]])])
        z, mol, q = np.concatenate([z, [1]]), np.concatenate([mol, [1]]), np.zeros(2, np.float32)
        V = np.concatenate([V, np.ones((1, 1, 3), np.float32)], axis=1)
    return SimpleNamespace(name=name, coord=c.astype(np.float32), numbers=z.astype(np.int64), mol=mol, charge=q, mult=None, cell=None,
                           pbc=None, coul=dict(coulomb="dsf", dsf_rc=8.0, dsf_alpha=0.2), d3=None, V=V, nse=False)


DSF_BIG = 72
_DSF7 = dict(coulomb="dsf", dsf_rc=7.0, dsf_alpha=0.2)
BUILDERS = {
    "mols-none": lambda n: _mols(n, dict(coulomb="none")),
    # six directions: 47 + 6 * 47 = 329 stacked rows, the split GEMMs; the first direction alone (94 rows) takes the exact-fp32 ones
    "mols-simple": lambda n: _mols(n, dict(coulomb="simple"), k=6),
    # the 40-atom molecule spans 6.98 A, inside the cutoff; at 72 atoms (span 9.8 A) 5.7 % of its pairs lie beyond 7 A
    "mols-dsf": lambda n: _mols(n, _DSF7, big=DSF_BIG),
    "tiny3-dsf8": lambda n: _tiny(n, 1, unit=True),
    "tiny1-TTF": lambda n: _tiny(n, 0, pbc=(True, True, False), unit=True),
    "tiny2-flags": lambda n: _tiny(n, 1, systems=(0, 1), pbc=((True, True, True), (True, False, True))),
    "mols-simple-d3": lambda n: _mols(n, dict(coulomb="simple"), d3=_d3(15.0)),
    "tiny3-dsf8-d3": lambda n: _tiny(n, 1, d3=_d3(9.0)),
    "nse-mols-d3": lambda n: _mols(n, dict(coulomb="simple"), d3=_d3(15.0), nse=True),
    "nse-tiny1-TTF": lambda n: _tiny(n, 0, pbc=(True, True, False), nse=True, charge=1.0, mult=2.0),
    "lone-atom": lambda n: _lone_atom(n, "simple"),
    "lone-atom-none": lambda n: _lone_atom(n, "none"),
    "cluster1728": lambda n: _cluster(n),
}
HVP_CASES = tuple(BUILDERS)
CHARGE_RESPONSE_CASES = ("mols-none", "tiny3-dsf8", "tiny1-TTF", "tiny2-flags", "nse-mols-d3", "nse-tiny1-TTF", "lone-atom")
SMALL_CASES = tuple(n for n in BUILDERS if n != "cluster1728")  # small enough for an autograd Hessian


def case(name: str):
    if name not in _CASES:
        _CASES[name] = BUILDERS[name](name)
    return _CASES[name]


def cluster_with_far_atom():
    if "cluster1728+H" not in _CASES:
        _CASES["cluster1728+H"] = _cluster("cluster1728+H", with_far_atom=True)
    return _CASES["cluster1728+H"]


def oracle_kwargs(c, d3: bool = True) -> dict:
    """Keywords of oracle.aimnet2_oracle.evaluate for the case (everything but the model and the request)."""
    kw = dict(cell=c.cell, pbc=c.pbc, mult=c.mult, **c.coul)
    if d3 and c.d3 is not None:
        kw["dftd3"] = dict(c.d3, **d3_tables())
    return kw


def lists(c, om64):
    """The oracle's wrapped coordinates and its short-range list (evaluation intermediates), and the long-range list at the case's
    cutoff with the case's own pbc flags ((3,) or (n_cell, 3)); infinite cutoff for 'simple', none for 'none'."""
    from oracle import aimnet2_oracle as O

    ref = O.evaluate(om64, c.coord, c.numbers, c.charge, c.mol, return_intermediates=True, forces=False, **oracle_kwargs(c, d3=False))
    xw = ref["coord_wrapped"]
    nbl = shl = None
    if c.coul["coulomb"] != "none":
        rc = float("inf") if c.coul["coulomb"] == "simple" else c.coul["dsf_rc"]
        nbl, shl = O.neighbor_list(xw, rc, c.mol, c.cell, c.pbc)
    return ref, xw, nbl, shl


def sweep(c, om64, V=None):
    """oracle.aimnet2_analytic.evaluate_hvp of the case (no D3: the sweep does not carry it) with its intermediates."""
    from oracle import aimnet2_analytic as AN

    ref, xw, nbl, shl = lists(c, om64)
    kw = {k: v for k, v in c.coul.items() if k != "coulomb"}
    spec = AN.evaluate_hvp(om64, xw, c.numbers, c.charge, c.mol, ref["nbmat"], c.V if V is None else V, shifts=ref.get("shifts"),
                           cell=c.cell, coulomb=c.coul["coulomb"], nbmat_lr=nbl, shifts_lr=shl, mult=c.mult, return_intermediates=True,
                           **kw)
    return ref, spec


def hessian(c, om64, d3: bool):
    """Dense autograd Hessian [3N, 3N] and the forces of oracle.aimnet2_oracle.evaluate, with or without the case's D3 term."""
    from oracle import aimnet2_oracle as O

    n = len(c.numbers)
    r = O.evaluate(om64, c.coord, c.numbers, c.charge, c.mol, hessian=True, forces=True, **oracle_kwargs(c, d3=d3))
    return r["hessian"].reshape(3 * n, 3 * n), r["forces"]


def reference(c, om64) -> dict:
    """hv [K, N, 3], forces, charges, t_q [K, N, nq] (spin_charges) in fp64; with D3 also hv_d3 = H_d3 v (inside hv)."""
    if c.name not in _REFS:
        n, K = len(c.numbers), len(c.V)
        ref, spec = sweep(c, om64)
        out = {"hv": np.asarray(spec["hv"], np.float64), "forces": np.asarray(spec["forces"], np.float64),
               "charges": np.asarray(ref["charges"], np.float64), "t_q": np.asarray(spec["_t_q1"], np.float64),
               "spin_charges": np.asarray(ref["spin_charges"], np.float64) if "spin_charges" in ref else None, "hv_d3": None}
        if c.d3 is not None:
            # H_without v is the sweep's own product: tests/test_tangent_branch_fixtures.py holds it to the autograd Hessian without
            # the term at 1e-9, so one dense Hessian (the one with D3) is formed here
            H, f = hessian(c, om64, True)
            out["hv_sweep"] = out["hv"]
            out["hv"] = (c.V.reshape(K, 3 * n).astype(np.float64) @ H).reshape(K, n, 3)
            out["hv_d3"], out["forces"] = out["hv"] - out["hv_sweep"], np.asarray(f, np.float64)
        _REFS[c.name] = out
    return _REFS[c.name]


def d3_gradient_fn(c, om64):
    """x [N, 3] -> dE_d3/dx in fp64 on the D3 list of the wrapped geometry (the engine keeps that list for its displaced copies)."""
    from oracle import aimnet2_oracle as O

    _, xw, _, _ = lists(c, om64)
    n, par = len(c.numbers), dict(c.d3, **d3_tables())
    nb3, sh3 = O.neighbor_list(xw, par["cutoff"], c.mol, c.cell, c.pbc)
    nb3_t = torch.as_tensor(nb3)
    sh3_t = None if sh3 is None else torch.as_tensor(sh3).double()
    cell_t = None if c.cell is None else torch.as_tensor(np.asarray(c.cell)).double()
    z_p = torch.cat([torch.as_tensor(c.numbers), torch.zeros(1, dtype=torch.long)])
    mol_p = torch.cat([torch.as_tensor(c.mol), torch.as_tensor(c.mol[-1:])])

    def grad(x):
        xp = torch.cat([torch.as_tensor(np.asarray(x, np.float64)), torch.zeros(1, 3, dtype=torch.float64)]).requires_grad_(True)
        d, _, mask = O._distances(xp, nb3_t, sh3_t, cell_t, mol_p)
        e = O.dftd3_energy(d, mask, z_p, nb3_t, mol_p, len(c.charge), par).sum()
        return torch.autograd.grad(e, xp)[0][:n].numpy()

    return np.asarray(xw, np.float64), grad


def d3_stencil(c, om64):
    """The engine's dispersion block in fp64: the 4-point central difference (h = 4e-3 A, every direction scaled by its largest
    per-atom norm) of the oracle's own D3 gradient: [K, N, 3]."""
    xw, grad = d3_gradient_fn(c, om64)
    h, out = D3_STENCIL_H, []
    for v in c.V.astype(np.float64):
        s = np.linalg.norm(v, axis=-1).max()
        u = v / s
        out.append((8.0 * (grad(xw + h * u) - grad(xw - h * u)) - (grad(xw + 2 * h * u) - grad(xw - 2 * h * u))) * (s / (12.0 * h)))
    return np.stack(out)


# ---- the engine's side -------------------------------------------------------------------------------------------------------------
def _t(a, dt=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dt).cuda()


def engine_args(eng, c, coord=None):
    """(coord, numbers, mol_idx, charge) on the device; two channels: charge [n_mol, 2] = (alpha, beta) from charge and mult."""
    q = np.atleast_1d(np.asarray(c.charge, dtype=np.float32))
    if eng.nq == 2:
        mt = np.ones_like(q) if c.mult is None else np.atleast_1d(np.asarray(c.mult, dtype=np.float32))
        q = np.stack([0.5 * q + 0.5 * (mt - 1), 0.5 * q - 0.5 * (mt - 1)], -1)
    return _t(c.coord if coord is None else coord), _t(c.numbers, torch.int32), _t(c.mol, torch.int32), _t(q)


def cell_kwargs(c) -> dict:
    """cell= and pbc= of HipEngine.hvp / charge_response: three flags as a tuple, per-system flags as an [n_cell, 3] tensor."""
    if c.cell is None:
        return {}
    pbc = tuple(bool(b) for b in c.pbc) if c.pbc.ndim == 1 else torch.as_tensor(c.pbc)
    return dict(cell=_t(c.cell), pbc=pbc)


def run_hvp(eng, c, V=None, want_forces=True):
    if c.d3 is not None:
        eng.set_dftd3_tables(d3_tables())
    out = eng.hvp(*engine_args(eng, c), _t(c.V if V is None else V), want_forces=want_forces, dftd3=c.d3, **c.coul, **cell_kwargs(c))
    return {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}


def run_charge_response(eng, c):
    out = eng.charge_response(*engine_args(eng, c), _t(c.V), **cell_kwargs(c))
    return {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}


# ---- gates -------------------------------------------------------------------------------------------------------------------------
def hv_gate(ref, k=slice(None)) -> float:
    gate = 1e-5 + 3e-5 * np.abs(ref["hv"][k]).max()
    if ref["hv_d3"] is not None:
        gate += D3_RELATIVE * np.abs(ref["hv_d3"][k]).max()
    return float(gate)


def tangent_gate(ref_values) -> float:
    return float(1e-5 + 3e-5 * np.abs(ref_values).max())


def dmu_reference(c, ref):
    """sum_i t_q_i x_i + q_i v_i per molecule in fp64 [K, n_mol, 3] from the oracle's values and the coordinates as given, and the
    gate of dq and of the charges propagated through that sum [K, n_mol]."""
    x, v = c.coord.astype(np.float64), c.V.astype(np.float64)
    tq, q = ref["t_q"].sum(-1), ref["charges"]
    n_mol, K = len(c.charge), len(v)
    dmu, bound = np.zeros((K, n_mol, 3)), np.zeros((K, n_mol))
    g = tangent_gate(tq)
    for m in range(n_mol):
        at = c.mol == m
        dmu[:, m] = np.einsum("ki,ic->kc", tq[:, at], x[at]) + np.einsum("i,kic->kc", q[at], v[:, at])
        bound[:, m] = g * np.abs(x[at]).max(-1).sum() + CHARGE_ATOL * np.abs(v[:, at]).max(-1).sum(-1)
    return dmu, bound
