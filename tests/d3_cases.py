"""The inputs and the fp64 reference of tests/test_gpu_dftd3_fp64.py, shared with tests/test_d3_cases.py (which pins, without a GPU,
the reference to the golden outputs of the reference module's own twin, the properties the cases are there for, and that the
reference is sensitive to the errors the GPU test is meant to see).

A case is a namespace: name, coord (float32, as given to the engine; periodic cases lie inside their cell, so nothing is wrapped),
numbers, mol, charge (zeros), cell (None, [3, 3] or [n_cell, 3, 3]).  `d3_reference(case, dtype, mutate, par)` is the DFT-D3(BJ) term
ALONE: energy [n_mol], forces [N, 3] and stress [n_cell, 3, 3] (None without a cell) from oracle.aimnet2_oracle.neighbor_list at the
D3 cutoff, `_distances` and `dftd3_energy` with autograd, the stress through a per-system strain matrix as oracle.evaluate takes it.
The coordinates are the float32 inputs cast to `dtype`; dtype = float32 is the "twin" whose distance from fp64 the gates are built on.
The tables are the committed Z <= 17 slice zero-padded to Z = 54: an element outside the slice (Br in `edges`) has c6ab = 0 and
rcov = r4r2 = 0, which is what aimnet_engine_set_dftd3 uploads for such a slot.

Cases (recipes fixed; every number below was measured on the CPU, tests/test_d3_cases.py asserts the properties):
  het27    periodic, 27 atoms (N % 4 = 3), cell [[7.1,0,0],[1.3,6.4,0],[-0.9,1.1,6.8]], sites (ijk + 0.5) / 3 + U(-0.08, 0.08) from
           default_rng(7), numbers a permutation of [1,5,6,7,8,9,14,15,16,17] resized to 27 drawn after the jitter: nref classes 2 (H),
           3 (Cl), 4 (F), 5 (B, C, N, O, Si, P, S); at 12 A the rows are 640 wide with lattice shifts up to +-2
  het27x2  het27 and a second system (seed 8, cell x 1.07 with another shear) in one batch: two cells, per-system stress
  edges    four molecules, 10 atoms: a lone C (empty row, cn = 0), O...S at 10.5 A (inside the switching window 9.6 - 12 A), H-F at
           1.1 A, and a CH3Br-like molecule whose Br has no table entry (its pairs give nothing, it still enters its neighbours' cn)
Parameter sets: par12 (golden s8 / a1 / a2, s6 = 1, cutoff 12, smoothing fraction 0.2), par9 (cutoff 9, no switch, s6 = 0.75),
and `par(cutoff, ...)` for the others."""
from __future__ import annotations

import inspect
from types import SimpleNamespace

import numpy as np
import torch

from conftest import golden
from oracle import aimnet2_oracle as O

Z_PAD = 54
ELEMENTS = (1, 5, 6, 7, 8, 9, 14, 15, 16, 17)
HET_CELL = np.array([[7.1, 0.0, 0.0], [1.3, 6.4, 0.0], [-0.9, 1.1, 6.8]])
HET_CELL_2 = 1.07 * np.array([[7.1, 0.0, 0.0], [-0.8, 6.4, 0.0], [0.6, -1.2, 6.8]])

# ---- gates of tests/test_gpu_dftd3_fp64.py (provenance: its docstring; the stress figure is re-derived by tests/test_d3_cases.py) --------
ENERGY_GATE = 6e-6          # eV per molecule: the project's D3 gate (tests/test_gpu_parity.py::test_dftd3_term_matches_reference_twin)
FORCE_GATE = 5e-6           # eV/A: the same test's force gate
DIFFERENCING = 2.0 ** -21   # of max|total|: eight fp32 roundings (2^-24 each) over the two runs whose difference is the D3 share
STRESS_GATE = 8e-8          # eV/A^3: 16 x the largest |float32 twin - fp64| (4.9e-9, het27 / par12) over GATE_CASES, one digit, up;
                            # the twin depends on the host's CPU: this is the tightest reading met (tests/test_d3_cases.py)
STRESS_GATE_CEILING = 1e-6  # a tenth of conftest.STRESS_ATOL: above it the test would add nothing
SENSITIVITY = 100.0         # every mutation of the claim moves E, F and stress by at least this many gates

_CASES: dict = {}
_REFS: dict = {}
_TABLES: dict = {}


def tables(n_z: int | None = None) -> dict:
    """The committed table slice (c6ab / cn_ref [18, 18, 5, 5], rcov / r4r2 [18]) as it is, or zero-padded to `n_z` elements."""
    if n_z not in _TABLES:
        t = golden("dftd3_subset")
        out = {k: np.asarray(t[k], np.float32) for k in ("c6ab", "cn_ref", "rcov", "r4r2")}
        if n_z is not None:
            z = out["rcov"].shape[0]
            for k in ("c6ab", "cn_ref"):
                big = np.zeros((n_z, n_z, 5, 5), np.float32)
                big[:z, :z] = out[k]
                out[k] = big
            for k in ("rcov", "r4r2"):
                big = np.zeros(n_z, np.float32)
                big[:z] = out[k]
                out[k] = big
        _TABLES[n_z] = out
    return _TABLES[n_z]


def par(cutoff: float, smoothing_fraction: float = 0.2, s6: float | None = None) -> dict:
    g = golden("dftd3")
    return dict(s6=float(g["s6"]) if s6 is None else s6, s8=float(g["s8"]), a1=float(g["a1"]), a2=float(g["a2"]), cutoff=float(cutoff),
                smoothing_fraction=float(smoothing_fraction))


PARS = {"par12": lambda: par(12.0), "par9": lambda: par(9.0, 0.0, 0.75), "par10": lambda: par(10.0), "par9s": lambda: par(9.0)}


def get_par(p) -> dict:
    return dict(PARS[p]() if isinstance(p, str) else p)


def zero_strength(p: dict) -> dict:
    """The same term with s6 = s8 = 0: same plan, lists and riders; damp, de and dE/dcn of csrc/d3.hip are exactly zero."""
    return dict(p, s6=0.0, s8=0.0)


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def _het_system(seed: int, cell: np.ndarray):
    rng = np.random.default_rng(seed)
    ijk = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij"), -1).reshape(27, 3)
    frac = (ijk + 0.5) / 3.0 + rng.uniform(-0.08, 0.08, size=(27, 3))
    numbers = rng.permutation(np.resize(np.array(ELEMENTS), 27))
    return (frac @ cell).astype(np.float32), numbers.astype(np.int64)


def _case(name, coord, numbers, mol, cell):
    n_mol = int(mol.max()) + 1
    return SimpleNamespace(name=name, coord=np.ascontiguousarray(coord, np.float32), numbers=np.asarray(numbers, np.int64),
                           mol=np.asarray(mol, np.int64), charge=np.zeros(n_mol, np.float32),
                           cell=None if cell is None else np.asarray(cell, np.float32))


def _het27():
    c, z = _het_system(7, HET_CELL)
    return _case("het27", c, z, np.zeros(27, np.int64), HET_CELL)


def _het27x2():
    c1, z1 = _het_system(7, HET_CELL)
    c2, z2 = _het_system(8, HET_CELL_2)
    return _case("het27x2", np.concatenate([c1, c2]), np.concatenate([z1, z2]), np.repeat([0, 1], 27), np.stack([HET_CELL, HET_CELL_2]))


def _edges():
    ch3br = np.array([[0.0, 0.0, 0.0], [1.94, 0.0, 0.0], [-0.36, 1.03, 0.0], [-0.36, -0.51, 0.89], [-0.36, -0.51, -0.89]])  # C Br H H H
    parts = [(np.array([[0.3, -0.2, 0.1]]), [6]),
             (np.array([[20.0, 0.0, 0.0], [20.0 + 10.5 / np.sqrt(3.0)] + [10.5 / np.sqrt(3.0)] * 2]), [8, 16]),
             (np.array([[0.0, 20.0, 0.0], [0.0, 20.0, 1.1]]), [1, 9]),
             (ch3br + np.array([0.0, 0.0, 20.0]), [6, 35, 1, 1, 1])]
    coord = np.concatenate([p for p, _ in parts])
    numbers = np.concatenate([z for _, z in parts])
    mol = np.concatenate([np.full(len(z), m) for m, (_, z) in enumerate(parts)])
    return _case("edges", coord, numbers, mol, None)


def _golden(section: str):
    g = golden("dftd3")
    z = g[section + "_numbers"]
    mol = g["batch_mol_idx"] if section == "batch" else np.zeros(len(z), np.int64)
    return _case("golden-" + section, g[section + "_coord"], z, mol, g["pbc_cell"] if section == "pbc" else None)


BUILDERS = {"het27": _het27, "het27x2": _het27x2, "edges": _edges, "golden-taxol": lambda: _golden("taxol"),
            "golden-batch": lambda: _golden("batch"), "golden-pbc": lambda: _golden("pbc")}
PERIODIC_CASES = ("het27", "het27x2")
# the periodic (case, parameters) the GPU test holds, and the periodic golden section: what STRESS_GATE is taken over
GATE_CASES = (("het27", "par12"), ("het27", "par9"), ("het27", "par10"), ("het27x2", "par12"), ("golden-pbc", "par12"))
LONE_ATOM, BR_ATOM = 0, 6  # in `edges`


def case(name: str):
    if name not in _CASES:
        _CASES[name] = BUILDERS[name]()
    return _CASES[name]


def lists(c, cutoff: float):
    """oracle.neighbor_list of the case at `cutoff`: (nbmat [N + 1, M] with the sentinel N, shifts [N + 1, M, 3] or None)."""
    return O.neighbor_list(c.coord, float(cutoff), c.mol, None if c.cell is None else c.cell.astype(np.float64))


def min_distance(c) -> float:
    nb, sh = lists(c, 4.0)
    x = torch.cat([torch.as_tensor(c.coord).double(), torch.zeros(1, 3, dtype=torch.float64)])
    mol_p = torch.cat([torch.as_tensor(c.mol), torch.as_tensor(c.mol[-1:])])
    d, _, mask = O._distances(x, torch.as_tensor(nb), None if sh is None else torch.as_tensor(sh).double(),
                              None if c.cell is None else torch.as_tensor(c.cell).double(), mol_p)
    return float(d.masked_fill(mask, np.inf).min())


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def _rewritten(old: str, new: str):
    """oracle.dftd3_energy with one piece of its text replaced (exactly one occurrence): the deliberate errors that live inside it."""
    src = inspect.getsource(O.dftd3_energy)
    assert src.count(old) == 1, f"oracle.dftd3_energy no longer contains {old!r} exactly once"
    scope = dict(vars(O))
    exec(compile(src.replace(old, new), "<mutated dftd3_energy>", "exec"), scope)
    return scope["dftd3_energy"]


def _swap_rows(t: dict, za: int, zb: int) -> dict:
    perm = np.arange(t["rcov"].shape[0])
    perm[[za, zb]] = perm[[zb, za]]
    return {"c6ab": t["c6ab"][perm][:, perm], "cn_ref": t["cn_ref"][perm][:, perm], "rcov": t["rcov"][perm], "r4r2": t["r4r2"][perm]}


# name -> (parameters, tables, energy function) -> the same three with one deliberate error
MUTATIONS = {
    "no_switch": lambda p, t, f: (dict(p, smoothing_fraction=0.0), t, f),
    "swap_si_p": lambda p, t, f: (p, _swap_rows(t, 14, 15), f),
    "cnref_j_not_transposed": lambda p, t, f: (p, t, _rewritten("cn_ref[zj, zi].transpose(-1, -2)", "cn_ref[zj, zi]")),
    "no_drop_rule": lambda p, t, f: (p, t, _rewritten("& (shifted >= -12.0)", "")),
}
CLAIMED_MUTATIONS = ("no_switch", "swap_si_p", "cnref_j_not_transposed")  # no_drop_rule: below 100 gates on het27 (test_d3_cases.py)


def d3_reference(c, dtype=torch.float64, mutate: str | None = None, par="par12") -> dict:
    """energy [n_mol], forces [N, 3], stress [n_cell, 3, 3] or None of the D3 term alone, as float64 arrays computed in `dtype`.
    Unmutated results are computed once per (case, parameters, dtype) and handed out read-only."""
    p = get_par(par)
    key = (c.name, tuple(sorted(p.items())), dtype)
    if mutate is None and key in _REFS:
        return _REFS[key]
    p, t, energy_fn = (MUTATIONS[mutate] if mutate else (lambda *a: a))(p, tables(Z_PAD), O.dftd3_energy)
    n, n_mol = len(c.numbers), len(c.charge)
    nb, sh = lists(c, p["cutoff"])
    nb_t = torch.as_tensor(nb)
    sh_t = None if sh is None else torch.as_tensor(sh).to(dtype)
    cell_t = None if c.cell is None else torch.as_tensor(c.cell).to(dtype)
    x = torch.cat([torch.as_tensor(c.coord).to(dtype), torch.zeros(1, 3, dtype=dtype)]).requires_grad_(True)
    z_p = torch.cat([torch.as_tensor(c.numbers), torch.zeros(1, dtype=torch.long)])
    mol_p = torch.cat([torch.as_tensor(c.mol), torch.as_tensor(c.mol[-1:])])
    xs, cell_s, strain = x, cell_t, None
    if cell_t is not None:  # oracle.evaluate: one strain matrix, or one per system
        if cell_t.ndim == 2:
            strain = torch.eye(3, dtype=dtype, requires_grad=True)
            xs, cell_s = x @ strain, cell_t @ strain
        else:
            strain = torch.eye(3, dtype=dtype).unsqueeze(0).repeat(cell_t.shape[0], 1, 1).requires_grad_(True)
            xs, cell_s = (x.unsqueeze(1) @ strain[mol_p]).squeeze(1), cell_t @ strain
    d, _, mask = O._distances(xs, nb_t, sh_t, cell_s, mol_p)
    e = energy_fn(d, mask, z_p, nb_t, mol_p, n_mol, dict(p, **t))
    grads = torch.autograd.grad(e.sum(), [x] + ([strain] if strain is not None else []))
    out = {"energy": e.detach().double().numpy().copy(), "forces": (-grads[0][:n]).double().numpy().copy(), "stress": None}
    if strain is not None:
        vol = torch.linalg.det(cell_t.detach()).abs().reshape(-1, 1, 1)
        out["stress"] = (grads[1].reshape(-1, 3, 3) / vol).double().numpy().copy()
    if mutate is None:
        for v in out.values():
            if v is not None:
                v.setflags(write=False)
        _REFS[key] = out
    return out


def deviation(a: dict, b: dict) -> dict:
    """max|a - b| of energy, forces and stress (0.0 where there is no stress)."""
    return {k: float(np.abs(a[k] - b[k]).max()) if a[k] is not None else 0.0 for k in ("energy", "forces", "stress")}


def twin_deviation(c, par="par12") -> dict:
    """|float32 twin - fp64| of the reference itself: what fp32 arithmetic costs this term on this case (pairwise torch sums)."""
    return deviation(d3_reference(c, torch.float32, par=par), d3_reference(c, torch.float64, par=par))


def one_digit_up(x: float) -> float:
    e = int(np.floor(np.log10(x)))
    return float(np.ceil(x / 10.0 ** e - 1e-9)) * 10.0 ** e


def force_gate(total_forces) -> float:
    return FORCE_GATE + DIFFERENCING * float(np.abs(total_forces).max())


def stress_gate(total_stress) -> float:
    return STRESS_GATE + DIFFERENCING * float(np.abs(total_stress).max())
