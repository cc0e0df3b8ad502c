"""The DFT-D3 term ALONE against its fp64 reference (tests/d3_cases.py::d3_reference) on every element class, list source and branch
of csrc/d3.hip, the coordination-number rider of csrc/nlist.hip and the table repacking of aimnet_engine_set_dftd3.

Isolating the term: D3 share = eval(dftd3 = par) - eval(dftd3 = par with s6 = s8 = 0).  Everything else is identical in the two runs -
plan, lists, riders, the DSF pair terms that ride on the D3 pair pass - and in d3.hip `damp`, `de` and dE/dcn are exactly zero in the
second, so the difference is the dispersion term on every branch.  In each pair of runs the charges are bitwise equal and the status
words equal.  Once (`edges`, coulomb "simple") the zero-strength run is held bitwise to a run without the term.

Branches (the plan values are asserted from the options the engine sent, as tests/test_gpu_request_kinds.py::plan_facts does):
  branch              case      engine keywords                          eval_plan.h                                    kinds
  het27-none          het27     none, par12                              d3 = Built, cn rider                           FS F E
  het27-none-cn0      het27     same, d3_cn_rides = 0                    d3_cn_kernel                                   FS
  het27-dsf12         het27     dsf rc 12, par12                         DsfInD3: d3_pair_kernel<.., DSF = true>        FS E
  het27-dsf13-d3_10   het27     dsf rc 13, par12 at cutoff 10            d3 = Built beside the walk (DsfWalk)           FS
  het27-par9          het27     none, par9 (no switch, s6 = 0.75)        r_off == r_on                                  FS
  het27-lists         het27     none, par12, nbmat + shifts (5 A) and    d3 = Imported                                  FS
                                nbmat_d3 + shifts_d3 from the oracle
  het27x2-none        het27x2   none, par12                              two cells, per-system stress                   FS
  het27x2-dsf12       het27x2   dsf rc 12, par12                         two cells, DsfInD3                             FS
  edges-simple        edges     simple, par12                            non-binned build (d3_cn_kernel), empty row     F E
  edges-dsf9          edges     dsf rc 9, par12 at cutoff 9              DsfInD3 on one shared matrix (d3 = LongRange)  F
On `edges`: the lone atom's D3 energy and force are exactly 0.0; the Br atom (no table entry) has the reference's force, nonzero
through its neighbours' coordination numbers.  Energies of the E kind have the bits of the F / FS kinds, as d3.hip claims.

Gates (tests/d3_cases.py holds the constants, tests/test_d3_cases.py their premises):
  energy  6e-6 eV per molecule: the project's D3 gate (test_gpu_parity.test_dftd3_term_matches_reference_twin); the float32 twin of
          the reference sits <= 1.1e-6 eV (pbc96) and <= 3e-7 eV (het27) from fp64.
  forces  5e-6 eV/A (the same test's gate) + 2^-21 max|F_total|: each run's fp32 force is a handful of fp32 additions into fgrad,
          each rounding by at most 2^-24 |F|; eight of them over both runs.  2e-7 with the cold weights used here.
  stress  8e-8 eV/A^3 + 2^-21 max|stress_total|: 16 x the largest |float32 twin - fp64| over the periodic cases (4.9e-9, het27 /
          par12; pbc96 2.9e-9), rounded up to one digit.  16 covers the hardware rcp / rsq / exp2 (1 ulp each) and 600 - 950 fp32 pair
          terms per atom summed in lane order where torch sums pairwise.  Below the ceiling of 1e-6 (a tenth of STRESS_ATOL).
Measured deviations: profiles/dftd3_fp64.md (from the "d3-fp64" lines this module prints)."""
from __future__ import annotations

import contextlib

import numpy as np
import pytest
import torch

import d3_cases as D
from aimnetcentral_amd.engine import same_cutoff

pytestmark = pytest.mark.gpu

KINDS = {"E": dict(forces=False, stress=False), "F": dict(forces=True, stress=False), "FS": dict(forces=True, stress=True)}
NONE, DSF12 = dict(coulomb="none"), dict(coulomb="dsf", dsf_rc=12.0)
# branch -> (case, engine keywords, parameter set, caller-supplied lists, engine options, kinds, expected plan)
BRANCHES = {
    "het27-none": ("het27", NONE, "par12", False, {}, ("FS", "F", "E"), dict(d3="Built", lr_term="None", cn_rides=True)),
    "het27-none-cn0": ("het27", NONE, "par12", False, {"d3_cn_rides": 0}, ("FS",), dict(d3="Built", lr_term="None", cn_rides=False)),
    "het27-dsf12": ("het27", DSF12, "par12", False, {}, ("FS", "E"), dict(d3="Built", lr_term="DsfInD3", cn_rides=True)),
    "het27-dsf13-d3_10": ("het27", dict(coulomb="dsf", dsf_rc=13.0), "par10", False, {}, ("FS",),
                          dict(d3="Built", lr_term="DsfWalk", cn_rides=True)),
    "het27-par9": ("het27", NONE, "par9", False, {}, ("FS",), dict(d3="Built", lr_term="None", cn_rides=True)),
    "het27-lists": ("het27", NONE, "par12", True, {}, ("FS",), dict(d3="Imported", lr_term="None", cn_rides=False)),
    "het27x2-none": ("het27x2", NONE, "par12", False, {}, ("FS",), dict(d3="Built", lr_term="None", cn_rides=True)),
    "het27x2-dsf12": ("het27x2", DSF12, "par12", False, {}, ("FS",), dict(d3="Built", lr_term="DsfInD3", cn_rides=True)),
    "edges-simple": ("edges", dict(coulomb="simple"), "par12", False, {}, ("F", "E"), dict(d3="Built", lr_term="SimpleInSr", cn_rides=False)),
    "edges-dsf9": ("edges", dict(coulomb="dsf", dsf_rc=9.0), "par9s", False, {}, ("F",), dict(d3="LongRange", lr_term="DsfInD3", cn_rides=False)),
}
BBOX_ATOMS_PER_MOL = 1500  # csrc/engine.h, bbox_applies: none of these cases reaches the bounding-box grid

_REFS: dict = {}


def reference(name, par):
    """(fp64 reference, |float32 twin - fp64|) of a case and parameter set: once per module, read-only."""
    if (name, par) not in _REFS:
        c = D.case(name)
        _REFS[name, par] = (D.d3_reference(c, torch.float64, par=par), D.twin_deviation(c, par))
    return _REFS[name, par]


@contextlib.contextmanager
def engine_as(eng, **options):
    """The session's engine with the DFT-D3 tables of the committed slice and `options`; switches and row capacities put back."""
    saved = (eng.max_nb, dict(eng._max_nb_lr), {k: eng.get_option(k) for k in options})
    try:
        eng.set_dftd3_tables(D.tables())
        for k, v in options.items():
            eng.set_option(k, v)
        yield eng
    finally:
        for k, v in saved[2].items():
            eng.set_option(k, v)
        eng.max_nb, eng._max_nb_lr = saved[0], saved[1]


def caller_lists(c, rc_sr: float, rc_d3: float) -> dict:
    n = len(c.numbers)
    nb, sh = D.lists(c, rc_sr)
    nb3, sh3 = D.lists(c, rc_d3)
    return dict(nbmat=torch.from_numpy(nb[:n]), shifts=torch.from_numpy(sh[:n].astype(np.int32)),
                nbmat_d3=torch.from_numpy(nb3[:n]), shifts_d3=torch.from_numpy(sh3[:n].astype(np.int32)))


def evaluate(eng, c, ekw, dftd3, kind, lists=None):
    """One HipEngine.eval: (outputs as numpy arrays, copy of the status words).  A device error ends the session - nothing more is
    started on a GPU that has faulted."""
    dev = eng.device
    kw = dict(ekw, **KINDS[kind], **(lists or {}))
    if c.cell is not None:
        kw["cell"] = torch.from_numpy(c.cell).to(dev)
    try:
        r = eng.eval(torch.from_numpy(c.coord).to(dev), torch.from_numpy(c.numbers).to(dev), torch.from_numpy(c.mol).to(dev),
                     torch.from_numpy(c.charge).to(dev), dftd3=dftd3, **kw)
        res = {k: v.cpu().numpy() for k, v in r.items()}
    except RuntimeError as exc:
        if any(s in str(exc) for s in ("HIP error", "hipError", "illegal memory", "kernel launch failed", "code -2")):
            pytest.exit(f"device error in {c.name} [{kind}]: {exc}", returncode=3)
        raise
    return res, np.array(eng.last_status).copy()


def plan_facts(eng, c, ekw, p, ext: bool) -> dict:
    """What csrc/eval_plan.h decides for the D3 term of the evaluation the engine ran last, from the options it sent."""
    opt, _ = eng._last_request
    n, n_mol, pbc = len(c.numbers), len(c.charge), c.cell is not None
    assert opt.dftd3 == 1 and n < BBOX_ATOMS_PER_MOL * n_mol  # (no bounding-box grid, no list-free walk of a molecule)
    dsf = ekw["coulomb"] == "dsf"
    same = same_cutoff(p["cutoff"], ekw.get("dsf_rc", 15.0))
    lr_list = dsf and not pbc  # ListFrom::Built (not ext), or Imported - neither with ext here (no nbmat_lr is passed)
    d3_in_lr = dsf and opt.max_nb_lr > 0 and same
    lr_term = {"none": "None", "simple": "SimpleInSr"}.get(ekw["coulomb"]) or ("DsfInD3" if not ext and same else "DsfWalk" if pbc and not ext else "DsfMatrix")
    d3 = "LongRange" if d3_in_lr and lr_list and not ext else "Imported" if ext else "Built"
    binned = not ext and pbc
    return dict(d3=d3, lr_term=lr_term, cn_rides=bool(d3 == "Built" and eng.get_option("d3_cn_rides") and binned))


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def share(a, b, n_cell):
    """The D3 term as the difference of two evaluations, in float64."""
    out = {"energy": a["energy"].astype(np.float64) - b["energy"], "forces": None, "stress": None}
    if "forces" in a:
        out["forces"] = a["forces"].astype(np.float64) - b["forces"]
    if "stress" in a:
        out["stress"] = (a["stress"].astype(np.float64) - b["stress"]).reshape(n_cell, 3, 3)
    return out


@pytest.mark.parametrize("branch", list(BRANCHES))
def test_d3_share_meets_the_fp64_reference(hip_engine_cold, branch):
    name, ekw, par, ext, options, kinds, expected = BRANCHES[branch]
    c, p = D.case(name), D.get_par(par)
    ref, twin = reference(name, par)
    n_cell = 0 if c.cell is None else c.cell.reshape(-1, 3, 3).shape[0]
    lists = caller_lists(c, float(hip_engine_cold.spec.rc), p["cutoff"]) if ext else None
    problems, energies = [], {}
    with engine_as(hip_engine_cold, **options) as eng:
        evaluate(eng, c, ekw, p, kinds[0], lists)  # settles the row capacities
        for kind in kinds:
            a, st_a = evaluate(eng, c, ekw, p, kind, lists)
            facts = plan_facts(eng, c, ekw, p, ext)
            b, st_b = evaluate(eng, c, ekw, D.zero_strength(p), kind, lists)
            what = f"{branch} [{kind}]"
            if facts != expected:
                problems.append(f"{what}: plan {facts}, expected {expected}")
            if not bits_equal(a["charges"], b["charges"]):
                problems.append(f"{what}: the charges of the two runs differ by {np.abs(a['charges'] - b['charges']).max():.3e}")
            if not np.array_equal(st_a, st_b):
                problems.append(f"{what}: status {st_a.tolist()} against {st_b.tolist()}")
            if st_a[4] <= 0 and facts["d3"] == "Built":
                problems.append(f"{what}: no D3 list was built (status {st_a.tolist()})")
            got = share(a, b, n_cell)
            gates = {"energy": D.ENERGY_GATE, "forces": D.force_gate(a["forces"]) if "forces" in a else None,
                     "stress": D.stress_gate(a["stress"]) if "stress" in a else None}
            cells = []
            for key in ("energy", "forces", "stress"):
                if got[key] is None:
                    cells.append(f"{key} -")
                    continue
                err = float(np.abs(got[key] - ref[key]).max())
                cells.append(f"{key} {err:.2e} twin {twin[key]:.2e} gate {gates[key]:.2e}")
                if not err <= gates[key]:
                    problems.append(f"{what}: {key} of the D3 share off by {err:.3e} > {gates[key]:.3e} (|ref| {np.abs(ref[key]).max():.3e})")
            print(f"d3-fp64 | {branch} | {kind} | " + " | ".join(cells))
            energies[kind] = (a["energy"], b["energy"])
            if name == "edges":
                if got["energy"][0] != 0.0 or (got["forces"] is not None and got["forces"][D.LONE_ATOM].any()):
                    problems.append(f"{what}: the lone atom has D3 energy {got['energy'][0]!r}, force {None if got['forces'] is None else got['forces'][D.LONE_ATOM]}")
                if got["forces"] is not None:
                    d_br = float(np.abs(got["forces"][D.BR_ATOM] - ref["forces"][D.BR_ATOM]).max())
                    if not (d_br <= gates["forces"] and got["forces"][D.BR_ATOM].any() and ref["forces"][D.BR_ATOM].any()):
                        problems.append(f"{what}: Br force {got['forces'][D.BR_ATOM]} against {ref['forces'][D.BR_ATOM]}")
        for kind in kinds[1:]:  # an energy-only evaluation returns the bits of a force evaluation (csrc/d3.hip, d3_pair_kernel)
            for which, e, e0 in zip(("with D3", "zero strength"), energies[kind], energies[kinds[0]]):
                if not bits_equal(e, e0):
                    problems.append(f"{branch}: energy of {kind} ({which}) differs from {kinds[0]} by {np.abs(e - e0).max():.3e}")
    assert not problems, f"{len(problems)} check(s) failed:\n  " + "\n  ".join(problems)


def test_zero_strength_term_changes_no_bit(hip_engine_cold):
    """`edges`, coulomb "simple": the evaluation with the term at s6 = s8 = 0 against the evaluation without the term.  The D3 launches
    add +-0 to ecoul and fgrad; the rest of the plan differs (a second list is built, eval_plan.h: one_list) but computes the same
    numbers: energy, forces and charges are bitwise equal."""
    c, ekw, p = D.case("edges"), dict(coulomb="simple"), D.get_par("par12")
    with engine_as(hip_engine_cold) as eng:
        evaluate(eng, c, ekw, p, "F")
        zero, _ = evaluate(eng, c, ekw, D.zero_strength(p), "F")
        off, _ = evaluate(eng, c, ekw, None, "F")
    for key in ("energy", "forces", "charges"):
        d = np.abs(zero[key].astype(np.float64) - off[key]).max()
        print(f"d3-fp64 | edges-simple zero strength against no term | F | {key} {d:.2e}")
        assert bits_equal(zero[key], off[key]), f"{key}: zero-strength D3 differs from no D3 by {d:.3e}"


def test_gates_see_swapped_table_rows_on_the_engine(hip_engine_cold):
    """The comparison above is not blind on the device either: with the Si and P rows of the uploaded tables swapped (a wrong
    species slot in aimnet_engine_set_dftd3 would do the same), het27 misses every gate by more than 100 times - the figures the
    reference shows for this error on the CPU (tests/test_d3_cases.py: 4.7e-2 eV, 1.4e-1 eV/A, 8.7e-4 eV/A^3)."""
    c, p = D.case("het27"), D.get_par("par12")
    ref, _ = reference("het27", "par12")
    with engine_as(hip_engine_cold) as eng:
        try:
            eng.set_dftd3_tables(D._swap_rows(D.tables(), 14, 15))
            evaluate(eng, c, NONE, p, "FS")
            a, _ = evaluate(eng, c, NONE, p, "FS")
            b, _ = evaluate(eng, c, NONE, D.zero_strength(p), "FS")
        finally:
            eng.set_dftd3_tables(D.tables())
    got = share(a, b, 1)
    gates = {"energy": D.ENERGY_GATE, "forces": D.force_gate(a["forces"]), "stress": D.stress_gate(a["stress"])}
    for key, gate in gates.items():
        err = float(np.abs(got[key] - ref[key]).max())
        print(f"d3-fp64 | het27-none, Si and P rows swapped | FS | {key} {err:.2e} = {err / gate:.0f} gates")
        assert err >= D.SENSITIVITY * gate, f"{key}: swapped rows move the D3 share by {err:.3e} only, gate {gate:.3e}"
