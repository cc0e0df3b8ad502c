"""tests/d3_cases.py without a GPU: the fp64 reference of the DFT-D3 term alone is anchored to the golden outputs of the reference
module's own twin, the cases have the properties they are named for, the stress gate is what its rule gives, and the reference
moves by at least 100 GPU gates under each deliberate error of the claim - so tests/test_gpu_dftd3_fp64.py cannot be blind to them.

Measured on the CPU (het27, par12; gates: energy 6e-6 eV, forces 5e-6 + 2^-21 x 0.47 = 5.2e-6 eV/A, stress 8e-8 + 2^-21 x 7e-3 = 8.3e-8 eV/A^3):
  mutation                  |dE| eV    |dF| eV/A   |dstress| eV/A^3
  no_switch                 3.1e-2     1.7e-3      2.1e-4
  swap_si_p                 4.7e-2     1.4e-1      8.7e-4
  cnref_j_not_transposed    3.4e-1     3.7e-1      5.3e-3
  no_drop_rule              3.8e-7     6.5e-6      1.6e-7    (0.06, 1.3 and 2 gates: NOT part of the claim - the GPU test does not
                                                              establish the e^-12 drop rule on this case)"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import d3_cases as D
from conftest import STRESS_ATOL, golden
from oracle import aimnet2_oracle as O


@pytest.mark.parametrize("section,cutoff", [("taxol", 15.0), ("batch", 15.0), ("pbc", 12.0)])
def test_reference_is_anchored_to_the_reference_twin(section, cutoff):
    """Half the GPU gates: 3e-6 eV and 2.5e-6 eV/A (measured: taxol 1.8e-6 / 5.3e-8, batch 6.1e-7 / 2.5e-7, pbc 8.3e-7 / 2.8e-8)."""
    g = golden("dftd3")
    r = D.d3_reference(D.case("golden-" + section), torch.float64, par=D.par(cutoff))
    de, df = np.abs(r["energy"] - g[section + "_energy"]).max(), np.abs(r["forces"] - g[section + "_forces"]).max()
    print(f"d3 anchor | {section} | dE {de:.2e} | dF {df:.2e}")
    assert de <= D.ENERGY_GATE / 2 and df <= D.FORCE_GATE / 2


def test_reference_agrees_with_the_oracle_evaluation(synth_sd_cold):
    """The stand-alone term is the term oracle.evaluate adds (same list, same strain convention): in fp64, evaluation with minus
    without it, on the coordinates as oracle.evaluate wraps them (in fp32: a move of up to 1e-6 A)."""
    c = D.case("het27x2")
    model = O.OracleModel(synth_sd_cold, torch.float64)
    kw = dict(mol_idx=c.mol, cell=c.cell, coulomb="none", stress=True)
    a = O.evaluate(model, c.coord, c.numbers, c.charge, dftd3=dict(D.get_par("par12"), **D.tables(D.Z_PAD)), return_intermediates=True, **kw)
    b = O.evaluate(model, c.coord, c.numbers, c.charge, **kw)
    assert np.abs(a["coord_wrapped"] - c.coord).max() < 2e-6  # the case lies inside its cells
    r = D.d3_reference(D._case("het27x2-as-wrapped", a["coord_wrapped"], c.numbers, c.mol, c.cell), torch.float64)
    assert np.abs(a["_e_dftd3"] - r["energy"]).max() <= 1e-12
    assert np.abs(a["forces"] - b["forces"] - r["forces"]).max() <= 1e-12
    assert np.abs(a["stress"] - b["stress"] - r["stress"]).max() <= 1e-13


@pytest.mark.parametrize("name", D.PERIODIC_CASES)
def test_periodic_cases_have_the_properties_they_are_there_for(name):
    c = D.case(name)
    t = D.tables()
    nref = (np.einsum("zaa->za", t["c6ab"][np.arange(18), np.arange(18)]) != 0).sum(-1)  # as aimnet_engine_set_dftd3 counts them
    assert D.min_distance(c) >= 1.2
    for m in range(len(c.charge)):
        z = c.numbers[c.mol == m]
        assert len(z) == 27 and len(z) % 4 == 3 and set(z) == set(D.ELEMENTS)
        assert set(nref[z]) == {2, 3, 4, 5}
    assert nref[5] == 5 and abs(t["cn_ref"][5, 5, 4, 0] - 4.59) < 0.01  # B's irregular last reference
    nb, sh = D.lists(c, 12.0)
    n = len(c.numbers)
    assert np.abs(sh).max() >= 2
    assert (nb[:n] != n).sum(-1).max() > 256  # several trips of the kernels' list loops (64 x 4 and 64 x 2 slots per trip)
    x = torch.cat([torch.as_tensor(c.coord).double(), torch.zeros(1, 3, dtype=torch.float64)])
    mol_p = torch.cat([torch.as_tensor(c.mol), torch.as_tensor(c.mol[-1:])])
    d, _, mask = O._distances(x, torch.as_tensor(nb), torch.as_tensor(sh).double(), torch.as_tensor(c.cell).double(), mol_p)
    assert int(((d > 9.6) & (d < 12.0) & ~mask).sum()) > 0  # pairs inside the switching window


def test_edges_case_has_the_properties_it_is_there_for():
    c = D.case("edges")
    assert len(c.numbers) == 10 and list(np.bincount(c.mol)) == [1, 2, 2, 5]
    assert c.numbers[D.LONE_ATOM] == 6 and c.numbers[D.BR_ATOM] == 35 and 35 >= D.tables()["rcov"].shape[0]  # Br: outside the slice
    assert abs(np.linalg.norm(c.coord[2].astype(np.float64) - c.coord[1]) - 10.5) < 1e-5  # O...S: inside 9.6 - 12 A
    assert abs(np.linalg.norm(c.coord[4].astype(np.float64) - c.coord[3]) - 1.1) < 1e-6   # H-F
    r = D.d3_reference(c, torch.float64)
    assert r["energy"][0] == 0.0 and not r["forces"][D.LONE_ATOM].any()
    assert r["energy"][1] < 0.0  # the switched pair contributes
    assert np.isfinite(r["forces"]).all() and np.abs(r["forces"][D.BR_ATOM]).max() > 1e-6  # through its neighbours' cn alone
    # ... and Br's own pairs give nothing: without Br's cn contribution to C and H the molecule is CH3 with the same energy function
    no_br = D._case("edges-no-br", np.delete(c.coord, D.BR_ATOM, 0), np.delete(c.numbers, D.BR_ATOM), np.delete(c.mol, D.BR_ATOM), None)
    assert abs(D.d3_reference(no_br, torch.float64)["energy"][3] - r["energy"][3]) < 1e-3 * abs(r["energy"][3])


def test_stress_gate_is_what_its_rule_gives():
    """16 x the largest |float32 twin - fp64| over the periodic cases, rounded up to one digit; not above a tenth of STRESS_ATOL.
    The twin is torch's float32 arithmetic on the host's CPU and its strain gradient cancels heavily, so the figure depends on the
    host: 4.9e-9 eV/A^3 (het27, par12) where the constant was fixed, 4.0e-8 (pbc96: 1.5e-7) on the CPU beside the MI355X
    (profiles/dftd3_fp64.md).  The constant is the tighter
    reading, and what holds on every host is asserted: it is never looser than the rule gives there.
    The energy gate's premise too: the float32 twin sits within 1.1e-6 eV (pbc96) and 3e-7 eV (het27) of fp64 - a third of the gate
    at most."""
    dev = {}
    for name, p in D.GATE_CASES:  # (par12 is the golden periodic section's own parameter set)
        dev[name, p] = D.twin_deviation(D.case(name), p)
        print(f"d3 twin | {name} | {p} | " + " | ".join(f"{k} {v:.2e}" for k, v in dev[name, p].items()))
    worst = max(v["stress"] for v in dev.values())
    assert D.STRESS_GATE <= D.one_digit_up(16.0 * worst), f"16 x {worst:.3e}"
    assert D.STRESS_GATE <= D.STRESS_GATE_CEILING and abs(D.STRESS_GATE_CEILING - STRESS_ATOL / 10) < 1e-20
    assert max(v["energy"] for v in dev.values()) <= D.ENERGY_GATE / 3


def _het27_totals(oracle32_cold):
    c = D.case("het27")
    tot = O.evaluate(oracle32_cold, c.coord, c.numbers, c.charge, mol_idx=c.mol, cell=c.cell, coulomb="none", stress=True,
                     dftd3=dict(D.get_par("par12"), **D.tables(D.Z_PAD)))
    return tot["forces"], tot["stress"]


@pytest.mark.parametrize("mutation", D.CLAIMED_MUTATIONS)
def test_reference_moves_by_a_hundred_gates_under_each_deliberate_error(mutation, oracle32_cold):
    c = D.case("het27")
    f_tot, s_tot = _het27_totals(oracle32_cold)
    gates = {"energy": D.ENERGY_GATE, "forces": D.force_gate(f_tot), "stress": D.stress_gate(s_tot)}
    moved = D.deviation(D.d3_reference(c, torch.float64, mutate=mutation), D.d3_reference(c, torch.float64))
    print(f"d3 sensitivity | {mutation} | " + " | ".join(f"{k} {moved[k]:.2e} = {moved[k] / gates[k]:.0f} gates" for k in gates))
    for k in gates:
        assert moved[k] >= D.SENSITIVITY * gates[k], f"{mutation}: {k} moves by {moved[k]:.2e}, gate {gates[k]:.2e}"


def test_drop_rule_is_recorded_and_not_claimed(oracle32_cold):
    """Removing the e^-12 drop rule moves het27 by less than 100 gates in every quantity (module docstring): it stays out of
    CLAIMED_MUTATIONS.  Should a change of the case bring it above, it belongs in the claim."""
    c = D.case("het27")
    f_tot, s_tot = _het27_totals(oracle32_cold)
    gates = {"energy": D.ENERGY_GATE, "forces": D.force_gate(f_tot), "stress": D.stress_gate(s_tot)}
    moved = D.deviation(D.d3_reference(c, torch.float64, mutate="no_drop_rule"), D.d3_reference(c, torch.float64))
    print("d3 sensitivity | no_drop_rule | " + " | ".join(f"{k} {moved[k]:.2e} = {moved[k] / gates[k]:.2f} gates" for k in gates))
    assert "no_drop_rule" not in D.CLAIMED_MUTATIONS
    assert all(0.0 < moved[k] < D.SENSITIVITY * gates[k] for k in gates)
