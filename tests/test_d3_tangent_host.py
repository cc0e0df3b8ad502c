"""The premises of tests/test_gpu_hvp_d3.py, without a GPU (tests/d3_tangent_yardstick.py holds the functions and the constants):

  * the yardstick (fp64 double backward of oracle.dftd3_energy) is pinned to Richardson-extrapolated central differences of
    d3_cases.d3_reference forces, is symmetric, and equals the closed form the kernels implement (include/aimnet_hip.h);
  * GATE follows the rule of d3_cases.STRESS_GATE: never looser than 16 x the largest |float32 twin - fp64| / max|H_d3 v| met on this
    host over the held (case, parameters, direction) combinations, and below the ceiling (a third of tangent_cases.D3_RELATIVE);
  * no (a, b) exponent of a held case lies within 1e-3 of the -12 cut (fp32 and fp64 agree on the mask);
  * sensitivity, omissions made through d3_cases._rewritten: freezing cn (C6 held constant) moves H_d3 v by ~100 % of its maximum,
    freezing cn_j alone by ~50 % - thousands of gates; detaching the switch is claimed only on the direction that displaces the O...S pair of
    `edges` along its bond, where it reaches 10 gates, and is listed as unclaimed elsewhere;
  * what the coordination number's own accuracy costs: 4.3 x its error, of max|H_d3 v| (het27);
  * AIMNet2Calculator.set_dftd3_hessian against the recording fake engine, and the symbols.
Every figure is printed before it is asserted."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import d3_cases as D
import d3_tangent_yardstick as Y
import tangent_cases as T
from aimnetcentral_amd import _lib
from fake_engine import FakeEngine, fake_calculator
from test_calculator_requests import TABLES, V, _spec

KINDS = ("random", "unit")


def _rel(a, b, ref):
    return float(np.abs(a - b).max() / np.abs(ref).max())


@pytest.mark.parametrize("name", ["edges", "het27", "het27x2"])
def test_yardstick_is_pinned_to_differences_of_the_reference_forces(name):
    c = D.case(name)
    V1 = np.concatenate([Y.directions(c, 1), Y.directions(c, 1, "unit")])
    ref, rich = Y.yardstick(c, "par12", V1), Y.richardson(c, "par12", V1)
    for k in range(2):
        r = _rel(ref[k], rich[k], ref[k])
        print(f"d3-tangent | richardson | {name} | direction {k} | {r:.2e} of max|H v| = {np.abs(ref[k]).max():.3e}")
        assert r <= 1e-8


@pytest.mark.parametrize("name,par", Y.HELD)
def test_yardstick_is_symmetric_and_the_closed_form_is_the_yardstick(name, par):
    c = D.case(name)
    V2 = Y.directions(c, 2)
    h = Y.yardstick(c, par, V2)
    a, b = float((V2[0].astype(np.float64) * h[1]).sum()), float((V2[1].astype(np.float64) * h[0]).sum())
    scale = np.abs(V2).max() ** 2 * np.abs(h).max() * V2[0].size
    print(f"d3-tangent | symmetry | {name} | {par} | v0.Hv1 {a:.12e} v1.Hv0 {b:.12e} | {abs(a - b) / scale:.1e} of scale")
    assert abs(a - b) <= 1e-12 * scale
    for kind in KINDS + (("bond",) if name == "edges" else ()):
        Vk = Y.directions(c, 3, kind)
        r = _rel(Y.closed_form(c, par, Vk), Y.yardstick(c, par, Vk), Y.yardstick(c, par, Vk))
        print(f"d3-tangent | closed form | {name} | {par} | {kind} | {r:.2e}")
        assert r <= 1e-12


def test_gate_follows_its_rule():
    dev = {}
    for name, par in Y.HELD:
        c = D.case(name)
        for K in (1, 3, 5):
            for kind in KINDS:
                dev[name, par, K, kind] = Y.twin_deviation(c, par, Y.directions(c, K, kind))
    worst_key = max(dev, key=dev.get)
    worst = dev[worst_key]
    for key in sorted(dev, key=dev.get)[-5:]:
        print(f"d3-tangent | twin | {key} | {dev[key]:.2e}")
    print(f"d3-tangent | gate | 16 x {worst:.2e} = {16 * worst:.2e} -> {D.one_digit_up(16 * worst):.0e}; GATE {Y.GATE:.0e}, ceiling {Y.GATE_CEILING:.0e}")
    assert Y.GATE <= D.one_digit_up(Y.TWIN_FACTOR * worst), f"16 x {worst:.3e} on {worst_key}"
    assert Y.GATE <= Y.GATE_CEILING and abs(Y.GATE_CEILING - 1e-4) < 1e-20 and Y.GATE_CEILING <= T.D3_RELATIVE / 3
    assert worst <= Y.GATE / 3  # the premise: fp32 arithmetic alone sits well inside the gate


def test_no_exponent_of_a_held_case_sits_at_the_cut():
    for name, par in Y.HELD:
        m = Y.mask_margin(D.case(name), par)
        print(f"d3-tangent | mask margin | {name} | {par} | {m:.2e}")
        assert m > Y.MASK_MARGIN


FREEZE_CN = ("    cn = cn_ij.sum(-1)", "    cn = cn_ij.sum(-1).detach()")
FREEZE_CN_J = ("    cn_j = cn[nbmat].unsqueeze(-1).unsqueeze(-1)", "    cn_j = cn.detach()[nbmat].unsqueeze(-1).unsqueeze(-1)")
DETACH_SWITCH = ("    e_ij = (-c6ij * damping * sw)", "    e_ij = (-c6ij * damping * sw.detach())")


@pytest.mark.parametrize("name", ["het27", "edges"])
def test_gate_sees_a_frozen_coordination_number(name):
    c = D.case(name)
    Vk = Y.directions(c, 3)
    ref = Y.yardstick(c, "par12", Vk)
    for what, (old, new), floor in (("cn frozen", FREEZE_CN, 0.5), ("cn_j frozen", FREEZE_CN_J, 0.25)):
        r = _rel(Y.yardstick(c, "par12", Vk, energy_fn=D._rewritten(old.strip(), new.strip())), ref, ref)
        print(f"d3-tangent | sensitivity | {name} | {what} | {r:.2e} of max = {r / Y.GATE:.0f} gates")
        assert r >= floor and r >= D.SENSITIVITY * Y.GATE


def test_switch_derivatives_are_claimed_on_the_bond_direction_only():
    c = D.case("edges")
    fn = D._rewritten(DETACH_SWITCH[0].strip(), DETACH_SWITCH[1].strip())
    seen = {}
    for kind in ("bond", "random", "unit"):
        Vk = Y.directions(c, 3, kind)
        ref = Y.yardstick(c, "par12", Vk)
        seen[kind] = _rel(Y.yardstick(c, "par12", Vk, energy_fn=fn), ref, ref)
        print(f"d3-tangent | sensitivity | edges | switch detached | {kind} | {seen[kind]:.2e} of max = {seen[kind] / Y.GATE:.1f} gates"
              + ("" if kind == "bond" else "  (unclaimed)"))
    assert seen["bond"] >= 10 * Y.GATE


def test_what_the_coordination_number_costs():
    """The exponents -4 (cn - cnref)^2 are steep: an error e of every cn moves H_d3 v by ~4 e of its maximum on het27, so the fp32
    cn of the primal pass (a few 1e-7) costs ~1e-6, inside the gate; the centred moments keep the C6 derivatives at that level."""
    c = D.case("het27")
    Vk = Y.directions(c, 3)
    ref = Y.yardstick(c, "par12", Vk)
    for e in (1e-7, 1e-6):
        r = _rel(Y.closed_form(c, "par12", Vk, cn_error=e), ref, ref)
        print(f"d3-tangent | cn error {e:.0e} | {r:.2e} of max = {r / e:.1f} x")
        assert r <= 10 * e
    assert _rel(Y.closed_form(c, "par12", Vk, cn_error=1e-6), ref, ref) <= Y.GATE / 5


# ---- the calculator and the bindings ------------------------------------------------------------------------------------------------
class RecordingHvpEngine(FakeEngine):
    def hvp(self, coord, numbers, mol_idx, charge, vectors, **kw):
        self.hvp_calls.append(dict(kw, K=int(vectors.shape[0]), n=int(coord.shape[0])))
        return {"hv": torch.zeros_like(vectors)}


WATER_CELL = dict(coord=[[0.0, 0.0, 0.1173], [0.0, 0.7572, -0.4692], [0.0, -0.7572, -0.4692]], numbers=[8, 1, 1], charge=0.0,
                  cell=np.eye(3, dtype=np.float32) * 9.0)


def test_calculator_arms_the_block_and_only_with_the_term(monkeypatch):
    calc = fake_calculator(monkeypatch, RecordingHvpEngine, spec=_spec(True), dftd3_data=TABLES)
    assert calc._dftd3_hessian is None
    calc.hessian_vector_product(WATER_CELL, V)
    assert "d3_tangent" not in calc.engine.hvp_calls[-1] and calc.engine.hvp_calls[-1]["dftd3"] is not None  # the default: today's call
    calc.set_dftd3_hessian("analytic")
    calc.hessian_vector_product(WATER_CELL, V)
    assert calc.engine.hvp_calls[-1]["d3_tangent"] is True
    out = calc(WATER_CELL, hessian=True)
    assert out["hessian"].shape == (3, 3, 3, 3) and calc.engine.hvp_calls[-1]["d3_tangent"] is True and calc.engine.hvp_calls[-1]["K"] == 9
    calc.set_pme_hessian("analytic")  # combinable: both switches in one call of the sweep
    calc.set_lrcoulomb_method("pme")
    calc.hessian_vector_product(WATER_CELL, V)
    last = calc.engine.hvp_calls[-1]
    assert last["d3_tangent"] is True and last["pme_tangent"] is True and last["coulomb"] == "pme"
    n_hvp, n_eval = len(calc.engine.hvp_calls), len(calc.engine.calls)
    calc.hvp_method = "fd"  # differences of forces do not read the switch
    calc.hessian_vector_product(WATER_CELL, V)
    assert len(calc.engine.hvp_calls) == n_hvp and len(calc.engine.calls) > n_eval
    calc.hvp_method = "analytic"
    calc.set_dftd3_hessian(None)
    calc.hessian_vector_product(WATER_CELL, V)
    assert "d3_tangent" not in calc.engine.hvp_calls[-1]
    for bad in ("fd", "Analytic", True, 1):
        with pytest.raises(ValueError, match="set_dftd3_hessian"):
            calc.set_dftd3_hessian(bad)


def test_calculator_without_the_term_never_sends_the_keyword(monkeypatch):
    calc = fake_calculator(monkeypatch, RecordingHvpEngine)
    calc.set_dftd3_hessian("analytic")
    calc.hessian_vector_product(WATER_CELL, V)
    assert "d3_tangent" not in calc.engine.hvp_calls[-1]


def test_symbols():
    assert {"aimnet_engine_set_dftd3_tangent", "aimnet_debug_dftd3_tangent"} <= set(_lib.EXPORTED_SYMBOLS)
    lib = _lib.load()
    assert lib.aimnet_engine_set_dftd3_tangent(None, 1) == _lib.E_INVALID
    assert lib.aimnet_debug_dftd3_tangent(None, None, None, None, 0, None, None, None, None, 0, None) == _lib.E_INVALID
