"""The DFT-D3 block under strain, host side (CPU only): tests/d3_strain_yardstick.py itself, the calculator's plumbing and the bindings.

  * the yardstick (fp64 double backward of oracle.dftd3_energy with respect to the coordinates and a per-system strain matrix) meets
    the 4-point difference along the path where that difference is smooth (het27 / par12, het27 / par9: 1e-6 absolute), the rotation
    and the mixed identity of tests/strain_cases.py to 1e-10 on every held case, d3_tangent_yardstick.yardstick at eps = 0 to 1e-9, and
    the closed form the kernels implement to 1e-9 relative;
  * GATE_HV / GATE_DS follow their rule on this host, every claimed mutation of the closed form sits at least d3_cases.SENSITIVITY gates
    away on a held (case, direction), and no exponent of a held case lies within MASK_MARGIN of the -12 cut;
  * AIMNet2Calculator.strain_response / elastic_constants with the external term: one armed call after set_dftd3_hessian("analytic"),
    a NotImplementedError that names the setter and no call otherwise;
  * aimnet_engine_set_strain_terms is exported and refuses a null engine.
Every comparison prints its figures before it asserts."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import d3_cases as D
import d3_strain_yardstick as SY
import d3_tangent_yardstick as Y
import strain_cases as SC
from aimnetcentral_amd import _lib, elasticity
from fake_engine import fake_calculator
from test_calculator_requests import TABLES, _spec
from test_strain_host import CELL, EPS, StrainEngine


def _case(name, par):
    c, p = SY.held(name, par)
    V, E = SY.directions(c)
    return c, p, V, E


@pytest.mark.parametrize("name,par", SY.SMOOTH)
def test_yardstick_meets_the_difference_where_it_is_smooth(name, par):
    c, p, V, E = _case(name, par)
    ref = SY.yardstick(c, p, V, E)
    worst = [0.0, 0.0]
    for k in range(len(V)):
        dG, dS = SY.difference4(c, p, V[k], E[k])
        e = (float(np.abs(dG - ref["hv"][k]).max()), float(np.abs(dS - ref["dS"][k]).max()))
        print(f"d3-strain | difference | {name} | {par} | direction {k} | hv {e[0]:.2e} dS {e[1]:.2e}")
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    assert worst[0] <= 1e-6 and worst[1] <= 1e-6


@pytest.mark.parametrize("name,par", SY.HELD)
def test_yardstick_satisfies_the_two_identities(name, par):
    c, p, V, E = _case(name, par)
    ref = SY.yardstick(c, p, V, E)
    rg, rs = SC.rotation_residual(ref["G"], ref["S"], ref["hv"][8], ref["dS"][8], E[8])
    print(f"d3-strain | rotation | {name} | {par} | dG - G w {rg:.2e} | dS - (S w + w^T S) {rs:.2e}")
    assert rg <= 1e-10 and rs <= 1e-10
    n_cell = ref["S"].shape[0]
    mol = np.asarray(c.mol) if n_cell > 1 else np.zeros(len(c.numbers), np.int64)
    for k in range(7):  # the displacement (direction 7) against the six Voigt strains and the non-symmetric one (its own v taken out)
        only_eps = SY.yardstick(c, p, np.zeros_like(V[k : k + 1]), E[k : k + 1])["hv"][0]
        res = SC.mixed_residual(mol, n_cell, ref["G"], V[7], E[k], ref["dS"][7], only_eps)
        print(f"d3-strain | mixed | {name} | {par} | strain {k} | {np.abs(res).max():.2e}")
        assert np.abs(res).max() <= 1e-10


@pytest.mark.parametrize("name,par", SY.HELD)
def test_without_a_strain_it_is_the_displacement_yardstick_and_the_closed_form_is_the_yardstick(name, par):
    c, p, V, E = _case(name, par)
    ref = SY.yardstick(c, p, V, E)
    # (d3_tangent_yardstick lists the coordinates as they are: it is given the wrapped ones, which are the case's own for d3_cases)
    cw = SimpleNamespace(**{**vars(c), "name": c.name + "~wrapped", "coord": np.array(SY.wrapped(c))})
    plain = Y.yardstick(cw, p, V[7:8].astype(np.float32))
    d0 = float(np.abs(ref["hv"][7] - plain[0]).max())
    cf = SY.closed_form(c, p, V, E)
    r = {"hv": SY.rel_hv(cf["hv"], ref["hv"]), "dS": SY.rel_dS(cf["dS"], ref["dS"]),
         "G": float(np.abs(cf["G"] - ref["G"]).max() / np.abs(ref["G"]).max()), "S": float(np.abs(cf["S"] - ref["S"]).max() / np.abs(ref["S"]).max())}
    print(f"d3-strain | eps = 0 | {name} | {par} | {d0:.2e} | closed form: " + " ".join(f"{k} {v:.2e}" for k, v in r.items()))
    assert d0 <= 1e-9
    assert all(v <= 1e-9 for v in r.values())
    if par is not None:  # G and S are the reference's own forces and stress
        f = D.d3_reference(c, torch.float64, par=par)
        vol = np.abs(np.linalg.det(np.asarray(c.cell, np.float64).reshape(-1, 3, 3)))[:, None, None]
        assert np.abs(ref["G"] + f["forces"]).max() <= 1e-12 and np.abs(ref["S"] / vol - f["stress"]).max() <= 1e-12


def test_gates_follow_their_rule():
    worst = [0.0, 0.0]
    for name, par in SY.HELD:
        c, p, V, E = _case(name, par)
        hv, dS = SY.twin_deviation(c, p, V, E)
        print(f"d3-strain | twin | {name} | {par} | hv {hv:.2e} dS {dS:.2e}")
        worst = [max(worst[0], hv), max(worst[1], dS)]
    rule = [D.one_digit_up(SY.TWIN_FACTOR * w) for w in worst]
    print(f"d3-strain | gate | hv: 16 x {worst[0]:.2e} -> {rule[0]:.0e}, GATE_HV {SY.GATE_HV:.0e} | dS: 16 x {worst[1]:.2e} -> {rule[1]:.0e}, "
          f"GATE_DS {SY.GATE_DS:.0e}")
    assert SY.TWIN_FACTOR == 16.0
    assert SY.GATE_HV >= rule[0] and SY.GATE_DS >= rule[1]  # never tighter than the rule gives here


def test_every_claimed_mutation_is_a_hundred_gates_away_somewhere():
    assert set(SY.CLAIMED_MUTATIONS) >= {"cn_pass_without_r_eps", "virial_without_tr_inc", "virial_without_cnforce_share"}
    best = dict.fromkeys(SY.CLAIMED_MUTATIONS, 0.0)
    for name, par in SY.HELD:
        c, p, V, E = _case(name, par)
        cf = SY.closed_form(c, p, V, E)
        top_hv, top_dS = np.abs(cf["hv"]).max(), np.abs(cf["dS"]).max(axis=(0, 2, 3))
        for m in SY.CLAIMED_MUTATIONS:
            mf = SY.closed_form(c, p, V, E, m)
            for k in range(len(V)):
                g_hv = np.abs(mf["hv"][k] - cf["hv"][k]).max() / top_hv / SY.GATE_HV
                g_dS = (np.abs(mf["dS"][k] - cf["dS"][k]).max(axis=(1, 2)) / top_dS).max() / SY.GATE_DS
                best[m] = max(best[m], float(g_hv), float(g_dS))
            print(f"d3-strain | sensitivity | {name} | {par} | {m} | best so far {best[m]:.0f} gates")
    assert all(v >= D.SENSITIVITY for v in best.values()), best


def test_no_exponent_of_a_held_case_sits_at_the_cut():
    for name, par in SY.HELD:
        c, p = SY.held(name, par)
        m = SY.mask_margin(c, p)
        print(f"d3-strain | mask margin | {name} | {par} | {m:.2e}")
        assert m > SY.MASK_MARGIN
        if par is not None:
            assert m == pytest.approx(Y.mask_margin(c, par), rel=1e-9)
    import tangent_cases as T

    m = SY.mask_margin(SC.case("tiny1-TTF"), T._d3(9.0))  # the calculator's case of tests/test_gpu_strain_d3.py (an open axis)
    print(f"d3-strain | mask margin | tiny1-TTF | 9 A | {m:.2e}")
    assert m > SY.MASK_MARGIN


# ---- the calculator and the bindings ------------------------------------------------------------------------------------------------
def test_calculator_carries_the_term_after_the_setter_and_refuses_before(monkeypatch):
    calc = fake_calculator(monkeypatch, StrainEngine, spec=_spec(True), dftd3_data=TABLES)
    assert calc._dftd3_hessian is None
    for what in (lambda: calc.strain_response(CELL, EPS), lambda: calc.elastic_constants(CELL)):
        with pytest.raises(NotImplementedError, match=r"DFT-D3.*set_dftd3_hessian\('analytic'\)"):
            what()
    assert not calc.engine.hvp_calls
    calc.set_dftd3_hessian("analytic")
    out = calc.strain_response(CELL, EPS)
    (call,) = calc.engine.hvp_calls
    assert call["d3_tangent"] is True and call["strain_terms"] == ("dftd3",) and call["dftd3"] is not None
    assert tuple(call["strain"].shape) == (2, 3, 3) and call["want_forces"] is True and call["K"] == 2
    assert out["stress_derivative"].shape == (2, 3, 3)
    ec = calc.elastic_constants(CELL)
    assert len(calc.engine.hvp_calls) == 2
    last = calc.engine.hvp_calls[-1]
    assert last["K"] == 15 and last["d3_tangent"] is True and last["strain_terms"] == ("dftd3",) and last["dftd3"] is not None
    assert np.array_equal(last["strain"][9:].numpy(), elasticity.voigt_strains().astype(np.float32))
    assert ec["born"].shape == (6, 6)
    calc.set_dftd3_hessian(None)
    with pytest.raises(NotImplementedError, match="DFT-D3"):
        calc.strain_response(CELL, EPS)
    assert len(calc.engine.hvp_calls) == 2


def test_calculator_without_the_term_never_sends_the_keywords(monkeypatch):
    calc = fake_calculator(monkeypatch, StrainEngine)
    calc.set_dftd3_hessian("analytic")
    calc.strain_response(CELL, EPS)
    (call,) = calc.engine.hvp_calls
    assert "d3_tangent" not in call and "strain_terms" not in call and call["dftd3"] is None


def test_symbol_and_null_engine():
    assert "aimnet_engine_set_strain_terms" in _lib.EXPORTED_SYMBOLS
    assert _lib.STRAIN_TERMS == {"dftd3": 1}
    lib = _lib.load()
    assert lib.aimnet_engine_set_strain_terms(None, 0) == _lib.E_INVALID
