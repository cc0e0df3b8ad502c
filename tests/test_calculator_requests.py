"""What AIMNet2Calculator sends to the engine, for every entry point that resolves the call's long-range terms and `pbc`, over a
product of calculator states and inputs (the recording FakeEngine of tests/fake_engine.py; CPU only).  One rule per question:
the Coulomb method, its DSF parameters, the Ewald accuracy, the DFT-D3 options and the `pbc` flags of a call do not depend on the
entry point it came in through, no call changes the calculator, and only `eval` announces the periodic "simple" -> DSF switch.
The expectations are written out from the setters' documented behaviour, not read off any entry point."""
from __future__ import annotations

import dataclasses
import itertools
import pathlib
import warnings

import numpy as np
import pytest

from aimnetcentral_amd import loader
from fake_engine import WATER, fake_calculator

TABLES = dict(np.load(str(pathlib.Path(__file__).parent / "golden" / "dftd3_subset.npz")))
D3_PARAMS = {"s8": 0.39, "a1": 0.57, "a2": 3.1, "s6": 1.0}
V = np.arange(18, dtype=np.float32).reshape(2, 3, 3)

# state -> (setter calls, (coulomb, dsf_rc, dsf_alpha) sent without a cell, the same with a cell, D3 cutoff)
DSF_DEFAULT = ("dsf", 15.0, 0.2)
STATES = {
    "none": ([], ("none", 15.0, 0.2), ("none", 15.0, 0.2), 15.0),
    "simple": ([], ("simple", 15.0, 0.2), DSF_DEFAULT, 15.0),
    "dsf8": ([("set_lrcoulomb_method", ("dsf",), dict(cutoff=8.0, dsf_alpha=0.25))], ("dsf", 8.0, 0.25), ("dsf", 8.0, 0.25), 15.0),
    "simple_after_dsf8": ([("set_lrcoulomb_method", ("dsf",), dict(cutoff=8.0, dsf_alpha=0.25)), ("set_lrcoulomb_method", ("simple",), {})],
                          ("simple", 8.0, 0.25), DSF_DEFAULT, 15.0),
    "simple_after_lr_cutoff10": ([("set_lr_cutoff", (10.0,), {})], ("simple", 15.0, 0.2), DSF_DEFAULT, 10.0),
    "ewald": ([("set_lrcoulomb_method", ("ewald",), dict(ewald_accuracy=1e-5))], None, ("ewald", 15.0, 0.2), 15.0),
    "pme": ([("set_lrcoulomb_method", ("pme",), {})], None, ("pme", 15.0, 0.2), 15.0),
}
ACCURACY = {"ewald": 1e-5, "pme": 1e-6}
CELLS = {"nocell": None, "cell": np.eye(3, dtype=np.float32) * 9.0}
# pbc input -> what the engine must receive, or the ValueError of `eval`
PBC = {
    "absent": (None, (True, True, True)),
    "mixed3": ([True, False, True], (True, False, True)),
    "row1x3": ([[True, False, True]], (True, False, True)),
    "bad2x3": ([[True, True, True], [True, False, True]], r"pbc must have shape \(3,\) or \(1, 3\), got \(2, 3\)"),
    "bad2": ([True, False], r"pbc must have shape \(3,\) or \(B, 3\)"),
}
ENTRIES = ("eval", "eval_hessian", "hvp", "hvp_fd", "charge_response")
ATTRS = ("coulomb_method", "coulomb_cutoff", "cutoff_lr")

_SPECS: dict[bool, object] = {}


def _spec(d3: bool):
    if not _SPECS:
        base = loader.synthetic_spec(0)
        _SPECS[False] = base
        _SPECS[True] = dataclasses.replace(base, metadata=dict(base.metadata, needs_dispersion=True, d3_params=D3_PARAMS))
    return _SPECS[d3]


def _calculator(monkeypatch, state: str, d3: bool):
    kw = dict(dftd3_data=TABLES) if d3 else {}
    if state == "none":
        kw["needs_coulomb"] = False
    calc = fake_calculator(monkeypatch, spec=_spec(d3), **kw)
    for name, args, kwargs in STATES[state][0]:
        getattr(calc, name)(*args, **kwargs)
    return calc


def _observable(calc):
    ext = calc.external_coulomb
    return tuple(getattr(calc, a) for a in ATTRS) + ((ext.dsf_rc, ext.dsf_alpha) if ext is not None else (None, None))


def _run(calc, entry: str, data):
    if entry == "eval":
        return calc.eval(data, forces=True)
    if entry == "eval_hessian":
        return calc.eval(data, forces=True, hessian=True)
    if entry == "charge_response":
        return calc.charge_response(data, V)
    calc.hvp_method = "fd" if entry == "hvp_fd" else "analytic"
    return calc.hessian_vector_product(data, V)


@pytest.mark.parametrize("state,d3,cell,pbc,entry", [
    pytest.param(*c, id="-".join(("d3" if x else "nod3") if isinstance(x, bool) else x for x in c))
    for c in itertools.product(STATES, (False, True), CELLS, PBC, ENTRIES)])
def test_request(monkeypatch, state, d3, cell, pbc, entry):
    calc = _calculator(monkeypatch, state, d3)
    _, open_request, periodic_request, d3_cutoff = STATES[state]
    request = periodic_request if cell == "cell" else open_request
    pbc_in, pbc_out = PBC[pbc]
    data = dict(WATER, **({"cell": CELLS[cell]} if cell == "cell" else {}), **({"pbc": pbc_in} if pbc_in is not None else {}))
    long_range = entry != "charge_response"  # the charges see no long-range term: nothing of it is resolved or sent
    if long_range and request is None:
        error = "requires a periodic 'cell'"  # raised before the pbc flags are looked at, as in `eval`
    else:
        error = pbc_out if isinstance(pbc_out, str) else None
    before = _observable(calc)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        try:
            if error is not None:
                with pytest.raises(ValueError, match=error):
                    _run(calc, entry, data)
            else:
                _run(calc, entry, data)
        finally:
            assert _observable(calc) == before
    switching = [w for w in caught if "Switching to DSF Coulomb for PBC" in str(w.message)]
    announced = entry in ("eval", "eval_hessian") and cell == "cell" and state.startswith("simple")
    assert len(switching) == (1 if announced else 0) and all(w.category is UserWarning for w in switching)
    eng = calc.engine
    if error is not None:
        assert not eng.calls and not eng.hvp_calls and not eng.charge_response_calls
        return
    if not long_range:
        assert [c["pbc"] for c in eng.charge_response_calls] == [pbc_out] and not eng.calls and not eng.hvp_calls
        return
    # which operator carried the request: `eval` alone, the tangent sweep, or differences of forces (always for "pme")
    fd = entry == "hvp_fd" or request[0] == "pme"
    n_eval = {"eval": 1, "eval_hessian": 1 + fd, "hvp": 0 + fd, "hvp_fd": 1}[entry]
    n_hvp = 0 if (fd or entry == "eval") else 1
    assert (len(eng.calls), len(eng.hvp_calls), len(eng.charge_response_calls)) == (n_eval, n_hvp, 0)
    dftd3 = dict(D3_PARAMS, cutoff=d3_cutoff, smoothing_fraction=0.2) if d3 else None
    for call in eng.calls + eng.hvp_calls:
        assert (call["coulomb"], call["dsf_rc"], call["dsf_alpha"]) == request
        assert call["dftd3"] == dftd3 and call["pbc"] == pbc_out
        if request[0] in ACCURACY:
            assert call["ewald_accuracy"] == ACCURACY[request[0]]
