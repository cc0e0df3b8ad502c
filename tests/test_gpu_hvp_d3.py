"""The analytic DFT-D3 block of the Hessian sweep (csrc/d3.hip: d3_tcn / d3_tpair / d3_tcnforce; armed by
aimnet_engine_set_dftd3_tangent, HipEngine.hvp(..., d3_tangent=True)).

  * the block ALONE (aimnet_debug_dftd3_tangent) against tests/d3_tangent_yardstick.py::yardstick - the fp64 double-backward product
    of oracle.dftd3_energy - at GATE (5e-5 of max|H_d3 v|, derived there), on the cases of tests/d3_cases.py: het27 with par12, par9
    and par10 (N % 4 = 3, 27 atoms in 7 blocks; rows on and off multiples of 64), het27x2 (two cells), edges (an empty row, a pair
    inside the switching window, an element without a table entry, two-atom molecules); K in {1, 3, 5}, random and unit directions;
    the D3 forces of the same call against d3_cases.d3_reference at its force gate;
  * the whole path armed on mols-simple-d3, tiny3-dsf8-d3 and nse-mols-d3 of tests/tangent_cases.py against their fp64 `hv` at the
    existing 1e-5 + 3e-5 max|hv|, the D3 allowance replaced by GATE max|hv_d3|;
  * K = 5 computed as 5, as 2 + 3 and as 1 x 5 is bitwise equal; two runs are bitwise equal; the forces of the armed sweep equal the
    unarmed sweep's bit for bit; armed, aimnet_engine_hvp_workspace_bytes is smaller than unarmed by at least the replicas (the lifted
    limits are held on the CPU, tests/test_tangent_plan_d3.py).
Unarmed behaviour is what the existing tests hold, unedited.  Every comparison prints its figures before it asserts."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import d3_cases as D
import d3_tangent_yardstick as Y
import tangent_cases as T
from aimnetcentral_amd import _lib, capacity

pytestmark = pytest.mark.gpu


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def block(eng, c, par, V, want_forces=True, **kw):
    """H_d3 v (and the D3 forces) of the armed block alone, as float32 numpy arrays."""
    dev = eng.device
    eng.set_dftd3_tables(D.tables())
    args = (torch.from_numpy(c.coord).to(dev), torch.from_numpy(c.numbers.astype(np.int32)).to(dev),
            torch.from_numpy(c.mol.astype(np.int32)).to(dev), torch.from_numpy(c.charge).to(dev))
    if c.cell is not None:
        kw["cell"] = torch.from_numpy(c.cell).to(dev)
    try:
        out = eng.hvp(*args, torch.from_numpy(np.ascontiguousarray(V, np.float32)).to(dev), coulomb="none", dftd3=D.get_par(par),
                      want_forces=want_forces, d3_tangent=True, _d3_block_only=True, **kw)
        return {k: v.cpu().numpy() for k, v in out.items()}
    except RuntimeError as exc:  # nothing more is started on a GPU that has faulted
        if any(s in str(exc) for s in ("HIP error", "hipError", "illegal memory", "kernel launch failed", "code -2")):
            pytest.exit(f"device error in the D3 block of {c.name}: {exc}", returncode=3)
        raise


@pytest.mark.parametrize("kind", ["random", "unit"])
@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("name,par", Y.HELD)
def test_block_alone_meets_the_yardstick(hip_engine_cold, name, par, K, kind):
    c = D.case(name)
    V = Y.directions(c, K, kind)
    ref = Y.yardstick(c, par, V)
    out = block(hip_engine_cold, c, par, V)
    top = np.abs(ref).max()
    err = np.abs(out["hv"].astype(np.float64) - ref).max()
    f_ref = D.d3_reference(c, torch.float64, par=par)["forces"]
    f_err = np.abs(out["forces"].astype(np.float64) - f_ref).max()
    print(f"d3-hvp | block | {name} | {par} | K {K} {kind} | max|H v| {top:.3e} | err {err:.3e} = {err / top:.2e} of max, gate {Y.GATE:.0e}, "
          f"ratio {err / (Y.GATE * top):.3f} | forces {f_err:.2e} gate {D.FORCE_GATE:.0e}")
    assert out["hv"].shape == ref.shape and top > 0.0
    assert err <= Y.GATE * top, f"{name}/{par} K={K} {kind}: {err:.3e} > {Y.GATE * top:.3e}"
    assert f_err <= D.FORCE_GATE
    if name == "edges":  # the lone atom: no neighbour, no curvature
        assert not out["hv"][:, D.LONE_ATOM].any() and not out["forces"][D.LONE_ATOM].any()


def test_block_sees_the_switch_on_the_bond_direction(hip_engine_cold):
    """edges, the O...S pair displaced along its bond (inside the switching window): the block meets the yardstick, and the yardstick
    with the switch's derivatives detached sits more than 10 gates away (tests/test_d3_tangent_host.py derives the figure)."""
    c = D.case("edges")
    V = Y.directions(c, 3, "bond")
    ref = Y.yardstick(c, "par12", V)
    out = block(hip_engine_cold, c, "par12", V)
    top = np.abs(ref).max()
    err = np.abs(out["hv"].astype(np.float64) - ref).max()
    print(f"d3-hvp | block | edges | par12 | bond | max|H v| {top:.3e} | err {err:.3e} = {err / top:.2e} of max, ratio {err / (Y.GATE * top):.3f}")
    assert err <= Y.GATE * top


def test_grouping_and_repetition_change_no_bit(hip_engine_cold):
    """K = 5 as one call, as 2 + 3 and as five single directions; and the same call twice."""
    for name, par in (("het27", "par12"), ("edges", "par12")):
        c = D.case(name)
        V = Y.directions(c, 5)
        whole = block(hip_engine_cold, c, par, V)["hv"]
        again = block(hip_engine_cold, c, par, V)["hv"]
        split = np.concatenate([block(hip_engine_cold, c, par, V[:2])["hv"], block(hip_engine_cold, c, par, V[2:])["hv"]])
        single = np.concatenate([block(hip_engine_cold, c, par, V[k : k + 1])["hv"] for k in range(5)])
        for what, other in (("twice", again), ("2 + 3", split), ("1 x 5", single)):
            d = np.abs(whole.astype(np.float64) - other).max()
            print(f"d3-hvp | bits | {name} | K = 5 against {what}: max|d| {d:.2e}")
            assert bits_equal(whole, other), f"{name}: K = 5 against {what} differs by {d:.3e}"


def _engines(c, hip_engine, hip_engine_nse, oracle64, oracle64_nse):
    return (hip_engine_nse, oracle64_nse) if c.nse else (hip_engine, oracle64)


def _run(eng, c, armed, V=None, want_forces=True):
    eng.set_dftd3_tables(T.d3_tables())
    out = eng.hvp(*T.engine_args(eng, c), T._t(c.V if V is None else V), want_forces=want_forces, dftd3=c.d3, d3_tangent=armed, **c.coul,
                  **T.cell_kwargs(c))
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", ["mols-simple-d3", "tiny3-dsf8-d3", "nse-mols-d3"])
def test_whole_path_armed(name, hip_engine, hip_engine_nse, oracle64, oracle64_nse):
    c = T.case(name)
    eng, om = _engines(c, hip_engine, hip_engine_nse, oracle64, oracle64_nse)
    ref = T.reference(c, om)
    armed, unarmed = _run(eng, c, True), _run(eng, c, False)
    gate = 1e-5 + 3e-5 * np.abs(ref["hv"]).max() + Y.GATE * np.abs(ref["hv_d3"]).max()
    err = np.abs(armed["hv"].astype(np.float64) - ref["hv"]).max()
    err_u = np.abs(unarmed["hv"].astype(np.float64) - ref["hv"]).max()
    # the block's own error: both sweeps share every other term bit for bit, so their difference is block against block
    d3_armed = np.abs((armed["hv"].astype(np.float64) - ref["hv_sweep"]) - ref["hv_d3"]).max()
    print(f"d3-hvp | whole | {name} | max|hv| {np.abs(ref['hv']).max():.3e} max|hv_d3| {np.abs(ref['hv_d3']).max():.3e} | armed {err:.3e} "
          f"unarmed {err_u:.3e} gate {gate:.3e} ratio {err / gate:.3f} | armed - (sweep + d3) {d3_armed:.3e}")
    assert err <= gate, f"{name}: {err:.3e} > {gate:.3e}"
    assert err_u <= T.hv_gate(ref)  # (today's block at today's gate: the switch is off again after an armed call)
    assert bits_equal(armed["forces"], unarmed["forces"]), "the forces of the armed sweep are not the unarmed sweep's bits"
    again = _run(eng, c, True)
    assert bits_equal(armed["hv"], again["hv"]) and bits_equal(armed["forces"], again["forces"])


def test_armed_workspace_is_smaller_by_at_least_the_replicas(hip_engine_cold):
    eng = hip_engine_cold
    c, p = D.case("het27"), D.get_par("par12")
    block(eng, c, "par12", Y.directions(c, 1), want_forces=False)  # settles the D3 row capacity
    n, n_mol = len(c.numbers), 1
    rq = capacity.Request("hvp", n, n_mol, True, _lib.COULOMB_NONE, 15.0, 0.2, 1e-6, p)
    opt = eng.fill_options(rq)
    sizes = {}
    try:
        for armed in (0, 1):
            _lib.check(eng.lib.aimnet_engine_set_dftd3_tangent(eng._h, armed), "aimnet_engine_set_dftd3_tangent")
            sizes[armed] = {K: int(eng.lib.aimnet_engine_hvp_workspace_bytes(eng._h, n, n_mol, K, C.byref(opt))) for K in (1, 2, 16)}
    finally:
        eng.lib.aimnet_engine_set_dftd3_tangent(eng._h, 0)
    for K in (1, 2, 16):
        replicas = 2 * 4 * K * n * int(opt.max_nb_d3) * 4
        print(f"d3-hvp | workspace | het27 K {K} | unarmed {sizes[0][K]} armed {sizes[1][K]} | replicas {replicas}")
        assert sizes[1][K] < sizes[0][K] and sizes[0][K] - sizes[1][K] >= replicas
    # per direction the armed block asks for 32 bytes per atom where the unarmed one asks for 4 (8 max_nb_d3 + 92)
    per_dir = {a: sizes[a][2] - sizes[a][1] for a in (0, 1)}
    assert per_dir[0] - per_dir[1] >= 2 * 4 * n * int(opt.max_nb_d3) * 4
