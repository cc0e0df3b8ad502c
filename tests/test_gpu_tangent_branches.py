"""aimnet_engine_hvp and aimnet_engine_charge_response (csrc/hvp.hip) against the fp64 oracle on the branches of csrc/tangent_plan.h
and of the tangent kernels that the other GPU tests do not reach: no Coulomb term, DSF without a cell, partial and per-system
periodicity, cells smaller than the cutoffs (lattice shifts of 2 and 3, self images, atoms outside their box), molecules of one to
three atoms, the D3 block on batches / per-system cells / two channels, the bounding-box list, and the three GEMM modes.  Inputs,
references and gates: tests/tangent_cases.py (tests/test_tangent_branch_fixtures.py pins on the CPU that each case is what its name
says).  Every comparison prints max|d|, its gate and their ratio before it asserts."""
from __future__ import annotations

import numpy as np
import pytest

import tangent_cases as T
from conftest import CHARGE_ATOL, assert_forces_close

pytestmark = pytest.mark.gpu


def _ratio(what, err, gate):
    err, gate = np.asarray(err, np.float64), np.asarray(gate, np.float64)
    r = float((err / gate).max()) if err.size else 0.0
    print(f"[tangent-branches] {what}: max|d| = {float(err.max()):.3e}, gate {float(gate.min()):.3e}, ratio {r:.3f}")
    assert (err <= gate).all(), f"{what}: ratio {r:.3f}"


def _engines(c, hip_engine, hip_engine_nse, oracle64, oracle64_nse):
    return (hip_engine_nse, oracle64_nse) if c.nse else (hip_engine, oracle64)


def _check_hvp(name, eng, c, ref, tag=""):
    out = T.run_hvp(eng, c)
    assert out["hv"].shape == ref["hv"].shape
    _ratio(f"{name}{tag} hv", np.abs(out["hv"] - ref["hv"]).max(), T.hv_gate(ref))
    f_err, f_top = np.abs(out["forces"] - ref["forces"]).max(), np.abs(ref["forces"]).max()
    print(f"[tangent-branches] {name}{tag} forces of the sweep: max|d| = {f_err:.3e}, gate {1e-5 + 1e-4 * f_top:.3e}, "
          f"ratio {f_err / (1e-5 + 1e-4 * f_top):.3f}")
    assert_forces_close(out["forces"], ref["forces"], f"{name}{tag} (forces of the sweep)")
    return out


@pytest.mark.parametrize("name", T.HVP_CASES)
def test_hvp(name, hip_engine, hip_engine_nse, oracle64, oracle64_nse):
    c = T.case(name)
    eng, om = _engines(c, hip_engine, hip_engine_nse, oracle64, oracle64_nse)
    ref = T.reference(c, om)
    _check_hvp(name, eng, c, ref)
    if name == "mols-simple":  # the first direction alone: 94 stacked rows, the exact-fp32 GEMMs (six directions: 329, the split ones)
        n = len(c.numbers)
        assert n + n <= T.SPLIT_GEMM_ROWS < n + len(c.V) * n
        one = T.run_hvp(eng, c, V=c.V[:1])
        _ratio(f"{name} hv, first direction alone", np.abs(one["hv"] - ref["hv"][:1]).max(), T.hv_gate(ref, slice(0, 1)))
    if name.startswith("lone-atom"):
        assert not ref["hv"].any()  # one atom: H = 0


@pytest.mark.parametrize("name", T.CHARGE_RESPONSE_CASES)
def test_charge_response(name, hip_engine, hip_engine_nse, oracle64, oracle64_nse):
    c = T.case(name)
    eng, om = _engines(c, hip_engine, hip_engine_nse, oracle64, oracle64_nse)
    ref = T.reference(c, om)
    out = T.run_charge_response(eng, c)
    K, n, n_mol = len(c.V), len(c.numbers), len(c.charge)
    assert out["dq"].shape == (K, n) and out["charges"].shape == (n,) and ("dspin" in out) == c.nse
    tq = ref["t_q"]
    _ratio(f"{name} dq", np.abs(out["dq"] - tq.sum(-1)).max(), T.tangent_gate(tq.sum(-1)))
    _ratio(f"{name} charges", np.abs(out["charges"] - ref["charges"]).max(), CHARGE_ATOL)
    if c.nse:
        _ratio(f"{name} dspin", np.abs(out["dspin"] - (tq[..., 0] - tq[..., 1])).max(), T.tangent_gate(tq[..., 0] - tq[..., 1]))
    if c.cell is None:
        assert out["dmu"].shape == (K, n_mol, 3)
        dmu, bound = T.dmu_reference(c, ref)
        _ratio(f"{name} dmu", np.abs(out["dmu"] - dmu).max(-1), bound)
    else:
        assert "dmu" not in out
    if name == "lone-atom":  # dq = 0 and dmu = q v
        assert not tq.any() and np.array_equal(dmu[:, 0], ref["charges"][0] * c.V[:, 0].astype(np.float64))


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("name", ["mols-dsf", "tiny3-dsf8"])
def test_gemm_modes(name, mode, hip_engine, oracle64):
    """The sweep with the exact-fp32 GEMMs everywhere (0) and the split GEMMs at every size (2): the same gates."""
    c = T.case(name)
    ref = T.reference(c, oracle64)
    before = hip_engine.get_option("gemm_bf3")
    hip_engine.set_option("gemm_bf3", mode)
    try:
        _check_hvp(name, hip_engine, c, ref, tag=f" gemm_bf3={mode}")
        if name == "tiny3-dsf8":
            out = T.run_charge_response(hip_engine, c)
            _ratio(f"{name} gemm_bf3={mode} dq", np.abs(out["dq"] - ref["t_q"].sum(-1)).max(), T.tangent_gate(ref["t_q"].sum(-1)))
    finally:
        hip_engine.set_option("gemm_bf3", before)


def test_cluster_rows_without_the_bounding_box_list(hip_engine, oracle64):
    """cluster1728 next to a second molecule of one hydrogen atom 60 A away: 1 729 atoms in 2 molecules are below the bounding-box
    list's threshold, the lists come from the other builder, and the cluster's rows meet the same fp64 reference."""
    c, far = T.case("cluster1728"), T.cluster_with_far_atom()
    n = len(c.numbers)
    assert T.bbox_applies(n, 1) and not T.bbox_applies(n + 1, 2)
    ref = T.reference(c, oracle64)
    out = T.run_hvp(hip_engine, far)
    _ratio("cluster1728 + H, cluster rows hv", np.abs(out["hv"][:, :n] - ref["hv"]).max(), T.hv_gate(ref))
    _ratio("cluster1728 + H, the lone atom's hv", np.abs(out["hv"][:, n:]).max(), 1e-5)
    assert_forces_close(out["forces"][:n], ref["forces"], "cluster1728 + H (forces of the sweep)")
