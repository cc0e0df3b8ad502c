"""Host side of the electrostatic embedding in the analytic Hessian sweep (no GPU): the yardstick of
tests/test_gpu_embedding_hessian.py (tests/embedding_hessian_yardstick.py) held to itself - Richardson agreement, symmetry, and that
every closed-form addend of the sweep's seeds matters at the gates -, the calculator's set_embedding_hessian against a recording
fake engine, the checks of csrc/tangent_plan.h with the new field through a stand-alone program, and the C entry points."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import embedding_hessian_yardstick as EH
from conftest import ROOT
from fake_engine import WATER, FakeEngine, fake_calculator
from test_chain_prefetch_plan import _host_compiler

SITES = dict(ext_coord=[[3.0, 0.0, 0.0], [0.0, 4.0, 0.0]], ext_charge=[0.4, -0.4])


def _model(c, oracle64, oracle64_nse):
    return oracle64_nse if c.nse else oracle64


# ---- (a) Richardson agreement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cold24", "batch5_mol0", "nse_b5_mol3"])
def test_richardson_extrapolants_agree(oracle64, oracle64_nse, name):
    """`yardstick` asserts |R(h, h/2) - R(h/2, h/4)| <= 1 % of the gate, on hv and on ext_hv.  Measured, first direction of each
    case: cold24 1.9e-7 (gate 4.8e-4) / 9.3e-10 (1.4e-5); batch5_mol0 1.8e-6 (1.5e-3) / 2.3e-9 (2.6e-5); nse_b5_mol3 3.7e-7
    (1.6e-3) / 1.9e-9 (2.8e-5).  cold24 is also held to the committed yardstick of the GPU tests (same inputs, same numbers)."""
    c = EH.case(name)
    y = EH.yardstick(c, _model(c, oracle64, oracle64_nse), c.V[:1])
    assert np.isfinite(y["hv"]).all() and np.abs(y["ext_hv"]).max() > 0
    if name in EH.GPU_CASES:
        g = EH.committed(name)
        assert np.abs(g["hv"][0] - y["hv"][0]).max() <= 1e-9 * np.abs(y["hv"]).max()
        assert np.abs(g["ext_hv"][0] - y["ext_hv"][0]).max() <= 1e-9 * np.abs(y["ext_hv"]).max()


def test_committed_yardsticks_passed_their_own_check():
    for name in EH.GPU_CASES:
        g = EH.committed(name)
        print(f"[embedding hessian] {name}: committed agreement hv {float(g['agree_hv']):.3e} (gate {EH.gate(g['hv']):.3e}), ext_hv "
              f"{float(g['agree_ext']):.3e} (gate {EH.gate(g['ext_hv']):.3e})")
        assert g["agree_hv"] <= EH.RICHARDSON_FRACTION * EH.gate(g["hv"])
        assert g["agree_ext"] <= EH.RICHARDSON_FRACTION * EH.gate(g["ext_hv"])
    g = EH.committed("cold24")
    assert g["uniform_agree_hv"] <= EH.RICHARDSON_FRACTION * EH.gate(g["uniform_hv"])
    assert g["uniform_agree_dhv"] <= EH.RICHARDSON_FRACTION * EH.gate(g["uniform_dhv"])


# ---- (b) symmetry ------------------------------------------------------------------------------------------------------------------
def test_dense_yardstick_hessian_is_symmetric(oracle64):
    """The 3n unit directions of the smallest molecule of batch5 (11 atoms): H = H^T to 1 % of the gate, and the mixed block is the
    derivative of the atom forces with respect to the sites (one site coordinate, by a central difference of the yardstick forces)."""
    c = EH.case("batch5_mol0")
    n = len(c.numbers)
    y = EH.yardstick(c, oracle64, np.eye(3 * n, dtype=np.float32).reshape(3 * n, n, 3))
    H = y["hv"].reshape(3 * n, 3 * n)
    asym = np.abs(H - H.T).max()
    print(f"[embedding hessian] batch5_mol0 dense: max|H - H^T| = {asym:.3e}, gate {EH.gate(H):.3e}")
    assert asym <= EH.RICHARDSON_FRACTION * EH.gate(H)
    # ext_hv[(i, c), A, a] = d2E / dX_Aa dx_ic: against -dF_ic / dX_Aa from displaced sites (fp64 throughout, h = 1e-4 A)
    import embedding_yardstick as Y

    ref = EH.model_at(c, oracle64, c.coord)
    A, a, h = 7, 1, 1e-4
    f = []
    for s in (+1, -1):
        X = c.X.astype(np.float64).copy()
        X[A, a] += s * h
        f.append(Y.embedded_reference(ref, c.coord.astype(np.float64), X, c.Q)["forces"])
    fd = -(f[0] - f[1]).reshape(3 * n) / (2 * h)
    assert np.abs(fd - y["ext_hv"][:, A, a]).max() <= 1e-6 * max(1.0, np.abs(fd).max())


# ---- (c) sensitivity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EH.GPU_CASES)
def test_every_closed_form_addend_matters(oracle64, oracle64_nse, name):
    """Dropping t_q g, q T v or J t_phi moves H v by at least 10 gates on every fixture of the GPU tests, with the sites of
    embedding_yardstick.sites as they are (2.5 - 8 A outside the molecule): none had to be brought closer.  Measured (max|addend| in
    gates): profiles/embedding_hessian.md."""
    c = EH.case(name)
    g = EH.committed(name)
    a = EH.addends(c, EH.model_at(c, _model(c, oracle64, oracle64_nse), c.coord))
    gate = EH.gate(g["hv"])
    assert np.abs(a["t_q"] - g["t_q"]).max() <= 1e-9
    for k in ("tq_g", "q_Tv", "J_tphi"):
        moved = np.abs(a[k]).max()
        print(f"[embedding hessian] {name}: without {k} H v moves by {moved:.4f} eV/A^2 = {moved / gate:.1f} gates ({gate:.2e})")
        assert moved >= 10 * gate, (name, k, moved / gate)
    T = a["T"]
    assert np.abs(np.trace(T, axis1=1, axis2=2)).max() <= 1e-12 * a["abs_T"].max()  # point charges: the trace vanishes


# ---- (d) the calculator against a recording fake engine -------------------------------------------------------------------------
class RecordingEngine(FakeEngine):
    def eval(self, *args, embedding=None, **kw):
        out = super().eval(*args, **kw)
        self.calls[-1]["embedding"] = embedding
        if embedding is not None:
            out["embedding_energy"] = torch.zeros(1, dtype=torch.float64)
            if embedding.get("want_ext_forces"):
                out["ext_forces"] = torch.zeros(embedding["ext_coord"].shape[0], 3)
        return out

    def hvp(self, *args, embedding=None, **kw):
        out = super().hvp(*args, **kw)
        self.hvp_calls[-1]["embedding"] = embedding
        if embedding is not None and embedding.get("want_ext_hv"):
            K, M = self.hvp_calls[-1]["K"], embedding["ext_coord"].shape[0]
            out["ext_hv"] = torch.arange(K * M * 3, dtype=torch.float32).view(K, M, 3)
        return out


@pytest.fixture()
def calc(monkeypatch):
    return fake_calculator(monkeypatch, RecordingEngine)


def test_default_mode_refuses_before_the_engine(calc):
    v = np.zeros((3, 3), np.float32)
    with pytest.raises(NotImplementedError, match="not carried by the tangent sweep"):
        calc.hessian_vector_product(dict(WATER, **SITES), v)
    with pytest.raises(NotImplementedError, match="energies and forces only"):
        calc(dict(WATER, **SITES), hessian=True)
    calc.set_embedding_hessian("fixed_sites")
    calc.set_embedding_hessian(None)  # back to the default
    with pytest.raises(NotImplementedError):
        calc.hessian_vector_product(dict(WATER, **SITES), v)
    with pytest.raises(ValueError, match="fixed_sites"):
        calc.set_embedding_hessian("moving_sites")
    assert calc.engine.calls == [] and calc.engine.hvp_calls == []


def test_fixed_sites_forwards_the_embedding(calc):
    calc.set_embedding_hessian("fixed_sites")
    v = np.zeros((2, 3, 3), np.float32)
    hv = calc.hessian_vector_product(dict(WATER, **SITES), v)
    emb = calc.engine.hvp_calls[-1]["embedding"]
    assert tuple(hv.shape) == (2, 3, 3) and set(emb) == {"ext_coord", "ext_charge"}
    assert emb["ext_coord"].dtype == torch.float32 and tuple(emb["ext_coord"].shape) == (2, 3) and tuple(emb["ext_charge"].shape) == (2,)
    # a per-atom potential: (N, 3, 3) or (N, 6) Hessians go through as they are given
    pot = dict(ext_potential=[0.1, 0.2, 0.3], ext_potential_grad=np.zeros((3, 3)))
    for ph in (np.zeros((3, 3, 3)), np.zeros((3, 6))):
        calc.hessian_vector_product(dict(WATER, **pot, ext_potential_hess=ph), v)
        emb = calc.engine.hvp_calls[-1]["embedding"]
        assert set(emb) == {"potential", "potential_grad", "potential_hess"} and tuple(emb["potential_hess"].shape) == ph.shape
        assert emb["potential_hess"].dtype == torch.float32 and tuple(emb["potential"].shape) == (3,)
    # without the keys nothing is passed
    calc.hessian_vector_product(WATER, v)
    assert calc.engine.hvp_calls[-1]["embedding"] is None
    # the dense Hessian: energy and forces of the same call take the term too; the mixed block only when it is asked for
    out = calc(dict(WATER, **SITES), forces=True, hessian=True)
    assert set(calc.engine.calls[-1]["embedding"]) == {"ext_coord", "ext_charge", "want_ext_forces"}
    assert calc.engine.hvp_calls[-1]["K"] == 9 and "want_ext_hv" not in calc.engine.hvp_calls[-1]["embedding"]
    assert tuple(out["hessian"].shape) == (3, 3, 3, 3) and "ext_hessian" not in out and "embedding_energy" in out
    calc.set_embedding_hessian("fixed_sites", mixed_block=True)
    out = calc(dict(WATER, **SITES), hessian=True)
    assert calc.engine.hvp_calls[-1]["embedding"]["want_ext_hv"] is True and "forces" not in out
    xh = out["ext_hessian"]  # (M, 3, N, 3) from ext_hv [(i, c)][A][a]
    assert tuple(xh.shape) == (2, 3, 3, 3)
    ext_hv = torch.arange(9 * 2 * 3, dtype=torch.float32).view(3, 3, 2, 3)
    assert all(float(xh[A, a, i, c]) == float(ext_hv[i, c, A, a]) for A in range(2) for a in range(3) for i in range(3) for c in range(3))
    # a batch of one in the (1, N, 3) layout
    calc.hessian_vector_product(dict(coord=[WATER["coord"]], numbers=[WATER["numbers"]], charge=[0.0], ext_coord=[SITES["ext_coord"]],
                                     ext_charge=[SITES["ext_charge"]]), v)
    assert tuple(calc.engine.hvp_calls[-1]["embedding"]["ext_coord"].shape) == (2, 3)


@pytest.mark.parametrize("extra,exc,match", [
    (dict(ext_potential=[0.1, 0.2, 0.3], ext_potential_grad=np.zeros((3, 3))), ValueError, "ext_potential_hess"),
    (dict(ext_potential=[0.1, 0.2, 0.3], ext_potential_hess=np.zeros((3, 6))), ValueError, "ext_potential_grad"),
    (dict(ext_potential=[0.1, 0.2, 0.3], ext_potential_grad=np.zeros((3, 3)), ext_potential_hess=np.zeros((3, 5))), ValueError, "shape"),
    (dict(SITES, ext_potential_hess=np.zeros((3, 6))), ValueError, "without ext_potential"),
    (dict(ext_coord=SITES["ext_coord"]), ValueError, "together"),
    (dict(SITES, cell=np.eye(3) * 20.0), ValueError, "non-periodic"),
])
def test_fixed_sites_rejections_come_before_the_engine(calc, extra, exc, match):
    calc.set_embedding_hessian("fixed_sites", mixed_block=True)
    with pytest.raises(exc, match=match):
        calc.hessian_vector_product(dict(WATER, **extra), np.zeros((3, 3), np.float32))
    with pytest.raises(exc, match=match):
        calc(dict(WATER, **extra), hessian=True)
    assert calc.engine.calls == [] and calc.engine.hvp_calls == []


def test_what_is_not_carried_still_raises(calc):
    calc.set_embedding_hessian("fixed_sites")
    v = np.zeros((3, 3), np.float32)
    data = dict(WATER, **SITES)
    pot = dict(WATER, ext_potential=[0.1, 0.2, 0.3], ext_potential_grad=np.zeros((3, 3)), ext_potential_hess=np.zeros((3, 6)),
               cell=np.eye(3) * 20.0)
    calc.hvp_method = "fd"  # differences of forces
    with pytest.raises(NotImplementedError, match="not carried by the tangent sweep"):
        calc.hessian_vector_product(data, v)
    with pytest.raises(NotImplementedError, match="energies and forces only"):
        calc(data, hessian=True)
    calc.hvp_method = "analytic"
    calc._coulomb_method = "pme"  # particle-mesh Ewald
    with pytest.raises(NotImplementedError, match="not carried by the tangent sweep"):
        calc.hessian_vector_product(pot, v)
    with pytest.raises(NotImplementedError, match="energies and forces only"):
        calc(pot, hessian=True)
    calc._coulomb_method = "simple"
    with pytest.raises(NotImplementedError, match="energies and forces only"):  # stress
        calc(pot, stress=True)
    with pytest.raises(NotImplementedError, match="energies and forces only"):
        calc(pot, stress=True, hessian=True)
    calc._dd = object()  # domain decomposition
    with pytest.raises(NotImplementedError):
        calc.hessian_vector_product(pot, v)
    with pytest.raises(NotImplementedError):
        calc(pot, hessian=True)
    calc._dd = None
    # more than one structure
    two = dict(coord=np.concatenate([WATER["coord"]] * 2), numbers=[8, 1, 1] * 2, charge=[0.0, 0.0], mol_idx=[0, 0, 0, 1, 1, 1], **SITES,
               ext_mol_idx=[0, 1])
    with pytest.raises(NotImplementedError, match="single structure"):
        calc(two, hessian=True)
    assert calc.engine.calls == [] and calc.engine.hvp_calls == []


def test_ase_adapter_hands_the_sites_to_the_hessian(calc):
    from aimnetcentral_amd.aimnet2ase import AIMNet2ASE

    class Atoms:
        def __init__(self):
            self.numbers, self.positions, self.cell = np.array([8, 1, 1]), np.array(WATER["coord"], dtype=float), None
            self.pbc, self.info = np.zeros(3, bool), {}

    ase_calc = AIMNet2ASE(calc, charge=0)
    atoms = Atoms()
    pc = ase_calc.embed(charges=[0.4, -0.4])
    pc.set_positions(np.array(SITES["ext_coord"]))
    H = ase_calc.get_hessian(atoms)  # the mode is not set: the bare Hessian, as before
    assert H.shape == (9, 9) and calc.engine.hvp_calls[-1]["embedding"] is None
    calc.set_embedding_hessian("fixed_sites")
    H = ase_calc.get_hessian(atoms)
    emb = calc.engine.hvp_calls[-1]["embedding"]
    assert H.shape == (9, 9) and tuple(emb["ext_coord"].shape) == (2, 3) and emb["ext_charge"].tolist() == pytest.approx([0.4, -0.4])
    ase_calc.embed()
    ase_calc.get_hessian(atoms)
    assert calc.engine.hvp_calls[-1]["embedding"] is None


# ---- (e) tangent_validate with the new field ----------------------------------------------------------------------------------------
def test_tangent_plan_with_an_armed_embedding(tmp_path):
    exe = str(tmp_path / "embedding_tangent_plan")
    base = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
            "-I", os.path.join(ROOT, "aimnetcentral_amd", "csrc"), os.path.join(ROOT, "tests", "embedding_tangent_plan_main.cpp"), "-o", exe]
    cxx = _host_compiler()  # (static sanitizer runtimes: see tests/test_chain_prefetch_plan.py)
    r = subprocess.run([cxx, "-static-libasan", "-static-libubsan", *base], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run([cxx, *base], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "embedding tangent plan ok" in r.stdout


# ---- the C entry points ----------------------------------------------------------------------------------------------------------
def test_entry_points_and_struct_mirror():
    from aimnetcentral_amd import _lib

    lib = _lib.load()
    assert {"aimnet_embedding_tangent_scratch_bytes", "aimnet_engine_set_embedding_tangent"} <= set(_lib.EXPORTED_SYMBOLS)
    assert lib.aimnet_abi_version() == 12
    assert [f[0] for f in _lib.EmbeddingTangent._fields_] == ["potential_hess", "ext_hv", "field", "scratch", "scratch_bytes"]
    assert C.sizeof(_lib.EmbeddingTangent) == 5 * 8
    assert C.sizeof(_lib.Embedding) == 8 + 8 * 8 + 8 + 8  # aimnet_embedding keeps its layout
    t = _lib.EmbeddingTangent()
    assert lib.aimnet_engine_set_embedding_tangent(None, None) == _lib.E_INVALID
    assert lib.aimnet_engine_set_embedding_tangent(None, C.byref(t)) == _lib.E_INVALID
    for bad in ((0, 1, 10), (10, 0, 10), (10, 1, -1)):
        assert lib.aimnet_embedding_tangent_scratch_bytes(*bad) == 0
    M = 3 * _lib.EMBED_CHUNK + 5
    small, big = lib.aimnet_embedding_tangent_scratch_bytes(10, 1, 0), lib.aimnet_embedding_tangent_scratch_bytes(10, 1, M)
    assert 0 < small < big and big - small >= 10 * 4 * 10 * 8 + M * 4  # ten doubles per (atom, slot) on top of the site index copy
    assert big > lib.aimnet_embedding_scratch_bytes(10, 1, M)  # (four there)
