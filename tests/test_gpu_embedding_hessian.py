"""The electrostatic embedding in the analytic Hessian sweep (csrc/embed.hip: the field pass with the field-gradient tensor,
embed_tseed_kernel, embed_tsite_kernel; aimnet_engine_set_embedding_tangent) on the GPU against the fp64 yardstick of
tests/embedding_hessian_yardstick.py: Richardson-extrapolated central differences of the embedded fp64 forces, committed as
tests/golden/embedding_hessian.npz (tests/test_embedding_hessian_host.py holds them to the script that wrote them).  Every comparison
prints its ratio to the gate before it asserts; the ratios are recorded in profiles/embedding_hessian.md.

Gates (none is fitted to the engine): the field sums ROUND = 8 * 2^-24 times the sum of the absolute terms (the pattern of
tests/test_gpu_embedding.py; the tensor's sum is sum_A |k Q / d^3|); hv and ext_hv the tangent sweep's own 1e-5 + 3e-5 max|ref|
(tests/tangent_cases.py::hv_gate), on hv plus the rounding of the field sums carried through the seeds, per direction and atom
ROUND (|t_q_i| sum|k Q / d^2| + 2 |q_i| |v_i|_2 sum|k Q / d^3|) with the oracle's q and t_q (|3 r r^T / d^2 - 1|_2 = 2)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import embedding_hessian_yardstick as EH
import embedding_yardstick as Y
from conftest import FORCE_ATOL, FORCE_RTOL, golden
from test_gpu_embedding import ROUND, _args, _np64, _ratio, _same_bits, _t

pytestmark = pytest.mark.gpu


def _embedding(c, X=None, Q=None, ext_mol=None, **kw):
    X, Q = (c.X, c.Q) if X is None else (X, Q)
    e = dict(ext_coord=_t(X), ext_charge=_t(Q), **kw)
    if len(c.charge) > 1:
        e["ext_mol_idx"] = _t(c.ext_mol if ext_mol is None else ext_mol, torch.int32)
    return e


def _hvp(eng, c, V=None, embedding=None, **kw):
    return eng.hvp(*_args(eng, c.coord, c.numbers, c.charge, c.mol, c.mult), _t(c.V if V is None else V), coulomb="simple",
                   **({} if embedding is None else {"embedding": embedding}), **kw)


def _check_field(what, got, x, X, Q, mol=None, ext_mol=None):
    """ext_field [N, 10] against numpy fp64 phi, grad phi, T at ROUND times the absolute sums of the terms."""
    phi, g, abs_phi, abs_g = Y.field(x, X, Q, mol, ext_mol)
    T, abs_T = EH.tensor(x, X, Q, mol, ext_mol)
    got = _np64(got)
    _ratio(what + " phi", np.abs(got[:, 0] - phi), ROUND * abs_phi)
    _ratio(what + " grad phi", np.abs(got[:, 1:4] - g).max(-1), ROUND * abs_g)
    _ratio(what + " T", np.abs(got[:, 4:] - EH.six(T)).max(-1), ROUND * abs_T)


# ---- 1. the field sums alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 255, 256, 257, 1023, 1024, 1025, 3 * 1024 + 5])
def test_field_sums_against_numpy(hip_engine, M):
    """One block of 256 threads per (atom, slot) strides over chunks of EMBED_CHUNK = 1024 sites: the sizes around the block and
    around the chunk, and four slots of one chunk each."""
    c = EH.case("cold24")
    X, Q = Y.sites(c.coord, M)
    res = _hvp(hip_engine, c, np.zeros((1, 24, 3), np.float32), _embedding(c, X, Q, want_field=True, want_ext_hv=True))
    assert tuple(res["ext_field"].shape) == (24, 10) and res["ext_field"].dtype == torch.float64
    assert tuple(res["ext_hv"].shape) == (1, M, 3) and float(res["ext_hv"].abs().max()) == 0.0 and float(res["hv"].abs().max()) == 0.0
    _check_field(f"M={M}", res["ext_field"], c.coord, X, Q)


def _two_cold24():
    c = EH.case("cold24")
    coord = np.concatenate([c.coord, c.coord + np.array([60.0, 0.0, 0.0], np.float32)])
    from types import SimpleNamespace

    return SimpleNamespace(coord=coord, numbers=np.concatenate([c.numbers] * 2), charge=np.zeros(2, np.float32), mol=np.repeat(np.arange(2), 24),
                           mult=None, V=np.zeros((1, 48, 3), np.float32))


def test_field_sums_of_a_skewed_batch(hip_engine):
    """The batch of tests/test_gpu_embedding.py::test_sums_of_a_skewed_batch: 3 * 1024 + 5 sites on the first molecule and one on
    the second - two slots, a slot of the first molecule sums two chunks."""
    b = _two_cold24()
    X0, Q0 = Y.sites(b.coord[:24], 3 * 1024 + 5)
    X1, Q1 = Y.sites(b.coord[24:], 1, 9)
    X, Q, em = np.concatenate([X0, X1]), np.concatenate([Q0, Q1]), np.concatenate([np.zeros(len(Q0), np.int64), [1]])
    res = _hvp(hip_engine, b, embedding=_embedding(b, X, Q, em, want_field=True))
    _check_field("skewed batch", res["ext_field"], b.coord, X, Q, b.mol, em)


def test_field_of_a_molecule_without_sites_is_zero(hip_engine):
    b = _two_cold24()
    X, Q = Y.sites(b.coord[:24], 64)
    em = np.zeros(64, np.int64)
    res = _hvp(hip_engine, b, embedding=_embedding(b, X, Q, em, want_field=True))
    assert float(res["ext_field"][24:].abs().max()) == 0.0  # the rows of the molecule without sites: exactly zero
    _check_field("batch with a bare molecule", res["ext_field"][:24], b.coord[:24], X, Q)


# ---- 2. hv and ext_hv against the yardstick -----------------------------------------------------------------------------------
def _hv_gate(c, g):
    """[K, N]: hv_gate of the total plus the ROUND allowance of the field sums through q and t_q (module docstring)."""
    _, _, _, abs_g = Y.field(c.coord, c.X, c.Q, c.mol, c.ext_mol)
    _, abs_T = EH.tensor(c.coord, c.X, c.Q, c.mol, c.ext_mol)
    vn = np.linalg.norm(c.V.astype(np.float64), axis=-1)
    return EH.gate(g["hv"]) + ROUND * (np.abs(g["t_q"]) * abs_g[None] + 2.0 * np.abs(g["charges"])[None] * vn * abs_T[None])


@pytest.mark.parametrize("name", EH.GPU_CASES)
def test_hv_and_ext_hv_against_the_yardstick(hip_engine, hip_engine_nse, name):
    c, g = EH.case(name), EH.committed(name)
    eng = hip_engine_nse if c.nse else hip_engine
    res = _hvp(eng, c, embedding=_embedding(c, want_ext_hv=True))
    bare = _hvp(eng, c)
    moved = float((res["hv"] - bare["hv"]).abs().max())
    print(f"[embedding hessian] {name}: max|Hv| {np.abs(g['hv']).max():.3f}, max|Hv - H_bare v| {moved:.3f} eV/A^2")
    _ratio(name + " hv", np.abs(_np64(res["hv"]) - g["hv"]).max(-1), _hv_gate(c, g))
    assert tuple(res["ext_hv"].shape) == g["ext_hv"].shape
    _ratio(name + " ext_hv", np.abs(_np64(res["ext_hv"]) - g["ext_hv"]), EH.gate(g["ext_hv"]))
    assert moved > 100 * EH.gate(g["hv"])  # (the term is there at all)


# ---- 3. per-atom mode ---------------------------------------------------------------------------------------------------------
def test_per_atom_potential_equals_the_point_charges(hip_engine):
    c, g = EH.case("hvp40"), EH.committed("hvp40")
    pc = _hvp(hip_engine, c, embedding=_embedding(c))
    phi, grad, _, _ = Y.field(c.coord, c.X, c.Q)
    T, _ = EH.tensor(c.coord, c.X, c.Q)
    for hess in (EH.six(T), T):  # [N, 6] and [N, 3, 3]
        pa = _hvp(hip_engine, c, embedding=dict(potential=_t(phi), potential_grad=_t(grad), potential_hess=_t(hess)))
        _ratio("hvp40 per-atom against point-charge mode", np.abs(_np64(pa["hv"]) - _np64(pc["hv"])).max(-1), _hv_gate(c, g))
    with pytest.raises(ValueError, match="potential_hess"):
        _hvp(hip_engine, c, embedding=dict(potential=_t(phi), potential_grad=_t(grad)))


# ---- 4. uniform field -----------------------------------------------------------------------------------------------------------
def test_uniform_field(hip_engine):
    """phi = -E.x, grad phi = -E, potential_hess = 0: H v - H_bare v against the yardstick (differences of -(q g + J phi)), at the
    hv gate of the total."""
    c, g = EH.case("cold24"), EH.committed("cold24")
    E, x = EH.UNIFORM_E, c.coord.astype(np.float64)
    res = _hvp(hip_engine, c, embedding=dict(potential=_t(-(x @ E)), potential_grad=_t(np.tile(-E, (24, 1))), potential_hess=_t(np.zeros((24, 6)))))
    bare = _hvp(hip_engine, c)
    print(f"[embedding hessian] uniform field: max|dHv| {np.abs(g['uniform_dhv']).max():.4f} eV/A^2")
    _ratio("cold24 uniform field hv", np.abs(_np64(res["hv"]) - g["uniform_hv"]), EH.gate(g["uniform_hv"]))
    _ratio("cold24 uniform field hv - hv(bare)", np.abs(_np64(res["hv"]) - _np64(bare["hv"]) - g["uniform_dhv"]), EH.gate(g["uniform_hv"]))


# ---- 5. periodic branch ---------------------------------------------------------------------------------------------------------
def test_constant_potential_in_a_periodic_cell_changes_nothing(hip_engine):
    """A property of the seed path under DSF with a cell, not a parity point (there is no periodic Jacobian yardstick): the NSE
    normalisation keeps sum_j t_q_j = 0, so a constant phi with zero gradient and Hessian leaves H v where it was."""
    g = golden("pbc96_dsf8_wrapped")
    n = 96
    kw = dict(cell=_t(g["cell"]), coulomb="dsf", dsf_rc=float(g["dsf_rc"]), dsf_alpha=float(g["dsf_alpha"]))
    args = _args(hip_engine, g["coord"], g["numbers"], [0.0], np.zeros(n, np.int64))
    V = _t(EH.directions(n))
    e = dict(potential=_t(np.full(n, 0.37)), potential_grad=_t(np.zeros((n, 3))), potential_hess=_t(np.zeros((n, 6))))
    res = hip_engine.hvp(*args, V, embedding=e, **kw)
    bare = hip_engine.hvp(*args, V, **kw)
    _ratio("pbc96 constant potential", np.abs(_np64(res["hv"]) - _np64(bare["hv"])), EH.gate(_np64(bare["hv"])))


# ---- 6. contract ----------------------------------------------------------------------------------------------------------------
def test_contract(hip_engine, monkeypatch):
    from aimnetcentral_amd import _lib, capacity, loader
    from aimnetcentral_amd.engine import HipEngine

    c = EH.case("cold24")
    n, K = 24, 3
    X, Q = Y.sites(c.coord, 3 * 1024 + 5)
    emb = _embedding(c, X, Q, want_ext_hv=True, want_field=True)
    args = _args(hip_engine, c.coord, c.numbers, c.charge, c.mol)
    e_eval = dict(ext_coord=_t(X), ext_charge=_t(Q), want_ext_forces=True)
    ev = hip_engine.eval(*args, forces=True, coulomb="simple", embedding=e_eval)
    a = _hvp(hip_engine, c, embedding=emb, want_forces=True)
    assert set(a) == {"hv", "forces", "ext_hv", "ext_field"}
    assert _same_bits(a, _hvp(hip_engine, c, embedding=emb, want_forces=True))
    # the workspace (the allocator hands the block of the same size out again) and both scratches filled with 0xFF
    rq = capacity.Request("hvp", n, 1, False, _lib.COULOMB_SIMPLE, 15.0, 0.2, 1e-6, None)
    opt = hip_engine.fill_options(rq)
    nbytes = int(hip_engine.lib.aimnet_engine_hvp_workspace_bytes(hip_engine._h, n, 1, K, C.byref(opt))) + 4096
    junk = torch.empty(nbytes, dtype=torch.uint8, device="cuda").fill_(0xFF)
    del junk
    hip_engine._emb_scratch.fill_(0xFF)
    hip_engine._emb_tangent_scratch.fill_(0xFF)
    assert _same_bits(a, _hvp(hip_engine, c, embedding=emb, want_forces=True))
    # K directions at once = one at a time; a forced split into sweeps of one direction: the same bits, ext_hv included
    for k in range(K):
        one = _hvp(hip_engine, c, c.V[k:k + 1], embedding=emb)
        assert torch.equal(one["hv"][0], a["hv"][k]) and torch.equal(one["ext_hv"][0], a["ext_hv"][k])
        assert torch.equal(one["ext_field"], a["ext_field"])
    monkeypatch.setattr(hip_engine, "HVP_BYTES_BUDGET", 1)
    assert _same_bits(a, _hvp(hip_engine, c, embedding=emb, want_forces=True))
    monkeypatch.undo()
    # the forces of the sweep are the embedded forces of eval
    _ratio("cold24 forces of the sweep against eval", np.abs(_np64(a["forces"]) - _np64(ev["forces"])),
           FORCE_ATOL + FORCE_RTOL * float(ev["forces"].abs().max()))
    # disarmed again: hvp computes what a fresh engine computes, eval with the embedding what it computed before
    after = _hvp(hip_engine, c, want_forces=True)
    fresh = _hvp(HipEngine(loader.synthetic_spec(0), "cuda:0"), c, want_forces=True)
    assert _same_bits(after, fresh) and set(after) == {"hv", "forces"}
    assert _same_bits(ev, hip_engine.eval(*args, forces=True, coulomb="simple", embedding=e_eval))
    # armed with sites plus a cell: refused by the C checks (HipEngine.hvp's own check comes first, so the structs are set by hand)
    with pytest.raises(ValueError, match="non-periodic"):
        _hvp(hip_engine, c, embedding=emb, cell=_t(np.eye(3) * 40.0))
    xc, qc = _t(X), _t(Q)
    s = _lib.Embedding(n_ext=len(Q), ext_coord=xc.data_ptr(), ext_charge=qc.data_ptr(), scratch=hip_engine._emb_scratch.data_ptr(),
                       scratch_bytes=hip_engine._emb_scratch.numel())
    ts = _lib.EmbeddingTangent(scratch=hip_engine._emb_tangent_scratch.data_ptr(), scratch_bytes=hip_engine._emb_tangent_scratch.numel())
    assert hip_engine.lib.aimnet_engine_set_embedding_tangent(hip_engine._h, C.byref(ts)) == _lib.E_INVALID  # no embedding set
    assert hip_engine.lib.aimnet_engine_set_embedding(hip_engine._h, C.byref(s)) == 0
    try:
        assert hip_engine.lib.aimnet_engine_set_embedding_tangent(hip_engine._h, C.byref(ts)) == 0
        with pytest.raises(_lib.HipLibraryError, match="non-periodic"):
            hip_engine.hvp(*args, _t(c.V), cell=_t(np.eye(3) * 40.0), coulomb="dsf", dsf_rc=8.0)
        ts.scratch_bytes = 16
        assert hip_engine.lib.aimnet_engine_set_embedding_tangent(hip_engine._h, C.byref(ts)) == 0
        with pytest.raises(_lib.HipLibraryError, match="scratch"):
            hip_engine.hvp(*args, _t(c.V))
        assert hip_engine.lib.aimnet_engine_set_embedding_tangent(hip_engine._h, None) == 0  # disarmed: refused as before
        with pytest.raises(_lib.HipLibraryError, match="not carried by the tangent sweep"):
            hip_engine.hvp(*args, _t(c.V))
    finally:
        assert hip_engine.lib.aimnet_engine_set_embedding(hip_engine._h, None) == 0
    assert torch.equal(_hvp(hip_engine, c)["hv"], fresh["hv"])


# ---- 7. through the calculator ----------------------------------------------------------------------------------------------------
def test_through_the_calculator(hip_engine):
    from aimnetcentral_amd import AIMNet2Calculator, loader, vibrations

    c = EH.case("cold24")
    n, M = 24, len(c.Q)
    calc = AIMNet2Calculator(loader.synthetic_spec(0), device="cuda:0")
    data = {"coord": c.coord, "numbers": c.numbers, "charge": 0.0, "ext_coord": c.X, "ext_charge": c.Q}
    with pytest.raises(NotImplementedError):
        calc(data, hessian=True)
    calc.set_embedding_hessian("fixed_sites", mixed_block=True)
    out = calc(data, forces=True, hessian=True)
    eye = np.eye(3 * n, dtype=np.float32).reshape(3 * n, n, 3)
    want = hip_engine.hvp(*_args(hip_engine, c.coord, c.numbers, c.charge, c.mol), _t(eye), coulomb=calc.coulomb_method or "none",
                          embedding=_embedding(c, want_ext_hv=True))
    H = want["hv"].view(3 * n, 3 * n)
    assert torch.equal(out["hessian"].reshape(3 * n, 3 * n), 0.5 * (H + H.T))
    assert tuple(out["ext_hessian"].shape) == (M, 3, n, 3)
    assert torch.equal(out["ext_hessian"], want["ext_hv"].view(n, 3, M, 3).permute(2, 3, 0, 1))
    _ratio("cold24 dense embedded Hessian: |H - H^T|", np.abs(_np64(H) - _np64(H).T), EH.gate(_np64(H)))
    ev = hip_engine.eval(*_args(hip_engine, c.coord, c.numbers, c.charge, c.mol), forces=True, coulomb=calc.coulomb_method or "none",
                         embedding=dict(ext_coord=_t(c.X), ext_charge=_t(c.Q), want_ext_forces=True))
    assert torch.equal(out["forces"], ev["forces"]) and torch.equal(out["energy"], ev["energy"])
    hv = calc.hessian_vector_product(data, c.V)
    assert torch.equal(hv, _hvp(hip_engine, c, embedding=_embedding(c))["hv"]) or calc.coulomb_method not in (None, "simple")
    masses = np.where(np.asarray(c.numbers) == 1, 1.008, 12.011)
    nu, modes = vibrations.normal_modes(out["hessian"].cpu().numpy(), masses)
    assert nu.shape == (3 * n,) and np.isfinite(nu).all() and modes.shape == (3 * n, 3 * n)
