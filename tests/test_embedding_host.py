"""Host side of the electrostatic embedding (no GPU): that the yardstick of tests/test_gpu_embedding.py IS the gradient of
sum_i q_i phi_i with the oracle's charges; the calculator's handling of the embedding keys against a recording fake engine (as
tests/test_host_logic.py does for the rest of its inputs); and the null-handle contract of the two C entry points."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import embedding_yardstick as Y
from conftest import golden

from aimnetcentral_amd import calculator as calc_mod
from aimnetcentral_amd import loader


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hvp40", "cold24"])
def test_yardstick_is_the_gradient_of_q_phi(oracle64, name):
    """Central difference of sum_i q_i(x) phi(x_i) at h = 1e-3 A along one random direction v against -F_emb . v; gate
    1e-3 |F_emb|_2 |v|_2 (the floor is the oracle's fp32 cast of the displaced coordinates).  Measured with v from
    default_rng(11): hvp40 fd -1.291441 / yardstick -1.291656 (gate 1.5e-2), cold24 -1.153372 / -1.153482 (gate 6.2e-3) eV/A.  The
    direct term q g alone (no charge response) gives +0.017 / +0.043: it misses by the whole (J phi) . v."""
    from oracle import aimnet2_oracle as O

    g = golden(name)
    coord, numbers, n = g["coord"], g["numbers"], len(g["numbers"])
    mol = np.zeros(n, np.int64)
    X, Q = Y.sites(coord)
    ref = Y.model_reference(oracle64, name, coord, numbers, 0.0, mol)
    emb = Y.embedded_reference(ref, coord, X, Q)
    v = np.random.default_rng(11).standard_normal((n, 3))
    x, h = np.asarray(coord, np.float64), 1e-3

    def e_emb(xd):
        q = np.asarray(O.evaluate(oracle64, xd, numbers, 0.0, mol, forces=False)["charges"], np.float64)
        return float((q * Y.field(np.asarray(xd, np.float32), X, Q)[0]).sum())

    fd = (e_emb(x + h * v) - e_emb(x - h * v)) / (2 * h)
    an = -(emb["f_emb"] * v).sum()
    direct = (ref["charges"][:, None] * emb["g"] * v).sum()
    gate = 1e-3 * np.linalg.norm(emb["f_emb"]) * np.linalg.norm(v)
    dmin = np.linalg.norm(np.asarray(coord, np.float64)[:, None] - X[None].astype(np.float64), axis=-1).min()
    print(f"[embedding] {name}: fd {fd:.6f}, yardstick {an:.6f}, direct term alone {direct:.6f}, gate {gate:.2e}; E_emb "
          f"{emb['e_emb'][0]:.3f} eV, max|F_emb| {np.abs(emb['f_emb']).max():.3f}, max|J phi| "
          f"{np.abs(emb['f_emb'] + ref['charges'][:, None] * emb['g']).max():.3f}, max|q g| "
          f"{np.abs(ref['charges'][:, None] * emb['g']).max():.3f} eV/A, closest site {dmin:.2f} A")
    assert abs(an - fd) <= gate
    assert abs(direct - fd) > gate


def test_site_force_is_minus_the_gradient_with_respect_to_the_site():
    """ext_forces = -dE_emb/dX_A at fixed q: a central difference of sum_i q_i phi_i in the site coordinate (numpy, fp64)."""
    rng = np.random.default_rng(3)
    x, q = rng.standard_normal((7, 3)), rng.uniform(-0.5, 0.5, 7)
    X, Q = 4.0 + rng.standard_normal((3, 3)), np.array([0.7, -0.4, 0.2])
    _, f, _, _ = Y.site_terms(x, q, X, Q)
    h = 1e-5
    for a in range(3):
        for c in range(3):
            Xp, Xm = X.copy(), X.copy()
            Xp[a, c] += h
            Xm[a, c] -= h
            fd = ((q * Y.field(x, Xp, Q)[0]).sum() - (q * Y.field(x, Xm, Q)[0]).sum()) / (2 * h)
            assert abs(-fd - f[a, c]) <= 1e-7 * (1.0 + abs(fd))
    # a positive site pushes a positive atom away: the force on the site points from the atom to the site
    _, f1, _, _ = Y.site_terms(np.zeros((1, 3)), [1.0], [[2.0, 0.0, 0.0]], [1.0])
    assert f1[0, 0] > 0 and abs(f1[0, 0] - Y.KE / 4.0) < 1e-12


# ---- the calculator against a recording fake engine ---------------------------------------------------------------------------
class FakeEngine:
    def __init__(self, spec, device):
        self.spec, self.device, self.calls, self.nq = spec, torch.device("cpu"), [], 1

    def set_dftd3_tables(self, tables):
        pass

    def eval(self, coord, numbers, mol_idx, charge, cell=None, forces=False, stress=False, **kw):
        self.calls.append(dict(kw, n=coord.shape[0], n_mol=charge.shape[0], forces=forces))
        n, emb = coord.shape[0], kw.get("embedding")
        out = {"energy": torch.arange(charge.shape[0], dtype=torch.float64), "charges": torch.arange(n, dtype=torch.float32) + 1}
        if forces:
            out["forces"] = torch.ones(n, 3)
        if emb is not None:
            out["embedding_energy"] = torch.full((charge.shape[0],), 7.0, dtype=torch.float64)
            if emb.get("want_ext_forces"):
                out["ext_forces"] = torch.arange(emb["ext_coord"].shape[0] * 3, dtype=torch.float32).view(-1, 3)
        return out


@pytest.fixture()
def calc(monkeypatch):
    orig = torch.as_tensor
    monkeypatch.setattr(calc_mod, "HipEngine", FakeEngine)
    monkeypatch.setattr(torch, "as_tensor", lambda data, dtype=None, device=None: orig(data, dtype=dtype, device="cpu"))
    c = calc_mod.AIMNet2Calculator(loader.synthetic_spec(0), device="cuda")
    c.device = "cpu"
    return c


WATER = dict(coord=[[0.0, 0.0, 0.1173], [0.0, 0.7572, -0.4692], [0.0, -0.7572, -0.4692]], numbers=[8, 1, 1], charge=0.0)
SITES = dict(ext_coord=[[3.0, 0.0, 0.0], [0.0, 4.0, 0.0]], ext_charge=[0.4, -0.4])


def test_keyword_appears_only_with_embedding_keys(calc):
    out = calc(WATER, forces=True)
    assert "embedding" not in calc.engine.calls[-1] and set(out) == {"energy", "charges", "forces"}
    out = calc(dict(WATER, ext_coord=None, ext_charge=None), forces=True)
    assert "embedding" not in calc.engine.calls[-1]
    out = calc(dict(WATER, **SITES), forces=True)
    emb = calc.engine.calls[-1]["embedding"]
    assert set(emb) == {"ext_coord", "ext_charge", "want_ext_forces"} and emb["want_ext_forces"] is True
    assert emb["ext_coord"].dtype == torch.float32 and tuple(emb["ext_coord"].shape) == (2, 3) and tuple(emb["ext_charge"].shape) == (2,)
    assert set(out) == {"energy", "charges", "forces", "embedding_energy", "ext_forces"} and tuple(out["ext_forces"].shape) == (2, 3)
    out = calc(dict(WATER, **SITES))
    assert calc.engine.calls[-1]["embedding"]["want_ext_forces"] is False and "ext_forces" not in out and "embedding_energy" in out
    out = calc(dict(WATER, ext_potential=[0.1, 0.2, 0.3], ext_potential_grad=np.zeros((3, 3))), forces=True)
    emb = calc.engine.calls[-1]["embedding"]
    assert set(emb) == {"potential", "potential_grad"} and tuple(emb["potential_grad"].shape) == (3, 3)
    assert "ext_forces" not in out and float(out["embedding_energy"][0]) == 7.0


def test_flat_batch_needs_and_passes_ext_mol_idx(calc):
    d = dict(coord=np.concatenate([WATER["coord"]] * 2), numbers=[8, 1, 1] * 2, charge=[0.0, 0.0], mol_idx=[0, 0, 0, 1, 1, 1], **SITES)
    with pytest.raises(ValueError, match="ext_mol_idx"):
        calc(d)
    calc(dict(d, ext_mol_idx=[0, 1]), forces=True)
    emb = calc.engine.calls[-1]["embedding"]
    assert emb["ext_mol_idx"].dtype == torch.int32 and emb["ext_mol_idx"].tolist() == [0, 1]


def test_dense_batch_flattens_with_a_repeated_molecule_index(calc):
    coord = np.zeros((2, 4, 3), np.float32)
    coord[:, :3] = WATER["coord"]
    numbers = np.array([[8, 1, 1, 0], [8, 1, 1, 1]])
    xc = np.arange(2 * 3 * 3, dtype=np.float32).reshape(2, 3, 3) + 5.0
    qc = np.array([[0.1, 0.2, 0.0], [0.3, 0.0, 0.0]], np.float32)  # zero charges pad the shorter lists
    pot = np.arange(8, dtype=np.float32).reshape(2, 4)
    out = calc(dict(coord=coord, numbers=numbers, charge=[0.0, 0.0], ext_coord=xc, ext_charge=qc, ext_potential=pot,
                    ext_potential_grad=np.ones((2, 4, 3), np.float32)), forces=True, validate_species=False)
    call = calc.engine.calls[-1]
    emb = call["embedding"]
    assert call["n"] == 7 and call["n_mol"] == 2
    assert emb["ext_mol_idx"].tolist() == [0, 0, 0, 1, 1, 1] and emb["ext_mol_idx"].dtype == torch.int32
    assert torch.equal(emb["ext_coord"], torch.from_numpy(xc.reshape(6, 3))) and torch.equal(emb["ext_charge"], torch.from_numpy(qc.reshape(6)))
    assert emb["potential"].tolist() == [0.0, 1.0, 2.0, 4.0, 5.0, 6.0, 7.0] and tuple(emb["potential_grad"].shape) == (7, 3)
    assert tuple(out["ext_forces"].shape) == (2, 3, 3) and tuple(out["embedding_energy"].shape) == (2,)
    assert torch.equal(out["ext_forces"].reshape(-1), torch.arange(18, dtype=torch.float32))


@pytest.mark.parametrize("extra,kw,exc", [
    (SITES, dict(stress=True), (NotImplementedError, ValueError)),
    (SITES, dict(hessian=True), (NotImplementedError, ValueError)),
    (dict(ext_coord=SITES["ext_coord"]), {}, ValueError),
    (dict(ext_charge=SITES["ext_charge"]), {}, ValueError),
    (dict(ext_coord=[[1.0, 2.0]], ext_charge=[0.1]), {}, ValueError),
    (dict(ext_coord=SITES["ext_coord"], ext_charge=[0.1]), {}, ValueError),
    (dict(SITES, ext_mol_idx=[0]), {}, ValueError),
    (dict(SITES, ext_mol_idx=[0.5, 0.5]), {}, ValueError),
    (dict(ext_coord=[["a", "b", "c"]], ext_charge=[0.1]), {}, ValueError),
    (dict(ext_mol_idx=[0, 0]), {}, ValueError),
    (dict(ext_potential=[0.1, 0.2]), {}, ValueError),
    (dict(ext_potential_grad=np.zeros((3, 3))), {}, ValueError),
    (dict(ext_potential=[0.1, 0.2, 0.3], ext_potential_grad=np.zeros((3, 2))), {}, ValueError),
    (dict(ext_potential=[0.1, 0.2, 0.3]), dict(forces=True), ValueError),
    (dict(SITES, cell=np.eye(3) * 20.0), {}, ValueError),
])
def test_rejections_come_before_the_engine(calc, extra, kw, exc):
    with pytest.raises(exc):
        calc(dict(WATER, **extra), **kw)
    assert calc.engine.calls == []


def test_other_entry_points_reject_the_keys(calc):
    with pytest.raises((NotImplementedError, ValueError)):
        calc.hessian_vector_product(dict(WATER, **SITES), np.zeros((3, 3), np.float32))
    calc._dd = object()  # domain decomposition on
    with pytest.raises((NotImplementedError, ValueError)):
        calc(dict(WATER, **SITES, cell=np.eye(3) * 20.0))
    assert calc.engine.calls == []


def test_ase_adapter_passes_the_sites_and_caches_their_forces(calc):
    from aimnetcentral_amd.aimnet2ase import AIMNet2ASE

    class Atoms:
        def __init__(self):
            self.numbers, self.positions, self.cell = np.array([8, 1, 1]), np.array(WATER["coord"], dtype=float), None
            self.pbc, self.info = np.zeros(3, bool), {}

        def copy(self):
            a = Atoms()
            a.positions = self.positions.copy()
            return a

    ase_calc = AIMNet2ASE(calc, charge=0)
    atoms = Atoms()
    ase_calc.calculate(atoms, ["energy"])
    assert "embedding" not in calc.engine.calls[-1]
    pc = ase_calc.embed(charges=[0.4, -0.4])
    ase_calc.calculate(atoms, ["energy"])  # no positions yet: not embedded
    assert "embedding" not in calc.engine.calls[-1]
    pc.set_positions(np.array(SITES["ext_coord"]))
    assert ase_calc.results == {}
    ase_calc.calculate(atoms, ["energy"])
    emb = calc.engine.calls[-1]["embedding"]
    assert emb["want_ext_forces"] is True and tuple(emb["ext_coord"].shape) == (2, 3) and calc.engine.calls[-1]["forces"] is True
    f = pc.get_forces(ase_calc)
    assert f.shape == (2, 3) and f.dtype == np.float64 and np.array_equal(f.reshape(-1), np.arange(6.0))
    n_calls = len(calc.engine.calls)
    pc.set_charges([0.1, 0.1])
    assert pc.forces is None
    assert pc.get_forces(ase_calc).shape == (2, 3) and len(calc.engine.calls) == n_calls + 1
    ase_calc.embed()
    ase_calc.calculate(atoms, ["energy"])
    assert "embedding" not in calc.engine.calls[-1]


# ---- the C entry points --------------------------------------------------------------------------------------------------------
def test_entry_points_with_null_handles():
    from aimnetcentral_amd import _lib

    lib = _lib.load()
    assert lib.aimnet_engine_set_embedding(None, None) == _lib.E_INVALID
    emb = _lib.Embedding(n_ext=0)
    assert lib.aimnet_engine_set_embedding(None, C.byref(emb)) == _lib.E_INVALID
    assert lib.aimnet_embedding_scratch_bytes(0, 1, 10) == 0
    assert lib.aimnet_embedding_scratch_bytes(10, 0, 10) == 0
    assert lib.aimnet_embedding_scratch_bytes(10, 1, -1) == 0
    small, big = lib.aimnet_embedding_scratch_bytes(10, 1, 0), lib.aimnet_embedding_scratch_bytes(10, 1, 3 * _lib.EMBED_CHUNK + 5)
    assert 0 < small < big
    # the partial sums: n_atoms * min(ceil(n_ext / EMBED_CHUNK), EMBED_MAX_SLOTS) * 4 doubles on top of the site index copy
    assert big - small >= 10 * 4 * 4 * 8 + (3 * _lib.EMBED_CHUNK + 5) * 4
    assert lib.aimnet_embedding_scratch_bytes(10, 1, 1000 * _lib.EMBED_CHUNK) - lib.aimnet_embedding_scratch_bytes(10, 1, 64 * _lib.EMBED_CHUNK) \
        <= (1000 - 64) * _lib.EMBED_CHUNK * 4 + 256


def test_struct_mirror_matches_the_header():
    """int32 n_ext (+ 4 bytes padding), eight pointers, void* scratch, size_t scratch_bytes: the header's field list."""
    from aimnetcentral_amd import _lib

    assert C.sizeof(_lib.Embedding) == 8 + 8 * 8 + 8 + 8
    assert [f[0] for f in _lib.Embedding._fields_] == ["n_ext", "ext_coord", "ext_charge", "ext_mol_idx", "potential", "potential_grad",
                                                       "ext_forces", "ext_potential", "energy", "scratch", "scratch_bytes"]
    assert {"aimnet_embedding_scratch_bytes", "aimnet_engine_set_embedding"} <= set(_lib.EXPORTED_SYMBOLS)


def test_describe_input_flags_knows_bit_7():
    from aimnetcentral_amd.engine import EXT_MOL_IDX_FLAG, describe_input_flags

    assert EXT_MOL_IDX_FLAG == 128
    text = describe_input_flags(128, 5)
    assert "ext_mol_idx" in text and "unknown" not in text
