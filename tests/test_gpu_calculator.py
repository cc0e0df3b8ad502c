"""AIMNet2Calculator API on the GPU: layouts, invariances, batched-vs-individual
(reference tests/test_calculator.py:979-1217) and the full-size config-3 properties."""
from __future__ import annotations

import warnings

import numpy as np
import pytest
import torch

from conftest import CHARGE_ATOL, assert_forces_close, energy_tol, golden
from aimnetcentral_amd import workloads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def calc():
    from aimnetcentral_amd import AIMNet2Calculator, loader

    return AIMNet2Calculator(loader.synthetic_spec(0), device="cuda:0")


def npy(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_flat_input_matches_reference_golden(calc):
    g = golden("taxol")
    out = npy(calc({"coord": g["coord"], "numbers": g["numbers"], "charge": 0.0}, forces=True))
    assert out["energy"].dtype == np.float64 and out["energy"].shape == (1,)
    assert abs(out["energy"][0] - g["energy"][0]) <= energy_tol(113)
    assert_forces_close(out["forces"], g["forces"], "taxol")
    assert np.abs(out["charges"] - g["charges"]).max() <= CHARGE_ATOL


def test_3d_batch_matches_reference_golden(calc):
    g = golden("dense3x14")
    out = npy(calc({"coord": g["coord"], "numbers": g["numbers"], "charge": g["charge"]}, forces=True))
    assert out["forces"].shape == (3, 14, 3) and out["charges"].shape == (3, 14) and out["energy"].shape == (3,)
    assert np.abs(out["energy"] - g["energy"]).max() <= energy_tol(14)
    assert_forces_close(out["forces"], g["forces"], "dense3x14")


def test_padded_dense_batch_equals_flat_and_individual(calc):
    """batched-vs-individual at 1e-5 eV / 1e-5 eV/A / 1e-4 e (test_calculator.py:1052-1217)."""
    c, z, mol, q = workloads.random_batch(6, 8, 31, seed=17)
    flat = npy(calc({"coord": c, "numbers": z, "mol_idx": mol, "charge": q}, forces=True))
    cp, zp = workloads.pad_batch(c, z, mol, 6)
    dense = npy(calc({"coord": cp, "numbers": zp, "charge": q}, forces=True))
    assert np.abs(dense["energy"] - flat["energy"]).max() == 0.0  # same engine layout underneath
    start = 0
    for m in range(6):
        n = int((mol == m).sum())
        one = npy(calc({"coord": c[mol == m], "numbers": z[mol == m], "charge": float(q[m])}, forces=True))
        assert abs(one["energy"][0] - flat["energy"][m]) < 1e-5
        assert np.abs(one["forces"] - flat["forces"][start : start + n]).max() < 1e-5 + 1e-4 * np.abs(one["forces"]).max()
        assert np.abs(one["charges"] - flat["charges"][start : start + n]).max() < 1e-4
        assert np.array_equal(dense["forces"][m, :n], flat["forces"][start : start + n])
        assert (dense["forces"][m, n:] == 0).all() and (dense["charges"][m, n:] == 0).all()
        start += n


def test_translation_and_rotation_invariance(calc):
    """test_calculator.py:979-1015."""
    g = golden("taxol")
    base = npy(calc({"coord": g["coord"], "numbers": g["numbers"], "charge": 0.0}, forces=True))
    shifted = npy(calc({"coord": g["coord"] + np.array([10.0, -5.0, 3.0], np.float32), "numbers": g["numbers"], "charge": 0.0}, forces=True))
    assert abs(shifted["energy"][0] - base["energy"][0]) < 1e-4
    assert_forces_close(shifted["forces"], base["forces"], "translation")
    th = 0.7
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]], dtype=np.float32)
    rot = npy(calc({"coord": g["coord"] @ R.T, "numbers": g["numbers"], "charge": 0.0}, forces=True))
    assert abs(rot["energy"][0] - base["energy"][0]) < 1e-4
    assert_forces_close(rot["forces"], base["forces"] @ R.T, "rotation")
    assert np.abs(rot["charges"] - base["charges"]).max() < 1e-5


def test_pbc_auto_switch_and_explicit_dsf(calc):
    g = golden("pbc96_dsf15")
    data = {"coord": g["coord"], "numbers": g["numbers"], "charge": 0.0, "cell": g["cell"]}
    with pytest.warns(UserWarning, match="Switching to DSF Coulomb for PBC"):
        out = npy(calc(data, forces=True, stress=True))
    assert calc.coulomb_method == "simple"
    assert abs(out["energy"][0] - g["energy"][0]) <= energy_tol(96)
    assert_forces_close(out["forces"], g["forces"], "pbc auto-switch")
    assert np.abs(out["stress"] - g["stress"]).max() < 1e-5 and out["stress"].shape == (3, 3)
    g8 = golden("pbc96_dsf8_wrapped")
    calc.set_lrcoulomb_method("dsf", cutoff=8.0, dsf_alpha=0.25)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            out = npy(calc({"coord": g8["coord"], "numbers": g8["numbers"], "charge": 0.0, "cell": g8["cell"]}, forces=True, stress=True))
        assert abs(out["energy"][0] - g8["energy"][0]) <= energy_tol(96)
        assert_forces_close(out["forces"], g8["forces"], "dsf8")
    finally:
        calc.set_lrcoulomb_method("simple")


def test_hvp_of_a_cell_under_simple_takes_the_default_dsf_like_eval(calc):
    """A cell under "simple" is evaluated with DSF at the setter's defaults (15 A, alpha 0.2) by every entry point: after
    set_lrcoulomb_method("dsf", 8.0, 0.25) and back to "simple", hessian_vector_product equals HipEngine.hvp called directly with
    15.0 / 0.2 on the same tensors bit for bit (the sweep is bitwise reproducible), and not the sweep at the left-over 8.0 / 0.25."""
    g = golden("pbc96_dsf15")
    data = {"coord": g["coord"], "numbers": g["numbers"], "charge": 0.0, "cell": g["cell"]}
    v = torch.randn(2, 96, 3, generator=torch.Generator().manual_seed(7))
    v = (v / v.flatten(1).norm(dim=1).view(2, 1, 1)).to(calc.device)
    t = calc.to_input_tensors(data)
    args = (t["coord"], t["numbers"], torch.zeros(96, dtype=torch.int32, device=calc.device), t["charge"], v)
    calc.set_lrcoulomb_method("dsf", cutoff=8.0, dsf_alpha=0.25)
    calc.set_lrcoulomb_method("simple")
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # only `eval` announces the switch
            hv = calc.hessian_vector_product(data, v)
    finally:
        calc.set_lrcoulomb_method("simple")
    want = calc.engine.hvp(*args, cell=t["cell"], coulomb="dsf", dsf_rc=15.0, dsf_alpha=0.2)["hv"]
    stale = calc.engine.hvp(*args, cell=t["cell"], coulomb="dsf", dsf_rc=8.0, dsf_alpha=0.25)["hv"]
    assert hv.shape == (2, 96, 3) and torch.equal(hv, want)
    assert (hv - stale).abs().max().item() > 0.0  # the two surfaces differ: the comparison above can see a stale parameter


def test_batched_cells(calc):
    g = golden("pbc2x96_dsf9")
    calc.set_lrcoulomb_method("dsf", cutoff=9.0)
    try:
        out = npy(calc({"coord": g["coord"], "numbers": g["numbers"], "mol_idx": g["mol_idx"], "charge": g["charge"],
                        "cell": g["cell"]}, forces=True, stress=True))
    finally:
        calc.set_lrcoulomb_method("simple")
    assert out["stress"].shape == (2, 3, 3)
    assert np.abs(out["energy"] - g["energy"]).max() <= energy_tol(96)
    assert_forces_close(out["forces"], g["forces"], "2 cells")
    assert np.abs(out["stress"] - g["stress"]).max() < 1e-5


def test_stress_matches_finite_difference_of_energy(calc):
    """reference gate: |stress - FD| < 5e-3 (tests/test_pbc.py:975-1024)."""
    g = golden("pbc96_dsf8_wrapped")
    calc.set_lrcoulomb_method("dsf", cutoff=8.0, dsf_alpha=0.25)
    try:
        cell = g["cell"].astype(np.float64)
        frac = g["coord"].astype(np.float64) @ np.linalg.inv(cell)
        out = npy(calc({"coord": g["coord"], "numbers": g["numbers"], "charge": 0.0, "cell": g["cell"]}, stress=True))
        vol = abs(np.linalg.det(cell))
        h = 2e-3
        for (a, b) in [(0, 0), (1, 1), (0, 2)]:
            es = []
            for sgn in (+1, -1):
                eps = np.eye(3)
                eps[a, b] += sgn * h
                c2 = cell @ eps
                e = npy(calc({"coord": (frac @ c2).astype(np.float32), "numbers": g["numbers"], "charge": 0.0,
                              "cell": c2.astype(np.float32)}))["energy"][0]
                es.append(e)
            fd = (es[0] - es[1]) / (2 * h) / vol
            assert abs(fd - out["stress"][a, b]) < 5e-3, (a, b, fd, out["stress"][a, b])
    finally:
        calc.set_lrcoulomb_method("simple")


def test_config3_full_size_periodicity_properties(calc):
    """BASELINE config 3 at full size (10 080 atoms): an exactly periodic supercell must reproduce the
    96-atom cell of the reference golden - E = 105 E_cell, per-image forces/charges identical, same
    stress - and net force zero.  Size-independent properties, no 10k-atom oracle run needed."""
    g = golden("pbc96_dsf15")
    cell = g["cell"].astype(np.float64)
    reps = (7, 3, 5)
    # replicate the golden's own (float32) coordinates so that the crystal is exactly periodic
    base = g["coord"].astype(np.float64)
    out_c = []
    for ix in range(reps[0]):
        for iy in range(reps[1]):
            for iz in range(reps[2]):
                out_c.append(base + ix * cell[0] + iy * cell[1] + iz * cell[2])
    coord = np.concatenate(out_c).astype(np.float32)
    numbers = np.tile(g["numbers"], 105)
    sc = (cell * np.array([[reps[0]], [reps[1]], [reps[2]]])).astype(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = npy(calc({"coord": coord, "numbers": numbers, "charge": 0.0, "cell": sc}, forces=True, stress=True))
    assert out["forces"].shape == (10080, 3)
    assert abs(out["energy"][0] / 105.0 - g["energy"][0]) < 5e-5
    f = out["forces"].reshape(105, 96, 3)
    assert_forces_close(f, np.broadcast_to(g["forces"], f.shape), "supercell images")
    q = out["charges"].reshape(105, 96)
    assert np.abs(q - g["charges"]).max() < CHARGE_ATOL
    assert np.abs(out["stress"] - g["stress"]).max() < 2e-5
    assert np.abs(out["forces"].sum(0)).max() < 5e-3  # net force ~ fp32 noise * 10k atoms
    assert abs(out["charges"].sum()) < 1e-3


def test_maximum_size_80k_atoms_stays_periodic(calc):
    """Eight times config 3 (80 640 atoms, 5.5 GB workspace): 64-bit indexing of the pair arrays, multi-round tile
    grids and the cell walk at scale.  Same size-independent property: 840 images of the 96-atom golden cell."""
    g = golden("pbc96_dsf15")
    cell = g["cell"].astype(np.float64)
    reps = (14, 6, 10)
    ix, iy, iz = np.meshgrid(np.arange(reps[0]), np.arange(reps[1]), np.arange(reps[2]), indexing="ij")
    off = ix.reshape(-1, 1) * cell[0] + iy.reshape(-1, 1) * cell[1] + iz.reshape(-1, 1) * cell[2]
    coord = (g["coord"].astype(np.float64)[None] + off[:, None, :]).reshape(-1, 3).astype(np.float32)
    n_img = off.shape[0]
    numbers = np.tile(g["numbers"], n_img)
    sc = (cell * np.array([[reps[0]], [reps[1]], [reps[2]]])).astype(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = npy(calc({"coord": coord, "numbers": numbers, "charge": 0.0, "cell": sc}, forces=True, stress=True))
    assert out["forces"].shape == (96 * n_img, 3) and np.isfinite(out["forces"]).all()
    assert abs(out["energy"][0] / n_img - g["energy"][0]) < 1e-4
    f = out["forces"].reshape(n_img, 96, 3)
    assert_forces_close(f, np.broadcast_to(g["forces"], f.shape), "80k supercell images")
    assert np.abs(out["stress"] - g["stress"]).max() < 2e-5


def test_config4_hessian_and_hvp_analytic(calc):
    """BASELINE config 4 shape: dense Hessian and H @ v of a 40-atom geometry against the reference's double-backward
    results (tests/golden/hvp40.npz) at the reference's own gate for itself, allclose(rtol = atol = 1e-3) elementwise
    (tests/test_hvp.py:75), and at the tighter 1e-4 / 2e-4 eV/A^2 the analytic tangent sweep (csrc/hvp.hip) delivers
    (measured 6.1e-5 on |H| <= 11.5 and 1.7e-4 on |Hv| <= 32: two fp32 evaluations of the same second derivative).
    The finite-difference operator over the forces stays as the independent cross-check at its own budget."""
    g = golden("hvp40")
    data = {"coord": g["coord"], "numbers": g["numbers"], "charge": float(g["charge"])}
    assert calc.hvp_method == "analytic"
    out = calc(data, forces=True, hessian=True)
    H = out["hessian"].cpu().numpy().reshape(120, 120)
    Href = g["hessian"].reshape(120, 120)
    assert np.allclose(H, Href, rtol=1e-3, atol=1e-3)
    assert np.abs(H - Href).max() <= 1e-4, np.abs(H - Href).max()
    assert np.abs(H - H.T).max() == 0.0
    assert_forces_close(out["forces"].cpu().numpy(), g["forces"], "hvp40")
    hv1 = calc.hessian_vector_product(data, torch.from_numpy(g["v1"])).cpu().numpy()
    hv4 = calc.hessian_vector_product(data, torch.from_numpy(g["v4"])).cpu().numpy()
    assert hv1.shape == (40, 3) and hv4.shape == (4, 40, 3)
    for got, ref in ((hv1, g["hv1"]), (hv4, g["hv4"])):
        assert np.allclose(got, ref, rtol=1e-3, atol=1e-3)
        assert np.abs(got - ref).max() <= 1e-4 + 1e-5 * np.abs(ref).max(), np.abs(got - ref).max()
    # the matrix-free products and the dense Hessian are the same operator
    assert np.abs(hv1.reshape(120) - H @ g["v1"].reshape(120)).max() < 2e-4
    # translation invariance of the energy: every row of H sums to zero over the atoms (size-independent property)
    assert np.abs(H.reshape(40, 3, 40, 3).sum(axis=2)).max() < 2e-4
    # cross-check: the 4th-order central difference of the analytic forces (h = 5e-3 A) agrees within ITS budget
    # (truncation ~2e-4 + 190 x force noise: 4.6e-4 on H, 2.3e-3 on H v measured)
    calc.hvp_method = "fd"
    try:
        Hfd = calc(data, hessian=True)["hessian"].cpu().numpy().reshape(120, 120)
        hv1_fd = calc.hessian_vector_product(data, torch.from_numpy(g["v1"])).cpu().numpy()
    finally:
        calc.hvp_method = "analytic"
    assert np.abs(Hfd - H).max() <= 2e-3 and np.abs(hv1_fd - hv1).max() <= 2e-3 + 2e-4 * np.abs(hv1).max()


def test_calculator_with_external_dftd3(oracle_d3):
    """needs_dispersion=True end to end: AIMNet2Calculator builds the external DFT-D3 state from the artifact's
    d3_params and the table file, and the result equals the oracle's evaluation with the same term."""
    from aimnetcentral_amd import AIMNet2Calculator, loader
    from oracle import aimnet2_oracle as O

    om, par, tables = oracle_d3
    spec = loader.synthetic_spec(0)
    spec.metadata = dict(spec.metadata, needs_dispersion=True, d3_params={k: par[k] for k in ("s6", "s8", "a1", "a2")})
    calc = AIMNet2Calculator(spec, device="cuda:0", dftd3_data=tables)
    assert calc.has_external_dftd3 and calc.cutoff_lr == float("inf") and calc.dftd3_cutoff == 15.0
    g = golden("taxol")
    out = npy(calc({"coord": g["coord"], "numbers": g["numbers"], "charge": 0.0}, forces=True))
    ref = O.evaluate(om, g["coord"], g["numbers"], 0.0, dftd3=dict(par, **tables))
    assert abs(out["energy"][0] - ref["energy"][0]) <= energy_tol(113)
    assert_forces_close(out["forces"], ref["forces"], "taxol + d3")
    base = npy(AIMNet2Calculator(loader.synthetic_spec(0), device="cuda:0")({"coord": g["coord"], "numbers": g["numbers"], "charge": 0.0}))
    assert abs((out["energy"][0] - base["energy"][0]) - golden("dftd3")["taxol_energy"][0]) < 6e-6


@pytest.fixture(scope="module")
def oracle_d3():
    from aimnetcentral_amd import synth
    from oracle import aimnet2_oracle as O

    g, t = golden("dftd3"), golden("dftd3_subset")
    par = dict(s6=float(g["s6"]), s8=float(g["s8"]), a1=float(g["a1"]), a2=float(g["a2"]), cutoff=15.0, smoothing_fraction=0.2)
    return O.OracleModel(synth.synthetic_state_dict(0), torch.float32), par, {k: t[k] for k in ("c6ab", "cn_ref", "rcov", "r4r2")}


def test_atom_order_does_not_matter(calc):
    """Permutation equivariance on a periodic system: the conv kernels process centres in the cell list's bin order
    (engine.hip `order`), so a shuffled file must give the same energy / stress and the permuted forces / charges."""
    g = golden("pbc96_dsf15")
    perm = np.random.default_rng(5).permutation(96)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = npy(calc({"coord": g["coord"], "numbers": g["numbers"], "charge": 0.0, "cell": g["cell"]}, forces=True, stress=True))
        b = npy(calc({"coord": g["coord"][perm], "numbers": g["numbers"][perm], "charge": 0.0, "cell": g["cell"]}, forces=True, stress=True))
    assert abs(a["energy"][0] - b["energy"][0]) <= energy_tol(96)
    assert_forces_close(b["forces"], a["forces"][perm], "shuffled")
    assert np.abs(b["charges"] - a["charges"][perm]).max() < CHARGE_ATOL
    assert np.abs(a["stress"] - b["stress"]).max() < 1e-5


def test_nse_calculator_open_shell(oracle32_nse, oracle64_nse):
    """Open-shell NSE family through the calculator API: `mult` input, spin_charges output, the reference golden
    (tests/golden/nse.npz), 3D batches, and the FD Hessian-vector product against a central difference of the oracle forces."""
    from aimnetcentral_amd import AIMNet2Calculator, loader
    from oracle import aimnet2_oracle as O

    calc = AIMNet2Calculator(loader.synthetic_spec(0, num_charge_channels=2), device="cuda:0")
    assert calc.is_nse
    g = golden("nse")
    data = {"coord": g["t40_coord"], "numbers": g["t40_numbers"], "charge": float(g["t40_charge"]), "mult": float(g["t40_mult"])}
    out = npy(calc(data, forces=True))
    assert set(out) == {"energy", "charges", "spin_charges", "forces"}
    assert abs(out["energy"][0] - g["t40_energy"][0]) <= energy_tol(40)
    assert_forces_close(out["forces"], g["t40_forces"], "nse t40")
    assert np.abs(out["spin_charges"] - g["t40_spin_charges"]).max() <= CHARGE_ATOL
    # the multiplicity matters: the doublet and the quartet of the same cation differ
    quartet = npy(calc(dict(data, mult=4.0)))
    assert abs(quartet["energy"][0] - out["energy"][0]) > 1e-3 and abs(quartet["spin_charges"].sum() - 3.0) < 1e-3
    # flat ragged batch with per-molecule multiplicities == the reference golden
    b = npy(calc({"coord": g["b5_coord"], "numbers": g["b5_numbers"], "mol_idx": g["b5_mol_idx"], "charge": g["b5_charge"],
                  "mult": g["b5_mult"]}, forces=True))
    # gate widened by the golden's own distance from the fp64 energy (1.2e-5 eV on the 30-atom cation), see test_gpu_parity.compare
    e64 = O.evaluate(oracle64_nse, g["b5_coord"], g["b5_numbers"], g["b5_charge"], g["b5_mol_idx"], mult=g["b5_mult"], forces=False)["energy"]
    assert (np.abs(b["energy"] - g["b5_energy"]) <= energy_tol(30) + np.abs(g["b5_energy"] - e64)).all()
    assert np.abs(b["spin_charges"] - g["b5_spin_charges"]).max() <= CHARGE_ATOL
    # H v by the calculator's finite differences vs a central difference of the fp64-free oracle forces along v
    n = 12
    sub = {"coord": g["t40_coord"][:n], "numbers": g["t40_numbers"][:n], "charge": 0.0, "mult": 3.0}
    v = torch.randn(n, 3, generator=torch.Generator().manual_seed(1))
    hv = calc.hessian_vector_product(sub, v).cpu().numpy()
    h = 2e-3
    u = v.numpy() / np.linalg.norm(v.numpy(), axis=-1).max()
    fp = O.evaluate(oracle32_nse, sub["coord"] + h * u, sub["numbers"], 0.0, mult=3.0)["forces"].astype(np.float64)
    fm = O.evaluate(oracle32_nse, sub["coord"] - h * u, sub["numbers"], 0.0, mult=3.0)["forces"].astype(np.float64)
    ref = -(fp - fm) / (2 * h) * np.linalg.norm(v.numpy(), axis=-1).max()
    assert np.abs(hv - ref).max() <= 2e-2 + 2e-3 * np.abs(ref).max(), (np.abs(hv - ref).max(), np.abs(ref).max())
