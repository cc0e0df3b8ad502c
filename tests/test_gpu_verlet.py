"""Verlet-skin reuse of the neighbour matrices across MD steps (aimnetcentral_amd/verlet.py; the
reference's static-geometry counterpart is StaticInputCache, aimnet/calculators/neighbors.py:150-250): along a random walk the
evaluations through kept matrices (cutoff + skin, pairs cut at the true cutoff by the kernels) agree with evaluations that
rebuild every list, at the reference's gates; the matrices are rebuilt exactly when an atom has left the skin."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from conftest import CHARGE_ATOL, STRESS_ATOL, assert_forces_close, elementwise_violations, energy_tol, golden, golden_section
from oracle import aimnet2_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle64_cold(synth_sd_cold):
    return O.OracleModel(synth_sd_cold, torch.float64)


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items() if k != "status"}


def _meets_oracle(res, o32, o64, c, z, mol, q, cell, what, dftd3=None, **kw):
    """One evaluation against the CPU oracle at the same coordinates, the way tests/test_gpu_parity.py::compare does it: fp32 oracle
    as partner (energy, charges, forces, stress where present), the energy gate widened by that partner's own distance from the
    fp64-oracle energy; conftest.py's gates, no other tolerance."""
    okw = {k: kw[k] for k in ("coulomb", "dsf_rc", "dsf_alpha") if k in kw}
    ref = O.evaluate(o32, c, z, q, mol, cell=cell, stress="stress" in res, dftd3=dftd3, **okw)
    e64 = O.evaluate(o64, c, z, q, mol, cell=cell, forces=False, dftd3=dftd3, **okw)["energy"]
    sizes = np.bincount(np.asarray(mol), minlength=len(np.atleast_1d(q)))
    assert np.isfinite(res["energy"]).all(), what
    err, slack = np.abs(res["energy"] - ref["energy"]), np.abs(ref["energy"] - e64)
    print(f"{what}: |dE| {err.max():.2e} eV (gate {energy_tol(sizes):.1e} + {slack.max():.1e})  "
          f"|dF| {np.abs(res['forces'] - ref['forces']).max():.2e}  |dq| {np.abs(res['charges'] - ref['charges']).max():.2e}")
    assert (err <= energy_tol(sizes) + slack).all(), f"{what}: energy {err.max():.3e} vs the oracle"
    assert np.abs(res["charges"] - ref["charges"]).max() <= CHARGE_ATOL, what
    assert_forces_close(res["forces"], ref["forces"], what + " vs the oracle")
    if "stress" in res:
        assert np.abs(res["stress"] - ref["stress"]).max() <= STRESS_ATOL, what


def _meets_golden_literally(res, g, what):
    """The reference's literal gates against a golden the unmodified reference produced (test_gpu_parity.py,
    test_cold_weights_at_the_reference_literal_gates): |dE| < 1e-5 eV, every force component inside allclose(1e-4, 1e-5)."""
    de = np.abs(res["energy"] - g["energy"]).max()
    bad, n, worst = elementwise_violations(res["forces"], g["forces"])
    print(f"{what}: |dE| {de:.2e} eV, worst force component at {worst:.2f} of the gate")
    assert de < 1e-5, f"{what}: |dE| = {de:.2e} eV"
    assert bad == 0, f"{what}: {bad} of {n} force components outside allclose(1e-4, 1e-5), worst {worst:.2f} x the gate"
    assert np.abs(res["charges"] - g["charges"]).max() <= CHARGE_ATOL, what
    if "stress" in g:
        assert np.abs(res["stress"] - g["stress"]).max() <= STRESS_ATOL, what


class _Shell:
    """Host-side book-keeping of one kept matrix (numpy + the oracle's brute-force list only, so it can be checked without a GPU):
    the pairs inside cutoff + skin at build time, followed along the walk.  `count(x)` = (kept pairs that now sit beyond the true
    cutoff - the skin shell -, kept pairs that crossed the true cutoff in either direction since the build)."""

    def __init__(self, rc, skin, mol, cell):
        self.rc, self.skin, self.mol = float(rc), float(skin), np.asarray(mol)
        self.cell = None if cell is None else np.asarray(cell, dtype=np.float64)

    def _d(self, x):
        return np.linalg.norm(x[self.j] + self.off - x[self.i], axis=1)

    def build(self, x):
        x = np.asarray(x, dtype=np.float64)
        n = len(x)
        xw = x if self.cell is None else O.wrap_into_cell(x, self.cell, self.mol, np.ones(3, bool)).astype(np.float64)
        nb, sh = O.neighbor_list(xw, self.rc + self.skin, self.mol, self.cell, None if self.cell is None else np.ones(3, bool))
        self.i, k = np.nonzero(nb[:n] < n)
        self.j = nb[self.i, k]
        self.off = 0.0 if sh is None else sh[self.i, k].astype(np.float64) @ self.cell
        self.frame = x - xw  # the build-time wrap: later coordinates are followed in the same frame
        self.inside0 = self._d(xw) < self.rc

    def count(self, x):
        inside = self._d(np.asarray(x, dtype=np.float64) - self.frame) < self.rc
        return int((~inside).sum()), int((inside != self.inside0).sum())


def _shells(eng, skin, mol, cell, kw):
    """One _Shell per kept matrix whose pairs are cut sharply: the short-range one, and the DSF one where there is one."""
    out = {"rc": _Shell(eng.spec.rc, skin, mol, cell)}
    if kw.get("coulomb") == "dsf":
        out["dsf_rc"] = _Shell(kw.get("dsf_rc", 15.0), skin, mol, cell)
    return out


def _walk(vl, eng, c0, z, mol, q, cell, steps, step_sigma, seed, oracle=None, oracle_dftd3=None, golden0=None, deferred=False, **kw):
    """oracle = (fp32, fp64) OracleModel: every step's `vl.eval` result is also held to the CPU oracle (_meets_oracle).  golden0:
    step 0 (the golden's own geometry) is held to the golden at the literal gates.  deferred: `sync=False, defer=True`, results
    read after one `check_deferred()` at the end.  worst["shell"][name] = the largest min(pairs in the skin shell, pairs that crossed
    the cutoff) over the REUSE steps: positive means the walk did exercise "pairs beyond the true cutoff contribute nothing"."""
    from aimnetcentral_amd.engine import HipEngine  # noqa: F401

    dev = eng.device
    rng = np.random.default_rng(seed)
    zt, mt, qt = (torch.as_tensor(a, device=dev) for a in (z, mol, q))
    ct = None if cell is None else torch.as_tensor(cell, dtype=torch.float32, device=dev)
    c = np.array(c0, dtype=np.float64)
    worst = dict(dE=0.0, viol=0, ratio=0.0, dq=0.0, ds=0.0)
    shells = _shells(eng, vl.skin, mol, cell, kw)
    worst["shell"] = {k: 0 for k in shells}
    held = []
    for step in range(steps):
        x = torch.as_tensor(c.astype(np.float32), device=dev)
        builds = vl.builds
        a = vl.eval(x, zt, mt, qt, cell=ct, forces=True, **(dict(kw, sync=False, defer=True) if deferred else kw))
        b = eng.eval(x, zt, mt, qt, cell=ct, forces=True, **kw)
        for name, sh in shells.items():
            if vl.builds != builds:
                sh.build(c.astype(np.float32))
            else:
                worst["shell"][name] = max(worst["shell"][name], min(sh.count(c.astype(np.float32))))
        held.append((step, c.astype(np.float32), a, b))
        c = c + rng.normal(0.0, step_sigma, c.shape)
    if deferred:
        vl.check_deferred()
    for step, c32, a, b in held:
        n_per = np.bincount(np.asarray(mol), minlength=len(np.atleast_1d(q)))
        worst["dE"] = max(worst["dE"], float((a["energy"] - b["energy"]).abs().max() / energy_tol(n_per)))
        v, _, r = elementwise_violations(a["forces"].cpu().numpy(), b["forces"].cpu().numpy())
        worst["viol"] += v
        worst["ratio"] = max(worst["ratio"], r)
        worst["dq"] = max(worst["dq"], float((a["charges"] - b["charges"]).abs().max()))
        if "stress" in a:
            worst["ds"] = max(worst["ds"], float((a["stress"] - b["stress"]).abs().max()))
        if golden0 is not None and step == 0:
            _meets_golden_literally(_np(a), golden0, "kept matrices on the golden geometry")
        if oracle is not None:
            # (the engine's `dftd3` holds the parameters only; the oracle's carries the tables as well)
            _meets_oracle(_np(a), oracle[0], oracle[1], c32, z, mol, q, cell, f"walk step {step}", dftd3=oracle_dftd3,
                          **{k: v for k, v in kw.items() if k != "dftd3"})
    print("walk:", worst, "builds", vl.builds, "reuses", vl.reuses)
    return worst


def _shell_was_exercised(w):
    assert all(v > 0 for v in w["shell"].values()), ("no reuse step of this walk had pairs both inside the skin shell and across the "
                                                      "cutoff since the build", w["shell"])


def test_periodic_dsf_with_stress_along_a_walk(hip_engine_cold, oracle32_cold, oracle64_cold):
    from aimnetcentral_amd import workloads
    from aimnetcentral_amd.verlet import VerletSkinLists

    c, z, cell = workloads.glucose_supercell((2, 1, 1))
    c = c + np.array([3.0, -20.0, 7.5])  # atoms start outside the cell: the build-time wrap offsets matter
    vl = VerletSkinLists(hip_engine_cold, skin=0.6)
    w = _walk(vl, hip_engine_cold, c, z, np.zeros(len(z), np.int64), np.zeros(1, np.float32), cell, 12, 0.03, 1,
              oracle=(oracle32_cold, oracle64_cold), coulomb="dsf", dsf_rc=9.0, stress=True)
    # (atoms that start outside the cell: the kept matrices see them in the build-time wrap frame, the fresh evaluation re-wraps them
    # on the device in fp32 - positions that differ by an ulp; over 12 steps x 576 force components at most a couple may touch the
    # literal gate, none beyond 1.5 x)
    assert w["dE"] <= 1.0 and w["viol"] <= 2 and w["ratio"] <= 1.5 and w["dq"] <= CHARGE_ATOL and w["ds"] <= STRESS_ATOL, w
    assert vl.builds + vl.reuses == 12 and 1 <= vl.builds <= 6 and vl.reuses >= 6, (vl.builds, vl.reuses)
    _shell_was_exercised(w)


def test_molecule_batch_simple_coulomb_and_forced_rebuild(hip_engine_cold, oracle32_cold, oracle64_cold):
    from aimnetcentral_amd import workloads
    from aimnetcentral_amd.verlet import VerletSkinLists

    c, z, mol, q = workloads.random_batch(12, 20, 40, seed=4)
    vl = VerletSkinLists(hip_engine_cold, skin=0.5)
    w = _walk(vl, hip_engine_cold, c, z, mol, q, None, 8, 0.02, 2, oracle=(oracle32_cold, oracle64_cold), coulomb="simple")
    assert w["dE"] <= 1.0 and w["viol"] == 0 and w["dq"] <= CHARGE_ATOL, w
    assert vl.builds < 8
    _shell_was_exercised(w)
    # one atom jumps by more than skin / 2: the very next evaluation rebuilds
    dev = hip_engine_cold.device
    b0 = vl.builds
    x = torch.as_tensor(c, device=dev)
    args = (torch.as_tensor(z, device=dev), torch.as_tensor(mol, device=dev), torch.as_tensor(q, device=dev))
    vl.eval(x, *args, forces=True)
    b1 = vl.builds
    x2 = x.clone()
    x2[5, 0] += 0.3
    a = vl.eval(x2, *args, forces=True)
    assert vl.builds == b1 + 1 and b1 >= b0
    b = hip_engine_cold.eval(x2, *args, forces=True)
    assert elementwise_violations(a["forces"].cpu().numpy(), b["forces"].cpu().numpy())[0] == 0
    _meets_oracle(_np(a), oracle32_cold, oracle64_cold, x2.cpu().numpy(), z, mol, q, None, "after the forced rebuild", coulomb="simple")


def test_dftd3_and_dsf_share_one_kept_matrix(hip_engine, oracle32, oracle64):
    from aimnetcentral_amd.verlet import VerletSkinLists

    g, t = golden("dftd3"), golden("dftd3_subset")
    tables = {k: t[k] for k in ("c6ab", "cn_ref", "rcov", "r4r2")}
    hip_engine.set_dftd3_tables(tables)
    rc = float(g["pbc_cutoff"])
    par = dict(s6=float(g["s6"]), s8=float(g["s8"]), a1=float(g["a1"]), a2=float(g["a2"]), cutoff=rc, smoothing_fraction=0.2)
    vl = VerletSkinLists(hip_engine, skin=0.5)
    for kw in (dict(coulomb="dsf", dsf_rc=rc, dftd3=par), dict(coulomb="dsf", dsf_rc=rc - 2.0, dftd3=par)):
        # hot weights, the D3 term in the oracle as well: the gates test_dftd3_periodic_energy_forces_stress_vs_oracle holds this cell to
        w = _walk(vl, hip_engine, g["pbc_coord"], g["pbc_numbers"], np.zeros(96, np.int64), np.zeros(1, np.float32), g["pbc_cell"], 5,
                  0.02, 3, oracle=(oracle32, oracle64), oracle_dftd3=dict(par, **tables), **kw)
        # hot weights: two fp32 evaluations in different pair orders (the engine's own lists are bin-ordered, imported ones are not)
        assert w["dE"] <= 3.0 and w["ratio"] <= 10.0 and w["dq"] <= CHARGE_ATOL, (kw, w)
        _shell_was_exercised(w)
    assert vl.builds >= 2 and vl.reuses >= 4


def test_deferred_mode_flags_an_atom_that_left_the_skin(hip_engine_cold):
    from aimnetcentral_amd import workloads
    from aimnetcentral_amd.engine import NeighborOverflowError
    from aimnetcentral_amd.verlet import VerletSkinLists

    c, z, mol, q = workloads.random_batch(6, 20, 30, seed=7)
    dev = hip_engine_cold.device
    args = (torch.as_tensor(z, device=dev), torch.as_tensor(mol, device=dev), torch.as_tensor(q, device=dev))
    vl = VerletSkinLists(hip_engine_cold, skin=0.4, rebuild_every=50)
    x = torch.as_tensor(c, device=dev)
    for k in range(4):
        vl.eval(x + 0.01 * k, *args, forces=True, sync=False, defer=True)
    vl.check_deferred()  # all inside the skin: passes, one build
    assert vl.builds == 1 and vl.reuses == 3
    vl.eval(x + 0.5, *args, forces=True, sync=False, defer=True)
    with pytest.raises(NeighborOverflowError):
        vl.check_deferred()
    vl.eval(x + 0.5, *args, forces=True, sync=False, defer=True)  # invalidated: rebuilt
    vl.check_deferred()
    assert vl.builds == 2


# ---- the kept-matrix path against goldens of the unmodified reference (tests/golden/coldw.npz) -------------------------------------
def _golden_case(name):
    g = golden_section(golden("coldw"), name)
    mol = g.get("mol_idx", np.zeros(len(g["numbers"]), dtype=np.int64))
    q = np.atleast_1d(g["charge"]).astype(np.float32)
    kw = dict(coulomb="dsf", dsf_rc=float(g["dsf_rc"]), dsf_alpha=float(g["dsf_alpha"]), stress=True) if "cell" in g else dict(coulomb="simple")
    return g, mol, q, g.get("cell"), kw


@pytest.mark.parametrize("name,skin,sigma,seed", [("pbc96", 0.5, 0.03, 5), ("rand8", 0.5, 0.03, 6)])
def test_walk_that_starts_on_a_reference_golden(hip_engine_cold, oracle32_cold, oracle64_cold, name, skin, sigma, seed):
    """Step 0 is the golden's own geometry: the kept-matrix evaluation meets the golden at the literal gates (no oracle of this
    repository in that chain); the following steps meet the oracle."""
    from aimnetcentral_amd.verlet import VerletSkinLists

    g, mol, q, cell, kw = _golden_case(name)
    vl = VerletSkinLists(hip_engine_cold, skin=skin)
    w = _walk(vl, hip_engine_cold, g["coord"], g["numbers"], mol, q, cell, 6, sigma, seed, oracle=(oracle32_cold, oracle64_cold),
              golden0=g, **kw)
    assert w["dE"] <= 1.0 and w["viol"] == 0 and w["dq"] <= CHARGE_ATOL and w["ds"] <= STRESS_ATOL, w
    assert vl.builds + vl.reuses == 6 and vl.reuses >= 1, (vl.builds, vl.reuses)
    _shell_was_exercised(w)


@pytest.mark.parametrize("name", ["pbc96", "rand8"])
def test_pairs_beyond_the_true_cutoff_contribute_nothing(hip_engine_cold, name):
    """No walk, no list builder of the engine: brute-force matrices of the ORACLE at cutoff + skin on the golden geometry go in as
    caller-supplied matrices, and the result meets the golden at the literal gates - the kernels that consume an imported matrix cut
    every pair at the true cutoff themselves.  The same call with matrices at the exact cutoffs differs by summation order only
    (other row positions of the same contributing pairs): the bound test_gpu_lists.py uses for "same pairs, other order"."""
    g, mol, q, cell, kw = _golden_case(name)
    eng, dev = hip_engine_cold, hip_engine_cold.device
    n, skin, rc = len(mol), 0.5, float(hip_engine_cold.spec.rc)
    pbc = None if cell is None else np.ones(3, bool)

    def lists(extra):
        nb, sh = O.neighbor_list(g["coord"], rc + extra, mol, cell, pbc)
        out = {"nbmat": torch.as_tensor(nb[:n]), "shifts": None if sh is None else torch.as_tensor(sh[:n]).to(torch.int32)}
        # 'simple' Coulomb sums 1 / d over EVERY entry of nbmat_lr (lr.py:311-331): no cutoff to test there, all pairs in both calls
        nbl, shl = O.neighbor_list(g["coord"], (kw["dsf_rc"] + extra) if cell is not None else float("inf"), mol, cell, pbc)
        out.update(nbmat_lr=torch.as_tensor(nbl[:n]), shifts_lr=None if shl is None else torch.as_tensor(shl[:n]).to(torch.int32))
        return out

    args = (torch.from_numpy(g["coord"]).to(dev), torch.from_numpy(g["numbers"]).to(dev), torch.from_numpy(mol).to(dev),
            torch.from_numpy(q).to(dev))
    ct = None if cell is None else torch.from_numpy(cell).to(dev)
    wide, exact = lists(skin), lists(0.0)
    extra = {k: int((wide[k] < n).sum() - (exact[k] < n).sum()) for k in ("nbmat", "nbmat_lr")}  # pairs inside the skin shell
    assert extra["nbmat"] > 0 and (cell is None or extra["nbmat_lr"] > 0), extra
    a = _np(eng.eval(*args, cell=ct, forces=True, **kw, **wide))
    b = _np(eng.eval(*args, cell=ct, forces=True, **kw, **exact))
    _meets_golden_literally(a, g, f"{name}, oracle matrices at cutoff + {skin} A")
    _meets_golden_literally(b, g, f"{name}, oracle matrices at the exact cutoffs")
    de, df = np.abs(a["energy"] - b["energy"]).max(), np.abs(a["forces"] - b["forces"]).max()
    dq = np.abs(a["charges"] - b["charges"]).max()
    ds = np.abs(a["stress"] - b["stress"]).max() if "stress" in a else 0.0
    msg = f"{name}: cutoff + skin against exact-cutoff matrices: |dE| {de:.3e} eV, |dF| {df:.3e} eV/A, |dq| {dq:.3e} e, |dstress| {ds:.3e}"
    print(msg)
    assert de <= 2e-5 and df <= 5e-5, msg


def test_deferred_mode_meets_the_oracle(hip_engine_cold, oracle32_cold, oracle64_cold):
    """`sync=False, defer=True`: the results of an in-skin walk, read after check_deferred(), at the same gates."""
    from aimnetcentral_amd import workloads
    from aimnetcentral_amd.verlet import VerletSkinLists

    c, z, cell = workloads.glucose_supercell((1, 1, 1))
    vl = VerletSkinLists(hip_engine_cold, skin=0.6, rebuild_every=50)
    w = _walk(vl, hip_engine_cold, c, z, np.zeros(len(z), np.int64), np.zeros(1, np.float32), cell, 5, 0.03, 8,
              oracle=(oracle32_cold, oracle64_cold), deferred=True, coulomb="dsf", dsf_rc=8.0, stress=True)
    assert w["dE"] <= 1.0 and w["viol"] == 0 and w["dq"] <= CHARGE_ATOL and w["ds"] <= STRESS_ATOL, w
    assert vl.builds == 1 and vl.reuses == 4
    _shell_was_exercised(w)


# ---- the reuse key: what the matrices depend on, nothing else ----------------------------------------------------------------------
def test_a_changed_molecule_assignment_rebuilds(hip_engine_cold, oracle32_cold, oracle64_cold):
    """Same coordinates, same shapes, another `mol_idx`: the rows hold same-molecule pairs only, so kept matrices of the old assignment
    would keep pairs across the new molecules (and, the other way round, miss pairs inside a merged one)."""
    from aimnetcentral_amd import workloads
    from aimnetcentral_amd.verlet import VerletSkinLists

    c, z, _, _ = workloads.random_batch(1, 40, 40, seed=11)
    dev = hip_engine_cold.device
    x, zt = torch.as_tensor(c, device=dev), torch.as_tensor(z, device=dev)
    one, two = np.zeros(40, np.int64), np.repeat(np.arange(2), 20)
    vl = VerletSkinLists(hip_engine_cold, skin=0.5)
    for k, (mol, q) in enumerate(((one, np.zeros(1, np.float32)), (two, np.zeros(2, np.float32)), (one, np.zeros(1, np.float32)))):
        a = vl.eval(x, zt, torch.as_tensor(mol, device=dev), torch.as_tensor(q, device=dev), forces=True, coulomb="simple")
        _meets_oracle(_np(a), oracle32_cold, oracle64_cold, c, z, mol, q, None, f"assignment {k}", coulomb="simple")
        assert vl.builds == k + 1, (k, vl.builds, vl.reuses)


def test_fresh_tensors_with_equal_contents_reuse_the_matrices(hip_engine_cold):
    from aimnetcentral_amd import workloads
    from aimnetcentral_amd.verlet import VerletSkinLists

    c, z, mol, q = workloads.random_batch(6, 20, 30, seed=7)
    dev = hip_engine_cold.device
    x = torch.as_tensor(c, device=dev)
    vl = VerletSkinLists(hip_engine_cold, skin=0.4)
    keep = []
    for k in range(4):  # (the earlier tensors stay alive: the allocator cannot hand the same address out again)
        keep.append((torch.as_tensor(z, device=dev).clone(), torch.as_tensor(mol, device=dev).clone(), torch.as_tensor(q, device=dev).clone()))
        vl.eval(x + 0.01 * k, *keep[-1], forces=True)
    assert len({t[0].data_ptr() for t in keep}) == 4
    assert vl.builds == 1 and vl.reuses == 3, (vl.builds, vl.reuses)


def test_a_changed_cell_at_unchanged_coordinates_rebuilds(hip_engine_cold, oracle32_cold, oracle64_cold):
    from aimnetcentral_amd import workloads
    from aimnetcentral_amd.verlet import VerletSkinLists

    c, z, cell = workloads.glucose_supercell((1, 1, 1))
    dev = hip_engine_cold.device
    mol, q = np.zeros(len(z), np.int64), np.zeros(1, np.float32)
    args = (torch.as_tensor(c, dtype=torch.float32, device=dev), torch.as_tensor(z, device=dev), torch.as_tensor(mol, device=dev),
            torch.as_tensor(q, device=dev))
    vl = VerletSkinLists(hip_engine_cold, skin=0.5)
    kw = dict(coulomb="dsf", dsf_rc=8.0, stress=True)
    for k, scale in enumerate((1.0, 1.0, 1.02)):
        cl = (cell * scale).astype(np.float32)
        a = vl.eval(*args, cell=torch.as_tensor(cl, device=dev), forces=True, **kw)
        assert (vl.builds, vl.reuses) == ((1, 0), (1, 1), (2, 1))[k], (k, vl.builds, vl.reuses)
    _meets_oracle(_np(a), oracle32_cold, oracle64_cold, c.astype(np.float32), z, mol, q, cl, "after the cell change", **kw)
