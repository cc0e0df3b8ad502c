"""Every request kind - energy only (E), forces (F), stress alone (S), forces + stress (FS) - against the oracle on every branch of
the evaluation plan (csrc/eval_plan.h).  `grad`, `want_f` and `want_s` steer the plan as much as the input does: the `GRAD = false`
instantiations of the pair kernels, the launch that owns the energy sums and the copy of the charges, the reverse-pair map and who
defines `fgrad` / `virial_atom` / `qbar` / the pair buffer first all depend on them, and the rest of the suite asks almost only
for forces (+ stress on a cell).

Per case and kind (HipEngine.eval; the oracle is computed once per case, with forces, and with stress where periodic):
 1. every output meets the gates of conftest.py against the fp32 oracle (energy widened by the fp32 oracle's distance from the fp64
    one, as test_gpu_parity.compare does; PME / Ewald: the gates of test_gpu_pme.py / test_gpu_ewald.py against the exact Ewald
    oracle; the random configurations: test_gpu_fuzz._compare); keys that were not asked for are absent;
 2. energy, charges and spin charges are bitwise equal in all kinds, forces in F and FS, stress in S and FS - with two exceptions by
    design, both on a cell where the force gather of the reverse-pair form rides on the virial launch (EvalPlan::pair_force_rides:
    layout.xe, i.e. conv_xe and N above split_max, with forces AND stress asked for):
    (a) stress of S against FS.  With layout.xe but no force request there is no reverse-pair map, so pass 0 of the backward runs
        conv_bwd_p0_kernel<STRESS, XE = false> (conv.hip): both halves of every pair with the gather of the neighbour's moments T_j,
        virial weight -1/2 per ordered pair.  FS runs conv_bwd_p0_kernel<STRESS, XE = true>: the pair's own half only, weight -1.
        The same virial, summed from other products in another order (engine.hip, Eval::backward: `P.rev_hash ? W.pairbuf : nullptr`);
    (b) energy of FS against E, and once more the stress, where in addition an energy rider sits beside the gather
        (EnergySum::StressRider: a walk ran) and "sums_whole" is on: launch_finalize then takes the one-block sums -
        energy_whole_block and the whole-cell branch of stress_partial_kernel (model.hip), eight / four atoms per thread and round -
        while E, F and S take energy_partial_block and the slice loop + stress_finish_kernel: the same fp64 terms in another
        association (test_gpu_prep.test_whole_cell_sums_agree_with_the_sliced_ones).
    These pairs are held at the conftest gates (STRESS_ATOL, energy_tol); energies stay bitwise wherever (b) does not apply, e.g. on
    a cell without a walk.  That (a) and (b) are all that differs is asserted too: with "p0_moments" = 0 (pass 0 on the generic
    kernel, no pair buffer in pass 0 for either kind) and "sums_whole" = 0 the stress of S has the bits of FS and the energies agree;
 3. the kinds run in the orders FS, E, S, F and E, S, F, FS on one warmed engine, each once on the workspace as the kind before left
    it and once more after the workspace was filled with 0xFF bytes (NaN as fp32 / fp64, -1 as int32): outputs and status words
    are bitwise those of the first evaluation of that kind.  The workspace is uninitialised memory by contract (torch.empty,
    dropped at every set_option), so an accumulation into a buffer that nothing defined first shows here;
 4. with each of the rider / preparation switches off, one at a time, the outputs are bitwise the default's ("sums_whole": at the
    relative bounds of test_whole_cell_sums_agree_with_the_sliced_ones; "energy_rides" where the whole sums apply: against the
    sliced sums, as test_gpu_prep does).  Two switches change the arithmetic by design and are held, in the quantities they touch,
    at the bounds test_gpu_prep.py already has for them, bitwise in the others: "nse_merged" = 0 (build_zbar_kernel reads the
    molecule sums of nse_bwd_reduce instead of forming them per block: the adjoint only - forces 2e-5 relative, stress 2e-6;
    test_molecule_sums_inside_build_zbar_agree_with_the_partial_sum_launch) and "d3_cn_rides" = 0 (the coordination numbers summed
    by a pass over the D3 matrix in slot order instead of per lane in the builder's candidate order: energy 1e-6 eV, forces 1e-5
    relative, stress 1e-7; test_d3_coordination_numbers_riding_on_the_matrix_build).

The cases, and the EvalPlan values each is there to reach (default switches; eval_plan.h).  prep: FS = FusedSmall, Sep = Separate,
SepR = SeparateSetupRider (every periodic case of the switch sweep takes it with prep_fused = 0).  energy / charges are given per kind as E / F / S / FS with O = OwnLaunch, FR = ForceRider, SR =
StressRider and EL = EnergyLaunch, W = Walk.  rev_lookup is None on the default engine up to 1 024 atoms (no layout.xe).

  case                    lr_term       energy (E/F/S/FS)  charges (E/F/S/FS)  nse      prep  remarks
  batch5-simple           SimpleInSr    O / FR             EL / FR             Merged   FS    energy_rides = 0: F takes O
  batch5-dsf9             DsfMatrix     O / FR             EL / FR             Merged   FS    lr = Built
  taxol-none              None          O / FR             EL / FR             Merged   FS
  taxol-dsf9-d3_9         DsfInD3       O / FR             EL / FR             Merged   FS    d3 = LongRange: one matrix
  taxol-dsf12-d3_9        DsfMatrix     O / FR             EL / FR             Merged   FS    lr = Built, d3 = Built: two lists
  taxol-simple-d3         SimpleInSr    O / FR             EL / FR             Merged   FS    d3 = Built
  nse-batch5              SimpleInSr    O / FR             EL / FR             Merged   FS    nq = 2, spin charges
  taxol-lists-simple      SimpleMatrix  O / FR             EL / FR             Merged   Sep   sr, lr = Imported
  taxol-lists-dsf9        DsfMatrix     O / FR             EL / FR             Merged   Sep   sr, lr = Imported
  organic600-simple       SimpleInSr    O / O              EL / EL             Merged   FS    layout.S = 2: no force rider
  pbc96_dsf8_wrapped-dsf  DsfWalk       O / FR / SR / SR   W                   Merged   FS
  pbc2x96_dsf9-dsf        DsfWalk       O / FR / SR / SR   W                   Merged   FS    two cells
  pbc96_dsf15-pbcTTF      DsfWalk       O / FR / SR / SR   W                   Merged   FS    one open axis
  pbc96_dsf15-none        None          O / FR / O / O     EL / FR / EL / EL   Merged   FS    stress without a walk
  pbc96-ewald             EwaldWalk     O / FR / SR / SR   W                   Merged   FS    ewald_recip<GRAD, STRESS>
  pbc96-pme               PmeWalk       O / FR / SR / SR   W                   Merged   FS    pme_recip<GRAD, STRESS>
  d3cell-12-12            DsfInD3       O / FR / O / O     EL / FR / EL / EL   Merged   FS    d3 = Built (no lr list on a cell): no walk
  d3cell-10-13            DsfWalk       O / FR / SR / SR   W                   Merged   FS    d3 = Built beside the walk
  nse-cell                DsfWalk       O / FR / SR / SR   W                   Merged   FS    nq = 2
  pbc96-lists             DsfMatrix     O / FR / O / O     EL / FR / EL / EL   Merged   Sep   sr, lr = Imported, shifts; stress
  glucose1152             DsfWalk       O / O / SR / SR    W                   Sliced   FS    layout.xe by N > split_max: rev_lookup None
                                                                                              (E, S) / OnWalk (F, FS); FS: the gather
                                                                                              rides, whole sums; once more with
                                                                                              prep_fused = 0 (SepR, status RiderOwned)
  big-xe1 / big-xe0 (engines of this module, split_max = 0, conv_xe = 1 / 0) repeat the periodic DSF, "none", D3 and taxol /
  batch5 cases on the one-wave-per-atom kernels.  xe1: layout.xe on every gradient request - S: pair buffer written by the pass > 0
  conv backward, never gathered (rev_lookup None), pass 0 in the combined form; F: launch_pair_force alone, energy O; FS: the gather
  rides on the virial launch, pass 0 in the XE form, whole sums only where the energies ride too (the walking cells);
  rev_lookup OnWalk (cells with a walk) against OnEnergyLaunch (molecules, "none").  xe0: the combined-adjoint kernels.
  fuzz-3 / 5 / 8 / 12 (test_gpu_fuzz.make_case): two periodic two-channel systems; two periodic systems with D3 at another cutoff
  (two charges); molecules with DSF + D3 at one cutoff (DsfInD3); four small charged molecules with DSF (DsfMatrix).

Measured margins: profiles/request_kinds.md (tests/tools/request_kinds_margins.py collects them from the lines this module prints)."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_gpu_fuzz as Z
import test_gpu_lists as LS
import test_gpu_parity as P
from conftest import CHARGE_ATOL, FORCE_ATOL, FORCE_RTOL, STRESS_ATOL, energy_tol, golden
from oracle import aimnet2_oracle as O

pytestmark = pytest.mark.gpu

KINDS = {"E": dict(forces=False, stress=False), "F": dict(forces=True, stress=False), "S": dict(forces=False, stress=True),
         "FS": dict(forces=True, stress=True)}
ORDERS = (("FS", "E", "S", "F"), ("E", "S", "F", "FS"))
BITWISE_SWITCHES = ("energy_rides", "status_rides", "status_owned", "setup_rides", "prep_fused")
# switches that change the association of a sum by design: the quantities they touch (module docstring, 4.)
ASSOCIATION_SWITCHES = {"nse_merged": ("forces", "stress"), "d3_cn_rides": ("energy", "forces", "stress")}
# ... and the bounds test_gpu_prep.py already holds these two switches to (test_molecule_sums_inside_build_zbar_agree_with_the_partial_
# sum_launch, test_d3_coordination_numbers_riding_on_the_matrix_build), as functions of the default's output
SWITCH_BOUNDS = {
    "nse_merged": {"forces": lambda b: 2e-5 * max(1.0, np.abs(b).max()), "stress": lambda b: 2e-6 * max(1e-2, np.abs(b).max())},
    "d3_cn_rides": {"energy": lambda b: 1e-6, "forces": lambda b: 1e-5 * max(1.0, np.abs(b).max()), "stress": lambda b: 1e-7},
}


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def _case(name, coord, numbers, mol, q, ekw, okw=None, cell=None, pbc=None, mult=None, d3=None, lists=None, gate="parity", sweep=True):
    """ekw: engine keywords (coulomb, dsf_rc ...); okw: the oracle's where they differ; q: molecular charges as the oracle takes them."""
    coord, numbers, mol = np.asarray(coord, np.float32), np.asarray(numbers, np.int64), np.asarray(mol, np.int64)
    q = np.atleast_1d(np.asarray(q, np.float32))
    okw = dict(ekw if okw is None else okw)
    tables = None
    if d3 is not None:
        tables = P._d3()[1]
        okw["dftd3"] = dict(d3, **tables)
    if cell is not None:
        cell = np.asarray(cell, np.float32)
        okw["cell"] = cell
        if pbc is not None:
            okw["pbc"] = np.array(pbc)
    if mult is not None:
        mult = np.broadcast_to(np.atleast_1d(np.asarray(mult, np.float32)), q.shape).copy()
        okw["mult"] = mult
    return SimpleNamespace(name=name, coord=coord, numbers=numbers, mol=mol, q=q, mult=mult, cell=cell, pbc=pbc, ekw=dict(ekw), okw=okw,
                           d3=d3, tables=tables, lists=lists, gate=gate, sweep=sweep, nse=mult is not None,
                           sizes=np.bincount(mol), periodic=cell is not None)


def _from_golden(name, fixture, ekw, **kw):
    g = golden(fixture)
    mol = g["mol_idx"] if "mol_idx" in g.files else np.zeros(len(g["numbers"]), dtype=np.int64)
    return _case(name, g["coord"], g["numbers"], mol, g["charge"], ekw, cell=g["cell"] if "cell" in g.files else None, **kw)


def _dsf_of(fixture):
    g = golden(fixture)
    return dict(coulomb="dsf", dsf_rc=float(g["dsf_rc"]), dsf_alpha=float(g["dsf_alpha"]))


def _taxol_lists(name, ekw, rc_lr):
    g = golden("taxol")
    n = len(g["numbers"])
    mol = np.zeros(n, dtype=np.int64)
    nb, _ = O.neighbor_list(g["coord"], 5.0, mol)
    nbl, _ = O.neighbor_list(g["coord"], rc_lr, mol)
    return _from_golden(name, "taxol", ekw, lists=dict(nbmat=torch.from_numpy(nb[:n]), nbmat_lr=torch.from_numpy(nbl[:n])))


def _pbc96_lists():
    """As test_gpu_lists.test_periodic_cell_with_caller_lists_and_unwrapped_coordinates: the matrices belong to the wrapped coordinates."""
    g = golden("pbc96_dsf8_wrapped")
    xw = O.wrap_into_cell(g["coord"].astype(np.float64), g["cell"].astype(np.float64), np.zeros(96, dtype=np.int64),
                          np.ones(3, bool)).astype(np.float32)
    nb, sh, nbl, shl = LS._periodic_lists(g, xw, 8.0)
    lists = dict(nbmat=torch.from_numpy(nb[:96]), shifts=torch.from_numpy(sh[:96].astype(np.int32)),
                 nbmat_lr=torch.from_numpy(nbl[:96]), shifts_lr=torch.from_numpy(shl[:96].astype(np.int32)))
    return _case("pbc96-lists", xw, g["numbers"], np.zeros(96, np.int64), g["charge"], _dsf_of("pbc96_dsf8_wrapped"), cell=g["cell"],
                 lists=lists)


def _d3_cell(name, rc_d3, rc_dsf):
    g = golden("dftd3")
    return _case(name, g["pbc_coord"], g["pbc_numbers"], np.zeros(96, np.int64), 0.0, dict(coulomb="dsf", dsf_rc=rc_dsf),
                 cell=g["pbc_cell"], d3=P._d3(rc_d3)[0])


def _nse_batch5():
    g = golden("nse")
    return _case("nse-batch5", g["b5_coord"], g["b5_numbers"], g["b5_mol_idx"], g["b5_charge"], dict(coulomb="simple"), mult=g["b5_mult"])


def _nse_cell():
    g = golden("nse")
    return _case("nse-cell", g["pbc_coord"], g["pbc_numbers"], np.zeros(96, np.int64), 0.0,
                 dict(coulomb="dsf", dsf_rc=float(g["pbc_dsf_rc"])), cell=g["pbc_cell"], mult=g["pbc_mult"])


def _organic600():
    from aimnetcentral_amd import workloads

    # (a blob this dense is hot - max|F| 2 400 eV/A, the fp32 oracle 2.6e-2 eV from the fp64 one - so its energy gate is mostly the
    # oracle's own distance; what it is here for are the two slices of the molecule sums and everything relative: forces, charges,
    # bitwise agreement of the kinds.  profiles/request_kinds.md has the figures of a calmer blob.)
    c, z = workloads.random_organic(600, np.random.default_rng(17))
    return _case("organic600-simple", c, z, np.zeros(600, np.int64), 0.0, dict(coulomb="simple"))


def _glucose1152():
    from aimnetcentral_amd import workloads

    c, z, cell = workloads.glucose_supercell((2, 2, 3))
    c = c + np.random.default_rng(3).normal(scale=0.02, size=c.shape)
    return _case("glucose1152", c, z, np.zeros(len(z), np.int64), 0.0, dict(coulomb="dsf", dsf_rc=8.0), cell=cell, sweep=False)


def _fuzz(seed):
    c, z, mol, q, mult, nse, kw, okw, d3, label = Z.make_case(seed)
    ekw = {k: v for k, v in kw.items() if k not in ("cell", "pbc", "stress")}
    case = _case(f"fuzz-{seed}", c, z, mol, q, ekw, cell=kw.get("cell"), pbc=kw.get("pbc"), mult=mult if nse else None, d3=d3, gate="fuzz")
    case.label = label
    return case


# (built lazily: golden files are read inside the tests, not at collection)
BUILDERS = {
    "batch5-simple": lambda: _from_golden("batch5-simple", "batch5", dict(coulomb="simple")),
    "batch5-dsf9": lambda: _from_golden("batch5-dsf9", "batch5", dict(coulomb="dsf", dsf_rc=9.0)),
    "taxol-none": lambda: _from_golden("taxol-none", "taxol", dict(coulomb="none")),
    "taxol-dsf9-d3_9": lambda: _from_golden("taxol-dsf9-d3_9", "taxol", dict(coulomb="dsf", dsf_rc=9.0), d3=P._d3(9.0, 0.25)[0]),
    "taxol-dsf12-d3_9": lambda: _from_golden("taxol-dsf12-d3_9", "taxol", dict(coulomb="dsf", dsf_rc=12.0), d3=P._d3(9.0, 0.25)[0]),
    "taxol-simple-d3": lambda: _from_golden("taxol-simple-d3", "taxol", dict(coulomb="simple"), d3=P._d3()[0]),
    "nse-batch5": _nse_batch5,
    "taxol-lists-simple": lambda: _taxol_lists("taxol-lists-simple", dict(coulomb="simple"), float("inf")),
    "taxol-lists-dsf9": lambda: _taxol_lists("taxol-lists-dsf9", dict(coulomb="dsf", dsf_rc=9.0), 9.0),
    "organic600-simple": _organic600,
    "pbc96_dsf8_wrapped-dsf": lambda: _from_golden("pbc96_dsf8_wrapped-dsf", "pbc96_dsf8_wrapped", _dsf_of("pbc96_dsf8_wrapped")),
    "pbc2x96_dsf9-dsf": lambda: _from_golden("pbc2x96_dsf9-dsf", "pbc2x96_dsf9", _dsf_of("pbc2x96_dsf9")),
    "pbc96_dsf15-pbcTTF": lambda: _from_golden("pbc96_dsf15-pbcTTF", "pbc96_dsf15", _dsf_of("pbc96_dsf15"), pbc=(True, True, False)),
    "pbc96_dsf15-none": lambda: _from_golden("pbc96_dsf15-none", "pbc96_dsf15", dict(coulomb="none")),
    "pbc96-ewald": lambda: _from_golden("pbc96-ewald", "pbc96_dsf15", dict(coulomb="ewald", ewald_accuracy=1e-6), gate="ewald"),
    "pbc96-pme": lambda: _from_golden("pbc96-pme", "pbc96_dsf15", dict(coulomb="pme", ewald_accuracy=1e-6),
                                      okw=dict(coulomb="ewald", ewald_accuracy=1e-6), gate="ewald"),
    "d3cell-12-12": lambda: _d3_cell("d3cell-12-12", 12.0, 12.0),
    "d3cell-10-13": lambda: _d3_cell("d3cell-10-13", 10.0, 13.0),
    "nse-cell": _nse_cell,
    "pbc96-lists": _pbc96_lists,
    "glucose1152": _glucose1152,
    "fuzz-3": lambda: _fuzz(3),
    "fuzz-5": lambda: _fuzz(5),
    "fuzz-8": lambda: _fuzz(8),
    "fuzz-12": lambda: _fuzz(12),
}
# the cases repeated on the one-wave-per-atom kernels (split_max = 0), reverse-pair form on and off
BIG_CASES = ("pbc96_dsf8_wrapped-dsf", "pbc2x96_dsf9-dsf", "pbc96_dsf15-none", "d3cell-12-12", "d3cell-10-13", "taxol-none",
             "taxol-dsf9-d3_9", "taxol-dsf12-d3_9", "taxol-simple-d3", "batch5-simple", "batch5-dsf9")
RUNS = [("default", c) for c in BUILDERS] + [(v, c) for v in ("big-xe1", "big-xe0") for c in BIG_CASES]
_IDS = [f"{v}/{c}" for v, c in RUNS]

_cases: dict = {}
_refs: dict = {}


def get_case(cid):
    if cid not in _cases:
        _cases[cid] = BUILDERS[cid]()
    return _cases[cid]


def get_ref(case, orc32, orc64):
    """(fp32 oracle with forces, and stress where periodic; fp64 oracle, energy only) of a case: computed once, shared, never changed."""
    if case.name not in _refs:
        okw = dict(case.okw)
        fuzz = case.gate == "fuzz"
        args = lambda: (case.coord.copy(), case.numbers.copy(), case.q.copy(), case.mol.copy())  # noqa: E731  (the oracle may hand its inputs back)
        ref = O.evaluate(orc32, *args(), stress=case.periodic, return_intermediates=fuzz, **okw)
        ref64 = O.evaluate(orc64, *args(), forces=False, stress=False, return_intermediates=fuzz, **okw)
        for r in (ref, ref64):
            for v in r.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _refs[case.name] = (ref, ref64)
    return _refs[case.name]


# ---- engines ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_engines():
    """Engines of this module on the large-system kernels (split_max = 0: one wave per atom on every fixture), with the reverse-pair
    form of the conv backward (layout.xe on every gradient request) and with the combined-adjoint kernels."""
    from aimnetcentral_amd import loader
    from aimnetcentral_amd.engine import HipEngine

    out = {}
    for name, xe in (("big-xe1", 1), ("big-xe0", 0)):
        eng = HipEngine(loader.synthetic_spec(0), "cuda:0")
        eng.set_option("split_max", 0)
        eng.set_option("conv_xe", xe)
        out[name] = eng
    return out


@pytest.fixture()
def pick(request, hip_engine, hip_engine_nse, oracle32, oracle32_nse, oracle64, oracle64_nse):
    """(variant, case id) -> (engine, case, fp32 reference, fp64 reference)."""
    def go(variant, cid):
        case = get_case(cid)
        if variant == "default":
            eng = hip_engine_nse if case.nse else hip_engine
        else:
            eng = request.getfixturevalue("big_engines")[variant]
        ref, ref64 = get_ref(case, *((oracle32_nse, oracle64_nse) if case.nse else (oracle32, oracle64)))
        if case.tables is not None:
            eng.set_dftd3_tables(case.tables)
        return eng, case, ref, ref64

    return go


def kinds_of(case):
    return ("E", "F", "S", "FS") if case.periodic else ("E", "F")


def evaluate(eng, case, kind, coord=None):
    """One HipEngine.eval of `kind`: (outputs as numpy arrays, copy of the status words).  A device error ends the session - nothing more
    is started on a GPU that has faulted."""
    dev = eng.device
    charge = P._nse_charge(case.q, case.mult) if case.nse else case.q
    kw = dict(case.ekw, **KINDS[kind])
    if case.periodic:
        kw["cell"] = torch.from_numpy(case.cell).to(dev)
        if case.pbc is not None:
            kw["pbc"] = case.pbc
    if case.lists:
        kw.update(case.lists)
    try:
        r = eng.eval(torch.from_numpy(case.coord if coord is None else coord).to(dev), torch.from_numpy(case.numbers).to(dev),
                     torch.from_numpy(case.mol).to(dev), torch.from_numpy(charge).to(dev), dftd3=case.d3, **kw)
        res = {k: v.cpu().numpy() for k, v in r.items()}
    except RuntimeError as exc:  # (HipLibraryError is one)
        if any(s in str(exc) for s in ("HIP error", "hipError", "illegal memory", "kernel launch failed", "code -2")):
            pytest.exit(f"device error in {case.name} [{kind}]: {exc}", returncode=3)
        raise
    return res, np.array(eng.last_status).copy()


def expected_keys(case, kind):
    keys = {"energy", "charges"}
    if case.nse:
        keys.add("spin_charges")
    if KINDS[kind]["forces"]:
        keys.add("forces")
    if KINDS[kind]["stress"]:
        keys.add("stress")
    return keys


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


class Problems(list):
    """Collects the failed checks of one test, so that one run reports all of them."""

    def check(self, ok, what):
        if not ok:
            self.append(what)

    def run(self, fn, *a, **kw):
        try:
            fn(*a, **kw)
        except AssertionError as exc:
            self.append(str(exc).splitlines()[0] if str(exc) else repr(exc))

    def done(self):
        assert not self, f"{len(self)} check(s) failed:\n  " + "\n  ".join(self)


# ---- assertion 1: the gates ---------------------------------------------------------------------------------------------------------
def fractions(case, res, ref, ref64, energy=None):
    """Measured error as a fraction of each gate (the same formulas as the gates; for the record in profiles/request_kinds.md)."""
    e = res["energy"] if energy is None else energy
    if case.gate == "fuzz":
        d = (ref["_e_atom"][: len(case.mol)].astype(np.float64) - ref64["_e_atom"][: len(case.mol)]) ** 2
        walk = np.zeros(len(case.sizes))
        np.add.at(walk, case.mol, d)
        gate = energy_tol(case.sizes) + np.abs(ref["energy"] - ref64["energy"]) + 3.0 * np.sqrt(walk)
        out = {"energy": float((np.abs(e - ref64["energy"]) / gate).max())}
    else:
        gate = energy_tol(case.sizes) + np.abs(np.asarray(ref["energy"]) - ref64["energy"])
        out = {"energy": float((np.abs(e - ref["energy"]) / gate).max())}
    dq = np.abs(res["charges"] - ref["charges"]).max()
    if case.nse:
        dq = max(dq, np.abs(res["spin_charges"] - ref["spin_charges"]).max())
    out["charge"] = float(dq / CHARGE_ATOL)
    if "forces" in res:
        f = np.asarray(ref["forces"], np.float64)
        out["force"] = float(np.abs(res["forces"] - f).max() / (FORCE_ATOL + FORCE_RTOL * np.abs(f).max()))
    if "stress" in res:
        out["stress"] = float(np.abs(res["stress"] - ref["stress"]).max() / STRESS_ATOL)
    return out


def gate(case, kind, res, ref, ref64, what, borrowed_forces=None, energy=None):
    """Assertion 1 for one kind."""
    assert set(res) == expected_keys(case, kind), f"{what}: keys {sorted(res)}"
    if case.gate == "fuzz":
        # test_gpu_fuzz._compare reads res["forces"] whatever was asked for: the kinds without forces lend the F kind's (held by its own call)
        shown = res if "forces" in res else dict(res, forces=borrowed_forces)
        Z._compare(shown, ref, ref64, case.mol, what, case.nse, energy)
        return
    (P._compare_nse if case.nse else P.compare)(res, ref, case.sizes, what, ref64["energy"])
    if case.gate == "ewald":  # test_gpu_ewald.test_cell_vs_oracle / test_gpu_pme.test_cell_vs_exact_ewald_oracle
        assert abs(res["energy"][0] - ref64["energy"][0]) <= energy_tol(case.sizes) + abs(ref["energy"][0] - ref64["energy"][0]), what


def first_pass(eng, case, ref, ref64, tag, prob):
    """Every admissible kind once (after one evaluation of the fullest kind has settled the row capacities): assertion 1."""
    kinds = kinds_of(case)
    evaluate(eng, case, kinds[-1])
    out = {}
    for kind in ("F",) + tuple(k for k in kinds if k != "F"):
        what = f"{tag} [{kind}]"
        res, st = evaluate(eng, case, kind)
        energy = None
        if case.gate == "fuzz" and case.periodic:
            # test_gpu_fuzz.test_random_configuration: the energy gate is applied to the evaluation that starts from the oracle's wrapped
            # coordinates, and the raw-coordinate evaluation agrees with it within the wrap's sensitivity
            energy = evaluate(eng, case, kind, ref["coord_wrapped"].astype(np.float32))[0]["energy"]
            f2 = np.zeros(len(energy))
            np.add.at(f2, case.mol, (ref["forces"].astype(np.float64) ** 2).sum(-1))
            prob.check((np.abs(res["energy"] - energy) <= 4.0 * np.sqrt(f2) * 2e-6 + energy_tol(case.sizes)).all(), f"{what}: raw against wrapped energy")
        prob.run(gate, case, kind, res, ref, ref64, what, out["F"][0]["forces"] if "F" in out else None, energy)
        fr = fractions(case, res, ref, ref64, energy)
        print(f"request-kinds margin | {tag} | {kind} | " + " | ".join(f"{k} {fr[k]:.3f}" if k in fr else f"{k} -" for k in ("energy", "force", "stress", "charge")))
        out[kind] = (res, st)
    return out


# ---- assertion 2: across the kinds ----------------------------------------------------------------------------------------------------
def plan_facts(eng, case):
    """What eval_plan.h decides for the FS request of this case, from the engine's own switches: (pair_force_rides, whole).
    pair_force_rides: the reverse-pair map exists (layout.xe: conv_xe, N above the engine's split_max) and its force gather rides on
    the virial launch of a cell.  whole: an energy rider sits beside that gather (EnergySum::StressRider - a walk ran) and
    "sums_whole" is on, so launch_finalize takes the one-block sums (up to 16 384 atoms)."""
    from aimnetcentral_amd.engine import same_cutoff

    n = len(case.mol)
    rides = case.periodic and eng.get_option("conv_xe") == 1 and n > eng.get_option("split_max")
    coulomb = case.ekw["coulomb"]
    in_d3 = coulomb == "dsf" and case.d3 is not None and same_cutoff(case.d3.get("cutoff", 15.0), case.ekw.get("dsf_rc", 15.0))
    walk = case.periodic and not case.lists and coulomb in ("dsf", "ewald", "pme") and not in_d3
    whole = rides and walk and eng.get_option("energy_rides") == 1 and eng.get_option("sums_whole") == 1 and n <= 16384
    return rides, whole


def across_kinds(eng, case, out, tag, prob):
    rides, whole = plan_facts(eng, case)
    base = out["E"][0]
    for kind, (res, _) in out.items():
        for key in ("energy", "charges", "spin_charges"):
            if key not in base:
                continue
            if key == "energy" and kind == "FS" and whole:  # energy_whole_block against energy_partial_block
                prob.check((np.abs(res[key] - base[key]) <= energy_tol(case.sizes)).all(), f"{tag}: energy of FS (whole sums) against E")
                print(f"request-kinds pair | {tag} | energy FS (whole sums) - E | {np.abs(res[key] - base[key]).max():.3e}")
                continue
            prob.check(bits_equal(res[key], base[key]), f"{tag}: {key} of {kind} differs from E by {np.abs(res[key] - base[key]).max():.3e}")
    if "FS" not in out:
        return
    d = np.abs(out["F"][0]["forces"] - out["FS"][0]["forces"]).max()
    prob.check(bits_equal(out["F"][0]["forces"], out["FS"][0]["forces"]), f"{tag}: forces of F and FS differ by {d:.3e}")
    d = np.abs(out["S"][0]["stress"] - out["FS"][0]["stress"]).max()
    if not rides:
        prob.check(bits_equal(out["S"][0]["stress"], out["FS"][0]["stress"]), f"{tag}: stress of S and FS differ by {d:.3e}")
        return
    # conv_bwd_p0_kernel<STRESS, XE = true> (FS) against <STRESS, XE = false> (S), and the whole-cell virial sum where `whole`
    prob.check(d <= STRESS_ATOL, f"{tag}: stress of S and FS (pass-0 pair forms{', whole sums' if whole else ''}) differ by {d:.3e}")
    print(f"request-kinds pair | {tag} | stress FS - S: pass-0 XE / combined form{' + whole sums' if whole else ''} | {d:.3e}")
    # ... and those two are all that differs: with pass 0 on the generic kernel (no pair buffer in pass 0 for either kind) and the
    # sliced sums, stress alone has the bits of forces + stress, and the energies agree again
    off = with_switch(eng, "p0_moments", lambda: with_switch(eng, "sums_whole", lambda: {k: evaluate(eng, case, k)[0] for k in ("E", "S", "FS")}))
    d = np.abs(off["S"]["stress"] - off["FS"]["stress"]).max()
    prob.check(bits_equal(off["S"]["stress"], off["FS"]["stress"]), f"{tag}: p0_moments = sums_whole = 0: stress of S and FS differ by {d:.3e}")
    for kind in ("S", "FS"):
        prob.check(bits_equal(off[kind]["energy"], off["E"]["energy"]), f"{tag}: p0_moments = sums_whole = 0: energy of {kind} differs from E")


# ---- assertion 3: order and workspace contents ------------------------------------------------------------------------------------------
def same_as(case, kind, got, want, what, prob):
    res, st = got
    for key in want[0]:
        if not bits_equal(res[key], want[0][key]):
            bad = ~np.isfinite(res[key])
            prob.append(f"{what}: {key} differs by {np.nanmax(np.abs(res[key] - want[0][key])):.3e}, {int(bad.sum())} non-finite")
    prob.check(np.array_equal(st, want[1]), f"{what}: status {st.tolist()} against {want[1].tolist()}")


def orders_and_poison(eng, case, out, tag, prob):
    for order in ORDERS:
        for kind in order:
            if kind not in out:
                continue
            what = f"{tag} [{kind} in {'-'.join(order)}]"
            same_as(case, kind, evaluate(eng, case, kind), out[kind], what + " after the kind before", prob)
            eng._ws.fill_(0xFF)  # the workspace has its final size for this kind now: NaN in every float, -1 in every int
            same_as(case, kind, evaluate(eng, case, kind), out[kind], what + " on a 0xFF workspace", prob)


@pytest.mark.parametrize("variant,cid", RUNS, ids=_IDS)
def test_kinds_meet_the_gates_agree_and_do_not_depend_on_the_workspace(pick, variant, cid):
    """Assertions 1 - 3 of the module docstring.  The poisoned evaluations run only after every kind has met its gates."""
    eng, case, ref, ref64 = pick(variant, cid)
    tag = f"{variant}/{cid}"
    prob = Problems()
    if not case.periodic:
        with pytest.raises(RuntimeError, match="stress requires a cell"):
            evaluate(eng, case, "S")
    out = first_pass(eng, case, ref, ref64, tag, prob)
    across_kinds(eng, case, out, tag, prob)
    prob.done()
    orders_and_poison(eng, case, out, tag, prob)
    if not case.sweep:  # no switch sweep at this size; the separate preparation kernels (SeparateSetupRider, status RiderOwned) run here
        off = with_switch(eng, "prep_fused", lambda: {k: evaluate(eng, case, k)[0] for k in out})
        for kind in out:
            for key, v in off[kind].items():
                prob.check(bits_equal(v, out[kind][0][key]), f"{tag} [{kind}] prep_fused = 0: {key}")
    prob.done()


# ---- assertion 4: the switches ----------------------------------------------------------------------------------------------------------
def with_switch(eng, option, fn):
    eng.set_option(option, 0)
    try:
        return fn()
    finally:
        eng.set_option(option, 1)


@pytest.mark.parametrize("variant,cid", [r for r in RUNS if r[1] != "glucose1152"], ids=[i for i in _IDS if not i.endswith("glucose1152")])
def test_rider_and_preparation_switches_change_nothing_in_any_kind(pick, variant, cid):
    """Assertion 4 of the module docstring."""
    eng, case, ref, ref64 = pick(variant, cid)
    tag = f"{variant}/{cid}"
    prob = Problems()
    kinds = kinds_of(case)
    evaluate(eng, case, kinds[-1])  # settles the row capacities
    def run_all():
        return {k: evaluate(eng, case, k)[0] for k in kinds}

    base = run_all()
    whole = plan_facts(eng, case)[1]
    sliced = with_switch(eng, "sums_whole", run_all)
    for option in BITWISE_SWITCHES + tuple(ASSOCIATION_SWITCHES):
        if option == "energy_rides" and whole:
            # without the energy riders nothing takes the whole sums: the bitwise claim is about the sliced sums, as in
            # test_gpu_prep.test_energy_sums_riding_on_the_stress_launches_bitwise
            off, base_o = with_switch(eng, "sums_whole", lambda: with_switch(eng, option, run_all)), sliced
        else:
            off, base_o = with_switch(eng, option, run_all), base
        loose = ASSOCIATION_SWITCHES.get(option, ())
        for kind in kinds:
            assert set(off[kind]) == set(base_o[kind])
            for key, a in off[kind].items():
                b = base_o[kind][key]
                if key not in loose or bits_equal(a, b):
                    prob.check(bits_equal(a, b), f"{tag} [{kind}] {option} = 0: {key} differs by {np.abs(a - b).max():.3e}")
                    continue
                d = np.abs(a.astype(np.float64) - b).max()
                tol = SWITCH_BOUNDS[option][key](b)
                print(f"request-kinds switch | {tag} | {kind} | {option} | {key} | {d:.3e} | {d / tol:.3f}")
                prob.check(d <= tol, f"{tag} [{kind}] {option} = 0: {key} differs by {d:.3e} > {tol:.1e}")
    # "sums_whole": another association of the fp64 sums (test_gpu_prep.test_whole_cell_sums_agree_with_the_sliced_ones)
    for kind in kinds:
        a, b = sliced[kind], base[kind]
        for key in a:
            if key == "energy":
                prob.check(np.abs(a[key] - b[key]).max() <= 1e-13 * np.abs(b[key]).max(), f"{tag} [{kind}] sums_whole = 0: energy")
            elif key == "stress":
                prob.check(np.abs(a[key] - b[key]).max() <= 3e-7 * np.abs(b[key]).max(), f"{tag} [{kind}] sums_whole = 0: stress")
            else:
                prob.check(bits_equal(a[key], b[key]), f"{tag} [{kind}] sums_whole = 0: {key}")
    prob.done()
