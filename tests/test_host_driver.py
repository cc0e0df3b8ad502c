"""The host driver of an evaluation - HipEngine.eval, hvp and check_deferred: which capacities they send, how they grow and shrink
them from the status words, the fp16-range fallback, the deferred bookkeeping - run on the CPU against a scripted stand-in for
libaimnet_hip.so.  The stand-in answers every aimnet_engine_eval / aimnet_engine_hvp with the next scripted status words (and finite
or NaN energies), written through the addresses it is handed, and records the options of every call.  The tensors are CPU tensors:
`data_ptr()` is a host address, `.cpu()` is the tensor itself.  Only attributes and methods of the public driver surface are used."""
from __future__ import annotations

import contextlib
import ctypes as C
import types
import warnings

import numpy as np
import pytest
import torch

from aimnetcentral_amd import _lib
from aimnetcentral_amd import engine as E

CLEAN_ROW = 100  # longest short-range row of an unscripted answer: 112 and 176 both keep their size (100 >= 0.5 * 176)


class ScriptedLib:
    def __init__(self, script=()):
        self.script = list(script)  # per call: (status words, energies finite?)
        self.options = {"gemm_h2": 1, "gemm_presplit": 1, "dsf_np_walk": 1}
        self.calls: list[dict] = []  # the numeric fields of every EvalOptions handed to eval / hvp (+ "k" for hvp)

    def aimnet_engine_workspace_bytes(self, h, n, n_mol, n_cell, opt):
        return 4096

    def aimnet_engine_hvp_workspace_bytes(self, h, n, n_mol, k, opt):
        return 1000 + 100 * k  # 100 B per direction

    def aimnet_engine_get_option(self, h, name, value):
        value._obj.value = self.options[name.decode()]
        return 0

    def aimnet_engine_set_option(self, h, name, value):
        self.options[name.decode()] = int(value)
        return 0

    def _answer(self, opt, status_ptr, **extra):
        self.calls.append({name: getattr(opt._obj, name) for name, _ in _lib.EvalOptions._fields_} | extra)
        status, finite = self.script.pop(0) if self.script else ([CLEAN_ROW, 0, 0, 0, 0, 0, 0, 0], True)
        C.memmove(status_ptr, (C.c_int32 * 8)(*status), 32)
        return finite

    def aimnet_engine_eval(self, h, inp, opt, out, ws, ws_bytes, stream):
        finite = self._answer(opt, out._obj.status)
        n_mol = inp._obj.n_mol
        C.memmove(out._obj.energy, (C.c_double * n_mol)(*([1.0 if finite else float("nan")] * n_mol)), 8 * n_mol)
        return 0

    def aimnet_engine_hvp(self, h, inp, opt, vectors, k, hv, forces, status, ws, ws_bytes, stream):
        self._answer(opt, status, k=int(k))
        return 0

    def aimnet_engine_charge_response_workspace_bytes(self, h, n, n_mol, k, opt):
        return 500 + 50 * k  # 50 B per direction

    def aimnet_engine_charge_response(self, h, inp, opt, vectors, k, charges, dq, dspin, dmu, status, ws, ws_bytes, stream):
        self._answer(opt, status, k=int(k), dspin=dspin is not None, dmu=dmu is not None)
        return 0

    def sent(self, field):
        return [c[field] for c in self.calls]


@pytest.fixture(autouse=True)
def _no_gpu(monkeypatch):
    stream = types.SimpleNamespace(cuda_stream=0, wait_stream=lambda other: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: stream)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())


def make_engine(lib, nq=1):
    """What HipEngine.__init__ leaves behind, without a library handle or a GPU."""
    e = object.__new__(E.HipEngine)
    e.spec, e.lib, e.device, e.dev_index, e.nq = types.SimpleNamespace(rc=5.0), lib, torch.device("cpu"), 0, nq
    e._h, e._keep, e._ws, e._ws_stream = None, [], None, None
    e.pending_status, e._pending_energy, e.last_status, e.has_dftd3 = [], [], None, False
    e.max_nb, e._max_nb_lr = 112, {}  # 112 = round16(int(0.2 * 4/3 pi 5^3)) = round16(104)
    e._ewald_nb_lr, e._ewald_max_k, e._pme_max_mesh, e._status7_pme = 0, 8192, 8192, False
    return e


def system(n=10, n_mol=1, periodic=False):
    g = torch.Generator().manual_seed(0)
    per = n // n_mol
    kw = dict(coord=torch.rand(n, 3, generator=g) * 8.0, numbers=torch.full((n,), 6, dtype=torch.int32),
              mol_idx=torch.arange(n_mol, dtype=torch.int32).repeat_interleave(per), charge=torch.zeros(n_mol))
    if periodic:
        kw["cell"] = torch.eye(3) * 10.0
    return kw


def st(s0=CLEAN_ROW, s1=0, s2=0, s3=0, s4=0, s5=0, s6=0, s7=0):
    return [s0, s1, s2, s3, s4, s5, s6, s7]


D3 = {"s8": 0.5, "a1": 0.4, "a2": 4.0}


def test_short_range_overflow_grows_then_a_quiet_call_shrinks():
    lib = ScriptedLib([(st(130, s2=1), True), (st(130), True)])
    eng = make_engine(lib)
    res = eng.eval(**system(), forces=True)
    assert lib.sent("max_nb") == [112, 176]  # round16(max(112 * 1.5, 130)) = round16(168)
    assert eng.max_nb == 176 and list(eng.last_status) == st(130)  # 130 >= 2/3 * 0.75 * 176 = 88: no shrink
    assert set(res) == {"energy", "charges", "forces"} and res["forces"].shape == (10, 3)
    lib.script = [(st(40), True)]
    eng.eval(**system())
    assert lib.sent("max_nb")[2:] == [176] and eng.max_nb == 64  # 40 < 88: max(16, round16(int(40 / 0.75))) = round16(53)


def test_nonperiodic_dsf_and_d3_at_one_cutoff_grow_one_entry():
    lib = ScriptedLib([(st(50, s1=3000, s3=1, s4=3100, s5=1), True), (st(50, s1=3000, s4=3100), True)])
    eng = make_engine(lib)
    eng.has_dftd3 = True
    eng.eval(**system(), coulomb="dsf", dftd3=D3)
    # start: round16(int(0.2 * 4/3 pi 15^3)) = round16(2827) = 2832; round16(max(2832 * 1.5, 3100)) = round16(4248) = 4256
    assert lib.sent("max_nb_lr") == [2832, 4256] and lib.sent("max_nb_d3") == [2832, 4256]
    assert eng._max_nb_lr == {15.0: 4256}  # 3000 and 3100 >= 0.5 * 4256: no shrink
    assert eng.max_nb == 80  # 50 < 2/3 * 0.75 * 112 = 56: round16(int(50 / 0.75)) = round16(66)
    assert lib.sent("dftd3") == [1, 1] and lib.sent("d3_cutoff") == [15.0, 15.0] and lib.sent("d3_smoothing_on") == [12.0, 12.0]
    with pytest.raises(RuntimeError, match="no DFT-D3 tables were uploaded"):
        make_engine(ScriptedLib()).eval(**system(), dftd3=D3)


def test_ewald_k_arrays_and_pme_mesh_grow_to_the_reported_need():
    lib = ScriptedLib([(st(s7=1000), True), (st(s7=1000), True)])
    eng = make_engine(lib)
    eng._ewald_max_k = 64
    eng.eval(**system(periodic=True), coulomb="ewald", stress=True)
    assert lib.sent("ewald_max_k") == [64, 1256] and eng._ewald_max_k == 1256  # (1000 * 5 // 4 + 7) // 8 * 8 = 1257 // 8 * 8
    assert lib.sent("flags") == [2, 2] and np.float32(lib.calls[0]["ewald_accuracy"]) == np.float32(1e-6)
    lib = ScriptedLib([(st(s7=20000), True), (st(s7=20000), True)])
    eng = make_engine(lib)
    eng._pme_max_mesh = 512
    eng.eval(**system(periodic=True), coulomb="pme")
    assert lib.sent("pme_max_mesh") == [512, 22564] and eng._pme_max_mesh == 22564  # 20000 * 9 // 8 + 64
    eng = make_engine(ScriptedLib([(st(s7=2**31 - 1), True)]))
    with pytest.raises(ValueError, match="more than 512 PME mesh points"):
        eng.eval(**system(periodic=True), coulomb="pme")


def test_pme_workspace_limit_shrinks_once_then_refuses():
    lib = ScriptedLib([(st(s7=900_000_000), True)])
    eng = make_engine(lib)
    eng._pme_max_mesh = 10**9  # 2 systems x 1e9 points x 40 B = 8.0e10 > 64 GiB = 6.87e10
    with pytest.raises(ValueError, match="exceeds the PME workspace limit"):
        eng.eval(**system(n_mol=2, periodic=True), coulomb="pme")
    assert lib.sent("pme_max_mesh") == [8192]  # shrunk to the starting capacity once ...
    assert eng._pme_max_mesh == 1_012_500_064  # ... grown to 900 000 000 * 9 // 8 + 64, which is beyond the limit as well


def test_fp16_range_fallback():
    lib = ScriptedLib([(st(), False), (st(), True)])
    eng = make_engine(lib)
    with pytest.warns(RuntimeWarning, match="exceeded fp16's range"):
        eng.eval(**system())
    assert len(lib.calls) == 2 and lib.options["gemm_h2"] == 0
    # non-finite with either operand form: not a range problem, the h2 form comes back and nobody is warned
    lib = ScriptedLib([(st(), False), (st(), False)])
    eng = make_engine(lib)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        eng.eval(**system())
    assert len(lib.calls) == 2 and lib.options["gemm_h2"] == 1
    # together with a row overflow the overflow is handled first (garbage rows also produce NaN)
    lib = ScriptedLib([(st(130, s2=1), False), (st(130), True)])
    eng = make_engine(lib)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        eng.eval(**system())
    assert lib.sent("max_nb") == [112, 176] and lib.options["gemm_h2"] == 1
    # the status bit of the device-side check counts as well (finite energies, non-finite forces), host_out reads every output
    lib = ScriptedLib([(st(s6=E.NONFINITE_FLAG), True), (st(), True)])
    with pytest.warns(RuntimeWarning, match="exceeded fp16's range"):
        res = make_engine(lib).eval(**system(), forces=True, host_out=True)
    assert len(lib.calls) == 2 and lib.options["gemm_h2"] == 0 and float(res["energy"][0]) == 1.0


def test_input_flags_come_first():
    eng = make_engine(ScriptedLib([(st(130, s2=1, s6=4), False)]))
    with pytest.raises(ValueError, match="HipEngine.eval: invalid input: mol_idx is not sorted"):
        eng.eval(**system())
    assert eng.max_nb == 112 and eng.lib.options["gemm_h2"] == 1


def test_caller_supplied_matrices_set_the_capacities():
    lib = ScriptedLib([(st(5, s1=7), True)])
    eng = make_engine(lib)
    nb, nb_lr = torch.full((10, 20), 10, dtype=torch.int32), torch.full((10, 40), 10, dtype=torch.int32)
    eng.eval(**system(), coulomb="dsf", nbmat=nb, nbmat_lr=nb_lr)
    assert lib.sent("max_nb") == [32] and lib.sent("max_nb_lr") == [48]  # round16(20), round16(40)
    assert eng.max_nb == 112 and eng._max_nb_lr.get(15.0, 2832) == 2832  # no growth, no shrink
    with pytest.raises(ValueError, match="HipEngine.eval: shifts given without nbmat"):
        eng.eval(**system(), shifts=torch.zeros(10, 20, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="periodic input needs the shifts of nbmat"):
        eng.eval(**system(periodic=True), coulomb="dsf", nbmat=nb, nbmat_lr=nb_lr)


def test_large_nonperiodic_dsf_sends_no_list_capacity():
    lib = ScriptedLib([(st(s1=2000, s4=2000), True)] * 6)  # (rows long enough to keep every capacity: 2000 >= 0.5 * 2832)
    eng = make_engine(lib)
    eng.has_dftd3 = True
    big = system(n=1500)
    eng.eval(**big, coulomb="dsf")  # 1500 atoms in one molecule: the bounding-box walk, no list
    eng.eval(**system(n=1499), coulomb="dsf")
    eng.eval(**big, coulomb="dsf", dftd3=D3)  # D3 at the same cutoff: the pair terms ride on the D3 list
    eng.eval(**big, coulomb="dsf", dftd3=D3 | {"cutoff": 12.0})
    lib.options["dsf_np_walk"] = 0
    eng.eval(**big, coulomb="dsf")
    eng.eval(**system(n=1500, periodic=True), coulomb="dsf")  # periodic DSF walks the cell grid
    assert lib.sent("max_nb_lr") == [0, 2832, 2832, 0, 2832, 0]
    assert lib.sent("max_nb_d3") == [0, 0, 2832, 1456, 0, 0]  # round16(int(0.2 * 4/3 pi 12^3)) = round16(1447)


def test_deferred_overflow_grows_every_long_range_entry():
    lib = ScriptedLib([(st(), True), (st(s1=3000, s3=1), True), (st(), True)])
    eng = make_engine(lib)
    eng._max_nb_lr[12.0] = 1456
    for _ in range(3):
        res = eng.eval(**system(), coulomb="dsf", sync=False, defer=True)
        assert set(res) == {"energy", "charges", "status"}
    assert len(eng.pending_status) == 3 and lib.sent("max_nb_lr") == [2832] * 3
    with pytest.raises(E.NeighborOverflowError, match="one of the last 3 deferred evaluations"):
        eng.check_deferred()
    # round16(max(2832 * 1.5, 3000, 0)) = 4256; round16(max(1456 * 1.5, 3000, 0)) = round16(3000) = 3008
    assert eng._max_nb_lr == {15.0: 4256, 12.0: 3008} and eng.max_nb == 112
    assert eng.pending_status == [] and list(eng.last_status) == st()
    eng.check_deferred()  # nothing pending: nothing to do


def test_deferred_range_error_and_flags():
    lib = ScriptedLib([(st(), True), (st(), False)])
    eng = make_engine(lib)
    for _ in range(2):
        eng.eval(**system(), sync=False, defer=True)
    with pytest.raises(E.ActivationRangeError, match="one of the last 2 deferred evaluations with fp16x2-split GEMM"):
        eng.check_deferred()
    assert lib.options["gemm_h2"] == 0 and eng.pending_status == [] and eng.max_nb == 112
    eng = make_engine(ScriptedLib([(st(s6=1), True)]))
    eng.eval(**system(), sync=False, defer=True)
    with pytest.raises(ValueError, match="invalid input in a deferred evaluation: atomic numbers outside"):
        eng.check_deferred()
    # status[7] of deferred PME evaluations counts mesh points
    eng = make_engine(ScriptedLib([(st(s7=20000), True)]))
    eng.eval(**system(periodic=True), coulomb="pme", sync=False, defer=True)
    with pytest.raises(E.NeighborOverflowError):
        eng.check_deferred()
    assert eng._pme_max_mesh == 22564 and eng._ewald_max_k == 8192  # 20000 * 9 // 8 + 64


def test_hvp_repeats_an_overflowed_sweep():
    lib = ScriptedLib([(st(), True), (st(130, s2=1), True)])
    eng = make_engine(lib)
    eng.HVP_BYTES_BUDGET = 200  # two directions of 100 B per sweep
    s = system()
    res = eng.hvp(**s, vectors=torch.ones(5, 10, 3), want_forces=True)
    assert lib.sent("k") == [2, 2, 2, 1] and lib.sent("max_nb") == [112, 112, 176, 176]  # round16(112 * 1.5)
    assert set(res) == {"hv", "forces"} and res["hv"].shape == (5, 10, 3) and eng.max_nb == 176  # hvp does not shrink
    with pytest.raises(ValueError, match="does not carry particle-mesh Ewald"):
        eng.hvp(**s, vectors=torch.ones(1, 10, 3), coulomb="pme")
    lib.script = [(st(s6=E.EWALD_LIST_SHORT_FLAG), True)]
    with pytest.raises(ValueError, match="HipEngine.hvp: invalid input: Ewald summation in the tangent sweep"):
        eng.hvp(**s, vectors=torch.ones(1, 10, 3))


def test_hvp_ewald_list_capacity_only_grows():
    # r_c = sqrt(-2 ln 1e-6) (V^2 / N)^(1/6) / sqrt(2 pi) (1 + 1e-5) = 5.2565 * 2.7180 = 14.287 A for 10 atoms in (10 A)^3:
    # round16(int(0.2 * 4/3 pi r_c^3)) = round16(2443) = 2448
    lib = ScriptedLib([(st(s1=5000, s3=1, s7=9000), True)])
    eng = make_engine(lib)
    eng.hvp(**system(periodic=True), vectors=torch.ones(1, 10, 3), coulomb="ewald")
    assert lib.sent("max_nb_lr") == [2448, 5008]  # round16(max(2448 * 1.5, 5000))
    assert lib.sent("ewald_max_k") == [8192, 11256]  # (9000 * 5 // 4 + 7) // 8 * 8
    assert lib.sent("k") == [1, 1] and eng._ewald_nb_lr == 5008 and eng._max_nb_lr == {}
    assert abs(lib.calls[0]["dsf_rc"] - 14.287) < 1e-3
    eng.hvp(**system(periodic=True), vectors=torch.ones(1, 10, 3), coulomb="ewald", ewald_accuracy=1e-3)  # a shorter r_c
    assert lib.sent("max_nb_lr")[2:] == [5008] and eng._ewald_nb_lr == 5008
    # DSF keeps a list per cutoff, periodic or not; with D3 at another cutoff a second one
    eng.has_dftd3 = True
    eng.hvp(**system(periodic=True), vectors=torch.ones(1, 10, 3), coulomb="dsf", dsf_rc=12.0, dftd3=D3)
    assert lib.sent("max_nb_lr")[3:] == [1456] and lib.sent("max_nb_d3")[3:] == [2832] and eng._max_nb_lr == {12.0: 1456, 15.0: 2832}


def test_charge_response_repeats_an_overflowed_sweep():
    lib = ScriptedLib([(st(), True), (st(130, s2=1), True)])
    eng = make_engine(lib)
    eng.HVP_BYTES_BUDGET = 100  # two directions of 50 B per sweep
    s = system()
    res = eng.charge_response(**s, vectors=torch.ones(5, 10, 3))
    assert lib.sent("k") == [2, 2, 2, 1] and lib.sent("max_nb") == [112, 112, 176, 176]  # round16(112 * 1.5)
    assert lib.sent("max_nb_lr") == [0] * 4 and lib.sent("coulomb") == [_lib.COULOMB_NONE] * 4  # the short-range rows are all it needs
    assert lib.sent("dspin") == [False] * 4 and lib.sent("dmu") == [True] * 4  # one channel; no cell: the dipole by default
    assert set(res) == {"charges", "dq", "dmu"} and res["dq"].shape == (5, 10) and res["dmu"].shape == (5, 1, 3)
    assert eng.max_nb == 176 and list(eng.last_status) == st()  # no shrink, as hvp
    lib.script = [(st(s6=4), True)]
    with pytest.raises(ValueError, match="HipEngine.charge_response: invalid input: mol_idx is not sorted"):
        eng.charge_response(**s, vectors=torch.ones(1, 10, 3))
    # the entry's own name in the messages of the input checks
    with pytest.raises(ValueError, match=r"HipEngine.charge_response: a 2-channel \(NSE\) model needs charge of shape"):
        make_engine(ScriptedLib(), nq=2).charge_response(**s, vectors=torch.ones(1, 10, 3))
    with pytest.raises(ValueError, match="HipEngine.charge_response: empty input"):
        eng.charge_response(**system(n=0), vectors=torch.ones(0, 0, 3))


def test_a_budget_of_one_byte_gives_one_call_per_direction():
    for method in ("hvp", "charge_response"):
        lib = ScriptedLib()
        eng = make_engine(lib)
        eng.HVP_BYTES_BUDGET = 1  # less than one direction's bytes (100 B, 50 B): a sweep is never empty
        getattr(eng, method)(**system(), vectors=torch.ones(3, 10, 3))
        assert lib.sent("k") == [1, 1, 1], method
