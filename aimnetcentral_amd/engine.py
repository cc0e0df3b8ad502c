"""HipEngine: thin Python owner of one `aimnet_engine` handle (include/aimnet_hip.h).

PyTorch-ROCm tensors are used purely as device buffers (`data_ptr()`), the HIP stream is torch's
current stream; there is no autograd and no torch compute on the hot path.  One engine per
device; not re-entrant (same contract as the reference calculator, calculator.py:283-328).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Any

import numpy as np

from . import _lib, capacity

_DTYPES = {4: "float32", 8: "float64"}
_INT_VIEWS = {"nb_idx", "nb_shift", "nb_cnt", "lr_idx", "lr_shift", "lr_cnt"}
# "ewald": the exact structure-factor sum (csrc/ewald.hip); "pme": the same splitting with the reciprocal sum on a mesh (csrc/pme.hip)
_METHODS = {"none": _lib.COULOMB_NONE, "simple": _lib.COULOMB_SIMPLE, "dsf": _lib.COULOMB_DSF, "ewald": _lib.COULOMB_EWALD,
            "pme": _lib.COULOMB_PME}
same_cutoff = capacity.same_cutoff  # (its callers take it from here)


@dataclass
class ModelSpec:
    """Architecture + host weights of one AIMNet2 core model (built by loader.py / synth.py)."""

    nfeature: int
    nshifts: int
    ncomb_v: int
    mlp_dims: list[list[int]]          # per pass: [n_in, hidden..., n_out]
    last_linear: list[bool]
    head_dims: list[int]
    rc: float
    eta: float
    shifts: list[float]
    sr_coulomb: bool
    sr_envelope: str
    sr_rc: float
    weights: dict[str, np.ndarray] = field(repr=False, default_factory=dict)  # state-dict keys
    metadata: dict[str, Any] = field(default_factory=dict)
    num_charge_channels: int = 1       # 2 = open-shell NSE family (aimnet2.py:21-28)


class ActivationRangeError(RuntimeError):
    """A DEFERRED evaluation produced non-finite energies while the fp16x2-split GEMM operands were in use: an MLP activation left
    fp16's range (|x| >= 65504, csrc/gemm_h2_common.h).  The engine has switched to the bf16x3 operands; repeat the evaluations
    since the last check (the synchronous path does this by itself)."""


class NeighborOverflowError(RuntimeError):
    """A neighbour row overflowed in a DEFERRED evaluation (the synchronous path retries by itself; nvalchemiops raises the
    exception of this name, neighbors.py:127-130)."""


EWALD_LIST_SHORT_FLAG = 64  # status[6] bit 6 (csrc/kernels.h STATUS_EWALD_LIST_SHORT): aimnet_engine_hvp, list cutoff below an Ewald r_c
EXT_MOL_IDX_FLAG = 128  # status[6] bit 7 (csrc/kernels.h STATUS_EXT_MOL_IDX): embedding, ext_mol_idx out of range or not sorted
NONFINITE_FLAG = 32  # status[6] bit 5 (csrc/kernels.h STATUS_NONFINITE): a non-finite energy or force was written - not an input flag


def describe_input_flags(flags: int, n_mol: int | None = None) -> str:
    """Text of the input sanity flags the engine raises in status[6] (it clamps for memory safety; the results are meaningless)."""
    what = []
    if flags & 1:
        what.append("atomic numbers outside [0, 63] (the embedding has 64 rows, core.py:49)")
    if flags & 2:
        what.append("mol_idx entries outside [0, %s) (n_mol is taken from the charge array)" % ("n_mol" if n_mol is None else n_mol))
    if flags & 4:
        what.append("mol_idx is not sorted (the atoms of a molecule must be contiguous)")
    if flags & 8:
        what.append("a caller-supplied neighbour matrix holds a lattice shift outside +-127 or an unshifted self pair")
    if flags & 16:
        what.append("a caller-supplied neighbour matrix is not a full symmetric matrix (an entry i -> j without exactly one mirror j -> i, "
                    "or a duplicated entry)")
    if flags & EWALD_LIST_SHORT_FLAG:
        what.append("Ewald summation in the tangent sweep: options.dsf_rc (the cutoff of the real-space list) is below a system's "
                    "real-space cutoff")
    if flags & EXT_MOL_IDX_FLAG:
        what.append("embedding: ext_mol_idx entries outside [0, %s) or not sorted (the sites of a molecule must be contiguous)"
                    % ("n_mol" if n_mol is None else n_mol))
    if flags & ~(31 | EWALD_LIST_SHORT_FLAG | EXT_MOL_IDX_FLAG):
        what.append(f"unknown flag bits {flags & ~(31 | EWALD_LIST_SHORT_FLAG | EXT_MOL_IDX_FLAG):#x}")
    return " and ".join(what) if what else "no flags"


class _OutBuffer:
    """Status words + every output of one evaluation in ONE allocation (16-byte aligned sections; the engine zeroes the status)."""

    def __init__(self, sections, device):
        import torch

        self.sections, self.spans, total = sections, [], 0  # (name, dtype, shape) and (offset, bytes) of every section
        for _, dt, shape in sections:
            nb = math.prod(shape) * dt.itemsize
            self.spans.append((total, nb))
            total += (nb + 15) // 16 * 16
        self.buf = torch.empty(total, dtype=torch.uint8, device=device)

    def views(self, buf):
        flat = [buf[o : o + nb].view(dt) for (_, dt, _), (o, nb) in zip(self.sections, self.spans)]  # (1-D sections need no reshape)
        return {name: v.view(shape) if len(shape) > 1 else v for (name, _, shape), v in zip(self.sections, flat)}


class _RangeFallback:
    """fp16x2-split GEMM operands (csrc/gemm_h2_common.h) hold |x| < 65504: an activation beyond that turns into inf / NaN and
    surfaces in the outputs.  `on`: that form is in use; `retrying`: a non-finite call is being repeated on the bf16x3 operands
    (fp32's range) - if THAT is finite the engine stays on them."""

    def __init__(self, eng: "HipEngine"):
        self.eng, self.retrying = eng, False
        self.on = bool(eng.get_option("gemm_h2")) and bool(eng.get_option("gemm_presplit"))

    def repeat(self, finite: bool) -> bool:  # after a synchronous call whose rows all fitted: whether to run it again
        if not finite and self.on:
            self.eng.set_option("gemm_h2", 0)
            self.on, self.retrying = False, True
            return True
        if self.retrying:
            self.retrying = False
            if finite:
                import warnings
                warnings.warn("HipEngine: an MLP activation of this model exceeded fp16's range (|x| >= 65504); the engine has "
                              "switched from the fp16x2-split to the bf16x3-split GEMM operands (set_option('gemm_h2', 0)) for "
                              "this and all later evaluations", RuntimeWarning, stacklevel=3)
            else:  # non-finite with either operand form: not a range problem of the h2 form
                self.eng.set_option("gemm_h2", 1)
        return False

    @staticmethod
    def deferred(eng: "HipEngine", n_evals: int) -> None:  # non-finite deferred results, rows fitted: switch and say so
        if eng.get_option("gemm_h2"):
            eng.set_option("gemm_h2", 0)
            raise ActivationRangeError("non-finite energies or forces in one of the last %d deferred evaluations with fp16x2-split GEMM "
                                       "operands: an activation may have left fp16's range; the engine now uses the bf16x3 operands - "
                                       "repeat them (if they stay non-finite the input itself is the cause)" % n_evals)


class HipEngine(capacity.Capacities):
    def __init__(self, spec: ModelSpec, device: str | int = 0):
        import torch

        self.spec = spec
        self.lib = _lib.load()  # raises HipLibraryError when the .so is missing: no fallback
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("HipEngine needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self.device = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        if self.device.type != "cuda":
            raise _lib.HipLibraryError(f"HipEngine device must be a GPU, got {self.device}")
        self.dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._keep: list[np.ndarray] = []
        arch = _lib.Arch()
        arch.nfeature, arch.nshifts, arch.ncomb_v = spec.nfeature, spec.nshifts, spec.ncomb_v
        arch.n_pass = len(spec.mlp_dims)
        for p, dims in enumerate(spec.mlp_dims):
            arch.n_layers[p] = len(dims) - 1
            for k, d in enumerate(dims):
                arch.layer_dims[p][k] = d
            arch.last_linear[p] = 1 if spec.last_linear[p] else 0
        arch.head_n_layers = len(spec.head_dims) - 1
        for k, d in enumerate(spec.head_dims):
            arch.head_dims[k] = d
        arch.rc, arch.eta = float(spec.rc), float(spec.eta)
        for g, s in enumerate(spec.shifts):
            arch.shifts[g] = float(s)
        arch.sr_coulomb = 1 if spec.sr_coulomb else 0
        arch.sr_envelope = 0 if spec.sr_envelope == "exp" else 1
        arch.sr_rc = float(spec.sr_rc)
        arch.n_charge_channels = self.nq = int(spec.num_charge_channels)

        w = _lib.Weights()
        sd = spec.weights

        def ptr(key: str, dtype=np.float32) -> int:
            a = np.ascontiguousarray(np.asarray(sd[key]), dtype=dtype)
            self._keep.append(a)
            return a.ctypes.data

        w.afv, w.agh_a, w.agh_q = ptr("afv.weight"), ptr("conv_a.agh"), ptr("conv_q.agh")
        for p, dims in enumerate(spec.mlp_dims):
            for layer in range(len(dims) - 1):
                w.mlp_w[p][layer] = ptr(f"mlps.{p}.{2 * layer}.weight")
                w.mlp_b[p][layer] = ptr(f"mlps.{p}.{2 * layer}.bias")
        for layer in range(len(spec.head_dims) - 1):
            w.head_w[layer] = ptr(f"outputs.energy_mlp.mlp.{2 * layer}.weight")
            w.head_b[layer] = ptr(f"outputs.energy_mlp.mlp.{2 * layer}.bias")
        w.sae = ptr("outputs.atomic_shift.shifts.weight", np.float64)
        handle = C.c_void_p()
        _lib.check(self.lib.aimnet_engine_create(C.byref(arch), C.byref(w), self.dev_index, C.byref(handle)), "aimnet_engine_create")
        self._h = handle
        self._keep.clear()  # weights are on the device now
        self._ws = self._ws_stream = None  # the workspace, and the stream of the last launch (the workspace is tied to it)
        self.pending_status: list = []  # status words of evaluations run with sync=False and defer=True (check_deferred)
        self._pending_energy: list = []  # their energies, while the h2 operand form is on (the fp16-range sentinel, check_deferred)
        capacity.Capacities.__init__(self, spec.rc)  # the row, k-array and mesh capacities and every rule that changes them
        self.last_status: np.ndarray | None = None
        self._status7_pme = False  # what status[7] of the pending deferred evaluations counts (mesh points or k entries)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                self.lib.aimnet_engine_destroy(h)
            except Exception:
                pass
            self._h = None

    # ------------------------------------------------------------------------------------------
    def set_option(self, name: str, value: int) -> None:
        """Engine switch for A/B and parity runs; the names and values are listed at aimnet_engine_set_option in
        include/aimnet_hip.h."""
        _lib.check(self.lib.aimnet_engine_set_option(self._h, name.encode(), int(value)), "aimnet_engine_set_option")
        self._ws = None  # the workspace layout depends on the switches

    def get_option(self, name: str) -> int:
        """Current value of an engine switch (aimnet_engine_get_option)."""
        v = C.c_int(0)
        _lib.check(self.lib.aimnet_engine_get_option(self._h, name.encode(), C.byref(v)), "aimnet_engine_get_option")
        return int(v.value)

    def set_dftd3_tables(self, tables: dict[str, Any]) -> None:
        """Upload the DFT-D3 reference tables (what DFTD3.__init__ reads from aimnet/dftd3_data.pt, lr.py:1405-1423):
        `c6ab`, `cn_ref` [Z,Z,5,5] and `rcov`, `r4r2` [Z] (see loader.load_dftd3_tables)."""
        arrs = {k: np.ascontiguousarray(np.asarray(tables[k]), dtype=np.float32) for k in ("c6ab", "cn_ref", "rcov", "r4r2")}
        nz = arrs["rcov"].shape[0]
        if arrs["c6ab"].shape != (nz, nz, 5, 5) or arrs["cn_ref"].shape != (nz, nz, 5, 5) or arrs["r4r2"].shape != (nz,):
            raise ValueError("DFT-D3 tables must be c6ab/cn_ref [Z,Z,5,5] and rcov/r4r2 [Z]")
        t = _lib.DftD3Tables()
        t.n_z = nz
        t.c6ab, t.cn_ref, t.rcov, t.r4r2 = (arrs[k].ctypes.data for k in ("c6ab", "cn_ref", "rcov", "r4r2"))
        _lib.check(self.lib.aimnet_engine_set_dftd3(self._h, C.byref(t)), "aimnet_engine_set_dftd3")
        self.has_dftd3 = True

    def check_deferred(self) -> None:
        """Synchronise once and verify the status words of every evaluation run with `sync=False, defer=True` since the last
        check: a device-resident MD driver calls this every K steps instead of paying one host read per step.  On a neighbour
        overflow the row capacity is grown (x1.5, as the synchronous path does) and NeighborOverflowError is raised - the
        evaluations since the last check are invalid and have to be repeated."""
        import torch

        if not self.pending_status:
            return
        st = torch.stack(self.pending_status).cpu().numpy()
        self.pending_status.clear()
        self.last_status = st[-1]
        energies, self._pending_energy = self._pending_energy, []
        if (st[:, 6] & ~NONFINITE_FLAG).any():  # (first: invalid input also produces non-finite outputs)
            raise ValueError("HipEngine: invalid input in a deferred evaluation: " +
                             describe_input_flags(int(np.bitwise_or.reduce(st[:, 6])) & ~NONFINITE_FLAG))
        rows_ok = not (st[:, 2].any() or st[:, 3].any() or st[:, 5].any())
        # (status[6] bit 5 covers the adjoint sweep too, which the energies alone would not)
        if rows_ok and (bool((st[:, 6] & NONFINITE_FLAG).any()) or not all(bool(torch.isfinite(e).all()) for e in energies)):
            _RangeFallback.deferred(self, len(st))
        if self.grow_deferred(st, self._status7_pme):
            raise NeighborOverflowError("neighbour-row overflow in one of the last %d deferred evaluations: their results are invalid; "
                                        "the row capacity has been grown - repeat them" % len(st))

    def _inputs(self, who: str, coord, numbers, mol_idx, charge, cell, pbc):
        """Device tensors of the right dtype and layout for `eval` / `hvp` / `charge_response` (`who`, for the messages): the filled
        aimnet_inputs and the tensors it points into (keep them alive for as long as it is used)."""
        import torch

        dev = self.device
        t = {"coord": coord.to(device=dev, dtype=torch.float32).contiguous(), "numbers": numbers.to(device=dev, dtype=torch.int32).contiguous(),
             "mol_idx": mol_idx.to(device=dev, dtype=torch.int32).contiguous(), "cell": None, "pbc_sys": None}
        charge = charge.to(device=dev, dtype=torch.float32)
        if self.nq == 2:
            if charge.ndim != 2 or charge.shape[1] != 2:
                raise ValueError(f"HipEngine.{who}: a 2-channel (NSE) model needs charge of shape [n_mol, 2] (alpha, beta)")
            charge = charge.t().contiguous()  # channel-major planes, include/aimnet_hip.h aimnet_inputs.charge
        elif who != "eval":
            charge = charge.reshape(-1)
        elif charge.ndim != 1:
            raise ValueError("HipEngine.eval: charge must have shape [n_mol]")
        t["charge"] = charge = charge.contiguous()
        n, n_mol = t["coord"].shape[0], charge.shape[-1]
        inp = _lib.Inputs(n_atoms=n, n_mol=n_mol)
        if n == 0 or n_mol == 0:
            raise ValueError(f"HipEngine.{who}: empty input" + (" (no atoms or no molecules)" if who == "eval" else ""))
        if cell is not None:
            t["cell"] = cell = cell.to(device=dev, dtype=torch.float32).contiguous()
            inp.cell, inp.n_cell = cell.data_ptr(), 1 if cell.ndim == 2 else cell.shape[0]
        # pbc: three flags, or per-system flags [n_cell, 3] (tensor / array): normalize_pbc, neighbors.py:309-321
        if cell is not None and not isinstance(pbc, (tuple, list)) and getattr(pbc, "ndim", 1) == 2:
            t["pbc_sys"] = pbc_sys = torch.as_tensor(pbc).to(device=dev, dtype=torch.int32).contiguous()
            if tuple(pbc_sys.shape) != (inp.n_cell, 3):
                raise ValueError(f"pbc must have shape (3,) or ({inp.n_cell}, 3), got {tuple(pbc_sys.shape)}")
            inp.pbc_sys, pbc = pbc_sys.data_ptr(), (True, True, True)
        elif not isinstance(pbc, (tuple, list)):
            pbc = tuple(bool(x) for x in torch.as_tensor(pbc).reshape(-1).tolist())
        inp.pbc[:] = [1 if bool(pbc[k]) else 0 for k in range(3)]
        inp.coord, inp.numbers, inp.mol_idx, inp.charge = (t[k].data_ptr() for k in ("coord", "numbers", "mol_idx", "charge"))
        return inp, t

    def _directions(self, who: str, vectors, n: int) -> tuple:
        """The tangent directions of `hvp` / `charge_response` (`who`, for the message): their number K and the [K, n, 3] device array."""
        import torch

        K = int(vectors.numel()) // (3 * n)
        if K == 0:
            raise ValueError(f"HipEngine.{who}: empty input")
        return K, vectors.to(device=self.device, dtype=torch.float32).reshape(-1, n, 3).contiguous()

    def _caller_lists(self, inp, t, lists) -> tuple:
        """Check the caller-supplied matrices `lists` = ((name, matrix, shifts), ...) of `eval`, enter them into `inp` (and `t`, which
        keeps them alive) and return their widths (0: not given)."""
        import torch

        n, widths = inp.n_atoms, []
        for key, mat, sh in lists:
            widths.append(0)
            if mat is None:
                if sh is not None:
                    raise ValueError(f"HipEngine.eval: shifts given without {key}")
                continue
            if lists[0][1] is None:
                raise ValueError("HipEngine.eval: nbmat_lr / nbmat_d3 are only read together with nbmat")
            mat = mat.to(device=self.device, dtype=torch.int32).contiguous()
            if mat.ndim != 2 or mat.shape[0] != n or mat.shape[1] < 1:
                raise ValueError(f"HipEngine.eval: {key} must have shape [{n}, width], got {tuple(mat.shape)}")
            if sh is not None:
                sh = sh.to(device=self.device, dtype=torch.int32).contiguous()
                if tuple(sh.shape) != (n, mat.shape[1], 3):
                    raise ValueError(f"HipEngine.eval: the shifts of {key} must have shape {(n, mat.shape[1], 3)}, got {tuple(sh.shape)}")
            elif t["cell"] is not None:
                raise ValueError(f"HipEngine.eval: periodic input needs the shifts of {key}")
            t[key], t["shifts" + key[5:]], widths[-1] = mat, sh, int(mat.shape[1])
            setattr(inp, key, mat.data_ptr())
            setattr(inp, "shifts" + key[5:], sh.data_ptr() if sh is not None else None)
            setattr(inp, key + "_width", widths[-1])
        return tuple(widths)

    def _workspace(self, need: int):
        """The one workspace, at least `need` bytes, ordered behind its last user; returns it and the current stream."""
        import torch

        if self._ws is None or self._ws.numel() < need:
            if self._ws is not None and self._ws_stream is not None:
                # earlier (possibly still running, sync=False) evaluations used the old workspace on that stream: keep the
                # caching allocator from handing its memory to another stream before they finish
                self._ws.record_stream(self._ws_stream)
            self._ws = None
            self._ws = torch.empty(int(need * 1.1) + 4096, dtype=torch.uint8, device=self.device)
        cur_stream = torch.cuda.current_stream(self.device)
        if self._ws_stream is not None and self._ws_stream != cur_stream:
            cur_stream.wait_stream(self._ws_stream)  # one workspace: evaluations on different streams are serialised
        self._ws_stream = cur_stream
        return self._ws, cur_stream.cuda_stream

    def _read_status(self, out: _OutBuffer, host_out: bool, watch: bool):
        """The one D2H sync of a step (the reference has one per list, neighbors.py:133): the status words, whether the results are
        finite (looked at only while the fp16-range fallback is `watch`ing) and, with `host_out`, the host copy of every output."""
        import torch

        # ONE D2H copy brings back the status words and every output (host_out), or the status words and the molecule energies
        # (adjacent sections): the energies are the fp16-range sentinel.  (A persistent pinned staging buffer was tried and
        # dropped: torch's pinned host memory is uncached for the CPU on this platform - reading 160 KB of results out of
        # it took 1.4 ms, and the evaluation as a whole 15 ms instead of 2.2, tests/tools/ase_prof2.py.)
        e0, e_bytes = out.spans[1]
        host = out.buf.cpu() if host_out else out.buf[: e0 + e_bytes].cpu()
        st = host[:32].view(torch.int32).numpy()
        # (periodic embedding sites: its two status words follow the engine's eight in the same section, and so in the same copy)
        self._emb_status = host[32:40].view(torch.int32).numpy() if out.spans[0][1] >= 40 else None
        watched = [] if not watch else [v for k, v in out.views(host).items() if k != "status"] if host_out else [host[e0:].view(torch.float64)]
        # (status[6] bit 5 = a non-finite energy or FORCE seen on the device: an overflow in the adjoint sweep leaves the energies finite)
        finite = all(bool(torch.isfinite(v).all()) for v in watched) and not (watch and int(st[6]) & NONFINITE_FLAG)
        return st, finite, host if host_out else None

    def eval(self, coord, numbers, mol_idx, charge, cell=None, pbc=(True, True, True), forces: bool = False, stress: bool = False,
             coulomb: str = "simple", dsf_rc: float = 15.0, dsf_alpha: float = 0.2, ewald_accuracy: float = 1e-6, sync: bool = True,
             dftd3: dict[str, float] | None = None, host_out: bool = False, defer: bool = False, nbmat=None, shifts=None,
             nbmat_lr=None, shifts_lr=None, nbmat_d3=None, shifts_d3=None, embedding: dict[str, Any] | None = None,
             _arm_periodic=None) -> dict[str, Any]:
        """One evaluation on device tensors (coord f32 [N,3], numbers/mol_idx i32 [N], charge f32
        [n_mol] - for a 2-channel NSE model [n_mol, 2] = the alpha / beta charges of aimnet2.py:94-100 -,
        cell f32 [3,3]|[n_mol,3,3]).  Returns device tensors (NSE: plus spin_charges); retries with x1.5 row
        capacity on neighbour overflow (neighbors.py:127-130).  `dftd3` = {s8, a1, a2[, s6, cutoff, smoothing_fraction]}
        adds the external DFT-D3(BJ) term (needs set_dftd3_tables).  All outputs and the status words live in ONE device
        buffer; `host_out=True` returns CPU tensors taken from the single D2H copy that fetches the status anyway (the
        ASE adapter's path: no further .cpu() round trips).
        `nbmat` (+ `shifts`, `nbmat_lr` / `shifts_lr`, `nbmat_d3` / `shifts_d3`): caller-supplied FULL neighbour matrices, int
        [N, width] with entries outside [0, N) as padding, integer shifts [N, width, 3] - the engine then builds no list and takes the
        coordinates as given (include/aimnet_hip.h, aimnet_inputs.nbmat).
        `embedding`: electrostatic embedding of the charges, E_emb = sum_i q_i phi_i (include/aimnet_hip.h, aimnet_embedding) - a
        dict with point charges `ext_coord` [M,3], `ext_charge` [M] (+ `ext_mol_idx` [M], sorted, for more than one molecule; with a
        cell they are refused unless `ewald_accuracy` (a float in (0, 1)) is among the keys: then the input must be fully periodic and
        the sites of a system are periodic with its cell, by Ewald summation at that accuracy - aimnet_embedding_periodic) and / or
        a per-atom `potential` [N] (V) with `potential_grad` [N,3] (V/A); `want_ext_forces` / `want_ext_potential` ask for the
        forces on the sites and the potential of the atoms' charges at them.  The energy and forces include the term; the
        result gains `embedding_energy` [n_mol] (and `ext_forces` [M,3], `ext_potential` [M]).  Not with `stress`."""
        import torch

        if embedding is not None:
            return self._eval_embedded(embedding, dict(
                coord=coord, numbers=numbers, mol_idx=mol_idx, charge=charge, cell=cell, pbc=pbc, forces=forces, stress=stress,
                coulomb=coulomb, dsf_rc=dsf_rc, dsf_alpha=dsf_alpha, ewald_accuracy=ewald_accuracy, sync=sync, dftd3=dftd3,
                host_out=host_out, defer=defer, nbmat=nbmat, shifts=shifts, nbmat_lr=nbmat_lr, shifts_lr=shifts_lr, nbmat_d3=nbmat_d3,
                shifts_d3=shifts_d3))
        inp, t = self._inputs("eval", coord, numbers, mol_idx, charge, cell, pbc)
        n, n_mol, cell = inp.n_atoms, inp.n_mol, t["cell"]
        method = _METHODS[coulomb]
        if method in capacity.EWALD_METHODS:
            if cell is None:
                raise ValueError(f"HipEngine.eval: coulomb={coulomb!r} needs a periodic cell (lr.py:655-657)")
            if nbmat is not None:
                raise ValueError("HipEngine.eval: Ewald summation does not take caller-supplied neighbour matrices")
            if not (0.0 < float(ewald_accuracy) < 1.0):
                raise ValueError("HipEngine.eval: ewald_accuracy must lie in (0, 1)")
        widths = self._caller_lists(inp, t, (("nbmat", nbmat, shifts), ("nbmat_lr", nbmat_lr, shifts_lr), ("nbmat_d3", nbmat_d3, shifts_d3)))
        np_walk_on = method == _lib.COULOMB_DSF and cell is None and bool(self.get_option("dsf_np_walk"))  # (read only where it matters)
        rq = capacity.Request("eval", n, n_mol, cell is not None, method, float(dsf_rc), float(dsf_alpha), float(ewald_accuracy), dftd3,
                              widths, (_lib.FORCES if forces else 0) | (_lib.STRESS if stress else 0), np_walk_on)
        # (_arm_periodic, from _eval_embedded: the status section carries the two words of aimnet_embedding_periodic behind the engine's)
        sections = [("status", torch.int32, (8 if _arm_periodic is None else 10,)), ("energy", torch.float64, (n_mol,)), ("charges", torch.float32, (n,))]
        sections += [("spin_charges", torch.float32, (n,))] if self.nq == 2 else []
        sections += [("forces", torch.float32, (n, 3))] if forces else []
        sections += [("stress", torch.float32, (max(inp.n_cell, 1), 3, 3))] if stress else []
        out = _OutBuffer(sections, self.device)
        res = out.views(out.buf)
        outs = _lib.Outputs(**{name: v.data_ptr() for name, v in res.items()})
        if _arm_periodic is not None:
            res["status"][8:].zero_()  # (without sites nothing writes them)
            _arm_periodic(res["status"].data_ptr() + 32)
        fallback, host = _RangeFallback(self), None
        while True:  # fill the options, run, read the status; then the fallback, growth, or shrink and leave
            opt = self.fill_options(rq)
            self._last_request = (opt, rq)
            ws, stream = self._workspace(int(self.lib.aimnet_engine_workspace_bytes(self._h, n, n_mol, inp.n_cell, C.byref(opt))))
            with torch.cuda.device(self.device):
                rc = self.lib.aimnet_engine_eval(self._h, C.byref(inp), C.byref(opt), C.byref(outs), ws.data_ptr(), ws.numel(), stream)
            _lib.check(rc, "aimnet_engine_eval")
            if not sync:
                break
            st, finite, host = self._read_status(out, host_out, fallback.on or fallback.retrying)
            self.last_status = st
            if int(st[6]) & ~NONFINITE_FLAG:  # input sanity flags raised by the engine (it clamps for memory safety, the results are meaningless)
                raise ValueError("HipEngine.eval: invalid input: " + describe_input_flags(int(st[6]) & ~NONFINITE_FLAG, n_mol))
            overflow = capacity.overflowed(st, opt)
            if not overflow and fallback.repeat(finite):  # (overflow before range: garbage rows are not finite either)
                continue
            if widths[0]:  # caller-supplied rows cannot overflow, and say nothing about the capacities of the engine's own lists
                break
            if not (overflow and self.grow(st, opt, rq)):
                self.shrink(st, opt, rq)
                break
        if host is not None:
            res = out.views(host)
        status = res.pop("status")
        if not sync:
            # no host round trip: the caller owns the overflow check (status[2], [3], [5] must be 0, include/aimnet_hip.h)
            # and reads it whenever it next synchronises - e.g. a device-resident MD loop once per block of steps
            res["status"] = status
            if defer:
                self.pending_status.append(status)  # verified in one go by check_deferred()
                self._status7_pme = method == _lib.COULOMB_PME
                if fallback.on:
                    self._pending_energy.append(res["energy"])
        if stress and cell is not None and cell.ndim == 2:
            res["stress"] = res["stress"][0]
        return res

    EMBEDDING_KEYS = ("ext_coord", "ext_charge", "ext_mol_idx", "potential", "potential_grad", "want_ext_forces", "want_ext_potential",
                      "ewald_accuracy")
    EMBEDDING_KEYS_HVP = EMBEDDING_KEYS + ("potential_hess", "want_ext_hv", "want_field")

    def _embedding_arrays(self, who: str, emb: dict[str, Any], keys, n: int, n_mol: int, periodic: bool) -> dict[str, Any]:
        """The checks `eval` and `hvp` share on an `embedding` dict: known keys, shapes, what goes with what.  Returns the device
        arrays `ext_coord`, `ext_charge`, `ext_mol_idx`, `potential`, `potential_grad` (None where not given) and `m`, the number of
        sites."""
        import torch

        who = f"HipEngine.{who}"
        unknown = set(emb) - set(keys)
        if unknown:
            raise ValueError(f"{who}: unknown embedding keys {sorted(unknown)}")
        dev, f32 = self.device, torch.float32
        xc, qc, mi = emb.get("ext_coord"), emb.get("ext_charge"), emb.get("ext_mol_idx")
        if (xc is None) != (qc is None):
            raise ValueError(f"{who}: embedding point charges need both ext_coord and ext_charge")
        m = 0
        if xc is not None:
            xc = torch.as_tensor(xc).to(device=dev, dtype=f32).contiguous()
            qc = torch.as_tensor(qc).to(device=dev, dtype=f32).contiguous()
            if xc.ndim != 2 or xc.shape[1] != 3 or tuple(qc.shape) != (xc.shape[0],):
                raise ValueError(f"{who}: ext_coord must be [M, 3] and ext_charge [M], got {tuple(xc.shape)}, {tuple(qc.shape)}")
            m = int(xc.shape[0])
            if m and periodic and emb.get("ewald_accuracy") is None:
                raise ValueError(f"{who}: embedding point charges take non-periodic input; pass a per-atom potential with a cell")
            if mi is not None:
                mi = torch.as_tensor(mi).to(device=dev, dtype=torch.int32).contiguous()
                if tuple(mi.shape) != (m,):
                    raise ValueError(f"{who}: ext_mol_idx must have shape ({m},), got {tuple(mi.shape)}")
            elif n_mol > 1 and m:
                raise ValueError(f"{who}: embedding point charges of more than one molecule need ext_mol_idx")
        elif mi is not None:
            raise ValueError(f"{who}: ext_mol_idx given without ext_coord")
        pot, pg = emb.get("potential"), emb.get("potential_grad")
        if pot is not None:
            pot = torch.as_tensor(pot).to(device=dev, dtype=f32).contiguous()
            if tuple(pot.shape) != (n,):
                raise ValueError(f"{who}: embedding potential must have shape ({n},), got {tuple(pot.shape)}")
        if pg is not None:
            if pot is None:
                raise ValueError(f"{who}: embedding potential_grad given without potential")
            pg = torch.as_tensor(pg).to(device=dev, dtype=f32).contiguous()
            if tuple(pg.shape) != (n, 3):
                raise ValueError(f"{who}: embedding potential_grad must have shape ({n}, 3), got {tuple(pg.shape)}")
        return {"ext_coord": xc, "ext_charge": qc, "ext_mol_idx": mi, "potential": pot, "potential_grad": pg, "m": m}

    def _embedding_scratch(self, attr: str, nbytes: int):
        """One buffer per kind (`attr`), grown on demand, ordered like the workspace (_workspace)."""
        import torch

        scratch = getattr(self, attr, None)
        if scratch is None or scratch.numel() < nbytes:
            if scratch is not None and self._ws_stream is not None:
                scratch.record_stream(self._ws_stream)
            scratch = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
            setattr(self, attr, scratch)
        return scratch

    def _eval_embedded(self, emb: dict[str, Any], kw: dict[str, Any]) -> dict[str, Any]:
        """`eval` with an embedding: check it, allocate its scratch and outputs, set it (aimnet_engine_set_embedding), evaluate,
        and switch it off again whatever happens."""
        import torch

        if set(emb) <= set(self.EMBEDDING_KEYS) and kw["stress"]:  # (an unknown key is reported first, by the shared checks)
            raise ValueError("HipEngine.eval: the embedding term has no stress")
        dev, f32 = self.device, torch.float32
        n = int(kw["coord"].shape[0])
        n_mol = int(kw["charge"].shape[0]) if self.nq == 2 else int(kw["charge"].numel())
        arr = self._embedding_arrays("eval", emb, self.EMBEDDING_KEYS, n, n_mol, kw["cell"] is not None)
        accuracy = emb.get("ewald_accuracy")
        if accuracy is not None:  # sites periodic with the cell (aimnet_engine_set_embedding_periodic)
            accuracy = float(accuracy)
            if not (0.0 < accuracy < 1.0):
                raise ValueError("HipEngine.eval: embedding ewald_accuracy must lie in (0, 1)")
            if kw["cell"] is None:
                raise ValueError("HipEngine.eval: embedding ewald_accuracy (periodic sites) needs a cell")
            if not bool(torch.as_tensor(kw["pbc"]).bool().all()):
                raise ValueError("HipEngine.eval: periodic embedding sites need a cell that is periodic along all three axes")
            if not kw["sync"]:
                raise ValueError("HipEngine.eval: periodic embedding sites are evaluated synchronously (the capacity of their k arrays "
                                 "is read back)")
            kw = dict(kw, pbc=(True, True, True))
        xc, qc, mi, pot, pg, m = (arr[k] for k in ("ext_coord", "ext_charge", "ext_mol_idx", "potential", "potential_grad", "m"))
        if pot is not None and pg is None and kw["forces"]:
            raise ValueError("HipEngine.eval: forces with an embedding potential need potential_grad")
        outs = {"embedding_energy": torch.empty(n_mol, dtype=torch.float64, device=dev)}
        if emb.get("want_ext_forces") and xc is not None:
            outs["ext_forces"] = torch.empty(m, 3, dtype=f32, device=dev)
        if emb.get("want_ext_potential") and xc is not None:
            outs["ext_potential"] = torch.empty(m, dtype=f32, device=dev)
        scratch = self._embedding_scratch("_emb_scratch", int(self.lib.aimnet_embedding_scratch_bytes(n, n_mol, m)))
        ptr = lambda v: v.data_ptr() if v is not None and v.numel() else None  # noqa: E731
        s = _lib.Embedding(n_ext=m, ext_coord=ptr(xc), ext_charge=ptr(qc), ext_mol_idx=ptr(mi), potential=ptr(pot), potential_grad=ptr(pg),
                           ext_forces=ptr(outs.get("ext_forces")), ext_potential=ptr(outs.get("ext_potential")),
                           energy=outs["embedding_energy"].data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
        try:
            while True:
                _lib.check(self.lib.aimnet_engine_set_embedding(self._h, C.byref(s)), "aimnet_engine_set_embedding")
                if accuracy is not None:  # its own k arrays, scratch and status words: nothing of the system's own Ewald sum is shared
                    max_k = self._emb_max_k
                    pscratch = self._embedding_scratch(
                        "_emb_periodic_scratch", int(self.lib.aimnet_embedding_periodic_scratch_bytes(n, n_mol, m, max_k)))

                    def arm(status_ptr: int, max_k=max_k, pscratch=pscratch) -> None:  # (eval owns the status words: its one buffer)
                        sp = _lib.EmbeddingPeriodic(accuracy=accuracy, max_k=max_k, status=status_ptr, scratch=pscratch.data_ptr(),
                                                    scratch_bytes=pscratch.numel())
                        _lib.check(self.lib.aimnet_engine_set_embedding_periodic(self._h, C.byref(sp)),
                                   "aimnet_engine_set_embedding_periodic")
                    res = self.eval(**kw, _arm_periodic=arm)
                else:
                    res = self.eval(**kw)
                if accuracy is None:
                    break
                need = int(self._emb_status[0])  # (read with the status copy of the evaluation: no round trip of its own)
                if need <= max_k:
                    break
                self._emb_max_k = capacity.ewald_k_capacity(need)  # the k boxes did not fit: their size is now known - repeat
        finally:
            self.lib.aimnet_engine_set_embedding(self._h, None)  # (disarms the periodic sites too)
        if kw["host_out"]:
            outs = {k: v.cpu() for k, v in outs.items()}
        res.update(outs)
        return res

    # ------------------------------------------------------------------------------------------
    HVP_BYTES_BUDGET = 6 << 30  # workspace of one tangent sweep; more directions than fit are processed in several sweeps
    # the tangent kernels put the direction index in grid.y (HIP limit 65535; 4 K with the finite-difference DFT-D3 block: 16383)
    HVP_MAX_DIRECTIONS = 65535
    # one direction costs ~3/4 us per atom (7.5 ms on 10 080 atoms, profiles/r3_hvp.md): calls that would run for more than
    # this many seconds are announced (or refused, HVP_ON_LONG) (a dense Hessian of a 10 k-atom crystal is 30 240 directions = minutes)
    HVP_MAX_SECONDS = 120.0
    HVP_ON_LONG = "warn"  # "warn": say so and run (the reference runs such requests too, slowly); "raise": refuse with a ValueError

    def hvp(self, coord, numbers, mol_idx, charge, vectors, cell=None, pbc=(True, True, True), coulomb: str = "simple",
            dsf_rc: float = 15.0, dsf_alpha: float = 0.2, want_forces: bool = False,
            dftd3: dict[str, float] | None = None, ewald_accuracy: float = 1e-6,
            embedding: dict[str, Any] | None = None, pme_tangent: bool = False, d3_tangent: bool = False,
            _d3_block_only: bool = False, strain=None, strain_terms: tuple[str, ...] = ()) -> dict[str, Any]:
        """Analytic Hessian-vector products (csrc/hvp.hip, aimnet_engine_hvp): vectors [K, N, 3] -> hv [K, N, 3] on the device
        (+ the forces of the same sweep with `want_forces`).  Inputs as `eval` (`pbc`: three flags or per-system [n_cell, 3]);
        with `dftd3` the dispersion block is added as a central difference of the D3 gradient inside the same call.  The K
        directions are processed in as many sweeps as the workspace budget asks for.  `coulomb`: "none", "simple", "dsf" or "ewald" (the exact structure-factor sum at
        `ewald_accuracy`, periodic cells only; `dsf_rc` / `dsf_alpha` are not read with it); "pme" raises - its tangent is not
        carried, AIMNet2Calculator takes differences of forces there - unless `pme_tangent=True` arms the mesh tangent
        (aimnet_engine_set_pme_tangent, csrc/pme.hip): the real-space term on a list of cutoff r_c <= 10 A, the mesh tangents of
        every direction at 40 bytes per mesh point, direction and system (they enter the split by HVP_BYTES_BUDGET); status[7]
        grows the mesh capacity and the sweep repeats, as in `eval`.  The engine's switch is on for the sweeps of such a call only.
        `d3_tangent=True` (with `dftd3`) arms the analytic dispersion block (aimnet_engine_set_dftd3_tangent, csrc/d3.hip): three
        tangent passes over the one D3 list instead of the central difference over four displaced copies of it per direction - 32
        bytes per direction and atom instead of the replicas (the split by HVP_BYTES_BUDGET sees the smaller figure), up to
        HVP_MAX_DIRECTIONS directions per sweep; also for the sweeps of this call only.
        `embedding`: the dict of `eval`, carried through the sweep with the atoms moving and the sites clamped
        (include/aimnet_hip.h, aimnet_embedding_tangent): a `potential` needs `potential_grad` and `potential_hess` [N,6] (xx, yy,
        zz, xy, xz, yz) or [N,3,3] beside it (zeros for a uniform field).  hv and the forces then include the term; `want_ext_hv`
        adds `ext_hv` [K, M, 3], the mixed atom-site block applied to the directions, `want_field` adds `ext_field` [N, 10] (phi,
        grad phi, grad grad phi as the sweep used them, float64).
        `strain` [K, 3, 3] (or [3, 3], the same for every direction) arms the strain tangent (aimnet_engine_set_strain_tangent):
        direction k is the path x -> x (1 + t strain_k) + t vectors_k, cell -> cell (1 + t strain_k), in the row-vector convention
        of the stress; any 3 x 3 matrix, shared by the systems of the batch.  The result gains `dvirial` [K, n_mol, 3, 3], the
        tangent of the un-normalised virial S_ab = sum_pairs r_a rbar_b (volume x stress) along the path, and `virial` [n_mol, 3, 3]
        (both float64); hv is dG/dt along the same path.  Needs a cell; coulomb "none" or "dsf"; no embedding; `dftd3` only as
        named next (the engine refuses the others before anything is launched).  36 bytes of workspace more per direction and
        atom; armed for the sweeps of this call only.
        `strain_terms=("dftd3",)` (with `strain`, `dftd3` and `d3_tangent=True`) lets the armed sweep carry the dispersion block
        (aimnet_engine_set_strain_terms): its pair tangents take r strain_k and it adds its share to `virial` and `dvirial`; no
        workspace of its own.  With the finite-difference block (`d3_tangent=False`) the engine refuses."""
        import torch

        inp, t = self._inputs("hvp", coord, numbers, mol_idx, charge, cell, pbc)
        n, n_mol, dev = inp.n_atoms, inp.n_mol, self.device
        K, vectors = self._directions("hvp", vectors, n)
        est = 0.75e-6 * n * K if n > 2000 else 0.0  # (small systems are launch-bound: ~0.04 force evaluations per direction)
        if est > self.HVP_MAX_SECONDS and self.HVP_ON_LONG == "raise":
            raise ValueError(f"HipEngine.hvp: {K} directions on {n} atoms would take ~{est:.0f} s (HVP_ON_LONG = 'raise')")
        if est > self.HVP_MAX_SECONDS:  # the reference computes such requests (slowly): warn, do not refuse
            import warnings
            warnings.warn(f"HipEngine.hvp: {K} directions on {n} atoms will take ~{est:.0f} s (~0.75 us per atom and direction on one "
                          f"MI355X, more with DFT-D3); a Krylov / Davidson solver needs tens of directions, not 3N "
                          f"(threshold: HipEngine.HVP_MAX_SECONDS = {self.HVP_MAX_SECONDS:.0f} s)", RuntimeWarning, stacklevel=2)
        if coulomb == "pme" and not pme_tangent:
            raise ValueError("HipEngine.hvp: the analytic tangent sweep does not carry particle-mesh Ewald; use coulomb='ewald' (the exact "
                             "sum) or differences of the forces (AIMNet2Calculator does: hvp_method 'fd' is taken automatically)")
        method = _METHODS[coulomb]
        lr_rc = float(dsf_rc)  # cutoff of the long-range list
        if method in capacity.EWALD_METHODS:
            if cell is None:
                raise ValueError(f"HipEngine.hvp: coulomb='{coulomb}' needs a periodic cell")
            if not (0.0 < float(ewald_accuracy) < 1.0):
                raise ValueError("HipEngine.hvp: ewald_accuracy must lie in (0, 1)")
            # the real-space term runs on a list: its cutoff is the largest r_c of the batch
            counts = torch.bincount(t["mol_idx"].long().clamp(0, n_mol - 1), minlength=n_mol).cpu().numpy()
            vols = np.abs(np.linalg.det(t["cell"].detach().cpu().numpy().astype(np.float64).reshape(-1, 3, 3)))
            vols = np.broadcast_to(vols, (n_mol,)) if vols.shape[0] == 1 else vols
            if vols.shape[0] != n_mol:
                raise ValueError("HipEngine.hvp: cell must be [3, 3] or [n_mol, 3, 3]")
            lr_rc = capacity.ewald_list_cutoff(vols, counts, float(ewald_accuracy))
            if method == _lib.COULOMB_PME:  # the mesh method caps r_c (csrc/pme.hip, PME_RC_MAX)
                lr_rc = min(lr_rc, capacity.PME_RC_MAX * (1.0 + 1e-5))
        rq = capacity.Request("hvp", n, n_mol, cell is not None, method, lr_rc, float(dsf_alpha), float(ewald_accuracy), dftd3)
        hv = torch.empty_like(vectors)
        f_out = torch.empty(n, 3, dtype=torch.float32, device=dev) if want_forces else None

        arm, outs = (lambda k0, kc: None), {}
        if embedding is not None:
            arm, outs = self._hvp_embedding(embedding, n, n_mol, K, cell is not None)

        def call(opt, k0, kc, *tail):
            arm(k0, kc)  # (the embedding's tangent struct names this sweep's slice of ext_hv)
            return self.lib.aimnet_engine_hvp(self._h, C.byref(inp), C.byref(opt), vectors[k0 : k0 + kc].data_ptr(), kc,
                                              hv[k0 : k0 + kc].data_ptr(), f_out.data_ptr() if f_out is not None else None, *tail)
        terms_mask = 0
        for name in strain_terms:
            if name not in _lib.STRAIN_TERMS:
                raise ValueError(f"HipEngine.hvp: unknown strain term {name!r} (known: {sorted(_lib.STRAIN_TERMS)})")
            terms_mask |= _lib.STRAIN_TERMS[name]
        if terms_mask and strain is None:
            raise ValueError("HipEngine.hvp: strain_terms names what a strain sweep carries: it needs strain")
        if strain is not None:
            eps = torch.as_tensor(strain).to(device=dev, dtype=torch.float32)
            if tuple(eps.shape) == (3, 3):
                eps = eps.expand(K, 3, 3)
            if tuple(eps.shape) != (K, 3, 3):
                raise ValueError(f"HipEngine.hvp: strain must have shape ({K}, 3, 3) or (3, 3), got {tuple(eps.shape)}")
            eps = eps.contiguous()
            outs["dvirial"] = torch.empty(K, n_mol, 3, 3, dtype=torch.float64, device=dev)
            outs["virial"] = torch.empty(n_mol, 3, 3, dtype=torch.float64, device=dev)
            arm_rest = arm

            def arm(k0, kc):  # noqa: F811  (the struct names this sweep's slice of the strains and of dvirial)
                arm_rest(k0, kc)
                st = _lib.StrainTangent(strain=eps[k0 : k0 + kc].data_ptr(), dvirial=outs["dvirial"][k0 : k0 + kc].data_ptr(),
                                        virial=outs["virial"].data_ptr())
                _lib.check(self.lib.aimnet_engine_set_strain_tangent(self._h, C.byref(st)), "aimnet_engine_set_strain_tangent")
        d3_armed = bool(d3_tangent) and dftd3 is not None
        if _d3_block_only:  # aimnet_debug_dftd3_tangent: the armed block alone (tests)
            if not d3_armed:
                raise ValueError("HipEngine.hvp: the dispersion block alone needs dftd3 and d3_tangent=True")

            def call(opt, k0, kc, *tail):  # noqa: F811
                if strain is not None:  # (this sweep's slice of the strains and of dvirial)
                    arm(k0, kc)
                return self.lib.aimnet_debug_dftd3_tangent(self._h, C.byref(inp), C.byref(opt), vectors[k0 : k0 + kc].data_ptr(), kc,
                                                           hv[k0 : k0 + kc].data_ptr(), f_out.data_ptr() if f_out is not None else None,
                                                           *tail)
        # grid.y limit of the tangent kernels (the finite-difference D3 block replicates every direction four times)
        kmax = self.HVP_MAX_DIRECTIONS // (4 if dftd3 is not None and not d3_armed else 1)
        if method == _lib.COULOMB_PME:  # a (direction, system) slice of the mesh transforms is a grid.y index
            kmax = max(1, min(kmax, self.HVP_MAX_DIRECTIONS // n_mol))
        mesh = method == _lib.COULOMB_PME  # (armed: unarmed requests were refused above)
        try:
            if mesh:  # the engine's switch is on for the sweeps of this call only: no state leaks from one call into the next
                _lib.check(self.lib.aimnet_engine_set_pme_tangent(self._h, 1), "aimnet_engine_set_pme_tangent")
            if d3_armed:  # (likewise)
                _lib.check(self.lib.aimnet_engine_set_dftd3_tangent(self._h, 1), "aimnet_engine_set_dftd3_tangent")
            if strain is not None:  # (likewise; armed without arrays, so that the size queries of the split see the armed state)
                _lib.check(self.lib.aimnet_engine_set_strain_tangent(self._h, C.byref(_lib.StrainTangent())),
                           "aimnet_engine_set_strain_tangent")
            if terms_mask:  # (likewise; arming with a struct leaves the mask, disarming below clears it)
                _lib.check(self.lib.aimnet_engine_set_strain_terms(self._h, terms_mask), "aimnet_engine_set_strain_terms")
            self._tangent_sweeps("hvp", self.lib.aimnet_engine_hvp_workspace_bytes, rq, K, kmax, call)
        finally:
            if mesh:
                self.lib.aimnet_engine_set_pme_tangent(self._h, 0)
            if d3_armed:
                self.lib.aimnet_engine_set_dftd3_tangent(self._h, 0)
            if embedding is not None:
                self.lib.aimnet_engine_set_embedding(self._h, None)  # (disarms the tangent too)
            if terms_mask:
                self.lib.aimnet_engine_set_strain_terms(self._h, 0)
            if strain is not None:
                self.lib.aimnet_engine_set_strain_tangent(self._h, None)
        res = {"hv": hv, "forces": f_out} if f_out is not None else {"hv": hv}
        res.update(outs)
        return res

    def _hvp_embedding(self, emb: dict[str, Any], n: int, n_mol: int, K: int, periodic: bool):
        """`hvp` with an embedding: the checks of `eval` (_embedding_arrays) and those of the tangent, the scratches and outputs; sets
        the embedding and returns (`arm`, outputs) - `arm(k0, kc)` arms the sweep of the directions [k0, k0 + kc)
        (aimnet_engine_set_embedding_tangent).  The caller switches the embedding off again."""
        import torch

        dev, f32 = self.device, torch.float32
        if emb.get("ewald_accuracy") is not None:
            raise NotImplementedError("HipEngine.hvp: periodic embedding sites (ewald_accuracy) are not carried by the tangent sweep")
        arr = self._embedding_arrays("hvp", emb, self.EMBEDDING_KEYS_HVP, n, n_mol, periodic)
        xc, qc, mi, pot, pg, m = (arr[k] for k in ("ext_coord", "ext_charge", "ext_mol_idx", "potential", "potential_grad", "m"))
        ph = emb.get("potential_hess")
        if pot is not None and (pg is None or ph is None):
            raise ValueError("HipEngine.hvp: an embedding potential needs potential_grad and potential_hess (zeros for a uniform field)")
        if ph is not None:
            if pot is None:
                raise ValueError("HipEngine.hvp: embedding potential_hess given without potential")
            ph = torch.as_tensor(ph).to(device=dev, dtype=f32)
            if tuple(ph.shape) == (n, 3, 3):
                ph = torch.stack([ph[:, 0, 0], ph[:, 1, 1], ph[:, 2, 2], ph[:, 0, 1], ph[:, 0, 2], ph[:, 1, 2]], dim=1)
            if tuple(ph.shape) != (n, 6):
                raise ValueError(f"HipEngine.hvp: embedding potential_hess must have shape ({n}, 6) or ({n}, 3, 3), got {tuple(ph.shape)}")
            ph = ph.contiguous()
        outs = {}
        if emb.get("want_ext_hv") and xc is not None:
            outs["ext_hv"] = torch.empty(K, m, 3, dtype=f32, device=dev)
        if emb.get("want_field"):
            outs["ext_field"] = torch.empty(n, 10, dtype=torch.float64, device=dev)
        scratch = self._embedding_scratch("_emb_scratch", int(self.lib.aimnet_embedding_scratch_bytes(n, n_mol, m)))
        tscratch = self._embedding_scratch("_emb_tangent_scratch", int(self.lib.aimnet_embedding_tangent_scratch_bytes(n, n_mol, m)))
        ptr = lambda v: v.data_ptr() if v is not None and v.numel() else None  # noqa: E731
        s = _lib.Embedding(n_ext=m, ext_coord=ptr(xc), ext_charge=ptr(qc), ext_mol_idx=ptr(mi), potential=ptr(pot), potential_grad=ptr(pg),
                           scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
        keep = (xc, qc, mi, pot, pg, ph)  # (the arrays the structs point into live as long as `arm` does)
        _lib.check(self.lib.aimnet_engine_set_embedding(self._h, C.byref(s)), "aimnet_engine_set_embedding")

        def arm(k0: int, kc: int, keep=keep) -> None:
            ext_hv = outs.get("ext_hv")
            ts = _lib.EmbeddingTangent(potential_hess=ptr(ph), ext_hv=ptr(ext_hv[k0 : k0 + kc]) if ext_hv is not None else None,
                                       field=ptr(outs.get("ext_field")), scratch=tscratch.data_ptr(), scratch_bytes=tscratch.numel())
            _lib.check(self.lib.aimnet_engine_set_embedding_tangent(self._h, C.byref(ts)), "aimnet_engine_set_embedding_tangent")
        return arm, outs

    def _tangent_sweeps(self, name: str, ws_bytes_fn, rq: capacity.Request, K: int, kmax: int, call) -> None:
        """The K directions of `hvp` / `charge_response` (`name`) in sweeps of at most `kmax`, and of as many as HVP_BYTES_BUDGET
        holds at `ws_bytes_fn`'s bytes per direction.  `call(opt, k0, kc, status, workspace, workspace_bytes, stream)` makes the C
        call for the directions [k0, k0 + kc); a sweep whose status words report an overflow is repeated at the grown capacities."""
        import torch

        n, n_mol, dev = rq.n, rq.n_mol, self.device
        status = torch.empty(8, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        ws_bytes = lambda k, opt: int(ws_bytes_fn(self._h, n, n_mol, k, C.byref(opt)))  # noqa: E731
        k0 = 0
        while k0 < K:
            opt = self.fill_options(rq)
            per_dir = ws_bytes(2, opt) - ws_bytes(1, opt)
            kc = max(1, min(K - k0, kmax, self.HVP_BYTES_BUDGET // max(1, per_dir)))
            ws = torch.empty(ws_bytes(kc, opt) + 4096, dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                rc = call(opt, k0, kc, status.data_ptr(), ws.data_ptr(), ws.numel(), stream)
            _lib.check(rc, "aimnet_engine_" + name)
            self.last_status = st = status.cpu().numpy()
            del ws
            if st[6]:
                raise ValueError(f"HipEngine.{name}: invalid input: " + describe_input_flags(int(st[6]), n_mol))
            if not self.grow(st, opt, rq):  # (an overflow: the capacities have grown - repeat this sweep)
                k0 += kc

    def charge_response(self, coord, numbers, mol_idx, charge, vectors, cell=None, pbc=(True, True, True),
                        want_dipole: bool | None = None) -> dict[str, Any]:
        """The charges and their directional derivatives (csrc/hvp.hip, aimnet_engine_charge_response: the forward tangent half
        of `hvp`, stopped at the final charges): vectors [K, N, 3] -> `charges` [N], `dq` [K, N], for a 2-channel model `dspin`
        [K, N] (tangent of alpha - beta), and `dmu` [K, n_mol, 3], the tangent of every molecule's dipole moment sum q x.  Inputs
        as `hvp`; no Coulomb method or dispersion term enters (the charges do not see them).  The dipole moment of a periodic
        cell is not defined: `want_dipole` defaults to `cell is None` and `want_dipole=True` with a cell raises.  The K
        directions are split into sweeps by HVP_BYTES_BUDGET with this entry's own (smaller) workspace per direction."""
        import torch

        if want_dipole is None:
            want_dipole = cell is None
        if want_dipole and cell is not None:
            raise ValueError("HipEngine.charge_response: the dipole moment of a periodic cell is not defined (want_dipole=True with a cell)")
        inp, t = self._inputs("charge_response", coord, numbers, mol_idx, charge, cell, pbc)
        n, n_mol, dev = inp.n_atoms, inp.n_mol, self.device
        K, vectors = self._directions("charge_response", vectors, n)
        rq = capacity.Request("hvp", n, n_mol, cell is not None, _lib.COULOMB_NONE, 0.0)  # the short-range rows are all it needs
        res = {"charges": torch.empty(n, dtype=torch.float32, device=dev), "dq": torch.empty(K, n, dtype=torch.float32, device=dev)}
        if self.nq == 2:
            res["dspin"] = torch.empty(K, n, dtype=torch.float32, device=dev)
        if want_dipole:
            res["dmu"] = torch.empty(K, n_mol, 3, dtype=torch.float32, device=dev)

        def call(opt, k0, kc, *tail):
            part = {k: v[k0 : k0 + kc].data_ptr() for k, v in res.items() if k != "charges"}
            return self.lib.aimnet_engine_charge_response(self._h, C.byref(inp), C.byref(opt), vectors[k0 : k0 + kc].data_ptr(), kc,
                                                          res["charges"].data_ptr(), part["dq"], part.get("dspin"), part.get("dmu"), *tail)
        self._tangent_sweeps("charge_response", self.lib.aimnet_engine_charge_response_workspace_bytes, rq, K, self.HVP_MAX_DIRECTIONS, call)
        return res

    def set_profiling(self, level: int, every: int = 1) -> None:
        """0 off, 1 GEMM-vs-rest, 2 per kernel family (HIP events on the eval stream); `every` = record them on every
        n-th evaluation only (the events cost ~3 % of a 2 ms step; read_profile()["evals"] says how many were covered)."""
        _lib.check(self.lib.aimnet_engine_set_profile_sampling(self._h, int(every)), "aimnet_engine_set_profile_sampling")
        _lib.check(self.lib.aimnet_engine_set_profiling(self._h, int(level)), "aimnet_engine_set_profiling")

    def read_profile(self, reset: bool = True) -> dict[str, float]:
        """Milliseconds per kernel family accumulated since the last reset."""
        nf = len(_lib.PROF_FAMILIES)
        buf = (C.c_double * (nf + 1))()
        _lib.check(self.lib.aimnet_engine_profile_read(self._h, buf, nf + 1, 1 if reset else 0), "aimnet_engine_profile_read")
        res = {k: float(buf[i]) for i, k in enumerate(_lib.PROF_FAMILIES)}
        res["evals"] = float(buf[nf])
        return res

    def gemm_flops_per_atom(self, backward: bool = True) -> float:
        """Algorithmic (unpadded) FLOPs per atom of all GEMM launches of one eval: 2 MACs forward,
        plus the input-gradient GEMMs of the backward; the k->1 head layer is a dot kernel."""
        macs = 0
        for dims in self.spec.mlp_dims:
            macs += sum(dims[i] * dims[i + 1] for i in range(len(dims) - 1))
        hd = self.spec.head_dims
        macs += sum(hd[i] * hd[i + 1] for i in range(len(hd) - 2))
        total = 2.0 * macs * (2 if backward else 1)
        # pass 0, first layer: the 256 embedding columns are folded into a per-element bias table at create time, the GEMM
        # runs over the 448 conv columns (engine.hip, emb_bias0) - not counted, it is not executed
        total -= 2.0 * 256 * self.spec.mlp_dims[0][1]
        if backward:
            # the pass-0 input gradient with respect to the (constant) embedding block is never formed:
            # the last backward GEMM of pass 0 has N = 448, not 704 (engine.hip, "only the conv columns")
            d0 = self.spec.mlp_dims[0]
            total -= 2.0 * 256 * d0[1]
        return total

    def debug_view(self, name: str):
        """Intermediate of the last eval as a torch tensor view into the workspace (tests only)."""
        import torch

        off, n_elem = C.c_size_t(), C.c_size_t()
        esz, stride = C.c_int32(), C.c_int32()
        rc = self.lib.aimnet_engine_debug_view(self._h, name.encode(), C.byref(off), C.byref(n_elem), C.byref(esz), C.byref(stride))
        if rc != 0:
            raise KeyError(name)
        raw = self._ws[off.value : off.value + n_elem.value * esz.value]
        if name in _INT_VIEWS:
            t = raw.view(torch.int32)
        elif esz.value == 16:
            t = raw.view(torch.float32)
        else:
            t = raw.view(getattr(torch, _DTYPES[esz.value]))
        if stride.value > 1:
            per = stride.value * (4 if esz.value == 16 else 1)
            t = t.view(-1, per)
        return t


# ---- stand-alone op wrappers (parity tests of the reference operator boundaries) ------------------
def neighbor_list(coord, cutoff: float, mol_idx=None, cell=None, pbc=(True, True, True), max_nb: int = 128, fill_value=None):
    """nvalchemiops-contract neighbour list on the GPU: returns (nbmat i32 [N,max_nb], num_nb i32 [N],
    shifts i32 [N,max_nb,3] | None, coord_wrapped f32 [N,3], status (max_count, overflow))."""
    import torch

    lib = _lib.load()
    dev = coord.device
    coord = coord.to(torch.float32).contiguous()
    n = coord.shape[0]
    if mol_idx is None:
        mol_idx = torch.zeros(n, dtype=torch.int32, device=dev)
    mol_idx = mol_idx.to(device=dev, dtype=torch.int32).contiguous()
    n_mol = int(mol_idx.max().item()) + 1
    fill = n if fill_value is None else int(fill_value)
    n_cell = 0
    if cell is not None:
        cell = cell.to(device=dev, dtype=torch.float32).contiguous()
        n_cell = 1 if cell.ndim == 2 else cell.shape[0]
    nbmat = torch.empty(n, max_nb, dtype=torch.int32, device=dev)
    shifts = torch.empty(n, max_nb, 3, dtype=torch.int32, device=dev) if cell is not None else None
    num = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    xw = torch.empty(n, 3, dtype=torch.float32, device=dev)
    nbytes = int(lib.aimnet_neighbor_list_workspace_bytes(n, n_mol, max_nb))
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    p3 = (C.c_int32 * 3)(*[1 if bool(b) else 0 for b in pbc])
    with torch.cuda.device(dev):
        rc = lib.aimnet_neighbor_list(coord.data_ptr(), mol_idx.data_ptr(), n, n_mol, cell.data_ptr() if cell is not None else None,
                                      n_cell, C.byref(p3), float(cutoff), int(max_nb), fill, nbmat.data_ptr(),
                                      shifts.data_ptr() if shifts is not None else None, num.data_ptr(), status.data_ptr(),
                                      xw.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "aimnet_neighbor_list")
    st = status.cpu().numpy()
    return nbmat, num, shifts, xw, (int(st[0]), int(st[1]))


def conv_sv_2d_sp_fwd(a, idx, g):
    """torch.ops.aimnet.conv_sv_2d_sp_fwd contract (conv_sv_2d_sp_wp.py:252-275)."""
    import torch

    lib = _lib.load()
    B, A, G = a.shape
    M = idx.shape[1]
    a = a.to(torch.float32).contiguous()
    idx = idx.to(torch.int32).contiguous()
    g = g.to(torch.float32).contiguous()
    out = torch.empty(B, A, G, 4, dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        rc = lib.aimnet_conv_sv_2d_sp_fwd(a.data_ptr(), idx.data_ptr(), g.data_ptr(), out.data_ptr(), B, A, G, M,
                                          torch.cuda.current_stream(a.device).cuda_stream)
    _lib.check(rc, "aimnet_conv_sv_2d_sp_fwd")
    return out


def conv_sv_2d_sp_bwd(grad_out, a, idx, g):
    """torch.ops.aimnet.conv_sv_2d_sp_bwd contract (conv_sv_2d_sp_wp.py:285-340): (grad_a, grad_g)."""
    import torch

    lib = _lib.load()
    B, A, G = a.shape
    M = idx.shape[1]
    grad_out = grad_out.to(torch.float32).contiguous()
    a = a.to(torch.float32).contiguous()
    idx = idx.to(torch.int32).contiguous()
    g = g.to(torch.float32).contiguous()
    grad_a = torch.empty_like(a)
    grad_g = torch.empty_like(g)
    with torch.cuda.device(a.device):
        rc = lib.aimnet_conv_sv_2d_sp_bwd(grad_out.data_ptr(), a.data_ptr(), idx.data_ptr(), g.data_ptr(), grad_a.data_ptr(),
                                          grad_g.data_ptr(), B, A, G, M, torch.cuda.current_stream(a.device).cuda_stream)
    _lib.check(rc, "aimnet_conv_sv_2d_sp_bwd")
    return grad_a, grad_g


def conv_sv_2d_sp_bwd_bwd(grad_out, grad2_a, grad2_g, a, idx, g):
    """torch.ops.aimnet.conv_sv_2d_sp_bwd_bwd contract (conv_sv_2d_sp_wp.py:342-446):
    (grad_grad_output [B,A,G,4], grad_a_double [B,A,G], grad_g_double [B,M,G,4])."""
    import torch

    lib = _lib.load()
    B, A, G = a.shape
    M = idx.shape[1]
    f = lambda t: t.to(torch.float32).contiguous()  # noqa: E731
    grad_out, grad2_a, grad2_g, a, g = f(grad_out), f(grad2_a), f(grad2_g), f(a), f(g)
    idx = idx.to(torch.int32).contiguous()
    ggo = torch.empty(B, A, G, 4, dtype=torch.float32, device=a.device)
    ga2 = torch.empty_like(a)
    gg2 = torch.empty_like(g)
    with torch.cuda.device(a.device):
        rc = lib.aimnet_conv_sv_2d_sp_bwd_bwd(grad_out.data_ptr(), grad2_a.data_ptr(), grad2_g.data_ptr(), a.data_ptr(), idx.data_ptr(),
                                              g.data_ptr(), ggo.data_ptr(), ga2.data_ptr(), gg2.data_ptr(), B, A, G, M,
                                              torch.cuda.current_stream(a.device).cuda_stream)
    _lib.check(rc, "aimnet_conv_sv_2d_sp_bwd_bwd")
    return ggo, ga2, gg2
