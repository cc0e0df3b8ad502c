"""How large the neighbour rows, the Ewald k arrays and the PME mesh start, how they grow when the status words of an evaluation
report an overflow, and how they shrink - the AdaptiveNeighborList policy of the reference (neighbors.py:49-147), written once.
`HipEngine` (eval, hvp, check_deferred), `DomainDecomposedEngine` and `VerletSkinLists` all come here.  No torch: plain values in,
plain values out, so the whole policy runs in CPU tests."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import _lib

EWALD_METHODS = (_lib.COULOMB_EWALD, _lib.COULOMB_PME)
PME_START_MESH = 8192  # starting capacity of one system's PME mesh (points)
PME_RC_MAX = 10.0  # Angstrom: cap of the mesh method's real-space cutoff (csrc/pme.hip)


def round16(n: int) -> int:
    return ((int(n) + 15) // 16) * 16


def start_capacity(rc: float) -> int:
    """Row capacity for cutoff `rc` at a density of 0.2 atoms per A^3 (neighbors.py:49-63): 112 @ 5 A, 2832 @ 15 A."""
    return round16(int(0.2 * 4.0 / 3.0 * math.pi * rc**3))


def grown(cap: int, *needed: int) -> int:
    """After an overflow (neighbors.py:127-130): half as much again, or what the status words say was needed."""
    return round16(int(max(cap * 1.5, *needed)))


def shrunk(capacity: int, actual_max: int, target_utilization: float = 0.75) -> int:
    """The shrink rule (neighbors.py:135-139): a row capacity used to less than 2/3 of the 75 % target shrinks to actual / 0.75
    (multiples of 16, at least 16) - next call's workspace and list traffic follow."""
    if actual_max < (2.0 / 3.0) * target_utilization * capacity:
        return max(16, round16(int(actual_max / target_utilization)))
    return capacity


def ewald_k_capacity(need: int) -> int:
    """The Ewald k boxes did not fit; status[7] says how many entries they have."""
    return (int(need) * 5 // 4 + 7) // 8 * 8


def pme_mesh_capacity(need: int) -> int:
    """The PME mesh of the largest system did not fit; status[7] says how many points it has."""
    if need >= 2**31 - 1:
        raise ValueError("HipEngine: a cell vector of this system needs more than 512 PME mesh points (csrc/pme.hip PME_MAX_AXIS); "
                         "use coulomb='dsf' or a looser ewald_accuracy")
    return int(need) * 9 // 8 + 64


def ewald_list_cutoff(volumes, counts, accuracy: float) -> float:
    """Cutoff of the real-space list of Ewald summation in `hvp`: the largest r_c over the systems' cell `volumes` and atom `counts` -
    the host copy of ewald_setup_kernel's formula (the device verifies it, status[6] bit 6), widened by the rounding between the two."""
    vols, counts = np.asarray(volumes, dtype=np.float64), np.asarray(counts, dtype=np.float64)
    eta = (vols * vols / np.maximum(counts, 1)) ** (1.0 / 6.0) / math.sqrt(2.0 * math.pi)
    return float(np.max(math.sqrt(-2.0 * math.log(float(accuracy))) * eta)) * (1.0 + 1e-5)


STRAIN_TANGENT_BYTES = 36  # the armed strain tangent (csrc/hvp.hip): 9 floats of virial per atom, and 9 per direction and atom


def strain_tangent_bytes(n: int, k: int) -> int:
    """Workspace the armed strain tangent adds to a sweep of `k` directions on `n` atoms: its two buffers, each rounded up to the
    256 bytes every workspace buffer is aligned to (aimnet_engine_hvp_workspace_bytes reports the sum while armed)."""
    up = lambda b: (int(b) + 255) // 256 * 256  # noqa: E731
    return up(STRAIN_TANGENT_BYTES * n) + up(STRAIN_TANGENT_BYTES * n * k)


def same_cutoff(a: float, b: float) -> bool:
    """`d3_cutoff == dsf_rc` as the engine decides it (engine.hip, d3_shares_lr_list / np_walk): on the float32 values of
    aimnet_eval_options - every host-side copy of that rule goes through here."""
    return bool(np.float32(a) == np.float32(b))


def builds_lr_list(n: int, n_mol: int, periodic: bool, lists_given: bool, method: int, np_walk_on: bool, d3_on: bool,
                   d3_same_cutoff: bool) -> bool:
    """Whether aimnet_engine_eval materialises a long-range list (and so needs max_nb_lr > 0): the host copy of
    `eval_plan(...).lr == ListFrom::Built`, i.e. of plan_np_walk (csrc/eval_plan.h) with bbox_applies (csrc/engine.h) as its
    `bbox_ok`.  Periodic DSF walks the cell grid; so do non-periodic systems large enough for the bounding-box grid, unless the
    pair terms ride on a D3 list of the same cutoff.  tests/test_np_walk_rule.py holds the two against each other."""
    bbox_ok = n >= 1500 * n_mol  # bbox_applies(N, n_mol)
    np_walk = np_walk_on and bbox_ok and not (d3_on and d3_same_cutoff)
    return method == _lib.COULOMB_DSF and not periodic and not lists_given and not np_walk


@dataclass(frozen=True)
class Request:
    """What one `eval` / `hvp` call asks for, as far as the capacities and the options depend on it."""
    kind: str  # "eval" | "hvp"
    n: int
    n_mol: int
    periodic: bool
    method: int  # _lib.COULOMB_*
    lr_rc: float  # cutoff of the long-range list (dsf_rc; hvp with Ewald: the largest real-space cutoff of the batch)
    dsf_alpha: float = 0.2
    accuracy: float = 1e-6
    dftd3: dict | None = None
    widths: tuple = (0, 0, 0)  # of caller-supplied nbmat, nbmat_lr, nbmat_d3 (0: not given)
    flags: int = 0  # _lib.FORCES | _lib.STRESS
    np_walk_on: bool = True  # engine switch dsf_np_walk

    @property
    def d3_rc(self) -> float:
        return float(self.dftd3.get("cutoff", 15.0))


def overflowed(st, opt) -> bool:
    """One of the engine's own buffers was too small for this evaluation (its results are garbage: grow and repeat)."""
    return bool(st[2] or st[3] or st[5] or (opt.coulomb == _lib.COULOMB_EWALD and st[7] > opt.ewald_max_k) or
                (opt.coulomb == _lib.COULOMB_PME and st[7] > opt.pme_max_mesh))


class Capacities:
    """The capacities one engine keeps between calls.  `HipEngine` derives from this."""

    has_dftd3 = False
    _last_request = None  # (options, request) of the last aimnet_engine_eval (DomainDecomposedEngine grows from them)
    _pme_shrunk_for = None  # the request whose PME mesh capacity went back to the start (once per call)

    def __init__(self, rc: float):
        self.max_nb = start_capacity(rc)
        self._max_nb_lr: dict[float, int] = {}
        self._ewald_nb_lr = 0     # row capacity of the real-space list of Ewald summation in `hvp` (0: sized from r_c at first use)
        self._ewald_max_k = 8192  # capacity of the Ewald k arrays (entries; grows to what status[7] reports)
        self._emb_max_k = 8192    # of the periodic embedding's own k arrays (grows to what its status[0] reports, HipEngine._eval_embedded)
        self._pme_max_mesh = PME_START_MESH  # of one system's PME mesh (points; every system of a batch gets a slice)

    def lr_capacity(self, rc: float) -> int:
        return self._max_nb_lr.setdefault(rc, start_capacity(rc))

    _lr_capacity = lr_capacity

    def fill_options(self, rq: Request) -> _lib.EvalOptions:
        """aimnet_eval_options of `rq` at the current capacities."""
        opt = _lib.EvalOptions()
        opt.flags, opt.coulomb, opt.dsf_rc, opt.dsf_alpha, opt.max_nb = rq.flags, rq.method, rq.lr_rc, rq.dsf_alpha, self.max_nb
        if rq.kind == "hvp":  # the tangent sweep runs DSF on a list, periodic or not
            opt.max_nb_lr = self.lr_capacity(rq.lr_rc) if rq.method == _lib.COULOMB_DSF else 0
        elif rq.method == _lib.COULOMB_DSF and not rq.periodic:
            cap, d3 = self.lr_capacity(rq.lr_rc), rq.dftd3 is not None  # (the cutoff gets its entry whether or not a list is built)
            same = d3 and same_cutoff(rq.d3_rc, rq.lr_rc)
            opt.max_nb_lr = cap if builds_lr_list(rq.n, rq.n_mol, rq.periodic, bool(rq.widths[0]), rq.method, rq.np_walk_on, d3, same) else 0
        if rq.method in EWALD_METHODS:
            opt.ewald_accuracy, opt.ewald_max_k = rq.accuracy, self._ewald_max_k
            if rq.kind == "hvp":
                # r_c changes with every cell, atom count and accuracy: ONE capacity of its own (as _ewald_max_k for the k entries),
                # not a key per cutoff in _max_nb_lr; it only grows (an overflow repeats the sweep)
                self._ewald_nb_lr = opt.max_nb_lr = max(self._ewald_nb_lr, start_capacity(rq.lr_rc))
                if rq.method == _lib.COULOMB_PME:  # the armed mesh tangent: every (direction, system) slice has this many points
                    opt.pme_max_mesh = self._pme_max_mesh
            else:
                # the mesh workspace is n_mol slices of the LARGEST system's mesh this engine has seen (40 B per point): after one big
                # cell, a batch of many small ones would ask for n_mol x that.  Shrink to the starting capacity once per call (status[7]
                # grows it back to what THIS batch needs); if the batch itself is beyond the limit, say so instead of running out of
                # memory.  (the PME kernels index the systems through grid.y: <= 65 535)
                n_mol = rq.n_mol
                if rq.method == _lib.COULOMB_PME and (n_mol > 65535 or n_mol * self._pme_max_mesh * 40 > 64 << 30):
                    if n_mol > 65535 or self._pme_shrunk_for is rq or self._pme_max_mesh <= PME_START_MESH:
                        raise ValueError(f"HipEngine.eval(coulomb='pme'): {n_mol} systems x a mesh of {self._pme_max_mesh} points for the "
                                         "largest of them exceeds the PME workspace limit (64 GiB, 65 535 systems); split the batch, or use "
                                         "coulomb='ewald' / 'dsf'")
                    self._pme_shrunk_for, self._pme_max_mesh = rq, PME_START_MESH
                opt.pme_max_mesh = self._pme_max_mesh
        if rq.widths[0]:  # caller-supplied matrices: the row capacities are their widths (nothing can overflow)
            opt.max_nb, opt.max_nb_lr = round16(rq.widths[0]), round16(rq.widths[1]) if rq.widths[1] else 0
        if rq.dftd3 is not None:
            if not self.has_dftd3:
                raise RuntimeError("dftd3 requested but no DFT-D3 tables were uploaded (HipEngine.set_dftd3_tables)")
            d = rq.dftd3
            opt.dftd3, opt.d3_cutoff = 1, rq.d3_rc
            opt.d3_s6, opt.d3_s8, opt.d3_a1, opt.d3_a2 = float(d.get("s6", 1.0)), float(d["s8"]), float(d["a1"]), float(d["a2"])
            opt.d3_smoothing_on = rq.d3_rc * (1.0 - float(d.get("smoothing_fraction", 0.2)))
            opt.max_nb_d3 = self.lr_capacity(rq.d3_rc)
            if rq.widths[0]:
                opt.max_nb_d3 = round16(rq.widths[2] or rq.widths[1]) if (rq.widths[2] or rq.widths[1]) else 16
        return opt

    def grow(self, st, opt: _lib.EvalOptions, rq: Request) -> bool:
        """Grow what the status words `st` of the call made with (`opt`, `rq`) report as too small; True if anything grew (the
        call has to be repeated)."""
        if st[2]:
            self.max_nb = grown(self.max_nb, st[0])
        if st[3] and rq.kind == "hvp" and rq.method in EWALD_METHODS:
            self._ewald_nb_lr = grown(opt.max_nb_lr, st[1])
        elif st[3]:
            self._max_nb_lr[rq.lr_rc] = grown(opt.max_nb_lr, st[1])
        if opt.coulomb == _lib.COULOMB_EWALD and st[7] > opt.ewald_max_k:  # the k boxes did not fit: their size is now known
            self._ewald_max_k = ewald_k_capacity(st[7])
        if opt.coulomb == _lib.COULOMB_PME and st[7] > opt.pme_max_mesh:  # the mesh did not fit: its size is now known
            self._pme_max_mesh = pme_mesh_capacity(int(st[7]))
        if st[5]:  # D3 list (it may be stored in the LR buffers: grow both capacities)
            self._max_nb_lr[rq.d3_rc] = grown(max(opt.max_nb_d3, opt.max_nb_lr), st[4])
        return overflowed(st, opt)

    def grow_deferred(self, st, status7_pme: bool) -> bool:
        """`grow` for a stack of status rows [K, 8] whose requests are no longer at hand: every long-range capacity grows by the
        larger of the long-range and the D3 need."""
        rows, lr, need = bool(st[:, 2].any()), bool(st[:, 3].any() or st[:, 5].any()), int(st[:, 7].max())
        # status[7]: PME mesh points of the largest system, or Ewald k entries (0 for the other methods)
        mesh, k = status7_pme and need > self._pme_max_mesh, not status7_pme and need > self._ewald_max_k
        if rows:
            self.max_nb = grown(self.max_nb, st[:, 0].max())
        for rc in list(self._max_nb_lr) if lr else ():
            self._max_nb_lr[rc] = grown(self._max_nb_lr[rc], st[:, 1].max(), st[:, 4].max())
        if mesh:
            self._pme_max_mesh = pme_mesh_capacity(need)
        if k:
            self._ewald_max_k = ewald_k_capacity(need)
        return rows or lr or mesh or k

    def shrink(self, st, opt: _lib.EvalOptions, rq: Request) -> None:
        """After a synchronous evaluation that fitted: `shrunk` on the lists it built."""
        self.max_nb = shrunk(self.max_nb, int(st[0]))
        if opt.max_nb_lr > 0:
            self._max_nb_lr[rq.lr_rc] = shrunk(self._max_nb_lr[rq.lr_rc], int(st[1]))
        if rq.dftd3 is not None and opt.max_nb_d3 > 0 and st[4] > 0:
            self._max_nb_lr[rq.d3_rc] = shrunk(self._max_nb_lr[rq.d3_rc], int(st[4]))
