"""The cases and the fp64 reference of tests/test_gpu_conv_kernels.py, shared with tests/test_conv_cases.py (which checks, without a GPU,
that the reference agrees with autograd and with oracle/aimnet2_analytic.py, that the case table reaches every kernel instantiation, and
that the gates see the faults the GPU test is there for).  Host only: nothing here imports the library or touches a GPU.

What is under test: the conv kernels of csrc/conv.hip that every evaluation runs, ONE launch at a time through the aimnet_debug_conv_*
hooks - conv_fwd_kernel, unconcat_kernel, conv_bwd_kernel, unconcat_p0_kernel + conv_bwd_p0_kernel, pair_force_kernel.

Reference.  Plain torch in the requested dtype; the formulas are the `# kernel: conv_fwd / unconcat / conv_bwd` blocks of
oracle/aimnet2_analytic.py::evaluate (whose `radial_basis` is imported, not restated), per DIRECTED list entry p = (i -> j, u, d):
    F1[p] = rbar_ji: the half built on the centre's features a_i and the neighbour's Sbar_j   (conv_bwd_kernel's XE pair buffer)
    R[p]  = rbar_ij: the half built on the neighbour's features a_j and the centre's Sbar_i   (= F1[mirror p] on a symmetric list)
    combined form:      fgrad_i += sum_m F1 - R,            virial_i += sum_m -1/2 d u (x) (F1 - R)
    reverse-pair (XE):  pairbuf[p] (+)= F1[p],              virial_i += sum_m -d u (x) F1;   pair_force: fgrad_i + sum_m pb[p] - pb[mirror p]
    pass-0 moments XE:  pairbuf[p] += -R[p],                virial_i += sum_m -d u (x) (-R)  (conv_bwd_p0_kernel: "own moments only")
The per-atom virials of the combined and the reverse-pair forms are different partitions of one total: each is compared with its own
partition, the two forms with each other on the total ("virial_total", a block with its own yardstick).
Who adds what (read from conv_bwd_kernel's epilogue): the KERNEL forms abar_out = abar_in + xbar[:, :256] + conv term and
qbar_out = qbar_in + xbar[:, 704 : 704 + nq] + conv term itself (oracle: the `unconcat` block's `abar + xb[:, :A*G]` and `qbar + xb[:, c0:c0+nq]`
lines); unconcat_kernel writes only the vector planes 1..3 of Sbar - the scalar plane is read from xbar[:, 256:512] by conv_bwd itself.
The reference mirrors exactly that split.
Inputs are the fp32 arrays the kernel receives, promoted exactly; the geometry is the (u, d) of `pg` as given.  Each kernel gets the
ROUNDED fp64 result of the stage before it (Vsave for unconcat, Sbar for conv_bwd), so no kernel inherits another's rounding.

Lists are synthetic symmetric multigraphs (make_graph): every undirected edge has a random unit u and d in [0.7, rc), one in twelve
within 1e-3 of rc, and is stored as (i -> j, u, d) and (j -> i, -u, d); repeated pairs and self pairs i -> i (+u and -u in one row) come
out of the stub pairing as they fall - images in a cell smaller than the cutoff.  So 37 atoms carry any row count.  Entries within a row
are in random order; entries past a row's count hold valid-but-wrong ids and NaN geometry.

Row counts: REQUIRED (+ REQUIRED_DENSE with cap 208 where the reverse-pair form is off), around the forward chunk 64, the backward chunk
48, the four-wave split's ceil(cnt / 4) quarters and REV_ROW_MAX = 128.  A 37-atom case holds all of them; 7- and 13-atom cases hold a
rotating window, one atom's count is free (parity of the stub pairing).  Atom counts: 7 (split, < 8 blocks), 13 with split_max 0 (tail
of one wave), 37 with split_max 0 (10 blocks: the XCD-range path of atom_loop, uneven ranges), 37 split (37 blocks).

Magnitudes: a ~ N(0, 0.55) (the spread of a synth.py embedding row, afv = base + N(0, 0.15) with |base| ~ 0.5), q ~ N(0, 0.3) (the
synthetic model's charges), xbar ~ N(0, 0.5); agh / afv from synth.synthetic_state_dict(0) (two charge channels: the NSE variant of the
same seed), rc, eta and the shifts from loader.synthetic_spec(0).

Gate (per output block, test_conv_cases.py asserts how it is built): max(4 x yardstick, 8 x 2^-24 x |ref64|_max), yardstick =
|ref32 - ref64|_max of the block with this same reference evaluated in fp32 on the CPU.  Never derived from a kernel's output.

Case table: CASES (`case_table()` prints it); `instantiation(case)` names the template instantiation(s) a case launches, test_conv_cases.py asserts that the table
reaches all 21 + 36 + 4 of them and every unconcat_kernel<NQ>."""
from __future__ import annotations

import itertools
from dataclasses import dataclass
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import torch

from oracle.aimnet2_analytic import radial_basis

A, G, H = 16, 16, 12
NF, NV = A * G, A * H
CH_FWD, CH_BWD, CH_P0, REV_ROW_MAX, P0_AFV_LDS = 64, 48, 64, 128, 8  # csrc/conv.hip
REQUIRED = (0, 1, 2, 3, 5, 47, 48, 49, 63, 64, 65, 96, 127, 128)
REQUIRED_DENSE = REQUIRED + (129, 200)
CAP, CAP_DENSE, CAP_SMALL = 128, 208, 40
ELEMENTS = (1, 5, 6, 7, 8, 9, 14, 15, 16, 17, 33, 34, 35, 53)  # the finite non-zero rows of the synthetic embedding table
A_SCALE, Q_SCALE, XBAR_SCALE = 0.55, 0.3, 0.5
GATE_YARD, GATE_ULP = 4.0, 8.0 * 2.0**-24
H2_REL = 2.0**-23  # the h2 row format's documented representation error (include/aimnet_hip.h), relative, added to the gate


@dataclass(frozen=True)
class Case:
    name: str
    family: str          # "fwd", "bwd" (unconcat + conv_bwd [+ pair_force]), "p0" (unconcat_p0 + conv_bwd_p0 [+ pair_force])
    n: int
    cap: int
    nq: int = 0
    split_max: int = 0   # 0: one wave per atom; 1024: four waves per atom
    order: bool = False  # a random processing order instead of NULL
    ldx: int = 704
    x_split: int = 0     # fwd: 0 fp32 row, 1 bf3, 2 h2
    nelem: int = 0       # > 0: pass-0 form, a = embedding table, row_of = atomic numbers of `nelem` elements
    moments: bool = False  # fwd: ask for the element-moment kernel
    need_abar: bool = False
    stress: bool = False
    xe: bool = False     # reverse-pair form (pairbuf given)
    pb_accum: bool = False
    abar_in: bool = False
    window: int = 0      # which window of the required row counts a small case takes
    seed: int = 0

    @property
    def split(self) -> bool:
        return self.n <= self.split_max


def instantiation(c: Case) -> tuple[str, ...]:
    """the kernel template instantiation(s) the launchers select for this case (launch_conv_fwd / _bwd / _bwd_p0 of csrc/conv.hip)"""
    b = lambda v: "true" if v else "false"  # noqa: E731
    if c.family == "fwd":
        p0m = c.moments and c.nelem > 0 and c.nq == 0 and not c.split
        return (f"conv_fwd_kernel<{c.nq}, {b(c.split)}, {b(p0m)}, {c.x_split}>",)
    if c.family == "bwd":
        xe = c.xe and not c.split
        return (f"unconcat_kernel<{c.nq}>", f"conv_bwd_kernel<{c.nq}, {b(c.need_abar)}, {b(c.stress)}, {b(c.split)}, {b(xe)}>") + \
            (("pair_force_kernel",) if xe else ())
    return ("unconcat_p0_kernel", f"conv_bwd_p0_kernel<{b(c.stress)}, {b(c.xe)}>") + (("pair_force_kernel",) if c.xe else ())


ALL_INSTANTIATIONS = frozenset(
    [f"conv_fwd_kernel<{nq}, {sp}, false, {x3}>" for nq in (0, 1, 2) for sp in ("false", "true") for x3 in (0, 1, 2)]
    + [f"conv_fwd_kernel<0, false, true, {x3}>" for x3 in (0, 1, 2)]
    + [f"unconcat_kernel<{nq}>" for nq in (0, 1, 2)]
    + [f"conv_bwd_kernel<{nq}, {na}, {st}, {sp}, {xe}>" for nq in (0, 1, 2) for na in ("false", "true") for st in ("false", "true")
       for sp, xe in (("false", "false"), ("true", "false"), ("false", "true"))]
    + ["unconcat_p0_kernel", "pair_force_kernel"]
    + [f"conv_bwd_p0_kernel<{st}, {xe}>" for st in ("false", "true") for xe in ("false", "true")])


def _ldx_choices(nq: int) -> tuple[int, ...]:
    return {0: (704, 736, 768), 1: (736, 768), 2: (768,)}[nq]


def _build_cases() -> tuple[Case, ...]:
    out: list[Case] = []
    k = 0

    def add(**kw):
        nonlocal k
        k += 1
        c = Case(seed=1000 + k, window=k, order=bool(k % 2), **kw)
        out.append(c)

    # ---- forward: nq x split x row format, pass 0 through row gathers (split and not) and through element moments -------------------
    for i, (nq, split, x3) in enumerate(itertools.product((0, 1, 2), (False, True), (0, 1, 2))):
        n = (7, 37)[i % 2] if split else (13, 37)[i % 2]
        ld = _ldx_choices(nq)
        add(name=f"fwd_nq{nq}_{'split' if split else 'wave'}_x{x3}_n{n}", family="fwd", n=n, cap=CAP_DENSE if n == 37 else (CAP, CAP_DENSE)[i % 2],
            nq=nq, split_max=1024 if split else 0, ldx=ld[i % len(ld)], x_split=x3)
    for i, (split, x3) in enumerate(itertools.product((False, True), (0, 1, 2))):  # pass-0 row gathers: a = afv, row_of = numbers
        n = (37, 7)[i % 2] if split else (37, 13)[i % 2]
        add(name=f"fwd_rowof_{'split' if split else 'wave'}_x{x3}_n{n}", family="fwd", n=n, cap=CAP_DENSE if n == 37 else CAP,
            split_max=1024 if split else 0, ldx=(768, 704, 736)[i % 3], x_split=x3, nelem=(4, 12, 1)[i % 3])
    for i, (x3, nelem) in enumerate(((0, 12), (1, 4), (2, 1), (0, 4), (2, 12))):  # element moments (one wave per atom only)
        add(name=f"fwd_moments_x{x3}_e{nelem}_n{(37, 13)[i % 2]}", family="fwd", n=(37, 13)[i % 2], cap=CAP_DENSE if i % 2 == 0 else CAP,
            ldx=(704, 768, 736)[i % 3], x_split=x3, nelem=nelem, moments=True)
    add(name="fwd_cap40_nq1_wave_n13", family="fwd", n=13, cap=CAP_SMALL, nq=1, ldx=736)  # the `lane < cap` guard of the row prefetch
    add(name="fwd_cap40_moments_n13", family="fwd", n=13, cap=CAP_SMALL, nelem=4, moments=True)
    # ---- backward: nq x need_abar x stress x (one wave per atom, split, reverse-pair) ---------------------------------------------
    for i, (nq, na, st, form) in enumerate(itertools.product((0, 1, 2), (False, True), (False, True), ("wave", "split", "xe"))):
        n = {"wave": (13, 37), "split": (37, 7), "xe": (37, 13)}[form][(i // 3) % 2]
        xe = form == "xe"
        cap = CAP if xe else (CAP_DENSE if n == 37 else (CAP, CAP_DENSE)[i % 2])
        ld = _ldx_choices(nq)
        add(name=f"bwd_nq{nq}_{'abar' if na else 'noabar'}_{'stress' if st else 'nostress'}_{form}_n{n}", family="bwd", n=n, cap=cap, nq=nq,
            split_max=1024 if form == "split" else 0, ldx=ld[(i // 2) % len(ld)], need_abar=na, stress=st, xe=xe, pb_accum=xe and (nq + na + st) % 2 == 1,
            abar_in=na and i % 4 < 2, nelem=(0, 4, 0, 12)[i % 4] if nq == 0 else 0)
    add(name="bwd_cap40_nq1_wave_n13", family="bwd", n=13, cap=CAP_SMALL, nq=1, ldx=736, need_abar=True, stress=True)
    add(name="bwd_xe_given_but_split_n7", family="bwd", n=7, cap=CAP, nq=1, ldx=768, split_max=1024, need_abar=True, xe=True)  # pairbuf ignored
    # ---- pass-0 species moments: stress x reverse-pair, 1 / 4 / 12 elements present (12 > P0_AFV_LDS) --------------------------------
    for i, (st, xe, nelem) in enumerate(((False, False, 12), (True, False, 4), (False, True, 1), (True, True, 12), (True, False, 1),
                                         (False, True, 4), (True, True, 4), (False, False, 1))):
        n = (37, 13)[i % 2]
        add(name=f"p0_{'stress' if st else 'nostress'}_{'xe' if xe else 'comb'}_e{nelem}_n{n}", family="p0", n=n,
            cap=CAP if xe else (CAP_DENSE if n == 37 else CAP), ldx=(704, 736, 768)[i % 3], stress=st, xe=xe, nelem=nelem)
    add(name="p0_cap40_n13", family="p0", n=13, cap=CAP_SMALL, stress=True, nelem=4)
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------------------------
def row_counts(c: Case, rng) -> np.ndarray:
    """the row count of every atom: the required counts that fit `cap` (all of them on 37 atoms, a window on fewer), the rest free"""
    req = [v for v in (REQUIRED if c.cap <= CAP else REQUIRED_DENSE) if v <= c.cap]
    n_req = min(len(req), c.n - 1)
    start = (c.window * 5) % len(req)
    picked = [req[(start + t) % len(req)] for t in range(n_req)]
    free = rng.integers(4, min(c.cap, 40) + 1, c.n - n_req).tolist()
    cnt = np.array(picked + free, dtype=np.int64)
    if cnt.sum() % 2:  # the stub pairing needs an even total: the last (free) atom gives way
        cnt[-1] += 1 if cnt[-1] < c.cap else -1
    return cnt[rng.permutation(c.n)]


def make_graph(n: int, cap: int, cnt: np.ndarray, rc: float, rng, garbage: bool = True):
    """symmetric multigraph with the given row counts -> nb_idx [n][cap] i32, nb_cnt [n] i32, pg [n][cap][4] f32, rev [n][cap] i32
    (rev: position of the mirror entry in the row of nb_idx[i][m], the definition csrc/conv.hip gives for the reverse-pair map)"""
    stubs = np.repeat(np.arange(n), cnt)
    rng.shuffle(stubs)
    ne = len(stubs) // 2
    u = rng.normal(size=(ne, 3))
    u = (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    d = rng.uniform(0.7, rc, ne)
    near = rng.random(ne) < 1.0 / 12.0
    d[near] = rc - rng.uniform(1e-5, 1e-3, near.sum())
    d = np.minimum(d.astype(np.float32), np.nextafter(np.float32(rc), np.float32(0)))
    rows: list[list[tuple[int, int, int]]] = [[] for _ in range(n)]  # (edge, side, neighbour)
    for e in range(ne):
        i, j = int(stubs[2 * e]), int(stubs[2 * e + 1])
        rows[i].append((e, 0, j))
        rows[j].append((e, 1, i))
    junk = rng.integers(0, n, (n, cap)).astype(np.int32)  # (drawn either way: the clean twin of a case is the same graph)
    nb_idx = junk if garbage else np.zeros((n, cap), np.int32)
    pg = np.full((n, cap, 4), np.nan, np.float32) if garbage else np.tile(np.array([0, 0, 0, 1], np.float32), (n, cap, 1))
    rev = np.full((n, cap), -1, np.int32)
    where = {}
    for i in range(n):
        assert len(rows[i]) == cnt[i] <= cap
        for m, t in enumerate(rng.permutation(len(rows[i]))):
            e, side, j = rows[i][t]
            nb_idx[i, m] = j
            pg[i, m, :3] = u[e] if side == 0 else -u[e]
            pg[i, m, 3] = d[e]
            where[(e, side)] = (i, m)
    for (e, side), (i, m) in where.items():
        rev[i, m] = where[(e, 1 - side)][1]
    return nb_idx, cnt.astype(np.int32), pg, rev


@lru_cache(maxsize=None)
def model_tables():
    """afv [64][256], agh_a, agh_q (one and two channels) of the synthetic model; rc, eta, shifts of its spec; the slot tables the
    engine derives from afv (csrc/engine.hip, aimnet_engine_create)"""
    from aimnetcentral_amd import loader, synth

    sd1, sd2 = synth.synthetic_state_dict(0), synth.synthetic_state_dict(0, num_charge_channels=2)
    spec = loader.synthetic_spec(0)
    afv = np.asarray(sd1["afv.weight"], np.float32)
    finite = [z for z in range(64) if np.isfinite(afv[z]).all()]
    bad = [z for z in range(64) if z not in finite]
    z_of_slot = np.array(finite + bad[:1], np.int32)
    slot_of_z = np.full(64, len(finite), np.int32)
    slot_of_z[finite] = np.arange(len(finite))
    return SimpleNamespace(afv=afv, agh_a=np.asarray(sd1["conv_a.agh"], np.float32),
                           agh_q={1: np.asarray(sd1["conv_q.agh"], np.float32), 2: np.asarray(sd2["conv_q.agh"], np.float32)},
                           rc=float(spec.rc), eta=float(np.float32(spec.eta)), shifts=np.asarray(spec.shifts, np.float32)[:G].copy(),
                           z_of_slot=z_of_slot, slot_of_z=slot_of_z, nslots=len(z_of_slot))


@lru_cache(maxsize=None)
def inputs(c: Case, garbage: bool = True) -> SimpleNamespace:
    """every fp32 / int32 array the hooks receive for this case (numpy, read-only by convention)"""
    mt = model_tables()
    rng = np.random.default_rng(c.seed)
    f32 = lambda shape, s: (rng.normal(size=shape) * s).astype(np.float32)  # noqa: E731
    cnt = row_counts(c, rng)
    nb_idx, nb_cnt, pg, rev = make_graph(c.n, c.cap, cnt, mt.rc, rng, garbage)
    x = SimpleNamespace(case=c, n=c.n, cap=c.cap, nq=c.nq, nb_idx=nb_idx, nb_cnt=nb_cnt, pg=pg, rev=rev, rc=mt.rc, eta=mt.eta,
                        shifts=mt.shifts.copy(), agh_a=mt.agh_a, agh_q=mt.agh_q[c.nq] if c.nq else None,
                        order=rng.permutation(c.n).astype(np.int32) if c.order else None)
    if c.nelem:
        elems = np.array(ELEMENTS)[rng.permutation(len(ELEMENTS))[: c.nelem]]
        x.numbers = np.concatenate([elems, rng.choice(elems, c.n - len(elems))])[rng.permutation(c.n)].astype(np.int32) \
            if c.n >= len(elems) else rng.choice(elems, c.n).astype(np.int32)
        x.a, x.row_of = mt.afv, x.numbers
        x.aslot = mt.slot_of_z[x.numbers].astype(np.int32)
        x.present = np.array([sum(1 << int(s) for s in set(x.aslot.tolist()))], np.uint64)
        x.z_of_slot, x.nslots = mt.z_of_slot, mt.nslots
    else:
        x.a, x.row_of = f32((c.n, NF), A_SCALE), None
    x.q = f32((c.nq, c.n), Q_SCALE) if c.nq else None
    if c.family != "fwd":
        x.xbar = f32((c.n, c.ldx), XBAR_SCALE)
        x.abar_in = f32((c.n, NF), XBAR_SCALE) if c.abar_in else None
        x.qbar_in = f32((c.nq, c.n), XBAR_SCALE) if c.nq else None
        x.fgrad0, x.virial0 = f32((c.n, 3), 0.1), f32((c.n, 9), 0.1)
        x.pairbuf0 = np.concatenate([f32((c.n, c.cap, 3), 0.1), np.zeros((c.n, c.cap, 1), np.float32)], axis=-1)
    return x


# ---- deliberate faults (tests/test_conv_cases.py: every one must break a gate) ----------------------------------------------------------
FAULTS = ("shift", "chunk_last", "quarter_last", "uz", "agh_q_channel", "run_merge", "mirror_sign")


def _first_row(x, pred):
    for i in range(x.n):
        if pred(int(x.nb_cnt[i])):
            return i
    return None


def apply_fault(x: SimpleNamespace, fault: str | None, stage: str):
    """-> (inputs with the fault applied, per-entry options of the reference) or None where the fault has no meaning for the case.
    stage: "fwd", "unconcat", "bwd" (conv_bwd / conv_bwd_p0), "pair_force"."""
    c = x.case
    y = SimpleNamespace(**vars(x))
    opt = SimpleNamespace(entry_w=None, jr=None, mirror_w=None)
    if fault is None:
        return y, opt
    ones = lambda: np.ones((x.n, x.cap))  # noqa: E731
    if fault == "shift":  # one shift of the 16 off by 1 %
        if stage not in ("fwd", "bwd"):
            return None
        y.shifts = x.shifts.copy()
        y.shifts[9] *= np.float32(1.01)
    elif fault == "chunk_last":  # the last entry of a full chunk dropped
        if stage not in ("fwd", "bwd"):
            return None
        ch = CH_FWD if stage == "fwd" else (CH_P0 if c.family == "p0" else CH_BWD)
        q4 = lambda cnt: (cnt + 3) // 4 if c.split else cnt  # noqa: E731  (split: the chunks of the first quarter)
        i = _first_row(x, lambda cnt: q4(cnt) >= ch)
        if i is None:
            return None
        opt.entry_w = ones()
        opt.entry_w[i, ch - 1] = 0.0
    elif fault == "quarter_last":  # split form, cnt % 4 != 0: the last entry of the last (short) quarter dropped
        if stage not in ("fwd", "bwd") or not c.split or c.family == "p0":
            return None
        i = _first_row(x, lambda cnt: cnt % 4 != 0 and cnt > 4)
        if i is None:
            return None
        opt.entry_w = ones()
        opt.entry_w[i, int(x.nb_cnt[i]) - 1] = 0.0
    elif fault == "uz":  # u_z negated on one entry
        if stage not in ("fwd", "bwd"):
            return None
        i = _first_row(x, lambda cnt: cnt >= 3)
        y.pg = x.pg.copy()
        y.pg[i, 1, 2] = -y.pg[i, 1, 2]
    elif fault == "agh_q_channel":  # agh_q of channel 1 used for channel 0
        if c.nq != 2 or stage not in ("fwd", "unconcat"):
            return None
        y.agh_q = x.agh_q.copy()
        y.agh_q[0] = x.agh_q[1]
    elif fault == "run_merge":  # moment forms: one element's run merged into its neighbour's
        moment_stage = (stage == "fwd" and instantiation(c)[0].split(", ")[2] == "true") or (stage == "bwd" and c.family == "p0")
        if not moment_stage or c.nelem < 2:
            return None
        z = x.numbers[x.nb_idx]
        jr = z.copy()
        for i in range(x.n):
            zs = list(dict.fromkeys(z[i, : x.nb_cnt[i]].tolist()))
            if len(zs) >= 2:
                jr[i, : x.nb_cnt[i]][z[i, : x.nb_cnt[i]] == zs[1]] = zs[0]
                break
        else:
            return None
        opt.jr = jr
    elif fault == "mirror_sign":  # the mirror entry's F1 taken with the wrong sign
        if not ((stage == "pair_force" and c.xe and not c.split) or (stage == "bwd" and not (c.xe and not c.split))):
            return None
        i = _first_row(x, lambda cnt: cnt >= 2)
        opt.mirror_w = ones()
        opt.mirror_w[i, 1] = -1.0
    else:
        raise ValueError(fault)
    return y, opt


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def _t(v, dt):
    return None if v is None else torch.as_tensor(np.asarray(v)).to(dt)


def _geometry(x, dt, opt):
    """valid mask, neighbour ids, (u, d) with the unused tail made harmless, radial basis (times the fault's entry weights)"""
    n, cap = x.n, x.cap
    valid = torch.arange(cap).unsqueeze(0) < torch.as_tensor(x.nb_cnt).long().unsqueeze(1)
    nb = torch.where(valid, torch.as_tensor(x.nb_idx).long(), torch.zeros((), dtype=torch.long))
    pg = x.pg if isinstance(x.pg, torch.Tensor) else _t(x.pg, dt)
    u = torch.where(valid.unsqueeze(-1), pg[..., :3], torch.zeros((), dtype=dt))
    d = torch.where(valid, pg[..., 3], torch.ones((), dtype=dt))
    basis = SimpleNamespace(rc=x.rc, eta=torch.tensor(x.eta, dtype=torch.float32).to(dt), shifts=_t(x.shifts, dt))
    gs, dgs = radial_basis(basis, d, valid)
    w = torch.ones(n, cap, dtype=dt) if opt.entry_w is None else _t(opt.entry_w, dt)
    return valid, nb, u, d, gs, dgs, w


def _rows(x, dt, nb, opt):
    """feature table, the centre's row of it, the row of every entry's neighbour"""
    a = x.a if isinstance(x.a, torch.Tensor) else _t(x.a, dt)
    if x.row_of is None:
        return a.view(-1, A, G), torch.arange(x.n), nb
    z = torch.as_tensor(x.row_of).long()
    jr = z[nb] if opt.jr is None else torch.as_tensor(opt.jr).long()
    return a.view(-1, A, G), z, jr


def ref_forward(x, dt=torch.float64, opt=None) -> dict:
    """conv_fwd_kernel: the row [a | S_s | |V|^2 | q | S^q_s | |V^q|^2] as blocks, V [n][A][H][3], Vq [n][nq][H][3]"""
    opt = opt or SimpleNamespace(entry_w=None, jr=None, mirror_w=None)
    valid, nb, u, d, gs, _, w = _geometry(x, dt, opt)
    tab, ri, jr = _rows(x, dt, nb, opt)
    gw = gs * w.unsqueeze(-1)
    one_u = torch.cat([torch.ones_like(d).unsqueeze(-1), u], dim=-1)
    S = torch.einsum("nmag,nmg,nmc->nagc", tab[jr], gw, one_u)
    V = torch.einsum("agh,nagk->nahk", _t(x.agh_a, dt), S[..., 1:])
    out = {"a": tab[ri].reshape(x.n, NF), "S_s": S[..., 0].reshape(x.n, NF), "V2": V.pow(2).sum(-1).reshape(x.n, NV), "Vsave": V}
    if x.nq:
        q = (x.q if isinstance(x.q, torch.Tensor) else _t(x.q, dt)).t()  # [n][nq]
        Sq = torch.einsum("nmq,nmg,nmc->nqgc", q[nb], gw, one_u)
        Vq = torch.einsum("qgh,nqgk->nqhk", _t(x.agh_q, dt), Sq[..., 1:])
        out.update(q=q, Sq_s=Sq[..., 0].reshape(x.n, -1), Vq2=Vq.pow(2).sum(-1).reshape(x.n, -1), Vqsave=Vq)
    return out


FWD_ROW_BLOCKS = ("a", "S_s", "V2", "q", "Sq_s", "Vq2")


def forward_row(out: dict) -> torch.Tensor:
    return torch.cat([out[k] for k in FWD_ROW_BLOCKS if k in out], dim=-1)


def ref_unconcat(x, V, Vq, dt=torch.float64) -> dict:
    """unconcat_kernel: Sbar [n][A][G][4] (component 0 = xbar[:, 256:512], which the kernel leaves in xbar), Sqbar [n][nq][G][4]"""
    xb = x.xbar if isinstance(x.xbar, torch.Tensor) else _t(x.xbar, dt)
    n = x.n
    Sbar = torch.empty(n, A, G, 4, dtype=dt)
    Sbar[..., 0] = xb[:, NF : 2 * NF].view(n, A, G)
    Sbar[..., 1:] = torch.einsum("agh,nahk->nagk", _t(x.agh_a, dt), 2.0 * V * xb[:, 2 * NF : 2 * NF + NV].view(n, A, H).unsqueeze(-1))
    out = {"Sbar": Sbar}
    if x.nq:
        c0, nq = 2 * NF + NV, x.nq
        Sqbar = torch.empty(n, nq, G, 4, dtype=dt)
        Sqbar[..., 0] = xb[:, c0 + nq : c0 + nq + nq * G].view(n, nq, G)
        vqbar = xb[:, c0 + nq + nq * G : c0 + nq + nq * G + nq * H].view(n, nq, H)
        Sqbar[..., 1:] = torch.einsum("qgh,nqhk->nqgk", _t(x.agh_q, dt), 2.0 * Vq * vqbar.unsqueeze(-1))
        out["Sqbar"] = Sqbar
    return out


def ref_pairs(x, Sbar, Sqbar, dt=torch.float64, opt=None) -> dict:
    """per directed entry: F1 (rbar_ji), R (rbar_ij); per atom: the conv terms of abar and qbar (times the fault's entry weights)"""
    opt = opt or SimpleNamespace(entry_w=None, jr=None, mirror_w=None)
    valid, nb, u, d, gs, dgs, w = _geometry(x, dt, opt)
    tab, ri, jr = _rows(x, dt, nb, opt)
    a_i, a_j = tab[ri], tab[jr]
    Sb_j = Sbar[nb]
    Pp = Sb_j[..., 0] - torch.einsum("nmk,nmagk->nmag", u, Sb_j[..., 1:])
    ab = torch.einsum("nmg,nmag->nag", gs * w.unsqueeze(-1), Pp)
    P = Sbar[..., 0].unsqueeze(1) + torch.einsum("nmk,nagk->nmag", u, Sbar[..., 1:])
    dbar_ij = torch.einsum("nmag,nmag,nmg->nm", a_j, P, dgs)
    ubar_ij = torch.einsum("nmg,nmag,nagk->nmk", gs, a_j, Sbar[..., 1:])
    dbar_ji = torch.einsum("nag,nmag,nmg->nm", a_i, Pp, dgs)
    ubar_ji = torch.einsum("nmg,nag,nmagk->nmk", gs, a_i, Sb_j[..., 1:])
    qacc = None
    if x.nq:
        q = (x.q if isinstance(x.q, torch.Tensor) else _t(x.q, dt)).t()
        Sq_j = Sqbar[nb]
        Pqp = Sq_j[..., 0] - torch.einsum("nmk,nmqgk->nmqg", u, Sq_j[..., 1:])
        qacc = torch.einsum("nmg,nmqg->nq", gs * w.unsqueeze(-1), Pqp)
        Pq = Sqbar[..., 0].unsqueeze(1) + torch.einsum("nmk,nqgk->nmqg", u, Sqbar[..., 1:])
        qj = q[nb]
        dbar_ij = dbar_ij + torch.einsum("nmq,nmqg,nmg->nm", qj, Pq, dgs)
        ubar_ij = ubar_ij + torch.einsum("nmq,nmg,nqgk->nmk", qj, gs, Sqbar[..., 1:])
        dbar_ji = dbar_ji + torch.einsum("nq,nmqg,nmg->nm", q, Pqp, dgs)
        ubar_ji = ubar_ji + torch.einsum("nq,nmg,nmqgk->nmk", q, gs, Sq_j[..., 1:])
    vm = valid.to(dt).unsqueeze(-1)
    dinv = (1.0 / d).unsqueeze(-1)
    R = (dbar_ij.unsqueeze(-1) * u + (ubar_ij - (ubar_ij * u).sum(-1, keepdim=True) * u) * dinv) * vm
    F1 = (-dbar_ji.unsqueeze(-1) * u + (ubar_ji - (ubar_ji * u).sum(-1, keepdim=True) * u) * dinv) * vm
    return {"F1": F1, "R": R, "ab": ab, "qacc": qacc, "w": w * valid.to(dt), "r": u * d.unsqueeze(-1) * vm, "nb": nb, "valid": valid}


def mirror_of(x, F, opt=None):
    """F[mirror p] for every entry p (0 where there is none), through the reverse-pair map"""
    valid = torch.arange(x.cap).unsqueeze(0) < torch.as_tensor(x.nb_cnt).long().unsqueeze(1)
    rev = torch.as_tensor(x.rev).long()
    ok = valid & (rev >= 0)
    nb = torch.where(ok, torch.as_tensor(x.nb_idx).long(), torch.zeros((), dtype=torch.long))
    out = F[nb, rev.clamp(min=0)] * ok.to(F.dtype).unsqueeze(-1)
    if opt is not None and opt.mirror_w is not None:
        out = out * torch.as_tensor(opt.mirror_w).to(F.dtype).unsqueeze(-1)
    return out


def ref_backward(x, Sbar, Sqbar, dt=torch.float64, opt=None) -> dict:
    """conv_bwd_kernel / conv_bwd_p0_kernel (+ pair_force_kernel) in the form the case selects: abar, qbar, fgrad, virial, F1 (the
    pair buffer), forces - each only where that form writes it"""
    c = x.case
    opt = opt or SimpleNamespace(entry_w=None, jr=None, mirror_w=None)
    p = ref_pairs(x, Sbar, Sqbar, dt, opt)
    w3 = p["w"].unsqueeze(-1)
    xb = x.xbar if isinstance(x.xbar, torch.Tensor) else _t(x.xbar, dt)
    out = {}
    if c.family == "bwd" and c.need_abar:
        out["abar"] = p["ab"].reshape(x.n, NF) + xb[:, :NF] + (0.0 if x.abar_in is None else _t(x.abar_in, dt))
    if c.family == "bwd" and c.nq:
        out["qbar"] = _t(x.qbar_in, dt) + xb[:, 2 * NF + NV : 2 * NF + NV + c.nq].t() + p["qacc"].t()
    xe = c.xe and not c.split
    fgrad0, vir0 = _t(x.fgrad0, dt), _t(x.virial0, dt)
    if not xe:
        # the mirror half as the kernel has it - from the centre's own Sbar and the neighbour's features (R), not through the map
        Rm = p["R"] if opt.mirror_w is None else p["R"] * _t(opt.mirror_w, dt).unsqueeze(-1)
        f = (p["F1"] - Rm) * w3
        out["fgrad"] = fgrad0 + f.sum(1)
        if c.stress:
            out["virial"] = vir0 + torch.einsum("nma,nmb->nab", -0.5 * p["r"], f).reshape(x.n, 9)
            out["virial_total"] = out["virial"].sum(0)
        return out
    own = p["F1"] if c.family == "bwd" else -p["R"]  # pass-0 moments: the half on the centre's OWN moments
    prev = _t(x.pairbuf0[..., :3], dt) if (c.pb_accum or c.family == "p0") else 0.0
    pb = (prev + own * w3) * p["valid"].to(dt).unsqueeze(-1)
    out["F1"] = pb
    if c.stress:
        out["virial"] = vir0 + torch.einsum("nma,nmb->nab", -p["r"], own * w3).reshape(x.n, 9)
        out["virial_total"] = out["virial"].sum(0)
    out["forces"] = -(fgrad0 + (pb - mirror_of(x, pb, opt)).sum(1))  # pair_force_kernel on the pair buffer as conv_bwd left it
    return out


# ---- one cached evaluation per (case, dtype): the shared reference of every test ------------------------------------------------------
@lru_cache(maxsize=None)
def stage_inputs(c: Case) -> SimpleNamespace:
    """fp32 inputs of the later stages, rounded from the fp64 reference of the earlier ones: Vsave / Vqsave (unconcat, unconcat_p0) and
    Sbar / Sqbar (conv_bwd)"""
    x = inputs(c)
    f = ref_forward(x)
    s = SimpleNamespace(Vsave=f["Vsave"].float().numpy(), Vqsave=f["Vqsave"].float().numpy() if c.nq else None)
    u = ref_unconcat(x, torch.as_tensor(s.Vsave).double(), None if s.Vqsave is None else torch.as_tensor(s.Vqsave).double())
    s.Sbar = u["Sbar"].float().numpy()
    s.Sqbar = u["Sqbar"].float().numpy() if c.nq else None
    return s


def reference(c: Case, dt=torch.float64, fault: str | None = None, stage: str | None = None) -> dict | None:
    """every output block of the case in `dt`; with a fault: the blocks of `stage` under that fault (None where it has no meaning)"""
    x = inputs(c)
    if c.family == "fwd":
        fx = apply_fault(x, fault, "fwd")
        return None if fx is None else ref_forward(fx[0], dt, fx[1])
    s = stage_inputs(c)
    out = {}
    if c.family == "bwd" and stage in (None, "unconcat"):
        fx = apply_fault(x, fault, "unconcat")
        if fx is None:
            return None
        out.update(ref_unconcat(fx[0], _t(s.Vsave, dt), _t(s.Vqsave, dt), dt))
        if stage == "unconcat":
            return out
    # pass 0 recomputes Sbar from xbar and Vsave inside unconcat_p0_kernel; conv_bwd receives the rounded Sbar
    if c.family == "p0":
        Sbar, Sqbar = ref_unconcat(x, _t(s.Vsave, dt), None, dt)["Sbar"], None
    else:
        Sbar, Sqbar = _t(s.Sbar, dt).clone(), _t(s.Sqbar, dt)
        Sbar[..., 0] = _t(x.xbar, dt)[:, NF : 2 * NF].view(x.n, A, G)
    fx = apply_fault(x, fault, stage or "bwd")
    if fx is None:
        return None
    out.update(ref_backward(fx[0], Sbar, Sqbar, dt, fx[1]))
    return out


@lru_cache(maxsize=None)
def ref64(c: Case) -> dict:
    return reference(c, torch.float64)


@lru_cache(maxsize=None)
def gates(c: Case) -> dict:
    """block -> (gate, yardstick, |ref64|_max); the gate is built from the reference alone"""
    r64, r32 = ref64(c), reference(c, torch.float32)
    out = {}
    for k, v in r64.items():
        yard = float((r32[k].double() - v).abs().max()) if v.numel() else 0.0
        top = float(v.abs().max()) if v.numel() else 0.0
        gate = max(GATE_YARD * yard, GATE_ULP * top)
        if c.family == "fwd" and c.x_split == 2 and k in FWD_ROW_BLOCKS:
            gate += H2_REL * top
        out[k] = (gate, yard, top)
    return out


CASES = _build_cases()


def case_table() -> str:
    """which case covers which instantiation, one line per case"""
    return "\n".join(f"{c.name:44s} n {c.n:2d} cap {c.cap:3d} ldx {c.ldx} order {int(c.order)}  {', '.join(instantiation(c))}" for c in CASES)

FAMILY_STAGES = {"fwd": ("fwd",), "bwd": ("unconcat", "bwd", "pair_force"), "p0": ("bwd", "pair_force")}
