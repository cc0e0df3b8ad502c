"""The conv kernels that every evaluation runs (csrc/conv.hip), ONE launch at a time through the aimnet_debug_conv_* hooks, against the fp64
reference of tests/conv_cases.py at its gate: per output block max(4 x |ref32 - ref64|_max, 8 x 2^-24 x |ref64|_max), built from the
reference alone (tests/test_conv_cases.py shows, without a GPU, that a wrong shift, a dropped chunk or quarter entry, a flipped u_z, a
swapped agh_q channel, a merged element run and a wrong mirror sign all break it).  No engine evaluation, no workload-sized input.

Every case (conv_cases.CASES: every template instantiation the three launchers can select, row counts around the chunk sizes, the split
quarters and the reverse-pair row limit, 7 / 13 / 37 atoms, processing orders, row strides, row formats, 1 / 4 / 12 elements) is launched
twice: every output block against fp64, no element excluded; the two launches bit for bit; rows without neighbours exactly; outputs a form
does not own left untouched.  Entries past a row's count hold valid-but-wrong ids and NaN geometry throughout; `test_garbage_*` shows
against a clean fill that they reach nothing.  Variants that compute the same numbers agree within twice the gate.

Each comparison prints `CONVK <case> <block> err yardstick err/yardstick gate` before it asserts (profiles/conv_kernels_fp64.md)."""
from __future__ import annotations

import ctypes as C
from dataclasses import replace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import conv_cases as K
from conv_cases import A, G, H, NF, NV
from test_gpu_split_gemm import unsplit2, unsplit3

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _lib():
    from aimnetcentral_amd import _lib

    return _lib.load(), _lib


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _d(v):
    if v is None:
        return None
    v = np.ascontiguousarray(v)
    if v.dtype == np.uint64:
        v = v.view(np.int64)
    return torch.from_numpy(v).to(DEV)


def _p(t):
    return None if t is None else t.data_ptr()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _basis(x):
    return C.c_float(x.rc), C.c_float(x.eta), (C.c_float * 16)(*[float(v) for v in x.shifts])


def _ok(rc, what):
    lib, L = _lib()
    assert rc == 0, f"{what}: {rc} {L.last_error()}"
    torch.cuda.synchronize()


UNSET = object()


# ---- launches -------------------------------------------------------------------------------------------------------------------------------
def run_fwd(x, *, split_max=None, order=UNSET, moments=None):
    """-> blocks (fp64, CPU, reference layouts), pad columns of the row, raw outputs"""
    lib, _ = _lib()
    c = x.case
    split_max = c.split_max if split_max is None else split_max
    order = x.order if order is UNSET else order
    moments = c.moments if moments is None else moments
    n, nq, ldx = x.n, x.nq, c.ldx
    if c.x_split == 0:
        xr = _nan(n, ldx)
    else:
        xr = torch.full((n, (3 if c.x_split == 1 else 2) * ldx), 0x7E5B, dtype=torch.int16, device=DEV)
    Vs, Vq = _nan(n, 3, NV), (_nan(n, nq, H, 3) if nq else None)
    keep = [_d(x.a), _d(x.row_of), _d(x.q), _d(x.nb_idx), _d(x.nb_cnt), _d(x.pg), _d(x.agh_a), _d(x.agh_q), _d(order)]
    a, row_of, q, nb_idx, nb_cnt, pg, agh_a, agh_q, od = keep
    rc, eta, sh = _basis(x)
    _ok(lib.aimnet_debug_conv_fwd(nq, _p(a), _p(row_of), _p(q), _p(nb_idx), _p(nb_cnt), _p(pg), x.cap, _p(agh_a), _p(agh_q), rc, eta, sh,
                                  _p(xr), ldx, _p(Vs), _p(Vq), n, _p(od), int(moments), split_max, c.x_split, _stream()), "conv_fwd")
    row = xr.double() if c.x_split == 0 else (unsplit3(xr, ldx) if c.x_split == 1 else unsplit2(xr, ldx))
    row = row.cpu()
    out = {"a": row[:, :NF], "S_s": row[:, NF : 2 * NF], "V2": row[:, 2 * NF : 2 * NF + NV],
           "Vsave": Vs.double().cpu().view(n, 3, A, H).permute(0, 2, 3, 1)}
    used = 2 * NF + NV
    if nq:
        out.update(q=row[:, used : used + nq], Sq_s=row[:, used + nq : used + nq + nq * G],
                   Vq2=row[:, used + nq + nq * G : used + nq * (1 + G + H)], Vqsave=Vq.double().cpu())
        used += nq * (1 + G + H)
    return out, row[:, used:], [xr, Vs] + ([Vq] if nq else [])


def _kernel_V(V):  # reference V [n][A][H][3] -> Vsave [n][3][192]
    return np.ascontiguousarray(np.transpose(V, (0, 3, 1, 2)).reshape(V.shape[0], 3, NV))


def run_unconcat(x, s):
    lib, _ = _lib()
    n, nq = x.n, x.nq
    Sbar, Sqbar = _nan(n, 4, A, G), (_nan(n, nq, G, 4) if nq else None)
    xbar, Vs, Vq, agh_a, agh_q = _d(x.xbar), _d(_kernel_V(s.Vsave)), _d(s.Vqsave), _d(x.agh_a), _d(x.agh_q)
    _ok(lib.aimnet_debug_unconcat(nq, _p(xbar), x.case.ldx, _p(Vs), _p(Vq), _p(agh_a), _p(agh_q), _p(Sbar), _p(Sqbar), n, _stream()),
        "unconcat")
    assert torch.isnan(Sbar[:, 0]).all(), "unconcat wrote the scalar plane of Sbar (conv_bwd reads it from xbar)"
    out = {"Sbar": Sbar.double().cpu().permute(0, 2, 3, 1).contiguous()}
    out["Sbar"][..., 0] = torch.from_numpy(x.xbar[:, NF : 2 * NF]).double().view(n, A, G)  # (where conv_bwd reads that plane)
    if nq:
        out["Sqbar"] = Sqbar.double().cpu()
    return out, [Sbar] + ([Sqbar] if nq else [])


def _valid(x):
    return torch.arange(x.cap).unsqueeze(0) < torch.as_tensor(x.nb_cnt).long().unsqueeze(1)


def _pair_force(x, lists, pairbuf, fgrad):
    lib, _ = _lib()
    forces, rev = _nan(x.n, 3), _d(x.rev)
    _ok(lib.aimnet_debug_pair_force(_p(lists[0]), _p(lists[1]), _p(rev), _p(pairbuf), x.cap, x.n, _p(fgrad), _p(forces), _stream()),
        "pair_force")
    return forces


def _pairbuf_blocks(x, pairbuf, before):
    v = _valid(x)
    pb = pairbuf.cpu()
    assert (pb[..., 3][v] == 0).all()
    assert torch.equal(pb[~v].view(torch.int32), before.cpu()[~v].view(torch.int32)), "pair buffer written past a row's count"
    return torch.where(v.unsqueeze(-1), pb[..., :3].double(), torch.zeros((), dtype=torch.float64))


def run_bwd(x, s, *, split_max=None, order=UNSET, xe=None, pb_zero=False):
    """conv_bwd (+ pair_force in the reverse-pair form) on the rounded fp64 Sbar / Sqbar -> blocks, raw outputs"""
    lib, _ = _lib()
    c = x.case
    split_max = c.split_max if split_max is None else split_max
    order = x.order if order is UNSET else order
    xe = c.xe if xe is None else xe
    n, nq = x.n, x.nq
    Sb = np.ascontiguousarray(np.transpose(s.Sbar, (0, 3, 1, 2)))
    Sb[:, 0] = np.nan  # the scalar plane lives in xbar: whatever is here must not be read
    a, row_of, q, Sbar, Sqbar = _d(x.a), _d(x.row_of), _d(x.q), _d(Sb), _d(s.Sqbar)
    nb_idx, nb_cnt, pg, xbar, od = _d(x.nb_idx), _d(x.nb_cnt), _d(x.pg), _d(x.xbar), _d(order)
    abar_in, abar_out, qbar_in, qbar_out = _d(x.abar_in), _nan(n, NF), _d(x.qbar_in), (_nan(nq, n) if nq else None)
    fgrad, virial = _d(x.fgrad0), _d(x.virial0)
    pb0 = (_d(x.pairbuf0) if (c.pb_accum or n <= split_max) else _nan(n, x.cap, 4)) if xe else None
    if pb_zero and xe:  # (variant comparisons: nothing from an earlier pass in the pair buffer)
        pb0 = torch.zeros(n, x.cap, 4, device=DEV)
    pairbuf = None if pb0 is None else pb0.clone()
    rc, eta, sh = _basis(x)
    _ok(lib.aimnet_debug_conv_bwd(nq, int(c.need_abar), int(c.stress), _p(a), _p(row_of), _p(q), _p(Sbar), _p(Sqbar), _p(nb_idx),
                                  _p(nb_cnt), _p(pg), x.cap, rc, eta, sh, _p(xbar), c.ldx, _p(abar_in), _p(abar_out), _p(qbar_in),
                                  _p(qbar_out), _p(fgrad), _p(virial), n, _p(od), _p(pairbuf), int(c.pb_accum), split_max, _stream()),
        "conv_bwd")
    out, raw = {}, [abar_out, fgrad, virial] + ([qbar_out] if nq else []) + ([pairbuf] if xe else [])
    if c.need_abar:
        out["abar"] = abar_out.double().cpu()
    else:
        assert torch.isnan(abar_out).all(), "abar_out written without need_abar"
    if nq:
        out["qbar"] = qbar_out.double().cpu()
    if c.stress:
        out["virial"] = virial.double().cpu()
        out["virial_total"] = out["virial"].sum(0)
    else:
        assert torch.equal(virial.cpu(), torch.from_numpy(x.virial0)), "virial written without a stress request"
    if xe and n > split_max:
        assert torch.equal(fgrad.cpu(), torch.from_numpy(x.fgrad0)), "the reverse-pair form touched fgrad"
        out["F1"] = _pairbuf_blocks(x, pairbuf, pb0)
        forces = _pair_force(x, (nb_idx, nb_cnt), pairbuf, fgrad)
        out["forces"] = forces.double().cpu()
        raw.append(forces)
    else:
        if xe:
            assert torch.equal(pairbuf.cpu(), pb0.cpu()), "the split form has no reverse-pair variant: pairbuf must stay as it was"
        out["fgrad"] = fgrad.double().cpu()
    return out, raw


def run_p0(x, s, *, order=UNSET, xe=None, pb_zero=False):
    lib, _ = _lib()
    c = x.case
    order = x.order if order is UNSET else order
    xe = c.xe if xe is None else xe
    n = x.n
    xbar, Vs, agh_a, afv, zos, present, aslot = (_d(x.xbar), _d(_kernel_V(s.Vsave)), _d(x.agh_a), _d(x.a), _d(x.z_of_slot), _d(x.present),
                                                  _d(x.aslot))
    nb_idx, nb_cnt, pg, od = _d(x.nb_idx), _d(x.nb_cnt), _d(x.pg), _d(order)
    T, fgrad, virial = _nan(n, x.nslots, 64), _d(x.fgrad0), _d(x.virial0)
    pb0 = (torch.zeros(n, x.cap, 4, device=DEV) if pb_zero else _d(x.pairbuf0)) if xe else None
    pairbuf = None if pb0 is None else pb0.clone()
    rc, eta, sh = _basis(x)
    _ok(lib.aimnet_debug_conv_bwd_p0(int(c.stress), _p(xbar), c.ldx, _p(Vs), _p(agh_a), _p(afv), _p(zos), x.nslots, _p(present), 1,
                                     _p(aslot), _p(nb_idx), _p(nb_cnt), _p(pg), x.cap, rc, eta, sh, _p(T), _p(fgrad), _p(virial), n,
                                     _p(od), _p(pairbuf), _stream()), "conv_bwd_p0")
    out, raw = {}, [fgrad, virial, T] + ([pairbuf] if xe else [])
    here = sorted(set(x.aslot.tolist()))
    Tc = T.cpu()
    assert torch.isfinite(Tc[:, here]).all() and torch.isnan(Tc[:, [k for k in range(x.nslots) if k not in here]]).all()
    if c.stress:
        out["virial"] = virial.double().cpu()
        out["virial_total"] = out["virial"].sum(0)
    else:
        assert torch.equal(virial.cpu(), torch.from_numpy(x.virial0))
    if xe:
        assert torch.equal(fgrad.cpu(), torch.from_numpy(x.fgrad0))
        out["F1"] = _pairbuf_blocks(x, pairbuf, pb0)
        forces = _pair_force(x, (nb_idx, nb_cnt), pairbuf, fgrad)
        out["forces"] = forces.double().cpu()
        raw.append(forces)
    else:
        out["fgrad"] = fgrad.double().cpu()
    return out, raw


def run_case(c, garbage=True, **kw):
    """every launch of the case -> (blocks, raw outputs)"""
    x = K.inputs(c, garbage)
    if c.family == "fwd":
        out, pad, raw = run_fwd(x, **kw)
        assert (pad == 0).all(), "the K padding of the row is not zero"
        return out, raw
    s = K.stage_inputs(c)
    if c.family == "p0":
        return run_p0(x, s, **kw)
    out, raw = run_unconcat(x, s)
    o2, r2 = run_bwd(x, s, **kw)
    out.update(o2)
    return out, raw + r2


# ---- comparisons ----------------------------------------------------------------------------------------------------------------------------
def _bits_equal(ra, rb):
    return all(torch.equal(p.contiguous().view(torch.uint8), q.contiguous().view(torch.uint8)) for p, q in zip(ra, rb))


def _against_fp64(c, out):
    ref, gates = K.ref64(c), K.gates(c)
    assert set(out) == set(ref), (sorted(out), sorted(ref))
    worst = []
    for k in sorted(ref):
        gate, yard, top = gates[k]
        err = float((out[k] - ref[k]).abs().max())
        print(f"CONVK {c.name} {k} err {err:.3e} yardstick {yard:.3e} ratio {err / yard if yard else 0.0:.2f} gate {gate:.3e} scale {top:.3e}")
        if not err <= gate:
            worst.append(f"{k}: |gpu - ref64| {err:.3e} > gate {gate:.3e} (yardstick {yard:.3e}, scale {top:.3e})")
    assert not worst, f"{c.name} [{', '.join(K.instantiation(c))}]: " + "; ".join(worst)


def _empty_rows_exact(c, out):
    x = K.inputs(c)
    z = torch.as_tensor(x.nb_cnt == 0)
    if not z.any():
        return
    if c.family == "fwd":
        for k in ("S_s", "V2", "Vsave", "Sq_s", "Vq2", "Vqsave"):
            if k in out:
                assert (out[k][z] == 0).all(), f"{k} of a row without neighbours"
        ai = x.a[x.row_of] if x.row_of is not None else x.a
        if c.x_split != 2:  # (bf3 is exact; h2 keeps fp32 only to 2^-23)
            assert torch.equal(out["a"][z], torch.from_numpy(ai).double()[z])
        return
    if "fgrad" in out:
        assert torch.equal(out["fgrad"][z], torch.from_numpy(x.fgrad0).double()[z])
    if "forces" in out:
        assert torch.equal(out["forces"][z], -torch.from_numpy(x.fgrad0).double()[z])
    if "virial" in out:
        assert torch.equal(out["virial"][z], torch.from_numpy(x.virial0).double()[z])
    if "abar" in out:
        want = torch.from_numpy(x.xbar[:, :NF] + (x.abar_in if x.abar_in is not None else np.float32(0)))
        assert torch.equal(out["abar"][z], want.double()[z])
    if "qbar" in out:
        want = torch.from_numpy(x.qbar_in + x.xbar[:, 2 * NF + NV : 2 * NF + NV + c.nq].T)
        assert torch.equal(out["qbar"][:, z], want.double()[:, z])


@pytest.mark.parametrize("c", K.CASES, ids=lambda c: c.name)
def test_kernel_against_fp64_and_repeatable(c):
    out, raw = run_case(c)
    out2, raw2 = run_case(c)
    _against_fp64(c, out)
    _empty_rows_exact(c, out)
    assert _bits_equal(raw, raw2), "two launches of the same case differ"


def _first(pred):
    return next(c for c in K.CASES if pred(c))


# one case per kernel form (the first of the table), the small-capacity rows and the densest element mix
GARBAGE_CASES = [_first(lambda c: c.family == "fwd" and c.nq == 1 and not c.split and c.n == 37),
                 _first(lambda c: c.family == "fwd" and c.nq == 2 and c.split and c.x_split == 2),
                 _first(lambda c: c.family == "fwd" and c.moments and c.nelem == 12),
                 _first(lambda c: c.family == "fwd" and c.cap == K.CAP_SMALL),
                 _first(lambda c: c.family == "bwd" and c.nq == 1 and c.stress and c.need_abar and not c.split and not c.xe),
                 _first(lambda c: c.family == "bwd" and c.nq == 2 and c.stress and c.need_abar and c.split),
                 _first(lambda c: c.family == "bwd" and c.nq == 1 and c.stress and c.need_abar and c.xe and not c.split),
                 _first(lambda c: c.family == "p0" and c.xe and c.stress and c.nelem == 12),
                 _first(lambda c: c.family == "p0" and not c.xe and c.nelem == 12)]


@pytest.mark.parametrize("c", GARBAGE_CASES, ids=lambda c: c.name)
def test_garbage_past_the_row_count_reaches_nothing(c):
    xg, xc = K.inputs(c), K.inputs(c, False)
    v = _valid(xg).numpy()
    assert (xg.nb_idx[v] == xc.nb_idx[v]).all() and (xg.pg[v] == xc.pg[v]).all() and np.isnan(xg.pg[~v]).all() and (xc.nb_idx[~v] == 0).all()
    out_g, _ = run_case(c)
    out_c, _ = run_case(c, False)
    for k in out_g:
        assert torch.equal(out_g[k], out_c[k]), k


# ---- variants that compute the same numbers -------------------------------------------------------------------------------------------------
def _agree(c, oa, ob, what, keys=None):
    gates = K.gates(c)
    for k in keys or sorted(set(oa) & set(ob)):
        err = float((oa[k] - ob[k]).abs().max())
        print(f"CONVV {c.name} {what} {k} diff {err:.3e} gate {gates[k][0]:.3e}")
        assert err <= 2.0 * gates[k][0], f"{c.name} {what} {k}: {err:.3e} > 2 x {gates[k][0]:.3e}"


def _pick(pred, k=3):
    got = [c for c in K.CASES if pred(c)]
    assert len(got) >= k
    return got[:: max(1, len(got) // k)][:k]


@pytest.mark.parametrize("c", _pick(lambda c: c.family == "fwd" and c.n == 37 and not c.moments, 4), ids=lambda c: c.name)
def test_forward_split_agrees_with_one_wave_per_atom(c):
    x = K.inputs(c)
    _agree(c, run_fwd(x, split_max=0)[0], run_fwd(x, split_max=1024)[0], "split/wave")


@pytest.mark.parametrize("c", _pick(lambda c: c.family == "bwd" and c.n == 37 and not c.xe, 4), ids=lambda c: c.name)
def test_backward_split_agrees_with_one_wave_per_atom(c):
    x, s = K.inputs(c), K.stage_inputs(c)
    _agree(c, run_bwd(x, s, split_max=0)[0], run_bwd(x, s, split_max=1024)[0], "split/wave")


@pytest.mark.parametrize("c", [c for c in K.CASES if c.family == "fwd" and c.moments], ids=lambda c: c.name)
def test_forward_moment_form_agrees_with_row_gathers(c):
    x = K.inputs(c)
    _agree(c, run_fwd(x, moments=True)[0], run_fwd(x, moments=False)[0], "moments/gathers")


@pytest.mark.parametrize("c", [c for c in K.CASES if c.family == "p0" and not c.xe], ids=lambda c: c.name)
def test_backward_moment_form_agrees_with_row_gathers(c):
    """conv_bwd_p0 against the generic conv_bwd on a = embedding table, row_of = atomic numbers (what "p0_moments" = 0 runs)"""
    x, s = K.inputs(c), K.stage_inputs(c)
    xg = SimpleNamespace(**vars(x))
    xg.case = replace(c, family="bwd")
    xg.abar_in = xg.qbar_in = None
    keys = ["fgrad"] + (["virial", "virial_total"] if c.stress else [])
    _agree(c, run_p0(x, s)[0], run_bwd(xg, s)[0], "moments/gathers", keys)


@pytest.mark.parametrize("c", _pick(lambda c: c.order, 6), ids=lambda c: c.name)
def test_processing_order_changes_nothing_beyond_rounding(c):
    _agree(c, run_case(c)[0], run_case(c, order=None)[0], "order/NULL")


@pytest.mark.parametrize("c", [c for c in K.CASES if c.xe and not c.split and c.family in ("bwd", "p0")], ids=lambda c: c.name)
def test_reverse_pair_form_agrees_with_combined_form(c):
    """XE + pair_force against the combined form: dE/dx per atom, the virial on its total (the per-atom partitions differ by design)"""
    x, s = K.inputs(c), K.stage_inputs(c)
    run = run_bwd if c.family == "bwd" else run_p0
    oxe, ocomb = run(x, s, pb_zero=True)[0], run(x, s, xe=False)[0]
    gates = K.gates(c)
    pairs = [("forces", -ocomb["fgrad"])] + ([("virial_total", ocomb["virial_total"])] if c.stress else [])
    for k, other in pairs:
        err = float((oxe[k] - other).abs().max())
        print(f"CONVV {c.name} xe/combined {k} diff {err:.3e} gate {gates[k][0]:.3e}")
        assert err <= 2.0 * gates[k][0], f"{c.name} {k}: {err:.3e} > 2 x {gates[k][0]:.3e}"


def test_hooks_reject_nonsense():
    lib, L = _lib()
    x = K.inputs(K.CASES[0])
    rc, eta, sh = _basis(x)
    buf = _nan(64)
    p = _p(buf)
    assert lib.aimnet_debug_conv_fwd(3, p, None, None, p, p, p, 8, p, None, rc, eta, sh, p, 704, p, None, 4, None, 0, 0, 0, _stream()) == L.E_INVALID
    assert lib.aimnet_debug_conv_fwd(0, p, None, None, p, p, p, 8, p, None, rc, eta, sh, p, 700, p, None, 4, None, 0, 0, 0, _stream()) == L.E_INVALID
    assert lib.aimnet_debug_conv_fwd(1, p, None, None, p, p, p, 8, p, None, rc, eta, sh, p, 736, p, None, 4, None, 0, 0, 0, _stream()) == L.E_INVALID
    assert lib.aimnet_debug_conv_fwd(0, p, None, None, p, p, p, 8, p, None, rc, eta, sh, p, 704, p, None, 4, None, 1, 0, 0, _stream()) == L.E_INVALID
    assert lib.aimnet_debug_unconcat(0, None, 704, p, None, p, None, p, None, 4, _stream()) == L.E_INVALID
    assert lib.aimnet_debug_conv_bwd(0, 1, 0, p, None, None, p, None, p, p, p, 8, rc, eta, sh, p, 704, None, None, None, None, p, None, 4, None,
                                     None, 0, 0, _stream()) == L.E_INVALID
    assert lib.aimnet_debug_conv_bwd_p0(0, p, 704, p, p, p, p, 65, p, 1, p, p, p, p, 8, rc, eta, sh, p, p, None, 4, None, None, _stream()) == L.E_INVALID
    assert lib.aimnet_debug_pair_force(p, p, None, p, 8, 4, p, p, _stream()) == L.E_INVALID
