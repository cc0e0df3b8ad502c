"""tests/conv_cases.py without a GPU: the case table reaches what it must, the fp64 reference is self-consistent (hand-written backward ==
autograd of the forward) and equals the conv blocks of oracle/aimnet2_analytic.py on a geometric cluster, the gate is built from the
reference alone, and every deliberate fault breaks a gate - so tests/test_gpu_conv_kernels.py would see the same fault in a kernel."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import conv_cases as K
from conv_cases import A, G, H, NF, NV

RTOL = 1e-10


def _close(got, ref, what):
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    assert err <= RTOL * max(scale, 1e-300), f"{what}: |diff| {err:.3e} at scale {scale:.3e}"


# ---- 1. the table ------------------------------------------------------------------------------------------------------------------------
def test_case_table_reaches_every_instantiation():
    seen = set()
    for c in K.CASES:
        seen |= set(K.instantiation(c))
    assert seen == K.ALL_INSTANTIATIONS
    assert len({c.name for c in K.CASES}) == len(K.CASES)


def _form(c):
    if c.family == "fwd":
        return "fwd_split" if c.split else ("fwd_moments" if c.moments else "fwd_wave")
    if c.family == "p0":
        return "p0_xe" if c.xe else "p0"
    return "bwd_split" if c.split else ("bwd_xe" if c.xe else "bwd_wave")


def test_row_counts_atom_counts_and_variants_are_all_present():
    counts, atoms = {}, {}
    for c in K.CASES:
        x = K.inputs(c)
        counts.setdefault(_form(c), set()).update(int(v) for v in x.nb_cnt)
        atoms.setdefault(_form(c), set()).add((c.n, c.split))
        assert x.nb_cnt.max() <= c.cap and (not (c.xe and not c.split) or c.cap <= K.REV_ROW_MAX)
    assert set(counts) == {"fwd_split", "fwd_moments", "fwd_wave", "p0", "p0_xe", "bwd_split", "bwd_xe", "bwd_wave"}
    for form, got in counts.items():
        need = K.REQUIRED if form.endswith("_xe") else K.REQUIRED_DENSE
        assert set(need) <= got, f"{form}: row counts {sorted(set(need) - got)} missing"
    assert atoms["fwd_split"] == atoms["bwd_split"] == {(7, True), (37, True)}
    for form in ("fwd_wave", "bwd_wave", "bwd_xe", "fwd_moments", "p0", "p0_xe"):
        assert atoms[form] == {(13, False), (37, False)}, form
    n_order = sum(c.order for c in K.CASES)
    assert abs(2 * n_order - len(K.CASES)) <= 1
    for fam in ("fwd", "bwd", "p0"):
        cs = [c for c in K.CASES if c.family == fam]
        assert {c.order for c in cs} == {False, True}
        assert any(c.cap == K.CAP_SMALL for c in cs)
        assert {c.ldx for c in cs} == {704, 736, 768}
    assert {c.nelem for c in K.CASES if c.family == "p0"} == {1, 4, 12} == {c.nelem for c in K.CASES if c.moments}
    assert {1, 4, 12} <= {c.nelem for c in K.CASES if c.family == "fwd" and not c.moments}
    assert 12 > K.P0_AFV_LDS
    assert {(c.xe and not c.split, c.pb_accum) for c in K.CASES if c.family == "bwd" and c.xe and not c.split} == {(True, False), (True, True)}


def test_lists_are_symmetric_multigraphs_with_interleaved_elements():
    selfs = repeats = near = runs = 0
    for c in K.CASES:
        x = K.inputs(c)
        for i in range(x.n):
            cnt = int(x.nb_cnt[i])
            js = x.nb_idx[i, :cnt]
            selfs += int((js == i).sum())
            repeats += cnt - len(set(js.tolist()))
            near += int((x.pg[i, :cnt, 3] > x.rc - 1e-3).sum())
            assert (x.pg[i, :cnt, 3] >= 0.7).all() and (x.pg[i, :cnt, 3] < x.rc).all()
            assert np.isnan(x.pg[i, cnt:]).all() and ((x.nb_idx[i, cnt:] >= 0) & (x.nb_idx[i, cnt:] < x.n)).all()
            for m in range(cnt):
                j, r = int(js[m]), int(x.rev[i, m])
                assert 0 <= r < x.nb_cnt[j] and x.nb_idx[j, r] == i and x.rev[j, r] == m and (j != i or r != m)
                assert (x.pg[j, r, :3] == -x.pg[i, m, :3]).all() and x.pg[j, r, 3] == x.pg[i, m, 3]  # bit for bit
            if c.nelem == 12 and cnt >= 48:
                z = x.numbers[js]
                runs = max(runs, 1 + int((z[1:] != z[:-1]).sum()))
    assert selfs > 50 and repeats > 500 and near > 100
    assert runs > 30  # many short runs of equal elements within one row


# ---- 2. self-consistency: the hand-written backward is the gradient of the forward --------------------------------------------------------
AUTOGRAD_CASES = [c for c in K.CASES if c.name in ("fwd_nq2_wave_x1_n37", "fwd_nq1_split_x0_n37", "fwd_nq0_wave_x0_n13",
                                                   "fwd_rowof_wave_x0_n37", "fwd_moments_x1_e4_n13", "fwd_cap40_nq1_wave_n13")]


def _exact_geometry(x):
    """fp64 leaves r = u d per directed entry (garbage entries made harmless) and the (u, d) they define exactly"""
    valid = torch.arange(x.cap).unsqueeze(0) < torch.as_tensor(x.nb_cnt).long().unsqueeze(1)
    pg = torch.as_tensor(x.pg).double()
    r = torch.where(valid.unsqueeze(-1), pg[..., :3] * pg[..., 3:], torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64))
    r.requires_grad_(True)
    d = r.norm(dim=-1)
    return r, torch.cat([r / d.unsqueeze(-1), d.unsqueeze(-1)], dim=-1)


def test_autograd_cases_exist():
    assert len(AUTOGRAD_CASES) == 6


@pytest.mark.parametrize("c", AUTOGRAD_CASES, ids=lambda c: c.name)
def test_backward_reference_equals_autograd_of_forward_reference(c):
    x0 = K.inputs(c)
    x = SimpleNamespace(**vars(x0))
    r, x.pg = _exact_geometry(x0)
    leaf_a = c.nelem == 0
    x.a = torch.as_tensor(x0.a).double().requires_grad_(leaf_a)
    if c.nq:
        x.q = torch.as_tensor(x0.q).double().requires_grad_(True)
    g = torch.Generator().manual_seed(c.seed)
    ncols = 2 * NF + NV + c.nq * (1 + G + H)
    xbar = torch.randn(c.n, ncols, generator=g, dtype=torch.float64) * K.XBAR_SCALE
    out = K.ref_forward(x)
    E = (K.forward_row(out) * xbar).sum()
    leaves = [r] + ([x.a] if leaf_a else []) + ([x.q] if c.nq else [])
    grads = torch.autograd.grad(E, leaves)
    rbar = grads[0]
    # hand-written: unconcat -> Sbar, then the per-entry halves
    xd = SimpleNamespace(**vars(x))
    xd.pg, xd.a, xd.xbar = x.pg.detach(), x.a.detach(), xbar
    if c.nq:
        xd.q = x.q.detach()
    un = K.ref_unconcat(xd, out["Vsave"].detach(), out["Vqsave"].detach() if c.nq else None)
    p = K.ref_pairs(xd, un["Sbar"], un.get("Sqbar"))
    _close(p["R"], rbar, "rbar_ij per entry")
    _close(p["F1"], K.mirror_of(x0, rbar), "F1 = rbar of the mirror entry")
    _close((p["F1"] - p["R"]).sum(1), (K.mirror_of(x0, rbar) - rbar).sum(1), "fgrad")
    if leaf_a:
        _close(p["ab"].reshape(c.n, NF) + xbar[:, :NF], grads[1], "abar")
    if c.nq:
        _close(p["qacc"].t() + xbar[:, 2 * NF + NV : 2 * NF + NV + c.nq].t(), grads[-1], "qbar")
    # the two partitions of the virial have one total; it is sum_p r_p (x) rbar_p
    W = torch.einsum("nma,nmb->ab", p["r"], rbar)
    _close(torch.einsum("nma,nmb->ab", -p["r"], p["F1"]), W, "virial total, reverse-pair partition")
    _close(torch.einsum("nma,nmb->ab", -0.5 * p["r"], p["F1"] - p["R"]), W, "virial total, combined partition")


def test_reference_equals_the_analytic_oracle_on_a_geometric_cluster():
    """20 atoms, list by brute force, the two-channel synthetic model in fp64: every conv block of aimnet2_analytic.evaluate, per pass"""
    from aimnetcentral_amd import synth
    from oracle import aimnet2_analytic as AN
    from oracle import aimnet2_oracle as O

    rng = np.random.default_rng(5)
    n = 20
    model = O.OracleModel(synth.synthetic_state_dict(0, num_charge_channels=2), torch.float64)
    rc = float(model.rc)
    xyz = rng.uniform(0.0, 5.5, (n, 3))
    z = rng.choice(np.array(K.ELEMENTS[:6]), n)
    dist = np.linalg.norm(xyz[:, None] - xyz[None], axis=-1)
    rows = [[j for j in range(n) if j != i and dist[i, j] < rc] for i in range(n)]
    cap = max(len(r) for r in rows)
    assert min(len(r) for r in rows) >= 3 and cap >= 10
    nbmat = np.full((n + 1, cap), n, np.int64)
    for i, r in enumerate(rows):
        nbmat[i, : len(r)] = r
    trace: dict = {}
    AN.evaluate(model, xyz, z, np.zeros(1), np.zeros(n, np.int64), nbmat, coulomb="none", stress=False, trace=trace)
    nb_cnt = np.array([len(r) for r in rows], np.int32)
    nb_idx = np.where(nbmat[:n] < n, nbmat[:n], 0).astype(np.int32)
    rvec = torch.as_tensor(xyz)[torch.as_tensor(nb_idx).long()] - torch.as_tensor(xyz).unsqueeze(1)
    d = rvec.norm(dim=-1)
    pg = torch.cat([rvec / d.unsqueeze(-1), d.unsqueeze(-1)], dim=-1)
    assert len(trace["fwd"]) == len(trace["bwd"]) >= 2
    for f, b in zip(trace["fwd"], reversed(trace["bwd"])):
        p = b["p"]
        nq = 0 if p == 0 else 2
        x = SimpleNamespace(n=n, cap=cap, nq=nq, nb_idx=nb_idx, nb_cnt=nb_cnt, pg=pg, rc=rc, eta=float(model.eta), shifts=model.shifts.numpy(),
                            agh_a=model.agh_a, agh_q=model.agh_q, a=f["a"].reshape(n, NF), row_of=None,
                            q=f["q"].t().contiguous() if nq else None, xbar=b["xb"])
        assert float(np.float32(x.eta)) == x.eta
        fw = K.ref_forward(x)
        _close(K.forward_row(fw), f["x"], f"pass {p}: forward row")
        _close(fw["Vsave"], f["V"], f"pass {p}: V")
        if nq:
            _close(fw["Vqsave"], f["Vq"], f"pass {p}: Vq")
        un = K.ref_unconcat(x, f["V"], f["Vq"])
        _close(un["Sbar"], b["Sbar"], f"pass {p}: Sbar")
        if nq:
            _close(un["Sqbar"], b["Sqbar"], f"pass {p}: Sqbar")
        pr = K.ref_pairs(x, un["Sbar"], un.get("Sqbar"))
        _close(pr["R"], b["rbar_ij"], f"pass {p}: rbar_ij")
        _close(pr["F1"], b["rbar_ji"], f"pass {p}: rbar_ji")
        if p > 0:
            _close(b["abar_in"] + b["xb"][:, :NF].view(n, A, G) + pr["ab"], b["abar_out"], f"pass {p}: abar")
            _close(b["qbar_in"] + b["xb"][:, 2 * NF + NV : 2 * NF + NV + nq] + pr["qacc"], b["qbar_out"], f"pass {p}: qbar")


# ---- 3. the gate ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.CASES[::7], ids=lambda c: c.name)
def test_gate_is_built_from_the_reference_alone(c):
    r64, r32 = K.ref64(c), K.reference(c, torch.float32)
    for k, (gate, yard, top) in K.gates(c).items():
        assert r32[k].dtype == torch.float32 and r64[k].dtype == torch.float64
        assert yard == float((r32[k].double() - r64[k]).abs().max()) and top == float(r64[k].abs().max())
        extra = K.H2_REL * top if (c.family == "fwd" and c.x_split == 2 and k in K.FWD_ROW_BLOCKS) else 0.0
        assert gate == max(4.0 * yard, 8.0 * 2.0**-24 * top) + extra
        assert top > 0.0 and gate < 1e-4 * top, (k, gate, top)  # an fp32-sized gate at the block's own scale
        if k not in ("a", "q"):
            assert yard > 0.0


# ---- 4. the cases discriminate -------------------------------------------------------------------------------------------------------------
# which stages a fault has a meaning for (conv_cases.apply_fault): unconcat has no basis and no list, pair_force only the mirror map
FAULT_STAGES = {
    "shift": ("fwd", "bwd", "p0"),
    "chunk_last": ("fwd", "bwd", "p0"),
    "quarter_last": ("fwd", "bwd"),            # the four-wave split exists in conv_fwd and conv_bwd only
    "uz": ("fwd", "bwd", "p0"),
    "agh_q_channel": ("fwd", "unconcat"),      # the only kernels that read agh_q
    "run_merge": ("fwd", "p0"),                # the moment forms: conv_fwd<.., P0M> and conv_bwd_p0
    "mirror_sign": ("bwd", "p0", "pair_force"),
}


def _breaks(c, fault, stage):
    bad = K.reference(c, torch.float32, fault, stage)
    if bad is None:
        return None
    good, gates = K.ref64(c), K.gates(c)
    return any(float((bad[k].double() - good[k]).abs().max()) > gates[k][0] for k in bad if k in good)


@pytest.mark.parametrize("fault,target", [(f, t) for f, ts in FAULT_STAGES.items() for t in ts])
def test_every_fault_breaks_a_gate_in_every_family(fault, target):
    family, stage = {"fwd": ("fwd", "fwd"), "unconcat": ("bwd", "unconcat"), "bwd": ("bwd", "bwd"), "p0": ("p0", "bwd"),
                     "pair_force": (None, "pair_force")}[target]
    applied = caught = 0
    for c in K.CASES:
        if family is not None and c.family != family:
            continue
        hit = _breaks(c, fault, stage)
        if hit is None:
            continue
        applied += 1
        caught += bool(hit)
        if caught:
            break
    assert applied > 0, "no case this fault applies to"
    assert caught > 0, f"{fault} slipped through all {applied} {target} cases it applies to"


def test_clean_fp32_reference_passes_every_gate():
    """the other half of discrimination: without a fault the fp32 twin sits inside the gate (by construction, factor 4)"""
    for c in K.CASES[::5]:
        assert _breaks(c, None, None) is False


def test_hooks_reject_null_pointers_without_touching_a_gpu():
    from aimnetcentral_amd import _lib

    lib = _lib.load()
    assert lib.aimnet_debug_conv_fwd(0, *[None] * 6, 8, None, None, 5.0, 14.5, None, None, 704, None, None, 4, None, 0, 0, 0, None) == _lib.E_INVALID
    assert lib.aimnet_debug_unconcat(0, None, 704, *[None] * 6, 4, None) == _lib.E_INVALID
    assert lib.aimnet_debug_conv_bwd(0, 0, 0, *[None] * 8, 8, 5.0, 14.5, None, None, 704, *[None] * 6, 4, None, None, 0, 0, None) == _lib.E_INVALID
    assert lib.aimnet_debug_conv_bwd_p0(0, None, 704, *[None] * 4, 16, None, 1, *[None] * 4, 8, 5.0, 14.5, *[None] * 4, 4, None, None, None) == _lib.E_INVALID
    assert lib.aimnet_debug_pair_force(None, None, None, None, 8, 4, None, None, None) == _lib.E_INVALID
