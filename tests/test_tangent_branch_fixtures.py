"""The inputs of tests/test_gpu_tangent_branches.py, pinned without a GPU: every case of tests/tangent_cases.py has the property its
branch is named for (pairs beyond the DSF cutoff inside a molecule, lattice shifts of 2 and more, self images, atoms outside the box,
no shift along an open axis, a periodicity that matters, a D3 block that matters and that the engine's stencil can resolve, stacked
rows on both sides of the GEMM switch, atom counts on both sides of the bounding-box threshold), and the fp64 tangent sweep that
serves as the reference equals the autograd Hessian of the oracle on every case small enough for one.  The references are the ones
the GPU tests use (one cache per process)."""
from __future__ import annotations

import os
from types import SimpleNamespace

import numpy as np
import pytest

import tangent_cases as T

TINY = ("tiny3-dsf8", "tiny1-TTF", "tiny2-flags", "tiny3-dsf8-d3", "nse-tiny1-TTF")
D3 = ("mols-simple-d3", "tiny3-dsf8-d3", "nse-mols-d3")


def _model(c, oracle64, oracle64_nse):
    return oracle64_nse if c.nse else oracle64


def test_case_tables():
    assert set(T.CHARGE_RESPONSE_CASES) <= set(T.HVP_CASES) and set(T.SMALL_CASES) == set(T.HVP_CASES) - {"cluster1728"}
    assert set(TINY) == {n for n in T.HVP_CASES if T.case(n).cell is not None} and set(D3) == {n for n in T.HVP_CASES if T.case(n).d3}
    for name in ("mols-none", "mols-simple", "mols-simple-d3", "nse-mols-d3"):
        assert tuple(np.bincount(T.case(name).mol)) == (1, 2, 40, 3, 1)
    assert T.case("mols-none").coul["coulomb"] == "none" and T.case("lone-atom-none").coul["coulomb"] == "none"
    assert len(T.case("lone-atom").numbers) == 1 and T.case("tiny3-dsf8").V.shape == (54, 18, 3) and T.case("tiny1-TTF").V.shape == (21, 7, 3)
    assert T.case("tiny3-dsf8").cell.shape == (3, 3, 3) and T.case("tiny2-flags").pbc.tolist() == [[True, True, True], [True, False, True]]


def test_mols_simple_runs_on_both_sides_of_the_gemm_switch():
    c = T.case("mols-simple")
    n, K = len(c.numbers), len(c.V)
    assert n + 1 * n <= T.SPLIT_GEMM_ROWS < n + K * n
    text = open(os.path.join(T.ROOT, "aimnetcentral_amd", "csrc", "engine.hip")).read()
    assert f"e->gemm_bf3 == 2 || (e->gemm_bf3 == 1 && M > {T.SPLIT_GEMM_ROWS})" in text


def test_mols_dsf_has_pairs_beyond_the_cutoff_inside_a_molecule(oracle64):
    c = T.case("mols-dsf")
    assert tuple(np.bincount(c.mol)) == T.ragged_sizes(T.DSF_BIG) and c.cell is None
    assert c.coul["dsf_rc"] >= float(oracle64.rc)
    x = c.coord[c.mol == 2].astype(np.float64)
    d = np.linalg.norm(x[:, None] - x[None], axis=-1)[np.triu_indices(len(x), 1)]
    frac = float((d > c.coul["dsf_rc"]).mean())
    print(f"mols-dsf: {frac:.3f} of the pairs of the {len(x)}-atom molecule lie beyond {c.coul['dsf_rc']} A (span {d.max():.2f} A)")
    assert frac >= 0.05


@pytest.mark.parametrize("name", TINY)
def test_tiny_cells_have_far_shifts_self_images_and_atoms_outside_the_box(name, oracle64, oracle64_nse):
    c = T.case(name)
    ref, xw, nbl, shl = T.lists(c, _model(c, oracle64, oracle64_nse))
    n = len(c.numbers)
    nb, sh = ref["nbmat"][:n], ref["shifts"][:n]
    valid = nb < n
    assert np.abs(sh[valid]).max() >= 2                            # the short-range list itself
    assert (valid & (nb == np.arange(n)[:, None])).any()           # an atom next to its own image
    assert np.abs(xw - c.coord).max() > 1.0                        # the engine has to wrap
    flags = np.broadcast_to(c.pbc.reshape(-1, 3), (len(c.charge), 3))
    for lst, s in ((nb, sh), (nbl[:n], shl[:n])):
        open_axis = ~flags[c.mol][:, None, :] & (lst < n)[..., None]
        assert not s[open_axis].any()                              # no shift along an open axis, short- and long-range list
    print(f"{name}: largest |shift| short-range {np.abs(sh[valid]).max((0,))}, long-range {np.abs(shl[:n][nbl[:n] < n]).max((0,))}, "
          f"{int((valid & (nb == np.arange(n)[:, None])).sum())} self images")


@pytest.mark.parametrize("name", ["tiny1-TTF", "tiny2-flags", "nse-tiny1-TTF"])
def test_open_axes_matter(name, oracle64, oracle64_nse):
    """The Hessian with the case's flags differs from the fully periodic one by more than 100 gates: flags that are dropped show."""
    c = T.case(name)
    om = _model(c, oracle64, oracle64_nse)
    full = SimpleNamespace(**dict(vars(c), pbc=np.ones(3, bool), name=name + " (fully periodic)"))
    H, _ = T.hessian(c, om, False)
    Hp, _ = T.hessian(full, om, False)
    gate = 1e-5 + 3e-5 * np.abs(H).max()
    print(f"{name}: max|H - H(fully periodic)| = {np.abs(H - Hp).max():.3e} = {np.abs(H - Hp).max() / gate:.0f} gates")
    assert np.abs(H - Hp).max() > 100 * gate
    if name == "tiny2-flags":  # the second system's flags, not only "some flag": system 0 is fully periodic in both
        at = np.repeat(c.mol == 1, 3)
        assert np.abs((H - Hp)[np.ix_(at, at)]).max() > 100 * gate and np.abs((H - Hp)[np.ix_(~at, ~at)]).max() <= 1e-9


@pytest.mark.parametrize("name", D3)
def test_d3_block_matters_and_the_stencil_resolves_it(name, oracle64, oracle64_nse):
    c = T.case(name)
    om = _model(c, oracle64, oracle64_nse)
    ref = T.reference(c, om)
    n, K = len(c.numbers), len(c.V)
    H, _ = T.hessian(c, om, True)
    H0, _ = T.hessian(c, om, False)
    v = c.V.reshape(K, 3 * n).astype(np.float64)
    # the sweep equals the autograd Hessian without the term, hence hv_d3 of the reference is (H - H0) v
    assert np.abs(ref["hv_sweep"] - (v @ H0).reshape(K, n, 3)).max() <= 1e-9
    assert np.abs(ref["hv_d3"] - (v @ (H - H0)).reshape(K, n, 3)).max() <= 1e-9
    assert np.abs(H - H0).max() > 0.1
    err, top = np.abs(T.d3_stencil(c, om) - ref["hv_d3"]).max(), np.abs(ref["hv_d3"]).max()
    print(f"{name}: max|H_d3| = {np.abs(H - H0).max():.3f} eV/A^2, max|H_d3 v| = {top:.3f}, 4-point stencil in fp64 off by {err:.3e} "
          f"({err / (T.D3_RELATIVE * top):.3f} of the D3 allowance)")
    assert err <= T.D3_RELATIVE * top / 3.0


@pytest.mark.parametrize("name", [n for n in T.SMALL_CASES if n not in D3])
def test_sweep_equals_the_autograd_hessian(name, oracle64, oracle64_nse):
    c = T.case(name)
    om = _model(c, oracle64, oracle64_nse)
    ref = T.reference(c, om)
    n, K = len(c.numbers), len(c.V)
    H, f = T.hessian(c, om, False)
    err = np.abs(ref["hv"] - (c.V.reshape(K, 3 * n).astype(np.float64) @ H).reshape(K, n, 3)).max()
    print(f"{name}: max|evaluate_hvp - v H(autograd)| = {err:.3e} on max|Hv| = {np.abs(ref['hv']).max():.3e}")
    assert err <= 1e-9 and np.abs(ref["forces"] - f).max() <= 1e-9
    if name.startswith("lone-atom"):
        assert not ref["hv"].any() and not ref["t_q"].any()


def test_cluster_is_on_both_sides_of_the_bounding_box_threshold():
    assert T.BBOX_ATOMS_PER_MOL == T.bbox_constant_in_header()
    c, far = T.case("cluster1728"), T.cluster_with_far_atom()
    assert (len(c.numbers), len(c.charge)) == (1728, 1) and (len(far.numbers), len(far.charge)) == (1729, 2)
    assert T.bbox_applies(1728, 1) and not T.bbox_applies(1729, 2)
    assert c.cell is None and c.V.shape == (1, 1728, 3) and np.array_equal(far.coord[:1728], c.coord) and np.array_equal(far.V[:, :1728], c.V)
    assert np.linalg.norm(far.coord[1728] - c.coord, axis=-1).min() > 60.0
