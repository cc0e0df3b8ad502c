"""aimnetcentral_amd/capacity.py on its own: the primitives of the row / k-array / mesh capacity policy and the `Capacities` object
every driver (HipEngine.eval, hvp, check_deferred, DomainDecomposedEngine, VerletSkinLists) takes them from.  No library, no torch."""
from __future__ import annotations

import numpy as np
import pytest

from aimnetcentral_amd import _lib
from aimnetcentral_amd import capacity as cap

DSF, EWALD, PME = _lib.COULOMB_DSF, _lib.COULOMB_EWALD, _lib.COULOMB_PME
D3 = {"s8": 0.5, "a1": 0.4, "a2": 4.0}


def st(s0=100, s1=0, s2=0, s3=0, s4=0, s5=0, s6=0, s7=0):
    return np.array([s0, s1, s2, s3, s4, s5, s6, s7], dtype=np.int32)


def test_primitives():
    assert [cap.round16(n) for n in (0, 1, 16, 17)] == [0, 16, 16, 32]
    assert cap.start_capacity(5.0) == 112 and cap.start_capacity(15.0) == 2832  # 0.2 * 4/3 pi rc^3 = 104.7, 2827.4
    assert cap.grown(112, 130) == 176 and cap.grown(112, 300) == 304 and cap.grown(64, 10, 97) == 112  # x1.5, or the largest need
    assert cap.shrunk(176, 40) == 64 and cap.shrunk(176, 88) == 176 and cap.shrunk(176, 87) == 128 and cap.shrunk(112, 0) == 16
    assert cap.ewald_k_capacity(1000) == 1256 and cap.ewald_k_capacity(8) == 16  # (need * 5 // 4 + 7) // 8 * 8
    assert cap.pme_mesh_capacity(20000) == 22564  # need * 9 // 8 + 64
    with pytest.raises(ValueError, match="more than 512 PME mesh points"):
        cap.pme_mesh_capacity(2**31 - 1)
    assert cap.same_cutoff(15.0, 15.0 + 1e-9) and not cap.same_cutoff(15.0, 15.001)  # on the float32 values


def test_builds_lr_list():
    big, small = (1500, 1), (1499, 1)
    assert cap.builds_lr_list(*small, False, False, DSF, True, False, False)
    assert not cap.builds_lr_list(*big, False, False, DSF, True, False, False)  # the bounding-box walk
    assert cap.builds_lr_list(2999, 2, False, False, DSF, True, False, False)  # 1499.5 atoms per molecule: a list
    assert cap.builds_lr_list(*big, False, False, DSF, False, False, False)  # switch off
    assert cap.builds_lr_list(*big, False, False, DSF, True, True, True)  # the pair terms ride on the D3 list
    assert not cap.builds_lr_list(*big, False, False, DSF, True, True, False)
    assert not cap.builds_lr_list(*small, True, False, DSF, True, False, False)  # periodic DSF walks the cell grid
    assert not cap.builds_lr_list(*small, False, True, DSF, True, False, False)  # the caller's lists
    assert not cap.builds_lr_list(*small, False, False, _lib.COULOMB_SIMPLE, True, False, False)


def engine_caps():
    c = cap.Capacities(5.0)
    c.has_dftd3 = True
    return c


def test_fill_options_and_growth_per_list():
    c = engine_caps()
    assert (c.max_nb, c._max_nb_lr, c._ewald_nb_lr, c._ewald_max_k, c._pme_max_mesh) == (112, {}, 0, 8192, 8192)
    assert c.lr_capacity(15.0) == c._lr_capacity(15.0) == 2832 and c._max_nb_lr == {15.0: 2832}
    rq = cap.Request("eval", 10, 1, False, DSF, 12.0, dftd3=D3, flags=_lib.FORCES)
    opt = c.fill_options(rq)
    assert (opt.flags, opt.coulomb, opt.max_nb, opt.max_nb_lr, opt.dftd3, opt.max_nb_d3) == (1, DSF, 112, 1456, 1, 2832)
    assert (opt.dsf_rc, opt.d3_cutoff, opt.d3_smoothing_on, opt.d3_s6) == (12.0, 15.0, 12.0, 1.0)
    assert not c.grow(st(), opt, rq) and c._max_nb_lr == {15.0: 2832, 12.0: 1456}
    assert c.grow(st(s1=1500, s3=1), opt, rq) and c._max_nb_lr == {15.0: 2832, 12.0: 2192}  # round16(1456 * 1.5)
    assert c.grow(st(130, s2=1, s4=5000, s5=1), opt, rq) and c.max_nb == 176 and c._max_nb_lr[15.0] == 5008  # round16(5000)
    c.shrink(st(40, s1=1000, s4=3000), c.fill_options(rq), rq)
    assert c.max_nb == 64 and c._max_nb_lr == {15.0: 5008, 12.0: 1344}  # 1000 < 0.5 * 2192: round16(1333); 3000 >= 0.5 * 5008
    # caller-supplied matrices: their widths, and the D3 list in nbmat_lr if it has no matrix of its own
    opt = c.fill_options(cap.Request("eval", 10, 1, False, DSF, 12.0, dftd3=D3, widths=(20, 40, 0)))
    assert (opt.max_nb, opt.max_nb_lr, opt.max_nb_d3) == (32, 48, 48)
    opt = c.fill_options(cap.Request("eval", 10, 1, False, _lib.COULOMB_SIMPLE, 15.0, dftd3=D3, widths=(20, 0, 0)))
    assert (opt.max_nb, opt.max_nb_lr, opt.max_nb_d3) == (32, 0, 16)
    c.has_dftd3 = False
    with pytest.raises(RuntimeError, match="no DFT-D3 tables"):
        c.fill_options(rq)


def test_d3_overflow_grows_from_the_larger_of_the_two_capacities():
    """The one rule for a D3 row overflow is eval's: from max(max_nb_d3, max_nb_lr).  With d3_cutoff != dsf_rc and the long-range
    capacity the larger one, hvp used to grow from max_nb_d3 alone (here round16(max(1456 * 1.5, 1500)) = 2192) and
    DomainDecomposedEngine from the D3 capacity with status[1] as a second need (round16(max(2184, 1500, 2000)) = 2192)."""
    for kind in ("eval", "hvp"):
        c = engine_caps()
        rq = cap.Request(kind, 10, 1, False, DSF, 15.0, dftd3=D3 | {"cutoff": 12.0})
        opt = c.fill_options(rq)
        assert (opt.max_nb_lr, opt.max_nb_d3) == (2832, 1456)
        assert c.grow(st(s1=2000, s4=1500, s5=1), opt, rq)
        assert c._max_nb_lr == {15.0: 2832, 12.0: 4256}  # round16(max(max(1456, 2832) * 1.5, 1500)) = round16(4248)


def test_ewald_and_pme():
    c = engine_caps()
    rq = cap.Request("eval", 10, 1, True, EWALD, 15.0, accuracy=1e-5)
    c._ewald_max_k = 64
    opt = c.fill_options(rq)
    assert (opt.ewald_max_k, opt.pme_max_mesh, opt.max_nb_lr) == (64, 8192, 0) and opt.ewald_accuracy == np.float32(1e-5)
    assert c.grow(st(s7=1000), opt, rq) and c._ewald_max_k == 1256 and not c.grow(st(s7=1000), c.fill_options(rq), rq)
    rq = cap.Request("eval", 10, 1, True, PME, 15.0)
    assert c.grow(st(s7=20000), c.fill_options(rq), rq) and c._pme_max_mesh == 22564 and c._ewald_max_k == 1256
    # hvp: the real-space list has ONE capacity, which follows the largest cutoff seen and never shrinks
    c = engine_caps()
    rq = cap.Request("hvp", 10, 1, True, EWALD, 9.0)
    opt = c.fill_options(rq)
    assert opt.max_nb_lr == c._ewald_nb_lr == 624 and opt.pme_max_mesh == 0  # round16(int(0.2 * 4/3 pi 9^3)) = round16(610)
    assert c.grow(st(s1=700, s3=1), opt, rq) and c._ewald_nb_lr == 944 and c._max_nb_lr == {}  # round16(624 * 1.5)
    assert c.fill_options(cap.Request("hvp", 10, 1, True, EWALD, 6.0)).max_nb_lr == 944


def test_pme_workspace_limit():
    c = engine_caps()
    c._pme_max_mesh = 10**9
    rq = cap.Request("eval", 20, 2, True, PME, 15.0)  # 2 x 1e9 x 40 B > 64 GiB
    assert c.fill_options(rq).pme_max_mesh == 8192 and c._pme_max_mesh == 8192  # once per call (= per request object) ...
    c._pme_max_mesh = 10**9
    with pytest.raises(ValueError, match="2 systems x a mesh of 1000000000 points"):
        c.fill_options(rq)
    assert c.fill_options(cap.Request("eval", 20, 2, True, PME, 15.0)).pme_max_mesh == 8192  # ... the next call may again
    with pytest.raises(ValueError, match="exceeds the PME workspace limit"):
        c.fill_options(cap.Request("eval", 70000, 70000, True, PME, 15.0))  # grid.y: at most 65 535 systems


def test_deferred_growth_has_no_request():
    c = engine_caps()
    c._max_nb_lr = {15.0: 2832, 12.0: 1456}
    rows = np.stack([st(), st(130, s1=3000, s2=1, s3=1, s4=3100), st(s7=9000)])
    assert c.grow_deferred(rows, False)
    # every long-range entry by the larger of status[1] and status[4]: round16(max(2832 * 1.5, 3100)), round16(max(2184, 3100))
    assert c.max_nb == 176 and c._max_nb_lr == {15.0: 4256, 12.0: 3104} and c._ewald_max_k == 11256 and c._pme_max_mesh == 8192
    assert not c.grow_deferred(np.stack([st(), st(s7=9000)]), False)
    assert c.grow_deferred(np.stack([st(s7=9000)]), True) and c._pme_max_mesh == 10189  # status[7] counts mesh points: 9000 * 9 // 8 + 64


def test_ewald_list_cutoff():
    from oracle import aimnet2_oracle as O

    # 10 atoms in a (10 A)^3 cell at 1e-6: the 14.287 A of tests/test_host_driver.py (test_hvp_ewald_list_capacity_only_grows)
    assert abs(cap.ewald_list_cutoff([1000.0], [10], 1e-6) - 14.287) < 1e-3
    for n, vol, acc in ((10, 1000.0, 1e-6), (96, 1234.5, 1e-4), (1, 27.0, 0.5)):
        want = O.ewald_parameters(n, vol, acc)[1] * (1.0 + 1e-5)  # f eta, widened
        assert abs(cap.ewald_list_cutoff(np.array([vol]), np.array([n]), acc) - want) <= 1e-12 * want
    # a batch: the larger of its systems' cutoffs (the list is built at one cutoff)
    one, two = cap.ewald_list_cutoff([1000.0], [10], 1e-6), cap.ewald_list_cutoff([8000.0], [10], 1e-6)
    assert two > one and cap.ewald_list_cutoff([1000.0, 8000.0], [10, 10], 1e-6) == two
    assert cap.ewald_list_cutoff([8000.0, 1000.0], [10, 10], 1e-6) == two
