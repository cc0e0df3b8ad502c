"""The engine's option table (csrc/engine.hip, OPTIONS): every switch that include/aimnet_hip.h lists reads back what was set, the
environment and set_option normalise alike, unknown names are errors and the retired "conv_mfma" and "overlap_coulomb" read 0 and accept only 0."""
from __future__ import annotations

import os
import re

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _header_options():
    text = open(os.path.join(ROOT, "include", "aimnet_hip.h")).read()
    block = text[text.index("/* Engine switches for A/B and parity runs"):text.index("int aimnet_engine_set_option(")]
    return re.findall(r'^ \*   "([a-z0-9_]+)"', block, flags=re.M)


def test_option_table():
    from aimnetcentral_amd import loader
    from aimnetcentral_amd._lib import HipLibraryError
    from aimnetcentral_amd.engine import HipEngine

    names = _header_options()
    assert "conv_mfma" in names and "overlap_coulomb" in names and len(names) == len(set(names)) == 21
    spec = loader.synthetic_spec(0)
    eng = HipEngine(spec, "cuda:0")
    for name in names:
        if name == "conv_mfma":
            continue
        v = eng.get_option(name)
        eng.set_option(name, v)
        assert eng.get_option(name) == v, name
    eng.set_option("gemm_bf3", 5)
    assert eng.get_option("gemm_bf3") == 2
    eng.set_option("split_max", -1)
    assert eng.get_option("split_max") == 1024
    eng.set_option("conv_xe", 2)
    assert eng.get_option("conv_xe") == 1
    with pytest.raises(HipLibraryError):
        eng.get_option("no_such_option")
    with pytest.raises(HipLibraryError):
        eng.set_option("no_such_option", 1)
    assert eng.get_option("conv_mfma") == 0
    eng.set_option("conv_mfma", 0)
    with pytest.raises(HipLibraryError, match="conv_mfma was removed"):
        eng.set_option("conv_mfma", 1)
    assert eng.get_option("overlap_coulomb") == 0
    eng.set_option("overlap_coulomb", 0)
    with pytest.raises(HipLibraryError, match="overlap_coulomb was removed"):
        eng.set_option("overlap_coulomb", 1)
    # the environment is read once, when an engine is created
    assert eng.get_option("gemm_chain") == 1
    old = os.environ.get("AIMNET_GEMM_CHAIN")
    os.environ["AIMNET_GEMM_CHAIN"] = "0"
    try:
        eng2 = HipEngine(spec, "cuda:0")
        assert eng2.get_option("gemm_chain") == 0
        assert eng.get_option("gemm_chain") == 1
    finally:
        if old is None:
            del os.environ["AIMNET_GEMM_CHAIN"]
        else:
            os.environ["AIMNET_GEMM_CHAIN"] = old
