"""`HipEngine.charge_response` against `HipEngine.hvp` on the same inputs: time per call and workspace per direction.  Cases: hvp40
with its 120 unit directions, taxol with 3 and with its 339 unit directions, the 96-atom DSF cell (pbc96_dsf8_wrapped) with 3.  HIP
events, 5 warm-up calls, median of 10, the two entries interleaved; both calls end with their one status read.  Record:
profiles/r7_charge_response.md."""
from __future__ import annotations

import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    from aimnetcentral_amd import _lib, capacity, loader
    from aimnetcentral_amd.engine import HipEngine

    eng = HipEngine(loader.synthetic_spec(0), "cuda:0")
    dev = eng.device

    def t(a, dt=torch.float32):
        return torch.as_tensor(np.asarray(a)).to(dt).to(dev)

    for name, K, kw in (("hvp40", 120, {}), ("taxol", 3, {}), ("taxol", 339, {}),
                        ("pbc96_dsf8_wrapped", 3, dict(coulomb="dsf", dsf_rc=8.0, dsf_alpha=0.25))):
        g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        n = len(g["numbers"])
        cell = t(g["cell"]) if "cell" in g.files else None
        args = (t(g["coord"]), t(g["numbers"], torch.int32), torch.zeros(n, dtype=torch.int32, device=dev), t([0.0]))
        v = torch.eye(3 * n, device=dev).view(3 * n, n, 3)[:K].contiguous() if K > 3 else \
            torch.randn(K, n, 3, generator=torch.Generator().manual_seed(11)).to(dev)
        runs = {"charge_response": lambda: eng.charge_response(*args, v, cell=cell),
                "hvp": lambda: eng.hvp(*args, v, cell=cell, **kw)}
        times = {k: [] for k in runs}
        for it in range(15):
            for k, f in runs.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                f()
                t1.record()
                torch.cuda.synchronize()
                if it >= 5:
                    times[k].append(t0.elapsed_time(t1))
        method = _lib.COULOMB_DSF if kw else _lib.COULOMB_SIMPLE
        opts = {"charge_response": eng.fill_options(capacity.Request("hvp", n, 1, cell is not None, _lib.COULOMB_NONE, 0.0)),
                "hvp": eng.fill_options(capacity.Request("hvp", n, 1, cell is not None, method, kw.get("dsf_rc", 15.0), kw.get("dsf_alpha", 0.2)))}
        rec = {"case": name, "n_atoms": n, "directions": K}
        for k in runs:
            f = getattr(eng.lib, f"aimnet_engine_{k}_workspace_bytes")
            per = int(f(eng._h, n, 1, 2, C.byref(opts[k]))) - int(f(eng._h, n, 1, 1, C.byref(opts[k])))
            rec[k] = {"median_ms": round(statistics.median(times[k]), 4), "min_ms": round(min(times[k]), 4),
                      "max_ms": round(max(times[k]), 4), "workspace_bytes_per_direction": per}
        rec["time_ratio"] = round(rec["charge_response"]["median_ms"] / rec["hvp"]["median_ms"], 3)
        rec["workspace_ratio"] = round(rec["charge_response"]["workspace_bytes_per_direction"] / rec["hvp"]["workspace_bytes_per_direction"], 3)
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
