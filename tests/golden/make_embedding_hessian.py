"""Writes tests/golden/embedding_hessian.npz: the fp64 yardstick of tests/embedding_hessian_yardstick.py for the cases the GPU tests
use (each takes tens of seconds to minutes on a CPU: 6 K evaluations of the fp64 oracle with the Jacobian of the charges).

    python tests/golden/make_embedding_hessian.py

Per case NAME: NAME_coord, NAME_V, NAME_X, NAME_Q (the inputs, checked by `committed`), NAME_hv [K, N, 3], NAME_ext_hv [K, M, 3],
NAME_agree_hv / NAME_agree_ext (the agreement of the two Richardson extrapolants), NAME_charges [N] and NAME_t_q [K, N] (the oracle's
charges and their tangents, for the rounding allowance of the gates); cold24 in the uniform field UNIFORM_E: cold24_uniform_hv,
cold24_uniform_dhv = H v - H_bare v and their agreements."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import embedding_hessian_yardstick as EH  # noqa: E402
from aimnetcentral_amd import synth  # noqa: E402
from oracle import aimnet2_oracle as O  # noqa: E402


def main():
    models = {False: O.OracleModel(synth.synthetic_state_dict(0), torch.float64),
              True: O.OracleModel(synth.synthetic_state_dict(0, None, 2), torch.float64)}
    out = {}
    for name in EH.GPU_CASES:
        c = EH.case(name)
        y = EH.yardstick(c, models[c.nse])
        ref = EH.model_at(c, models[c.nse], c.coord)
        K, n = c.V.shape[:2]
        out.update({f"{name}_coord": c.coord, f"{name}_V": c.V, f"{name}_X": c.X, f"{name}_Q": c.Q, f"{name}_hv": y["hv"],
                    f"{name}_ext_hv": y["ext_hv"], f"{name}_agree_hv": y["agree_hv"], f"{name}_agree_ext": y["agree_ext"],
                    f"{name}_charges": ref["charges"], f"{name}_t_q": c.V.reshape(K, 3 * n).astype(np.float64) @ ref["J"]})
    c = EH.case("cold24")
    y = EH.yardstick(c, models[False], E=EH.UNIFORM_E)
    out.update({"cold24_uniform_hv": y["hv"], "cold24_uniform_dhv": y["ext_hv"], "cold24_uniform_agree_hv": y["agree_hv"],
                "cold24_uniform_agree_dhv": y["agree_ext"]})
    np.savez_compressed(os.path.join(HERE, "embedding_hessian.npz"), **out)


if __name__ == "__main__":
    main()
