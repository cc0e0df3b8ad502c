"""The inputs of tests/test_gpu_dense_rows.py, pinned without a GPU: every geometry has the neighbour-row lengths its case is named
for (so that the GPU tests cannot drift back into rows of <= 128 entries), and on every one of them the fp32 CPU oracle sits within
HALF of the force, charge and stress gates from the fp64 oracle (so that a miss on the GPU is the engine's, not a regime in which
the reference itself cannot hold the gate).  The reference results are the ones the GPU tests use (one cache)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import test_gpu_dense_rows as D
from oracle import aimnet2_oracle as O


@pytest.fixture(scope="module")
def oracle64_cold(synth_sd_cold):
    return O.OracleModel(synth_sd_cold, torch.float64)


@pytest.mark.parametrize("name", list(D.CASES))
def test_rows_are_as_long_as_the_case_says(name):
    g = D.case(name)
    k = D.row_counts(g)
    every, longest_lo, longest_hi = g["rows"]
    print(f"{name}: {len(k)} atoms, rows {k.min()}-{k.max()}")
    assert k.min() >= every and longest_lo <= k.max() <= longest_hi, (name, int(k.min()), int(k.max()), g["rows"])


def test_the_ladder_and_the_other_cases_are_what_the_gpu_tests_say():
    k = {name: D.row_counts(D.case(name)) for name in ("s088", "s080", "s074", "s068", "g2x384")}
    assert k["s088"].max() <= 112                            # C: fits the presets 112, 128, 144 without overflow
    assert all(k[n].max() > 128 for n in ("s080", "s074", "s068")) and k["s068"].min() > 192
    assert k["s074"].max() >= 177                            # E
    assert all(v.min() > 64 for n, v in k.items() if n != "g2x384")  # more than one 64-lane lap in every row
    # G: both clusters in one batch, rows above 128 (interior of the denser cluster) next to rows of less than one lap (surface)
    assert (k["g2x384"] > 128).sum() >= 16 and (k["g2x384"] <= 64).sum() >= 64 and k["g2x384"][:384].max() > 64


def test_the_full_row_case_has_rows_of_exactly_128_with_a_margin():
    """d128: the longest row is exactly 128 - also for a cutoff moved by +-2e-4 A, far more than the engine's fp32 distances and its
    own wrap differ from the oracle's fp64 ones, so the engine counts the same."""
    g = D.case("d128")
    k = D.row_counts(g)
    assert k.max() == 128 and (k == 128).sum() == 4
    assert D.row_counts(g, 5.0 - 2e-4).max() == 128 and D.row_counts(g, 5.0 + 2e-4).max() == 128


def _inside_half_the_gates(refs, what):
    r = D.gate_ratios(*refs)
    print(what, "fp32 oracle vs fp64 oracle, fractions of the gates:", r, "|dE|", float(np.abs(refs[0]["energy"] - refs[1]["energy"]).max()))
    assert all(v <= 0.5 for v in r.values()), (what, r)


@pytest.mark.parametrize("name", list(D.CASES))
def test_fp32_oracle_is_within_half_the_gates_of_fp64(oracle32_cold, oracle64_cold, name):
    _inside_half_the_gates(D.references(name, oracle32_cold, oracle64_cold), name)


@pytest.mark.parametrize("mult", [1.0, 3.0])
def test_two_channel_weights_hold_the_same_condition_at_s080(mult):
    o32, o64 = D.nse_cold_oracles()
    _inside_half_the_gates(D.references("s080", o32, o64, tag=f"nse{mult}", mult=np.array([mult], np.float32)), f"s080 nse mult {mult:.0f}")


def test_hvp_bound_is_twice_the_fp32_oracles_distance(oracle32_cold, oracle64_cold):
    """The absolute bound of test_hvp_dense_rows: twice the fp32 analytic oracle's largest distance from the fp64 one on that case
    (the constant is the recorded measurement; fp32 summation order may move a re-measurement a little, not by a quarter)."""
    V, h64 = D.hvp_case(oracle64_cold)
    _, h32 = D.hvp_case(oracle32_cold, V)
    d = float(np.abs(np.asarray(h32["hv"], np.float64) - h64["hv"]).max())
    print(f"fp32 analytic oracle vs fp64: max|d(Hv)| = {d:.3e} on max|Hv| = {np.abs(h64['hv']).max():.3e}")
    assert 0.75 * D.HVP_FP32_DISTANCE <= d <= 1.25 * D.HVP_FP32_DISTANCE
    assert D.HVP_BOUND == 2 * D.HVP_FP32_DISTANCE <= 1e-5 + 3e-5 * np.abs(h64["hv"]).max()
