"""bench.py end to end on the GPU box: the single-GPU JSON contract, and the N > 1 control flow (barriers, max-over-ranks
timing, all-gather of the per-frame energies, rank 0's untimed per-family pass) with two ranks that share the one GPU
through the gloo backend (RCCL refuses two ranks on one device; BENCH_BACKEND is a test switch only)."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
        "data", "config", "roofline"}


def _last_json(out: str) -> dict:
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert lines, out[-2000:]
    return json.loads(lines[-1])


HEADLINE = KEYS - {"roofline"}


def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    """Without --full: one timed region of exactly --steps steps, the headline keys alone, and --dump-outputs writes what the last
    timed step returned; the same arguments give the same outputs again."""
    dumps = []
    for k in range(2):
        out = tmp_path / f"run{k}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--workload", "md1024",
                            "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        d = _last_json(r.stdout)
        assert set(d) == HEADLINE and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
        assert abs(d["value"] - d["config"]["atoms_per_gpu"] * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
        assert d["dtype"].startswith("f32 (fp16x2-split")
        assert sorted(os.listdir(out)) == ["charges.npy", "energy.npy", "forces.npy"]
        a = {n: np.load(out / (n + ".npy")) for n in ("energy", "charges", "forces")}
        assert a["energy"].shape == (128,) and a["charges"].shape == (6400,) and a["forces"].shape == (6400, 3)
        assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
        dumps.append(a)
    for n in dumps[0]:
        np.testing.assert_allclose(dumps[1][n], dumps[0][n], rtol=1e-6, atol=1e-6, err_msg=n)
    # N > 1 (two ranks on the one GPU over gloo): rank 0 prints the headline alone and dumps its outputs + the gathered energies
    out = tmp_path / "two_ranks"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29532", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ, BENCH_BACKEND="gloo"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    d = _last_json(r.stdout)
    assert set(d) == HEADLINE and d["n_gpus"] == 2 and d["config"]["atoms_per_gpu"] == 10080
    assert np.load(out / "forces.npy").shape == (10080, 3) and np.load(out / "stress.npy").shape == (3, 3)
    assert np.load(out / "energy_all_ranks.npy").shape == (2,)


def test_single_gpu_json_contract():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--workload", "md1024",
                        "--no-cpu-baseline", "--full"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    assert KEYS <= set(d) and d["n_gpus"] == 1 and d["steps"] == 3 and d["value"] > 0
    assert set(d["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic"}
    assert abs(d["value"] - d["config"]["atoms_per_gpu"] * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    # the record of the exact-fp32 kernels rides on the same line (measured after the timed region)
    ex = d["exact_f32"]
    assert ex["value"] > 0 and ex["roofline"]["peak"] == 157.3 and d["dtype"].startswith("f32 (fp16x2-split") and d["roofline"]["peak_fp32_matrix"] == 157.3
    # ... and so does the record of round 4's bf16x3-split operands (the range fallback); the line's own roof is the fp16x2 kernels'
    b3 = d["bf16x3_split"]
    assert b3["value"] > 0 and abs(b3["roofline"]["peak"] - 2500.0 / 6) < 1e-6 and abs(d["roofline"]["peak"] - 2500.0 / 3) < 1e-6
    assert abs(d["roofline"]["frac_vs_bf16x3_roof"] - 2 * d["roofline"]["frac"]) < 1e-9
    rep = d["timed_region_repeat"]
    # `value` is the MEDIAN of the five identical timed regions; the first region is kept beside it
    assert rep["regions"] == 5 and rep["min"] <= rep["median"] <= rep["max"] and abs(rep["median"] - d["ms_per_step"]) < 1e-9
    assert abs(rep["ms_per_step"][0] - d["first_region_ms"]) < 1e-9
    # BASELINE config 4 in the same run: the analytic Hessian at the reference's own gate, and well inside it
    h4 = d["hessian_config4"]
    assert h4["ok"] is True and h4["dH_max"] <= 1e-4 and h4["dHv4_max"] <= 4e-4 and h4["force_evals_per_direction"]["dense"] < 0.2


def test_default_workload_carries_the_parity_gate():
    """The default line (config 3) with the CPU baseline: `parity` compares engine and oracle on the two bounded samples."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--cpu-budget", "1", "--full"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    assert d["config"]["atoms_per_gpu"] == 10080 and d["cpu_baseline"]["kind"] == "port"
    p = d["parity"]
    assert p["ok"] is True and set(p) >= {"pbc2304", "md48x50", "ok"}
    for k in ("pbc2304", "md48x50"):
        assert p[k]["ok"] and p[k]["dF_max"] <= p[k]["gates"]["dF_max"] and p[k]["dq_max"] <= 1e-4
    # the crystal's energy is held against the fp64 oracle (the fp32 oracle itself sits 1.3e-3 eV from it, more than the plain gate:
    # tests/tools/pbc2304_margin.py) - and the engine is INSIDE the plain gate there, an order of magnitude closer than the fp32 oracle
    assert p["pbc2304"]["dE_vs"] == "fp64 oracle" and p["pbc2304"]["dE"] <= p["pbc2304"]["gates"]["dE"] and p["pbc2304"]["rms_ratio"] < 0.5
    for k in ("pbc2304", "md48x50"):
        v = p[k]["dF_elementwise_violations"]
        assert v["of"] == 3 * p[k]["atoms"] and 0 <= v["count"] < 0.02 * v["of"]
    # the cold-weight goldens of the unmodified reference at its LITERAL gates: zero force components outside allclose(1e-4, 1e-5)
    cg = d["parity_cold_goldens"]
    assert cg["ok"] is True and all(cg[k]["dF_elementwise_violations"]["count"] == 0 and cg[k]["dE"] < 1e-5 for k in ("taxol", "batch5", "rand8", "pbc96"))
    # ... and at the sizes the headline is quoted on (coldw_big.npz), in the default GEMM path, with no fp64 anchor
    assert all(cg[k]["ok"] and cg[k]["dF_elementwise_violations"]["count"] == 0 and cg[k]["dE_over_gate"] < 1.0 for k in ("pbc2304", "batch256"))
    assert cg["violations_total"] == 0 and cg["pbc2304"]["atoms"] == 2304
    # the honest fractions and the engine-reported configuration ride on the same line
    assert 0.0 < d["roofline_e2e"]["frac_mixed"] < d["roofline_e2e"]["frac"] < 1.0
    assert d["roofline"]["gemm_launches_per_step"] == 7 and "mfma_busy_frac_in_kernel" in d["roofline"]  # six MLP sweeps + the energy head
    assert d["roofline_gather"]["form"] == "reverse-pair" and "gemm_chain_kernel" in d["roofline"]["kernel"]
    assert abs(d["roofline"]["frac_e2e_fp32_matrix"] - d["roofline_e2e"]["frac"]) < 1e-12 and abs(d["roofline"]["frac_mixed"] - d["roofline_e2e"]["frac_mixed"]) < 1e-12
    # the same frame with Ewald summation (its own record): slower than DSF by the reciprocal-space kernels, not by a factor
    ew = d["ewald_config3"]
    assert d["ms_per_step"] < ew["ms_per_step"] < 1.5 * d["ms_per_step"] and ew["k_box_entries"] > 1000 and np.isfinite(ew["energy_eV"])


def test_two_ranks_share_the_gpu_over_gloo():
    env = dict(os.environ, BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29531", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    d = _last_json(r.stdout)
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and "cpu_baseline" not in d and "exact_f32" not in d
    # headline: config-3 replicas (N = 1 agrees with the single-GPU line); whole-job value = both ranks' atoms over the slowest rank
    assert d["config"]["atoms_per_gpu"] == 10080
    assert abs(d["value"] - 2 * d["config"]["atoms_per_gpu"] * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    # BASELINE configs[4] in the same run: 128 frames x 50 atoms per rank, energies of all ranks gathered every step
    md = d["scaling_md1024"]
    assert md["ranks_seen"] == 2 and md["frames_per_gpu"] == 128 and md["atoms_per_gpu"] == 6400 and md["scaling"] == "weak"
    assert abs(md["value"] - 2 * md["atoms_per_gpu"] * 1e3 / md["ms_per_step"]) < 1e-6 * md["value"]
