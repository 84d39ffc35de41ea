"""`bench.py --dump-outputs DIR`: what the timed path computed in its last step, as .npy files that two builds can be
compared by.  CPU tier: the writer's budget and its fixed sample; GPU tier: the files of a real run and their
reproducibility from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

LIMIT = 64 * 10 ** 6          # all files together, .npy headers included


def _sizes(d):
    return {f: os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_keeps_small_arrays_whole_and_samples_the_large_one(tmp_path):
    g = torch.Generator().manual_seed(1)
    xt, vt = torch.rand(1000, 3, generator=g), torch.rand(1000, 3, generator=g)
    grad = torch.rand(40 * 2 ** 20 // 4, generator=g)                       # 40 MiB: more than what is left for it
    budget = 20 * 2 ** 20
    info = bench.dump_outputs(str(tmp_path / "a"), {"xt": xt, "vt": vt, "grad": grad}, budget=budget)
    assert info["xt"] == (1000, 1000) and info["vt"] == (1000, 1000)
    assert 0 < info["grad"][0] < info["grad"][1] == grad.numel()
    assert sum(_sizes(tmp_path / "a").values()) <= budget + 3 * 1024
    assert np.array_equal(np.load(tmp_path / "a" / "xt.npy"), xt.numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "vt.npy"), vt.numpy())
    s = np.load(tmp_path / "a" / "grad.npy")
    assert s.dtype == np.float32 and s.shape == (info["grad"][0],)
    assert np.all(np.isin(s, grad.numpy()))                                 # a sample of the array's own values
    # the sample is fixed: a second dump of the same shapes takes the same rows
    bench.dump_outputs(str(tmp_path / "b"), {"xt": xt, "vt": vt, "grad": grad}, budget=budget)
    assert np.array_equal(np.load(tmp_path / "b" / "grad.npy"), s)


def test_dump_outputs_default_budget_fits_the_headline_outputs(tmp_path):
    """The headline's shapes (1M exit rays, 256^3 grid) under the default budget: under 64 MB in all."""
    xt = torch.zeros(1024 * 1024, 3)
    grad = torch.zeros(256 ** 3)
    bench.dump_outputs(str(tmp_path), {"xt": xt, "vt": xt, "grad": grad})
    sz = _sizes(tmp_path)
    assert set(sz) == {"xt.npy", "vt.npy", "grad.npy"} and sum(sz.values()) < LIMIT


def test_steps_and_warmup_are_validated():
    assert bench.parse_args(["--steps", "7", "--warmup", "0"]).steps == 7
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def _bench(out, steps):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", "1",
                        "--no-variants", "--no-cpu-baseline", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, "exactly ONE line on stdout"
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_dumps_the_last_step_reproducibly(gpu, tmp_path):
    a = _bench(tmp_path / "a", 2)
    b = _bench(tmp_path / "b", 3)
    assert a["steps"] == 2 and b["steps"] == 3
    n, R = a["config"]["rays_rank0"], a["config"]["grid"]
    for d in (tmp_path / "a", tmp_path / "b"):
        sz = _sizes(d)
        assert set(sz) == {"xt.npy", "vt.npy", "grad.npy"} and sum(sz.values()) < LIMIT
    xa, va, ga = (np.load(tmp_path / "a" / f) for f in ("xt.npy", "vt.npy", "grad.npy"))
    xb, vb, gb = (np.load(tmp_path / "b" / f) for f in ("xt.npy", "vt.npy", "grad.npy"))
    assert xa.shape == va.shape == (n, 3) and xa.dtype == np.float32
    assert ga.dtype == np.float32 and ga.ndim == 1 and 0 < ga.size < R ** 3
    assert np.all(np.isfinite(xa)) and np.all(np.isfinite(ga)) and np.any(ga != 0)
    # the same inputs in both runs: the forward march is bit-exact, the adjoint's fp32 atomics sum in any order
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)
    assert np.linalg.norm(ga.astype(np.float64) - gb) <= 1e-5 * np.linalg.norm(ga.astype(np.float64))
