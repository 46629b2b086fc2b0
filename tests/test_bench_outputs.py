"""bench.py --dump-outputs / --full: the output files (types, size cap, run-to-run identity) and
what a plain run's result line carries."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_dump_outputs_types_and_cap(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    g = torch.Generator().manual_seed(0)
    outs = {"loss": torch.tensor(1.5), "wide": torch.randn(3, 7, generator=g, dtype=torch.float64),
            "big": torch.randn(5000, generator=g), "ids": torch.arange(10)}
    args = argparse.Namespace(dump_outputs=str(tmp_path / "a"))
    bench.dump_outputs(args, outs)
    bench.dump_outputs(argparse.Namespace(dump_outputs=str(tmp_path / "b")), outs)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in outs}
    assert got["loss"].dtype == np.float32 and got["loss"].tolist() == [1.5]
    assert got["wide"].dtype == np.float64
    assert np.array_equal(got["wide"], outs["wide"].reshape(-1).numpy())
    assert got["ids"].dtype == np.float32 and got["ids"].tolist() == list(range(10))
    # over its share (4096 / 4 arrays = 1024 bytes = 256 floats): a sample of the array's own
    # elements in their order, the same one in every run
    big = outs["big"].numpy()
    assert got["big"].dtype == np.float32 and got["big"].shape == (256,)
    pos = np.searchsorted(np.sort(big), got["big"])
    assert np.array_equal(np.sort(big)[pos], got["big"])
    assert sum(a.nbytes for a in got.values()) <= 4096
    for n in outs:
        assert np.array_equal(got[n], np.load(tmp_path / "b" / f"{n}.npy"))
    # no directory given: nothing is written
    bench.dump_outputs(argparse.Namespace(dump_outputs=None), outs)
    assert sorted(os.listdir(tmp_path)) == ["a", "b"]


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """one plain run on a small graph: the result line has the headline keys and none of the
    --full legs, --steps is the number of timed steps, and the dump holds the NS step's loss,
    gradients and parameters (float32, finite, the loss the line reports)."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--scale",
                        "0.2", "--steps", "6", "--warmup", "2", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 6 and rec["warmup"] == 2 and rec["n_gpus"] == 1
    assert rec["unit"] == "edges/s" and rec["higher_is_better"] is True and rec["dtype"] == "fp32"
    assert rec["ms_per_step"] > 0 and rec["value"] > 0
    edges = rec["config"]["aggregated_edges_per_step_per_rank"] * 6
    assert rec["value"] == pytest.approx(edges / (rec["ms_per_step"] * 6e-3), rel=1e-6)
    for k in ("full_batch", "cpu_baseline", "ns_kernels_ms", "roofline", "sampler_roofline"):
        assert k not in rec
    assert sorted(os.listdir(out)) == ["grads.npy", "loss.npy", "params.npy"]
    d = {n: np.load(out / f"{n}.npy") for n in ("grads", "loss", "params")}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in d.values())
    assert d["loss"].shape == (1,) and float(d["loss"][0]) == rec["config"]["final_loss"]
    assert d["grads"].shape == d["params"].shape and d["params"].size > 1000
    assert np.abs(d["grads"]).max() > 0
