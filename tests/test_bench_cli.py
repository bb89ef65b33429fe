"""``bench.py`` options of a plain run, on CPU (torch backend, ResNet-8, 2 members x 4 images): ``--steps`` sets the
number of timed steps and the result line holds ``ms_per_step``; ``--dump-outputs DIR`` writes the last timed step's
losses, the members' BN statistics and the norms of their weights and of the update as ``.npy`` files; that step
starts from the seeded start condition, so the files are identical from run to run (the CPU path is deterministic);
``--full`` prints the same kind of line and adds the single weights to the dump."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--backend", "torch", "--resnet_size", "8", "--pop", "2",
        "--batch", "4"]


def _bench(extra, cwd):
    env = dict(os.environ, OMP_NUM_THREADS="1", PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""),
               CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + ARGS + extra, cwd=str(cwd), env=env,
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.timeout(300)
def test_bench_dump_outputs_and_full(tmp_path):
    outs = []
    for d, extra in (("a", []), ("b", ["--full"])):
        out = _bench(["--dump-outputs", str(tmp_path / d)] + extra, tmp_path)
        assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0
        assert out["unit"] == "images/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
        # 3 timed steps of 2 x 4 images: value and ms_per_step describe the same steps
        assert out["value"] == pytest.approx(8 / (out["ms_per_step"] / 1e3), rel=1e-2)
        outs.append({f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = outs
    assert sorted(a) == ["losses", "params_norm", "running"]
    assert sorted(b) == sorted(list(a) + ["params", "update_norm"])  # single weights and the update only with --full
    assert a["losses"].shape == (2,) and a["running"].shape[0] == 2 and b["params"].shape[0] == 2
    assert a["params_norm"].shape == (2,) and b["update_norm"].shape == (2,)
    assert sum(v.nbytes for v in b.values()) <= 64 << 20
    for k, v in b.items():
        assert v.dtype == (np.float64 if k.endswith("_norm") else np.float32) and np.isfinite(v).all(), k
    for k, v in a.items():
        np.testing.assert_array_equal(v, b[k], err_msg=k)
    assert (a["losses"] > 0).all() and (b["update_norm"] > 0).all()
    np.testing.assert_allclose(a["params_norm"], np.linalg.norm(b["params"].astype(np.float64), axis=1), rtol=1e-12)    # the last timed step starts from the seeded start condition whatever ran before it: a run of one step with no
    # warm-up writes the same arrays (later arguments override the earlier --steps / --warmup)
    one = _bench(["--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path / "c")], tmp_path)
    assert one["steps"] == 1
    for k, v in a.items():
        np.testing.assert_array_equal(v, np.load(tmp_path / "c" / (k + ".npy")), err_msg=k)


def test_bench_dump_sample_is_fixed():
    """Weights beyond the byte budget are cut to the same seeded columns for every member and every run."""
    import torch
    import bench

    class Eng:
        P, R = 3 * (bench.DUMP_BYTES // 16), 5
        state = torch.arange(2 * (P + R), dtype=torch.float32).reshape(2, P + R)
        params, running = state[:, :P], state[:, P:]

    import tempfile
    got = []
    for _ in range(2):
        with tempfile.TemporaryDirectory() as d:
            bench.dump_outputs(d, torch.tensor([0.5, 1.5]), Eng.params[[1, 0]], Eng.running[[1, 0]],
                               Eng.params[[1, 0]] - 1.0, 0, 1, full=True)
            got.append({f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)})
            assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 << 20
    a, b = got
    cols = a["params_columns"].astype(np.int64)
    assert len(cols) < Eng.P and (np.diff(cols) > 0).all()
    np.testing.assert_array_equal(a["params_columns"], b["params_columns"])
    np.testing.assert_array_equal(a["params"], Eng.params[[1, 0]][:, cols].numpy())
    np.testing.assert_array_equal(a["running"], Eng.running[[1, 0]].numpy())
