"""Dynamic per-member loss scaling of the fp16 HIP step (--loss_scale dynamic) on the GPU.

Kernel level, on the release, deterministic, fp16 and fp16-deterministic libraries (one child process per library, as
in tests/test_gpu_fp16.py: the library is chosen when it is loaded): the gradient finiteness pass
(``dtf_grad_finite_check``), the fused optimizer reading the scale table (``dtf_fused_optimizer_dyn``: bitwise the
static launch for a clean member, a bitwise no-op + zeroed gradients for a flagged one), the scale rule
(``dtf_loss_scale_update`` against engine/optim.py) and the head with ``HeadArgs.scale_tab`` (bitwise the scalar
``loss_scale`` launch of each member).  Whole step, on the two fp16 libraries, graph replay and eager: a member at
scale 2^40 overflows, keeps its parameters and slots to the bit and halves its scale while the others train as on a
static-scale-128 engine (bitwise in the deterministic build; in the release build within 4 x the deviation measured
between two runs of the static engine -- the values are printed, profiles/dynamic_loss_scale_pytest.log).  And
main_manager.py end to end.  The checks themselves are in tests/_dynamic_loss_scale_child.py."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "_dynamic_loss_scale_child.py")
LIBS = {"release": {}, "det": {"DTF_DETERMINISTIC": "1"}, "f16": {"DTF_HALF": "1"},
        "f16_det": {"DTF_HALF": "1", "DTF_DETERMINISTIC": "1"}}


def _env(lib):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("DTF_HALF", "DTF_DETERMINISTIC", "DTF_DEBUG", "DTF_LIB", "DTF_HIP_GRAPH"):
        env.pop(k, None)
    env.update(LIBS[lib])
    return env


def _child(lib, what):
    r = subprocess.run([sys.executable, "-u", CHILD, what], cwd=ROOT, env=_env(lib), capture_output=True, text=True,
                       timeout=280)
    out = r.stdout + r.stderr
    print(out[-6000:])
    assert r.returncode == 0 and ("DLS_OK " + what) in r.stdout, out[-6000:]
    want = "library: half=%s deterministic=%s" % ("f16" in lib, "det" in lib)
    assert want in r.stdout, (want, r.stdout[:200])
    return r.stdout


@pytest.mark.parametrize("lib", list(LIBS))
def test_kernels(lib):
    out = _child(lib, "kernels")
    assert out.count("finite_check P=1048579") == 9 and out.count("finite_check P=5 ") == 9
    assert "optimizer with table" in out and "scale update" in out and "head with scale_tab (slab form)" in out
    assert ("head with scale_tab (atomic form)" in out) == ("det" not in lib)


@pytest.mark.parametrize("lib", ["f16", "f16_det"])
def test_whole_step(lib):
    out = _child(lib, "step")
    assert "whole step (graph" in out and "whole step (eager" in out and out.count("DEVIATION") >= 2


def test_main_manager_end_to_end(tmp_path):
    cmd = [sys.executable, "-u", os.path.join(ROOT, "main_manager.py"), "2", "--model", "cifar10", "--resnet_size", "8",
           "--dtype", "fp16", "--loss_scale", "dynamic", "--max_train_steps", "6", "--rounds", "1",
           "--use_synthetic_data", "true", "--seed", "3", "--hooks", "logging", "--log_every_n_steps", "3",
           "--savedata", str(tmp_path / "savedata"), "--results_file", str(tmp_path / "results.txt")]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=_env("release"), capture_output=True, text=True, timeout=280)
    out = r.stdout + r.stderr
    print(out[-4000:])
    assert r.returncode == 0, out[-4000:]
    assert "loss_scale = " in r.stdout and "skipped_steps = " in r.stdout  # the logging hook line
    recs = [json.loads(l) for l in open(tmp_path / "savedata" / "metrics.jsonl")]
    rec = recs[-1]
    assert set(rec["loss_scale"]) == {"0", "1"} and set(rec["skipped_steps"]) == {"0", "1"}, rec
    for i in ("0", "1"):
        s, k = rec["loss_scale"][i], rec["skipped_steps"][i]
        assert 1.0 <= s <= 2.0 ** 15 and s == 2.0 ** 15 / 2 ** k and 0 <= k <= 6, rec  # halved once per skipped step
    assert rec["step_graph"] == ["captured"], rec
    assert rec["population"] == 2 and rec["best_acc"] == rec["best_acc"] and rec["mean_acc"] == rec["mean_acc"], rec
    best = json.load(open(tmp_path / "savedata" / "best_model.json"))
    assert best["best_acc"] == best["best_acc"]
