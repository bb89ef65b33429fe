"""The driver shared by the HIP step backends (engine/hip_step.py) on the CPU: plan caches, eval chunking, the import
layering of the ``hip_*`` modules and the release of captured graphs on distributed shutdown."""
import json
import os
import subprocess
import sys
import types

import pytest
import torch

from distributedtf_amd.engine import hip_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 4


class _FakePlan:
    """Records how it was built; as an eval plan, counts the labels equal to 1 per slot into ev_acc[0]."""
    built = []

    def __init__(self, be, slots, sizes, eval_mode=False):
        self.slots, self.sizes, self.eval = slots, sizes, eval_mode
        self.ev_acc = _CountedZero(2, CAP)
        self.loads = 0
        _FakePlan.built.append((tuple(slots), tuple(sizes), eval_mode))

    def load_eval(self, x, y):
        assert x.shape[0] == y.shape[0] == self.sizes[0]
        self.y = y
        self.loads += 1

    def run_eval(self):
        for s in self.slots:
            self.ev_acc.t[0, s] += float((self.y == 1).sum())


class _CountedZero:
    """ev_acc stand-in: a tensor that counts its zero_() calls (and starts dirty, so a missing zero_() shows)."""

    def __init__(self, *shape):
        self.t = torch.full(shape, 100.0)
        self.zeroed = 0

    def zero_(self):
        self.zeroed += 1
        self.t.zero_()

    def __getitem__(self, i):
        return self.t[i]


class _Backend(hip_step.HipBackend):
    _plan_cls = _FakePlan
    max_plans = 2
    max_eval_plans = 3


@pytest.fixture
def be(monkeypatch):
    monkeypatch.delenv("DTF_EVAL_CHUNK", raising=False)
    monkeypatch.setattr(_FakePlan, "built", [])
    return _Backend(types.SimpleNamespace(device=torch.device("cpu")))


def test_plan_is_cached_per_slots_and_sizes(be):
    p = be.plan([0, 1], [8, 8])
    assert be.plan([0, 1], [8, 8]) is p and be.plan((0, 1), (8, 8)) is p
    assert be.plan([0, 1], [8, 4]) is not p and be.plan([1, 0], [8, 8]) is not p
    assert _FakePlan.built == [((0, 1), (8, 8), False), ((0, 1), (8, 4), False), ((1, 0), (8, 8), False)]


def test_training_cache_clears_past_its_bound(be):
    plans = [be.plan([0], [n]) for n in (1, 2, 3)]  # the bound is exceeded only by the third plan
    assert list(be._plans.values()) == plans
    p4 = be.plan([0], [4])
    assert list(be._plans.values()) == [p4]
    assert be.plan([0], [1]) is not plans[0]  # rebuilt after the clear


def test_eval_cache_evicts_oldest_and_spares_training_plans(be):
    train = be.plan([0, 1], [8, 8])
    ev = [be.eval_plan([0, 1], m) for m in (1, 2, 3)]
    assert [p.sizes for p in ev] == [[1, 1], [2, 2], [3, 3]] and all(p.eval for p in ev)
    assert be.eval_plan([0, 1], 2) is ev[1]
    for m in range(4, 20):
        be.eval_plan([0, 1], m)
        assert len(be._eval_plans) == 3
    assert list(be._eval_plans) == [((0, 1), m) for m in (17, 18, 19)]  # oldest first out
    assert be.plan([0, 1], [8, 8]) is train and list(be._plans.values()) == [train]


def test_evaluate_population_chunks_with_a_remainder(be):
    x = torch.zeros(5, 3)
    y = torch.tensor([1, 0, 1, 1, 2])
    acc = be.evaluate_population([2, 0], x, y, chunk=2)
    assert acc == {2: 3 / 5.0, 0: 3 / 5.0}
    assert _FakePlan.built == [((2, 0), (2, 2), True), ((2, 0), (1, 1), True)]
    p2, p1 = be._eval_plans[((2, 0), 2)], be._eval_plans[((2, 0), 1)]
    assert (p2.loads, p1.loads) == (2, 1)
    assert (p2.ev_acc.zeroed, p1.ev_acc.zeroed) == (1, 1)
    # a second pass reuses the plans and zeroes each once more: the counts do not carry over
    assert be.evaluate_population([2, 0], x, y, chunk=2) == acc
    assert (p2.ev_acc.zeroed, p1.ev_acc.zeroed) == (2, 2) and len(_FakePlan.built) == 2


def test_evaluate_population_empty_inputs_build_no_plan(be):
    assert be.evaluate_population([0, 1], torch.zeros(0, 3), torch.zeros(0, dtype=torch.long)) == {0: 0.0, 1: 0.0}
    assert be.evaluate_population([], torch.zeros(5, 3), torch.zeros(5, dtype=torch.long)) == {}
    assert _FakePlan.built == []


def test_eval_chunk_comes_from_the_class_attributes(be, monkeypatch):
    x, y = torch.zeros(5, 3), torch.ones(5, dtype=torch.long)
    monkeypatch.setattr(_Backend, "eval_chunk", 4, raising=False)  # the default, no env variable set
    assert be.evaluate_population([0], x, y) == {0: 1.0}
    assert [b[1] for b in _FakePlan.built] == [(4,), (1,)]
    monkeypatch.setattr(_Backend, "eval_chunk_env", "DTF_EVAL_CHUNK_STUB", raising=False)
    monkeypatch.setenv("DTF_EVAL_CHUNK", "1")  # not this backend's variable
    monkeypatch.setenv("DTF_EVAL_CHUNK_STUB", "3")
    be.evaluate_population([0], x, y)
    assert [b[1] for b in _FakePlan.built[2:]] == [(3,), (2,)]
    be.evaluate_population([0], x, y, chunk=5)  # an explicit chunk wins over the environment
    assert [b[1] for b in _FakePlan.built[4:]] == [(5,)]


def test_backend_defaults_per_family():
    from distributedtf_amd.engine import hip_f32, hip_imagenet, hip_imagenet_f32, hip_mnist, hip_mnist_f32, hip_resnet
    got = {c.__name__: (c.max_plans, c.max_eval_plans, c.eval_chunk_env, c.eval_chunk, c._plan_cls.__name__)
           for c in (hip_resnet.HipResNetBackend, hip_f32.HipResNetF32Backend, hip_mnist.HipMnistBackend,
                     hip_mnist_f32.HipMnistF32Backend, hip_imagenet.HipImageNetBackend,
                     hip_imagenet_f32.HipImageNetF32Backend)}
    assert got == {
        "HipResNetBackend": (16, 9, "DTF_EVAL_CHUNK", 2000, "_StepPlan"),
        "HipResNetF32Backend": (4, 4, "DTF_EVAL_CHUNK", 2000, "_F32Plan"),
        "HipMnistBackend": (16, 4, "DTF_EVAL_CHUNK", 2500, "_MnistPlan"),
        "HipMnistF32Backend": (16, 4, "DTF_EVAL_CHUNK", 2500, "_MnistF32Plan"),
        "HipImageNetBackend": (4, 4, "DTF_EVAL_CHUNK_IMAGENET", 64, "_ImageNetPlan"),
        "HipImageNetF32Backend": (4, 4, "DTF_EVAL_CHUNK_IMAGENET", 64, "_ImageNetF32Plan"),
    }


_FRESH = """
import json, sys
from distributedtf_amd.engine import hip_step
from distributedtf_amd.parallel import comm
out = {"resnet_before_shutdown": "distributedtf_amd.engine.hip_resnet" in sys.modules}
class Plan: graph = object()
plan = Plan()
hip_step._LIVE_GRAPH_PLANS.add(plan)
comm.shutdown_distributed()  # no process group was initialised: only the graph release runs
out["graph_released"] = plan.graph is None and not hip_step._LIVE_GRAPH_PLANS
import distributedtf_amd.engine.hip_mnist
out["step_after_mnist"] = "distributedtf_amd.engine.hip_step" in sys.modules
out["resnet_after_mnist"] = "distributedtf_amd.engine.hip_resnet" in sys.modules
from distributedtf_amd.engine import hip_resnet
out["same_objects"] = [n for n in ("graph_state", "run_captured", "advance_steps", "upload_hyper", "same_batches")
                       if getattr(hip_resnet, n) is getattr(hip_step, n)]
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def fresh():
    """One fresh interpreter (what is imported is the point) serves the two tests below."""
    r = subprocess.run([sys.executable, "-c", _FRESH], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def test_import_layering_and_compatibility(fresh):
    assert fresh["step_after_mnist"] and not fresh["resnet_after_mnist"]
    assert fresh["same_objects"] == ["graph_state", "run_captured", "advance_steps", "upload_hyper", "same_batches"]


def test_shutdown_releases_captured_graphs(fresh):
    assert not fresh["resnet_before_shutdown"]  # only the shared module was loaded
    assert fresh["graph_released"]
