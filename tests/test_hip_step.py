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


# ---- HipPlan: the member layout, staging and launch-list runner every family's plan shares (no device needed)
class _StubPlan(hip_step.HipPlan):
    def __init__(self, slots, sizes, eval_mode=False, counts=None):
        be = types.SimpleNamespace(e=types.SimpleNamespace(capacity=3), dev=torch.device("cpu"), loss=torch.zeros(3),
                                   shadow=None)
        self._init_members(be, slots, sizes, eval_mode, counts=counts)
        self.x_in = torch.zeros(self.N, 2, 2)
        self.labels = torch.zeros(self.N, dtype=torch.int32)
        self.seen = []

    def _marker_note(self, tag):
        self.seen.append(("note", tag))


def test_plan_member_layout():
    p = _StubPlan([0, 2], [3, 2])
    assert p.first == {0: 0, 2: 3} and p.N == 5
    assert p.img_slot.tolist() == [0, 0, 0, 2, 2] and p.img_slot.dtype == torch.int32
    assert p.cnt.tolist() == [3.0, 0.0, 2.0]  # 0 in the idle slot
    assert p.slots_t.tolist() == [0, 2] and p.slots_long.dtype == torch.long and tuple(p.loss_sel.shape) == (2,)
    assert p.launches == [] and p.graph is None and p.ring is None and not p.eval
    # elastic form: the layout of the capacity sizes, the counts of the real ones
    q = _StubPlan([0, 2], [3, 3], counts=[1, 2])
    assert q.first == {0: 0, 2: 3} and q.N == 6 and q.cnt.tolist() == [1.0, 0.0, 2.0]


def test_plan_member_chunks():
    p = _StubPlan([0, 2], [3, 2])
    assert p._chunks(2).tolist() == [[0, 2, 0, 0], [2, 1, 0, 0], [3, 2, 0, 2]]
    assert p._chunks(1 << 30).tolist() == [[0, 3, 0, 0], [3, 2, 0, 2]]  # larger than any member: one row each
    assert p._chunks(lambda n: n - 1).tolist() == [[0, 2, 0, 0], [2, 1, 0, 0], [3, 1, 0, 2], [4, 1, 0, 2]]
    assert p._chunks(2).dtype == torch.int32 and p._chunk_rows(2, 0, 4) == []


def test_plan_load_eval_replicates_the_chunk():
    p = _StubPlan([0, 2], [2, 2], eval_mode=True)
    x, y = torch.arange(8.0).reshape(2, 2, 2), torch.tensor([5, 7])
    p.load_eval(x, y)
    assert torch.equal(p.x_in[:2], x) and torch.equal(p.x_in[2:], x) and p.labels.tolist() == [5, 7, 5, 7]
    with pytest.raises(AssertionError, match="same chunk"):
        _StubPlan([0, 2], [2, 1], eval_mode=True).load_eval(x, y)


def test_plan_load_batch_skips_an_unmodified_batch():
    p = _StubPlan([0, 2], [3, 2])
    batches = [(torch.full((3, 2, 2, 1), 1.0), torch.tensor([1, 1, 1])), (torch.full((2, 4), 2.0), torch.tensor([2, 2]))]
    p.load_batch(batches)
    assert p.x_in[:, 0, 0].tolist() == [1.0, 1.0, 1.0, 2.0, 2.0] and p.labels.tolist() == [1, 1, 1, 2, 2]
    p.x_in.zero_()
    p.load_batch(batches)  # the same storages, unmodified: nothing is staged again
    assert float(p.x_in.abs().sum()) == 0.0
    batches[1][0].add_(1.0)  # modified in place: staged again
    p.load_batch(batches)
    assert p.x_in[:, 0, 0].tolist() == [1.0, 1.0, 1.0, 3.0, 3.0]
    # a subset of the members lands in their own regions
    p.load_batch([(torch.full((2, 2, 2), 9.0), torch.tensor([4, 4]))], slots=[2])
    assert p.x_in[:, 0, 0].tolist() == [1.0, 1.0, 1.0, 9.0, 9.0] and p.labels.tolist() == [1, 1, 1, 4, 4]


def test_plan_runs_launchers_markers_and_names_a_failing_launcher(monkeypatch):
    monkeypatch.setattr(hip_step.ops, "stream", lambda: "STREAM")
    p = _StubPlan([0, 2], [3, 2], eval_mode=True)
    buf = torch.ones(3)

    def dtf_stub_ok(a, b, stream):
        p.seen.append(("ok", a, b, stream))
        return 0

    def dtf_stub_fail(stream):
        return 7

    p._add("zero", buf)
    p._add(dtf_stub_ok, 1, 2)
    p._add("note", "family marker")
    p.run_eval()
    assert p.seen == [("ok", 1, 2, "STREAM"), ("note", "family marker")] and buf.tolist() == [0.0, 0.0, 0.0]
    p._add(dtf_stub_fail)
    p._add("note", "not reached")
    with pytest.raises(RuntimeError, match="dtf_stub_fail failed with 7"):
        p.run_eval()
    assert p.seen[-1] == ("note", "family marker")
    with pytest.raises(AssertionError):
        _StubPlan([0], [1]).run_eval()  # a training plan is not an eval plan
