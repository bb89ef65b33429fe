"""Dynamic per-member loss scaling (``--loss_scale dynamic``), the parts that need no GPU: flag parsing, the rule
(``engine/optim.py loss_scale_update``, the oracle of the kernel tests), the PyTorch path of the population engine
(skip on overflow, bitwise-unchanged parameters, scale halved, step counter advanced), the row in the member's stream
state (resume), its reset on an exploit import, the reporting, and the launch list of the HIP step's "optim" marker."""
import json

import pytest
import torch

import main_manager
from distributedtf_amd.engine import optim
from distributedtf_amd.engine.population import PopulationEngine
from distributedtf_amd.models.engine_model import EngineModel
from distributedtf_amd.models.resnet import ResNetArch, cifar_config
from distributedtf_amd.utils.flags import get_loss_scale, parse_main_args

INIT = 2.0 ** 15


# ------------------------------------------------------------------------------------------------ flags
def test_flag_accepts():
    a = parse_main_args(["--model", "cifar10", "--dtype", "fp16", "--loss_scale", "dynamic"])
    kw = a.model_kwargs()
    assert a.backend == "auto" and kw["loss_scale"] == "dynamic" and kw["loss_scale_growth_steps"] == 2000
    a = parse_main_args(["--model", "cifar10", "--dtype", "fp16", "--loss_scale", "dynamic", "--backend", "hip",
                         "--loss_scale_growth_steps", "50"])
    assert a.backend == "hip" and a.model_kwargs()["loss_scale_growth_steps"] == 50
    # --backend torch: any family, any dtype
    for model, dtype in (("cifar10", "fp16"), ("cifar10", "fp32"), ("cifar10", "bf16"), ("imagenet", "fp16"),
                         ("mnist", "fp16"), ("mnist", "fp32")):
        a = parse_main_args(["--model", model, "--dtype", dtype, "--loss_scale", "dynamic", "--backend", "torch"])
        assert a.backend == "torch" and a.model_kwargs()["loss_scale"] == "dynamic"
    # families / dtypes whose --backend auto is the PyTorch path with a static scale go there with a dynamic one too
    assert parse_main_args(["--model", "cifar10", "--dtype", "fp32", "--loss_scale", "dynamic"]).backend == "torch"
    assert parse_main_args(["--model", "mnist", "--dtype", "fp16", "--loss_scale", "dynamic"]).backend == "torch"
    assert get_loss_scale("fp16", "dynamic") == "dynamic"


@pytest.mark.parametrize("argv", [
    ["--model", "cifar10", "--loss_scale", "dynamic"],  # bf16
    ["--model", "cifar10", "--dtype", "bf16", "--loss_scale", "dynamic", "--backend", "hip"],
    ["--model", "cifar10", "--dtype", "fp32", "--loss_scale", "dynamic", "--backend", "hip"],
    ["--model", "imagenet", "--dtype", "fp16", "--loss_scale", "dynamic"],
    ["--model", "imagenet", "--dtype", "fp16", "--loss_scale", "dynamic", "--backend", "hip"],
    ["--model", "cifar10", "--dtype", "fp16", "--loss_scale", "dynamic", "--loss_scale_growth_steps", "0"],
    ["--model", "cifar10", "--dtype", "fp16", "--loss_scale", "dynamics"],
])
def test_flag_rejects(argv, capsys):
    with pytest.raises(SystemExit):
        parse_main_args(argv)
    assert "loss_scale" in capsys.readouterr().err  # a message that names the flag


def test_numeric_loss_scale_unchanged():
    assert parse_main_args(["--model", "cifar10", "--dtype", "fp16", "--loss_scale", "64"]).model_kwargs()[
        "loss_scale"] == 64.0
    assert get_loss_scale("fp16", None) == 128 and get_loss_scale("fp32", 5) == 5
    with pytest.raises(SystemExit):
        parse_main_args(["--loss_scale", "-1"])
    assert "loss_scale_growth_steps" not in parse_main_args(["--model", "cifar10", "--dtype", "fp16"]).model_kwargs()


# ------------------------------------------------------------------------------------------------- rule
def test_rule():
    up = optim.loss_scale_update
    assert up([INIT, 7, 1, 3], 2000) == [INIT / 2, 0.0, 0.0, 4.0]  # overflow: halve, restart the run, count
    assert up([2.0, 0, 1, 0], 2000) == [1.0, 0.0, 0.0, 1.0]
    assert up([1.0, 5, 1, 1], 2000) == [1.0, 0.0, 0.0, 2.0]  # floor at 1
    assert up([INIT, 0, 0, 3], 2000) == [INIT, 1.0, 0.0, 3.0]  # clean: count
    assert up([INIT, 1997, 0, 0], 2000) == [INIT, 1998.0, 0.0, 0.0]
    assert up([INIT, 1998, 0, 0], 2000) == [INIT, 1999.0, 0.0, 0.0]  # not before the interval
    assert up([INIT, 1999, 0, 0], 2000) == [2 * INIT, 0.0, 0.0, 0.0]  # growth exactly at the interval
    assert up([2.0 ** 23, 2, 0, 0], 3) == [2.0 ** 24, 0.0, 0.0, 0.0]
    assert up([2.0 ** 24, 2, 0, 9], 3) == [2.0 ** 24, 0.0, 0.0, 9.0]  # cap at 2^24
    assert up([INIT, 0, 0, 0], 1) == [2 * INIT, 0.0, 0.0, 0.0]
    row = [INIT, 0.0, 0.0, 0.0]
    for flag in [0, 0, 1, 0, 0, 0, 1, 1]:  # interval 3: +1 +1 halve +1 +1 double halve halve
        row = up([row[0], row[1], flag, row[3]], 3)
    assert row == [INIT / 4, 0.0, 0.0, 3.0]
    assert optim.LOSS_SCALE_INIT == INIT and optim.LOSS_SCALE_GROWTH_STEPS == 2000 and optim.LOSS_SCALE_MAX == 2 ** 24


# --------------------------------------------------------------------------------------- PyTorch path
def _hp(opt="Momentum"):
    return {"opt_case": {"optimizer": opt, "lr": 0.05, "momentum": 0.9}, "batch_size": 4, "regularizer": "None",
            "weight_decay": 0.0, "initializer": "he_init", "decay_steps": 0, "decay_rate": 1.0}


def _engine(n=2, **kw):
    torch.manual_seed(0)
    arch = ResNetArch(cifar_config(8, 2))
    e = PopulationEngine(arch, n, "cpu", backend="torch", compute_dtype=torch.float32, loss_scale="dynamic", **kw)
    for i in range(n):
        assert e.add_member(None, _hp(), seed=3 + i) == i
    g = torch.Generator().manual_seed(1)
    batches = [(torch.randn(4, 32, 32, 3, generator=g), torch.randint(0, 10, (4,), generator=g)) for _ in range(n)]
    return e, batches


def test_torch_path_skips_on_overflow_then_updates():
    e, batches = _engine(loss_scale_growth_steps=2)
    assert e.dynamic_loss_scale and e.lscale.shape == (2, 4) and e.lscale.tolist() == [[INIT, 0, 0, 0]] * 2
    S_before = e.S
    real = e.backend.forward_backward
    poison = {"on": True}

    def forward_backward(slots, bs):
        out = real(slots, bs)
        if poison["on"]:
            e.grads[1, 17] = float("inf")  # member 1 overflows on this step
        return out

    e.backend.forward_backward = forward_backward
    hps, lrs = [_hp(), _hp()], [0.05, 0.05]
    before = e.state.clone()
    e.train_step([0, 1], batches, hps, lrs)
    # member 1: parameters and slots bitwise unchanged, scale halved, the step still counted
    hi = 3 * e.Pp + e.R  # the BN moving statistics are forward-only: they moved
    assert torch.equal(e.state[1, :3 * e.Pp].view(torch.int32), before[1, :3 * e.Pp].view(torch.int32))
    assert not torch.equal(e.state[1, 3 * e.Pp:hi], before[1, 3 * e.Pp:hi])
    assert e.lscale[1].tolist() == [INIT / 2, 0.0, 0.0, 1.0]
    assert e.host_step == [1, 1] and e.step_col().tolist() == [1.0, 1.0]
    assert not e.grads.any()  # no Inf survives into the next step
    # member 0 updated, finite
    assert not torch.equal(e.state[0, :e.P], before[0, :e.P]) and torch.isfinite(e.state[0]).all()
    assert e.lscale[0].tolist() == [INIT, 1.0, 0.0, 0.0]
    # the next clean step updates member 1; member 0 reaches the growth interval (2)
    poison["on"] = False
    mid = e.state.clone()
    e.train_step([0, 1], batches, hps, lrs)
    assert not torch.equal(e.state[1, :e.P], mid[1, :e.P]) and torch.isfinite(e.state).all()
    assert e.lscale[1].tolist() == [INIT / 2, 1.0, 0.0, 1.0]
    assert e.lscale[0].tolist() == [2 * INIT, 0.0, 0.0, 0.0]
    assert e.host_step == [2, 2] and e.S == S_before  # the table is not part of the state row


def test_torch_path_matches_static_scale():
    """A clean dynamic step is the static-scale step: same scale, same update (power-of-two scaling is exact)."""
    e, batches = _engine()
    torch.manual_seed(0)
    s = PopulationEngine(e.arch, 2, "cpu", backend="torch", compute_dtype=torch.float32, loss_scale=INIT)
    for i in range(2):
        s.add_member(None, _hp(), seed=3 + i)
    assert not s.dynamic_loss_scale and torch.equal(s.state, e.state)
    for eng in (e, s):
        eng.train_step([0, 1], batches, [_hp(), _hp()], [0.05, 0.05])
    assert torch.equal(e.state.view(torch.int32), s.state.view(torch.int32))


# ------------------------------------------------------------------------------ members: resume, exploit
def _members(tmp_path, n=2):
    from distributedtf_amd.models.cifar10_model import Cifar10Model
    from distributedtf_amd.pbt.cluster import sample_population
    EngineModel.reset_engines()
    hps = sample_population(n, seed=0)
    return [Cifar10Model(i, hps[i], str(tmp_path / "model_"), seed=0, resnet_size=8, device="cpu", backend="torch",
                         dtype="fp32", loss_scale="dynamic", loss_scale_growth_steps=7, use_synthetic_data=True)
            for i in range(n)]


def test_resume_restores_row(tmp_path):
    ms = _members(tmp_path)
    eng = ms[0].engine
    assert eng.dynamic_loss_scale and eng.loss_scale_growth_steps == 7 and ms[1].engine is eng
    eng.set_loss_scale_row(ms[1].slot, [256.0, 5.0, 0.0, 9.0])
    saved = json.loads(json.dumps(ms[1].stream_state()))  # as written to the population table
    assert saved["loss_scale"] == [256.0, 5.0, 0.0, 9.0]
    ms[1].ckpt_round = 0
    ms[1].save_checkpoint(wait=True)
    # a new process: fresh members, checkpoint import, then the stream state
    ms = _members(tmp_path)
    eng = ms[0].engine
    assert ms[1].load_checkpoint(round_tag=0)
    assert eng.loss_scale_row(ms[1].slot) == [INIT, 0.0, 0.0, 0.0]
    ms[1].restore_stream_state(saved)
    assert eng.loss_scale_row(ms[1].slot) == [256.0, 5.0, 0.0, 9.0]
    assert eng.loss_scale_row(ms[0].slot) == [INIT, 0.0, 0.0, 0.0]
    EngineModel.reset_engines()


def test_static_members_keep_their_stream_state(tmp_path):
    from distributedtf_amd.models.cifar10_model import Cifar10Model
    from distributedtf_amd.pbt.cluster import sample_population
    EngineModel.reset_engines()
    m = Cifar10Model(0, sample_population(1, seed=0)[0], str(tmp_path / "model_"), seed=0, resnet_size=8, device="cpu",
                     backend="torch", dtype="fp32", loss_scale=64.0, use_synthetic_data=True)
    assert not m.engine.dynamic_loss_scale and "loss_scale" not in m.stream_state()
    EngineModel.reset_engines()


def test_exploit_resets_row(tmp_path):
    from distributedtf_amd.parallel.comm import LocalComm
    from distributedtf_amd.parallel.dataplane import DataPlane
    ms = _members(tmp_path)
    eng = ms[0].engine
    eng.set_loss_scale_row(ms[0].slot, [64.0, 3.0, 0.0, 2.0])   # winner
    eng.set_loss_scale_row(ms[1].slot, [4.0, 6.0, 1.0, 11.0])   # loser
    eng.host_step[ms[0].slot] = 5
    DataPlane(LocalComm.create(1)[0]).execute([(0, 0, 1, 0)], {0: ms[0], 1: ms[1]}, steps={0: 5})
    assert torch.equal(eng.state[ms[1].slot], eng.state[ms[0].slot]) and eng.host_step[ms[1].slot] == 5
    assert eng.loss_scale_row(ms[1].slot) == [INIT, 0.0, 0.0, 11.0]  # initial scale, the skip count stays
    assert eng.loss_scale_row(ms[0].slot) == [64.0, 3.0, 0.0, 2.0]
    # the cross-rank form ends in the same hook (the row arrives in place, then on_state_imported)
    eng.set_loss_scale_row(ms[1].slot, [4.0, 6.0, 1.0, 11.0])
    ms[1].on_state_imported(5)
    assert eng.loss_scale_row(ms[1].slot) == [INIT, 0.0, 0.0, 11.0]
    EngineModel.reset_engines()


# ------------------------------------------------------------------------------------------ whole run
def test_main_manager_reports_and_resumes(tmp_path, monkeypatch, capsys):
    """metrics.jsonl and the logging hook carry loss_scale / skipped_steps; --resume continues with the saved scale
    (growth interval 2, 3 steps per round: [2^16, 1 clean step] after round 0, so 2^18 after round 1 -- 2^16 again if
    the row were lost, 2^17 if only its scale came back)."""
    monkeypatch.chdir(tmp_path)
    base = ["2", "--model", "cifar10", "--resnet_size", "8", "--use_synthetic_data", "true", "--seed", "4", "--backend",
            "torch", "--dtype", "fp32", "--loss_scale", "dynamic", "--loss_scale_growth_steps", "2",
            "--max_train_steps", "3", "--do_exploit", "false", "--do_explore", "false", "--hooks", "logging",
            "--log_every_n_steps", "1"]
    EngineModel.reset_engines()
    assert main_manager.main(base + ["--rounds", "1"]) == 0
    out = capsys.readouterr().out
    assert "loss_scale = 65536" in out and "skipped_steps = 0" in out
    recs = [json.loads(l) for l in open("savedata/metrics.jsonl")]
    assert recs[-1]["loss_scale"] == {"0": 65536.0, "1": 65536.0} and recs[-1]["skipped_steps"] == {"0": 0, "1": 0}
    EngineModel.reset_engines()
    assert main_manager.main(base + ["--rounds", "2", "--resume"]) == 0
    recs = [json.loads(l) for l in open("savedata/metrics.jsonl")]
    assert recs[-1]["round"] == 1 and recs[-1]["loss_scale"] == {"0": 262144.0, "1": 262144.0}
    assert recs[-1]["best_acc"] == recs[-1]["best_acc"]
    EngineModel.reset_engines()


def test_static_run_reports_no_loss_scale(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    EngineModel.reset_engines()
    assert main_manager.main(["2", "--model", "cifar10", "--resnet_size", "8", "--use_synthetic_data", "true", "--seed",
                              "4", "--backend", "torch", "--max_train_steps", "1", "--rounds", "1"]) == 0
    rec = json.loads(open("savedata/metrics.jsonl").readline())
    assert "loss_scale" not in rec and "skipped_steps" not in rec
    EngineModel.reset_engines()


# ---------------------------------------------------------------------- launch list of the "optim" marker
class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a, **kw):
            self.calls.append((name, kw))
        return f


@pytest.mark.parametrize("loss_scale,half", [(1.0, False), (128.0, True)])
def test_static_and_bf16_steps_launch_what_they_did(monkeypatch, loss_scale, half):
    """The "optim" marker of a static-scale (fp16) or bf16 step: the all-reduce and ONE fused-optimizer launch through
    the static entry point with grad_scale = 1 / loss_scale -- no finiteness pass, no table, no scale update."""
    from distributedtf_amd.engine import hip_step
    rec = _Recorder()
    monkeypatch.setattr(hip_step, "ops", rec)

    class E:
        dynamic_loss_scale = False
        state = grads = hyper = lscale = None
        Pp = P = n_reg = 0
        loss_scale_growth_steps = 2000

        def dp_sync_grads(self, slots):
            rec.calls.append(("dp_sync_grads", {}))

    class BE:
        pass

    be = BE()
    be.loss_scale = loss_scale
    hip_step.run_optimizer(E(), be, [0, 1], None, None)
    assert [c[0] for c in rec.calls] == ["dp_sync_grads", "fused_optimizer"]
    assert rec.calls[1][1] == {"shadow": None, "zero_grads": True, "grad_scale": 1.0 / loss_scale}
    rec.calls.clear()
    e = E()
    e.dynamic_loss_scale = True
    hip_step.run_optimizer(e, be, [0, 1], None, None)
    assert [c[0] for c in rec.calls] == ["dp_sync_grads", "grad_finite_check", "fused_optimizer", "loss_scale_update"]
    assert "lscale" in rec.calls[2][1] and "grad_scale" not in rec.calls[2][1]


def test_hip_backends_without_a_dynamic_path_refuse():
    from distributedtf_amd.engine.hip_step import HipBackend

    class E:
        dynamic_loss_scale = True
        device = torch.device("cpu")

    with pytest.raises(ValueError, match="dynamic loss scaling"):
        HipBackend(E())
