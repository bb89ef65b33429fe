"""Population-batched MNIST CNN training step on hand-written gfx950 kernels.

Reference model: ``mnist_model.py:62-126`` (conv5x5x32 -> pool -> conv5x5x64 -> pool -> dense 1024 ->
dropout 0.4 -> dense 10, sparse softmax CE).  One optimizer step of every resident member is a fixed
launch sequence over population-packed tensors (``ops/csrc/mnist.hip``, ``ops/csrc/gemm.hip``):

  wd_prep      conv2 weights -> flipped/transposed bf16 dgrad layout (tiny)
  conv1        fp32 direct conv + bias + ReLU + max-pool (argmax kept)        -> P1 [N,14,14,32] bf16
  conv2_fwd    MFMA implicit GEMM + bias + ReLU + max-pool in the epilogue   -> P2 [N,3136] bf16
  gemm NT      Z = P2 . W1^T per member (bf16 shadow weights)                -> Z [N,1024] fp32
  head         bias + ReLU + dropout + dense2 + CE, dense2 grads, dZ          -> dZ [N,1024] bf16
  gemm NN      dP2 = dZ . W1                                                   -> dP2 [N,3136] bf16
  gemm TN      dW1 += dZ^T . P2   (fp32, straight into the member's gradient row)
  conv2_dgrad  un-pool/mask + MFMA dgrad                                       -> dP1
  conv2_wgrad  dW2, db2 (ds_read_b64_tr_b16 fragments)
  conv1_wgrad  dW1c, db1c
  optimizer    fused launch over all members; also refreshes the bf16 shadow read by conv2 / dense1

The sequence is captured once per batch composition into a HIP graph and replayed.
Eval runs the forward kernels (conv1, conv2, the dense1 grouped GEMM, the head with dropout off) for every
member at once over chunks of the eval set (``evaluate_population``).
"""

from __future__ import annotations

import ctypes
from typing import List

import numpy as np
import torch

from .. import ops
from ..data.datasets import batch_len
from .hip_step import HipBackend, HipPlan, PinnedStager, _p

c_void_p, c_int, c_long, c_float = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float


class MnistArgs(ctypes.Structure):
    _fields_ = [
        ("x", c_void_p), ("labels", c_void_p), ("img_slot", c_void_p), ("work", c_void_p),
        ("params", c_void_p), ("p_mstride", c_long), ("grads", c_void_p), ("g_mstride", c_long),
        ("shadow", c_void_p), ("s_mstride", c_long), ("wd", c_void_p), ("wd_mstride", c_long),
        ("p1", c_void_p), ("am1", c_void_p), ("p2", c_void_p), ("am2", c_void_p), ("z", c_void_p), ("dz", c_void_p),
        ("dp2", c_void_p), ("dp1", c_void_p), ("loss", c_void_p), ("correct", c_void_p), ("cnt", c_void_p),
        ("rng", c_void_p), ("logits_out", c_void_p),
        ("off_c1w", c_int), ("off_c1b", c_int), ("off_c2w", c_int), ("off_c2b", c_int),
        ("off_d1w", c_int), ("off_d1b", c_int), ("off_d2w", c_int), ("off_d2b", c_int),
        ("drop_rate", c_float), ("train", c_int), ("dz32", c_void_p),
    ]


class GemmGroup(ctypes.Structure):
    _fields_ = [("a_off", c_long), ("b_off", c_long), ("c_off", c_long), ("M", c_int), ("N", c_int), ("K", c_int),
                ("Ms", c_int)]


class GemmArgs(ctypes.Structure):
    _fields_ = [("A", c_void_p), ("B", c_void_p), ("C", c_void_p), ("lda", c_long), ("ldb", c_long), ("ldc", c_long),
                ("groups", c_void_p), ("work", c_void_p)]


GEMM_OUT_F32, GEMM_OUT_BF16, GEMM_OUT_ACC = 0, 1, 2

_REGISTERED = False


def _register():
    global _REGISTERED
    if _REGISTERED:
        return
    P = ctypes.POINTER
    for name in ("dtf_mnist_conv1", "dtf_mnist_conv2_fwd", "dtf_mnist_head", "dtf_mnist_conv2_dgrad",
                 "dtf_mnist_conv2_wgrad", "dtf_mnist_conv1_wgrad"):
        ops.register(name, [P(MnistArgs), c_int, c_void_p])
    ops.register("dtf_mnist_wd_prep", [P(MnistArgs), c_void_p, c_int, c_void_p])
    ops.register("dtf_gemm_bf16", [P(GemmArgs), c_int, c_int, c_void_p])
    for name in ("dtf_mnist_args_size", "dtf_gemm_args_size", "dtf_gemm_group_size"):
        ops.register(name, [])
    L = ops.lib()
    for name, args in ops._SIGNATURES.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.argtypes = args
            fn.restype = c_int
    assert L.dtf_mnist_args_size() == ctypes.sizeof(MnistArgs), "MnistArgs ABI mismatch"
    assert L.dtf_gemm_args_size() == ctypes.sizeof(GemmArgs), "GemmArgs ABI mismatch"
    assert L.dtf_gemm_group_size() == ctypes.sizeof(GemmGroup), "GemmGroup ABI mismatch"
    _REGISTERED = True


def dropout_keep_mask(seed: int, counter: int, n_img: int, rate: float, features: int = 1024) -> np.ndarray:
    """Host replica of the head kernel's dropout hash: bool [n_img, features] (True = kept)."""
    from ..data.datasets import _mix32
    with np.errstate(over="ignore"):
        idx = (np.arange(n_img, dtype=np.uint32)[:, None] * np.uint32(features)
               + np.arange(features, dtype=np.uint32)[None, :])
        inner = _mix32((np.uint32(counter & 0xFFFFFFFF) * np.uint32(0x9E3779B9)).astype(np.uint32) + idx)
        h = _mix32(np.uint32(seed & 0xFFFFFFFF) ^ inner)
    thresh = np.uint32(min(int(rate * 4294967296.0), 0xFFFFFFFF))
    return h >= thresh


class GroupedGemm:
    """One grouped GEMM launch (a list of per-member problems) with its device tables."""

    def __init__(self, A, B, C, lda, ldb, ldc, problems, a_km, b_km, out, device):
        """problems: [(a_off, b_off, c_off, M, N, K[, Ms])] in elements; Ms = rows actually stored (<= M)."""
        problems = [tuple(p) + (0,) * (7 - len(p)) for p in problems]
        for (_, _, _, M, N, K, _) in problems:
            if not a_km:
                assert K % 32 == 0, "row-major A needs K % 32 == 0"
            else:
                assert M % 8 == 0
            if not b_km:
                assert K % 32 == 0, "[N][K] B needs K % 32 == 0"
            else:
                assert N % 8 == 0
        assert lda % 8 == 0 and ldb % 8 == 0
        groups = (GemmGroup * len(problems))()
        work = []
        for gi, (ao, bo, co, M, N, K, Ms) in enumerate(problems):
            groups[gi] = GemmGroup(ao, bo, co, M, N, K, Ms)
            for m0 in range(0, M, 64):
                for n0 in range(0, N, 64):
                    work.append([gi, m0, n0, 0])
        gbytes = torch.frombuffer(bytearray(bytes(groups)), dtype=torch.uint8)
        self.groups_t = gbytes.to(device)
        self.work_t = torch.tensor(work, dtype=torch.int32, device=device)
        self.args = GemmArgs(_p(A), _p(B), _p(C), lda, ldb, ldc, _p(self.groups_t), _p(self.work_t))
        self.mode = int(a_km) | (int(b_km) << 1) | (out << 2)
        self.nwork = len(work)
        self._keep = (A, B, C)

    def launch(self, stream):
        err = ops.lib().dtf_gemm_bf16(ctypes.byref(self.args), self.mode, self.nwork, stream)
        if err != 0:
            raise RuntimeError("gemm_bf16 launch failed: %d" % err)


class HipMnistBackend(HipBackend):
    _plan_cls = None  # _MnistPlan (set below); the fp32 backend: engine/hip_mnist_f32.py
    eval_chunk = 2500

    def __init__(self, engine):
        _register()
        self._init_shared(engine)
        for n in ("conv2_w", "dense1_w"):
            assert self.offs[n] % 8 == 0, "bf16 shadow operands must be 16-byte aligned"
        cap = engine.capacity
        self.shadow = torch.zeros(cap, engine.Pp, dtype=torch.bfloat16, device=self.dev)
        self.wd = torch.zeros(cap, 51200, dtype=torch.bfloat16, device=self.dev)

    def _init_shared(self, engine):
        """What the bf16 and the fp32 backend both hold: parameter offsets, loss / correct rows, dropout rng."""
        HipBackend.__init__(self, engine)
        arch = engine.arch
        self.offs = {n: arch.offsets[n][0] for n in arch.offsets}
        cap = engine.capacity
        self.loss = torch.zeros(cap, dtype=torch.float32, device=self.dev)
        self.correct = torch.zeros(cap, dtype=torch.float32, device=self.dev)
        self.rng = torch.zeros(2, dtype=torch.int32, device=self.dev)
        self.rng_seed = 0x5EED
        self.rng_counter = 0
        self.drop_rate = float(getattr(arch, "dropout", 0.4))
        # training plans also write the head's logits (the "probabilities" hook, reference mnist_model.py:149-151);
        # set before the first step (EngineModel._hooks): the flag is baked into a plan's captured launches
        self.keep_probs = False
        self._last_plan = None

    def _upload_rng(self, v):
        if getattr(self, "_rng_stage", None) is None:
            self._rng_stage = PinnedStager(2, torch.int32)
        self._rng_stage.upload(self.rng, v)

    def next_rng(self):
        self.rng_counter = (self.rng_counter + 1) & 0x7FFFFFFF
        return self.rng_seed, self.rng_counter

    def train_step(self, slots, batches, hparams, lrs):
        self.last_rng = self.next_rng()
        self._upload_rng(self.last_rng)
        loss = super().train_step(slots, batches, hparams, lrs)
        self._last_plan = self.plan(slots, [batch_len(b) for b in batches])  # the plan that just ran (cached)
        return loss

    def train_probabilities(self, slots):
        """Softmax of each member's last training batch (with dropout, as the reference's ``softmax_tensor`` in
        training mode): a list of [batch, 10] device tensors, or None when the plans do not keep logits."""
        p = self._last_plan
        if p is None or p.logits is None or p.eval:
            return None
        out = []
        for s in slots:
            if s not in p.first:
                out.append(None)
                continue
            f, n = p.first[s], p.sizes[p.slots.index(s)]
            out.append(torch.softmax(p.logits[f:f + n], dim=1))
        return out


class _MnistPlan(HipPlan):
    def __init__(self, be: HipMnistBackend, slots: List[int], sizes: List[int], eval_mode: bool = False):
        self._init_members(be, slots, sizes, eval_mode)
        e, dev, N = be.e, be.dev, self.N
        bf = torch.bfloat16
        self.x_in = torch.zeros(N, 28, 28, dtype=torch.float32, device=dev)
        self.labels = torch.zeros(N, dtype=torch.int32, device=dev)
        self.p1 = torch.empty(N, 196, 32, dtype=bf, device=dev)
        self.am1 = torch.empty(N, 196, 32, dtype=torch.uint8, device=dev)
        self.p2 = torch.empty(N, 3136, dtype=bf, device=dev)
        self.am2 = torch.empty(N, 3136, dtype=torch.uint8, device=dev)
        self.z = torch.empty(N, 1024, dtype=torch.float32, device=dev)
        # backward temporaries (eval plans: forward only)
        nb = 1 if self.eval else N
        self.dz = torch.empty(nb, 1024, dtype=bf, device=dev)
        self.dp2 = torch.empty(nb, 3136, dtype=bf, device=dev)
        self.dp1 = torch.empty(nb, 196, 32, dtype=bf, device=dev)
        self.ev_acc = torch.zeros(2, e.capacity, dtype=torch.float32, device=dev)  # eval: [correct, summed CE]
        self.logits = None
        o = be.offs
        a = MnistArgs()
        a.x, a.labels, a.img_slot = _p(self.x_in), _p(self.labels), _p(self.img_slot)
        a.params, a.p_mstride = _p(e.state), e.S
        a.grads, a.g_mstride = _p(e.grads), e.Pp
        a.shadow, a.s_mstride = _p(be.shadow), e.Pp
        a.wd, a.wd_mstride = _p(be.wd), 51200
        a.p1, a.am1, a.p2, a.am2 = _p(self.p1), _p(self.am1), _p(self.p2), _p(self.am2)
        a.z, a.dz, a.dp2, a.dp1 = _p(self.z), _p(self.dz), _p(self.dp2), _p(self.dp1)
        a.loss, a.correct, a.cnt, a.rng = _p(be.loss), _p(be.correct), _p(self.cnt), _p(be.rng)
        a.logits_out = None
        if be.keep_probs and not self.eval:
            self.logits = torch.zeros(N, 10, dtype=torch.float32, device=dev)
            a.logits_out = _p(self.logits)
        a.off_c1w, a.off_c1b, a.off_c2w, a.off_c2b = o["conv1_w"], o["conv1_b"], o["conv2_w"], o["conv2_b"]
        a.off_d1w, a.off_d1b, a.off_d2w, a.off_d2b = o["dense1_w"], o["dense1_b"], o["dense2_w"], o["dense2_b"]
        a.drop_rate = be.drop_rate
        a.train = 0 if self.eval else 1
        if self.eval:  # counts accumulate over the eval chunks in the plan's own buffers
            a.loss, a.correct = _p(self.ev_acc[1]), _p(self.ev_acc[0])
        self.args, self._copies = a, []  # the template: every launch reads its own copy over its own work table
        # work lists (img0, nimg, 0, slot): image chunks of one member.  Deterministic build: ONE chunk per member
        # for every launch that adds into per-member accumulators (dense / conv weight gradients, bias gradients,
        # loss, correct count) -- each address then receives a single add onto zero, and every partial sum is
        # formed in a fixed order inside its workgroup, so the step replays bitwise (the GEMMs own their tiles)
        det = ops.build_deterministic()
        whole = 1 << 30
        w_fwd = self._chunks(max(1, -(-N // 512)))
        Pp = e.Pp
        d1 = o["dense1_w"]
        fwd, dgr, wgr = [], [], []
        for s, n in zip(slots, sizes):
            f = self.first[s]
            fwd.append((f * 3136, s * Pp + d1, f * 1024, n, 1024, 3136))     # Z = P2 W^T
            dgr.append((f * 1024, s * Pp + d1, f * 3136, n, 3136, 1024))     # dP2 = dZ W
            wgr.append((f * 1024, f * 3136, s * Pp + d1, 1024, 3136, n))     # dW += dZ^T P2
        L = ops.lib()
        if not self.eval:
            self._add(L.dtf_mnist_wd_prep, ctypes.byref(self._args()), _p(self.slots_t), len(slots))
            self._add("zero", be.loss)
            self._add("zero", be.correct)
        # forward (eval -- mnist_model.py:167-172 ``mnist_classifier.evaluate`` -- stops after the head, dropout off)
        self._launch(L.dtf_mnist_conv1, n=N)
        self._launch(L.dtf_mnist_conv2_fwd, w_fwd)
        self._gemm(GroupedGemm(self.p2, be.shadow, self.z, 3136, 3136, 1024, fwd, False, False, GEMM_OUT_F32, dev))
        self._launch(L.dtf_mnist_head, self._chunks(whole if det else 16))
        if self.eval:
            return
        self._gemm(GroupedGemm(self.dz, be.shadow, self.dp2, 1024, 3136, 3136, dgr, False, True, GEMM_OUT_BF16, dev))
        self._gemm(GroupedGemm(self.dz, self.p2, e.grads, 1024, 3136, 3136, wgr, True, True, GEMM_OUT_ACC, dev))
        self._launch(L.dtf_mnist_conv2_dgrad, self._chunks(max(1, -(-N // 512))))
        self._launch(L.dtf_mnist_conv2_wgrad, self._chunks(whole if det else max(4, -(-N * 5 // 320))))
        self._launch(L.dtf_mnist_conv1_wgrad, self._chunks(whole if det else max(4, -(-N // 256))))
        self._add("optim", None)
        self._add("step", None)

    def _args(self, work=None):
        a = MnistArgs.from_buffer_copy(self.args)
        a.work = _p(work)
        self._copies.append(self._hold(a))
        self._hold(work)
        return a

    def _launch(self, fn, work=None, n=None):
        self._add(fn, ctypes.byref(self._args(work)), n if work is None else work.shape[0])

    def _gemm(self, g):
        self._hold(g)
        self._add(ops.lib().dtf_gemm_bf16, ctypes.byref(g.args), g.mode, g.nwork)

    def want_logits(self):
        if self.logits is None:
            self.logits = torch.zeros(self.N, 10, dtype=torch.float32, device=self.be.dev)
            for a in self._copies:  # (the head reads it; the launches keep seeing one set of arguments)
                a.logits_out = _p(self.logits)
        return self.logits


HipMnistBackend._plan_cls = _MnistPlan
