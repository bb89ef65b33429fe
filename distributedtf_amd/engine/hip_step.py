"""What every HIP step backend shares: the driver around a family's kernels.

A backend (``HipBackend``) owns the per-family device buffers, two bounded plan caches and the engine hooks every
family answers alike (shadow refresh, ``infer`` through ``want_logits``); a plan (``HipPlan``) holds the member layout,
the buffers and the launch list of one batch composition, stages its inputs (``load_batch``, ``load_eval``) and runs
the list (``_run_eager``), captured into a HIP graph on its first step (``run_captured``) and replayed afterwards.
The per-step host work -- optimizer hyper table (``upload_hyper``), small pinned uploads (``PinnedStager``), step
counters and loss gather inside the graph (``advance_steps``, ``LossRing``) -- lives here too, as does the release of
captured graphs before RCCL teardown (``release_graphs``).  The kernels, launch lists and family markers of each
family stay in its own ``hip_*`` module; this module imports none of them.
"""

from __future__ import annotations

import os
import weakref

import torch

from .. import ops
from ..data.datasets import IndexBatch, batch_len


def _p(t):
    return None if t is None else t.data_ptr()


def _log2(n):
    assert n > 0 and n & (n - 1) == 0, n
    return n.bit_length() - 1


def upload_hyper(e, slots, hparams, lrs):
    """Per-member optimizer hyper rows -> device table, skipped when only the step counter moved (the lr
    schedule is piecewise constant).  The captured step advances the table's step column on the device
    (``advance_steps``) and ``e._hyper_dev`` mirrors what the device holds, so a skip is exact -- also after
    an exploit import changes a member's step."""
    from .optim import H_STEP, hyper_row
    rows = [(s, hyper_row(hp, lr, e.host_step[s] + 1, True)) for s, hp, lr in zip(slots, hparams, lrs)]
    dev = getattr(e, "_hyper_dev", None)
    if dev is not None and dev.get("slots") == tuple(slots) and all(dev.get(s) == r for s, r in rows):
        return
    hy = torch.zeros(e.capacity, 8, dtype=torch.float32)
    for s, r in rows:
        hy[s] = torch.tensor(r)
    e.hyper.copy_(hy.pin_memory() if e.device.type == "cuda" else hy, non_blocking=True)
    e._hyper_dev = {s: list(r) for s, r in rows}
    e._hyper_dev["slots"] = tuple(slots)


class PinnedStager:
    """Small per-step host->device uploads through one pinned staging buffer.

    A pageable ``non_blocking`` copy is staged synchronously and waits for the stream to drain, so the host
    cannot queue step k+1 while step k runs.  Here the host waits only for the previous upload from this stager
    (issued at the start of the previous step) before overwriting the staging buffer."""

    def __init__(self, n, dtype):
        self.host = torch.empty(n, dtype=dtype).pin_memory() if torch.cuda.is_available() else None
        self.evt = None

    def upload(self, dst, values):
        if dst.device.type != "cuda" or self.host is None:
            dst.copy_(torch.tensor(list(values), dtype=dst.dtype))
            return
        if self.evt is None:
            self.evt = torch.cuda.Event()
        else:
            self.evt.synchronize()
        for i, v in enumerate(values):
            self.host[i] = v
        dst.copy_(self.host[:len(values)], non_blocking=True)
        self.evt.record()

    def upload_array(self, dst, src):
        """``upload`` of a host tensor of ``dst``'s dtype and size, copied into the staging buffer in one piece."""
        if dst.device.type != "cuda" or self.host is None:
            dst.copy_(src)
            return
        if self.evt is None:
            self.evt = torch.cuda.Event()
        else:
            self.evt.synchronize()
        self.host[:src.numel()].copy_(src)
        dst.copy_(self.host[:src.numel()], non_blocking=True)
        self.evt.record()


def note_step_advanced(e, slots):
    """Host mirror of ``advance_steps`` (call once per executed step)."""
    from .optim import H_STEP
    dev = getattr(e, "_hyper_dev", None)
    if dev is not None:
        for s in slots:
            if s in dev:
                dev[s][H_STEP] += 1.0


def advance_steps(e, slots_long, slots_i32=None, loss=None, loss_sel=None, ring=None):
    """Inside the captured step: per-member step counters (state column + hyper table) += 1 and, given
    ``loss``/``loss_sel``, the per-member losses gathered in slot-list order (one kernel when the int32 slot list is
    given).  ``ring`` = (rows [R, n] fp32, index int32 [1]): the losses go to the ring's next row instead of
    ``loss_sel`` (LossRing)."""
    from .optim import H_STEP
    if slots_i32 is not None and e.device.type == "cuda":
        rb, ri = (ring.rows, ring.idx) if ring is not None else (None, None)
        ops.check(ops.lib().dtf_step_end(_p(e.state), e.S, 3 * e.Pp + e.R, _p(e.hyper), H_STEP, _p(slots_i32),
                                         slots_i32.numel(), _p(loss), _p(loss_sel) if ring is None else None,
                                         _p(rb), _p(ri), rb.shape[0] if rb is not None else 0, ops.stream()),
                  "step_end")
        return
    one = torch.ones(slots_long.numel(), device=e.device)
    e.step_col().index_add_(0, slots_long, one)
    e.hyper[:, H_STEP].index_add_(0, slots_long, one)
    if loss_sel is not None:
        torch.index_select(loss, 0, slots_long, out=loss_sel)


def run_optimizer(e, be, slots, slots_i32, shadow):
    """The "optim" marker of a step's launch list (inside the captured graph): the gradient all-reduce of
    data-parallel member groups, then the fused optimizer, which unscales by the backend's static ``loss_scale``.

    With dynamic loss scaling (``e.dynamic_loss_scale``) the sequence is: all-reduce; the finiteness pass over the
    listed members' gradient rows (after the all-reduce, so every replica of a member decides alike); the fused
    optimizer reading the table (a flagged member keeps weights, slots and shadow, its gradients are zeroed); the
    scale rule.  No host synchronisation: the table lives on the device and the host reads it only on logging steps
    and at round end.  A skipped step still consumes its batch, still advances the step counters (the "step" marker
    that follows: the host mirrors ``host_step`` / ``_hyper_dev`` and PBT's lockstep rounds stay valid) and still
    updates the BN moving statistics (forward-only, independent of the scale)."""
    e.dp_sync_grads(slots)  # data-parallel member groups only (no-op otherwise)
    if not e.dynamic_loss_scale:
        ops.fused_optimizer(e.state, e.grads, e.hyper, e.Pp, e.P, e.n_reg, shadow=shadow, zero_grads=True,
                            grad_scale=1.0 / be.loss_scale)
        return
    ops.grad_finite_check(e.grads, e.Pp, e.P, slots_i32, e.lscale)
    ops.fused_optimizer(e.state, e.grads, e.hyper, e.Pp, e.P, e.n_reg, shadow=shadow, zero_grads=True, lscale=e.lscale)
    ops.loss_scale_update(e.lscale, e.hyper, slots_i32, e.loss_scale_growth_steps)


class LossRing:
    """Per-step member losses without a per-step copy: the captured step's step_end kernel writes each replay's
    losses into the next row of a [rows, n] device ring (the row index lives on the device), and the host hands out
    a VIEW of that row.  A view stays valid for ``rows`` later steps; engine_model._train_cycle clones a member's
    last loss when the member leaves the active set (before its view can be overwritten)."""

    ROWS = 4096

    def __init__(self, n, device):
        self.rows = torch.zeros(self.ROWS, n, dtype=torch.float32, device=device)
        self.idx = torch.zeros(1, dtype=torch.int32, device=device)
        self.k = 0  # host mirror of idx: steps executed

    def advance(self):
        self.k += 1

    def last(self):
        assert self.k > 0
        return self.rows[(self.k - 1) % self.ROWS]


_LIVE_GRAPH_PLANS = weakref.WeakSet()  # plans holding a captured step graph (released before RCCL teardown)


def release_graphs() -> int:
    """Drop every captured step graph (they are re-captured on the next step).  A graph that recorded an RCCL
    collective keeps that communicator busy: ``destroy_process_group`` then blocks forever (measured with the
    data-parallel step on the GPU box), so ``parallel.comm.shutdown_distributed`` calls this first."""
    n = 0
    for plan in list(_LIVE_GRAPH_PLANS):
        if plan.graph is not None:
            plan.graph = None
            n += 1
    _LIVE_GRAPH_PLANS.clear()
    return n


def run_captured(plan) -> None:
    """Run one step of ``plan``: the first call executes it eagerly (allocator / lazy init warm-up) and then
    captures the launch list into a HIP graph; later calls replay the graph.  A data-parallel step captures its
    RCCL gradient all-reduce with the rest of the step; if this RCCL build refuses a collective inside a capture,
    the plan falls back to eager launches (the warm-up already ran this step)."""
    be = plan.be
    if be.use_graph and plan.graph is None and not getattr(plan, "_no_graph", False):
        plan._run_eager()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        ok = False
        try:
            with torch.cuda.stream(s):
                g.capture_begin(capture_error_mode="thread_local")
                try:
                    plan._run_eager()
                finally:
                    g.capture_end()
            ok = True
        except RuntimeError as err:
            if plan.e.dp is None:
                raise
            import sys
            import warnings
            msg = "step graph capture with the data-parallel all-reduce failed (%s): eager launches" % err
            warnings.warn(msg)
            print("DTF WARNING: " + msg, file=sys.stderr, flush=True)
            torch.cuda.synchronize()
            plan._no_graph = True
            be.graph_fallbacks = getattr(be, "graph_fallbacks", 0) + 1
        torch.cuda.current_stream().wait_stream(s)
        if ok:
            plan.graph = g
            be.graphs_captured = getattr(be, "graphs_captured", 0) + 1
            _LIVE_GRAPH_PLANS.add(plan)
        return
    if plan.graph is not None:
        plan.graph.replay()
    else:
        plan._run_eager()


def graph_state(be):
    """How a HIP backend's steps run: "captured" (HIP-graph replay), "eager_fallback" (a data-parallel capture was
    refused and at least one plan runs its launches eagerly -- slow, recorded in the bench JSON and metrics.jsonl),
    "disabled" (DTF_HIP_GRAPH=0 / debug), "none" (nothing captured yet), or None (not a HIP backend)."""
    if not hasattr(be, "use_graph"):
        return None
    if not be.use_graph:
        return "disabled"
    if getattr(be, "graph_fallbacks", 0):
        return "eager_fallback"
    return "captured" if getattr(be, "graphs_captured", 0) else "none"


def same_batches(plan, batches) -> bool:
    """True if ``batches`` are the very (x, y) storages staged last step and unmodified since (tensor version
    counters); a reference to them is held so their memory cannot be recycled into a different batch."""
    key = tuple((x.data_ptr(), x.shape, x.stride(), x._version, y.data_ptr(), y.shape, y._version)
                for x, y in batches)
    if getattr(plan, "_batch_key", None) == key:
        return True
    plan._batch_key = key
    plan._batch_ref = list(batches)
    return False


class HipBackend:
    """Driver of a population-batched HIP step backend: plan caches, the plain train step and chunked evaluation.
    A family sets ``_plan_cls`` (constructed as ``_plan_cls(be, slots, sizes, eval_mode=False)``) and allocates its
    buffers -- ``loss`` and ``correct`` [capacity] among them."""

    name = "hip"
    accepts_index_batches = False
    _plan_cls = None
    max_plans = 16  # training plans: the whole cache is cleared past this many
    max_eval_plans = 4  # eval plans: the oldest is evicted at this many
    eval_chunk_env, eval_chunk = "DTF_EVAL_CHUNK", 2000  # images per eval forward: env switch, default
    shadow = None  # low-precision copy of the master rows that the fused optimizer also writes (bf16 families)
    loss_scale = 1.0  # static loss scaling of the fp16 builds
    dynamic_loss_scale_ok = False  # the family's head reads the engine's dynamic loss-scale table (CIFAR ResNet)

    def __init__(self, engine):
        if getattr(engine, "dynamic_loss_scale", False) and not self.dynamic_loss_scale_ok:
            raise ValueError("dynamic loss scaling: %s has no dynamic path (the fp16 CIFAR ResNet HIP step and the "
                             "torch backend have)" % type(self).__name__)
        self.e = engine
        self.dev = engine.device
        self._plans = {}
        self._eval_plans = {}
        self.use_graph = (os.environ.get("DTF_HIP_GRAPH", "1") == "1" and os.environ.get("DTF_DEBUG", "0") != "1")

    # ---- engine hooks
    def shadow_weights(self):
        return self.shadow

    def on_params_changed(self, slots):
        """Rows changed outside the optimizer (init, exploit import): refresh their low-precision shadow.  Families
        without one read the fp32 master rows, or prepare their weights inside every step."""
        slots = list(slots)
        if self.shadow is not None and slots:
            e = self.e
            self._rows = ops.shadow_refresh(e.state, self.shadow, slots, e.Pp, e.P)

    @torch.no_grad()
    def infer(self, slot, x):
        """Eval-mode logits of one member on the HIP forward kernels, for plans whose head writes them on request
        (``want_logits``); the other families build theirs."""
        p = self.eval_plan([slot], int(x.shape[0]))
        logits = p.want_logits()
        p.load_eval(x, torch.zeros(x.shape[0], dtype=torch.int32, device=x.device))
        p.run_eval()
        return logits.clone()

    # ---- plans
    def plan(self, slots, sizes):
        key = (tuple(slots), tuple(sizes))
        p = self._plans.get(key)
        if p is None:
            if len(self._plans) > self.max_plans:
                self._plans.clear()
            p = self._plan_cls(self, list(slots), list(sizes))
            self._plans[key] = p
        return p

    def eval_plan(self, slots, m):
        """Eval plans live in their own bounded cache: an eval pass never evicts the captured training graph."""
        key = (tuple(slots), int(m))
        plans = self._eval_plans
        p = plans.get(key)
        if p is None:
            if len(plans) >= self.max_eval_plans:
                plans.pop(next(iter(plans)))  # oldest first
            p = self._plan_cls(self, list(slots), [int(m)] * len(slots), eval_mode=True)
            plans[key] = p
        return p

    def train_step(self, slots, batches, hparams, lrs):
        e = self.e
        batches = [b.materialize() if isinstance(b, IndexBatch) else b for b in batches]
        sizes = [batch_len(b) for b in batches]
        p = self.plan(slots, sizes)
        upload_hyper(e, slots, hparams, lrs)
        p.load_batch(batches)
        p.run()
        note_step_advanced(e, slots)
        return p.loss_sel.clone()  # gathered inside the step graph

    def forward_backward(self, slots, batches):
        raise RuntimeError("%s runs whole steps: use train_step" % type(self).__name__)

    def train_correct(self, slots):
        """Correct predictions of each member's last training batch (head kernel count; device tensor)."""
        return self.correct[torch.as_tensor(list(slots), dtype=torch.long, device=self.dev)]

    @torch.no_grad()
    def evaluate_population(self, slots, x, y, chunk=None):
        """Eval accuracy of every member in ``slots`` on (x, y) in one population-batched forward per chunk of
        ``chunk`` images (all members see the same chunk); one host sync at the end."""
        n = int(x.shape[0])
        if n == 0 or not slots:
            return {s: 0.0 for s in slots}
        chunk = min(n, int(chunk or os.environ.get(self.eval_chunk_env, self.eval_chunk)))
        used = []
        for i in range(0, n, chunk):
            m = min(chunk, n - i)
            p = self.eval_plan(slots, m)
            if all(p is not q for q in used):
                p.ev_acc.zero_()
                used.append(p)
            p.load_eval(x[i:i + m], y[i:i + m])
            p.run_eval()
        correct = used[0].ev_acc[0].clone()
        for p in used[1:]:
            correct += p.ev_acc[0]
        vals = correct.cpu().tolist()
        return {s: vals[s] / float(n) for s in slots}


class HipPlan:
    """What every step plan shares: the member layout of one batch composition, input staging, and the step as a
    ``launches`` list.  An entry is (launcher, args), run as ``launcher(*args, stream)``, or one of the markers "zero"
    (args[0].zero_()), "optim" (gradient all-reduce of data-parallel groups + the fused optimizer; it also writes the
    backend's ``shadow`` and unscales by its ``loss_scale``) and "step" (step counters += 1, the backend's ``loss``
    gathered into ``loss_sel``, or into the plan's ``ring``).  Any other string is a family's own marker, run as the
    plan's ``_marker_<name>(*args)``.  A family's plan holds ``x_in`` [N, ...] fp32 and ``labels`` [N] int32."""

    ring = None  # a LossRing where the plan hands out views of the per-step losses (_StepPlan)

    def _init_members(self, be, slots, sizes, eval_mode=False, counts=None):
        """The layout of ``sizes[i]`` images of member ``slots[i]``, packed in slot-list order: ``first`` (slot ->
        first image), ``img_slot`` (image -> slot), ``cnt`` (slot -> images; ``counts`` where a member holds fewer
        than its region, 0 for slots outside the plan), the slot lists, and an empty launch list."""
        e, dev = be.e, be.dev
        self.be, self.e, self.eval = be, e, bool(eval_mode)
        self.slots, self.sizes, self.N = slots, sizes, sum(sizes)
        img_slot, self.first = [], {}
        for s, n in zip(slots, sizes):
            self.first[s] = len(img_slot)
            img_slot += [s] * n
        self.img_slot = torch.tensor(img_slot, dtype=torch.int32, device=dev)
        cnt = torch.zeros(e.capacity, dtype=torch.float32)
        for s, n in zip(slots, sizes if counts is None else counts):
            cnt[s] = float(n)
        self.cnt = cnt.to(dev)
        self.slots_t = torch.tensor(slots, dtype=torch.int32, device=dev)
        self.slots_long = torch.tensor(slots, dtype=torch.long, device=dev)
        self.loss_sel = torch.zeros(len(slots), dtype=be.loss.dtype, device=dev)
        self.launches, self._keep, self.graph = [], [], None

    def _add(self, fn, *args):
        self.launches.append((fn, args))

    def _hold(self, obj):
        """Keep ``obj`` (an argument struct, a work table) alive as long as the plan; returns it."""
        self._keep.append(obj)
        return obj

    def _chunk_rows(self, s, n, chunk):
        """Work rows (img0, nimg, 0, slot) over ``n`` images of member ``s`` in runs of ``chunk``."""
        f = self.first[s]
        return [[f + i, min(chunk, n - i), 0, s] for i in range(0, n, chunk)]

    def _chunks(self, chunk):
        """The int32 work table of every member's ``_chunk_rows``; ``chunk``: images per row, or a function of the
        member's image count."""
        rows = []
        for s, n in zip(self.slots, self.sizes):
            rows += self._chunk_rows(s, n, chunk(n) if callable(chunk) else chunk)
        return torch.tensor(rows, dtype=torch.int32, device=self.be.dev)

    # ---- input staging
    def load_batch(self, batches, slots=None):
        """Stage the members' (x, y) batches into their regions (``slots``: the members they belong to, default
        every plan member), unless they are the unmodified storages staged last step."""
        if same_batches(self, batches):
            return
        for s, (x, y) in zip(self.slots if slots is None else slots, batches):
            n, off = x.shape[0], self.first[s]
            self.x_in[off:off + n].copy_(x.reshape(n, *self.x_in.shape[1:]), non_blocking=True)
            self.labels[off:off + n].copy_(y, non_blocking=True)

    def load_eval(self, x, y):
        """The same eval chunk for every member: [m, ...] fp32 -> this plan's [members * m] input."""
        m, k = x.shape[0], len(self.slots)
        assert all(n == m for n in self.sizes), "eval plans hold the same chunk for every member"
        shp = tuple(self.x_in.shape[1:])
        self.x_in.view(k, m, *shp).copy_(x.reshape(1, m, *shp).expand(k, *([-1] * (len(shp) + 1))))
        self.labels.view(k, m).copy_(y.reshape(1, m).expand(k, -1))

    # ---- execution
    def _run_eager(self):
        e, be = self.e, self.be
        st = ops.stream()
        for fn, args in self.launches:
            if fn == "zero":
                args[0].zero_()
            elif fn == "optim":
                run_optimizer(e, be, self.slots, self.slots_t, be.shadow)
            elif fn == "step":
                # step counters + per-member losses gathered inside the step (graph): a replay leaves one copy
                advance_steps(e, self.slots_long, self.slots_t, be.loss, self.loss_sel, ring=self.ring)
            elif isinstance(fn, str):
                getattr(self, "_marker_" + fn)(*args)
            else:
                err = fn(*args, st)
                if err != 0:
                    raise RuntimeError("kernel launch %s failed with %d" % (ops.launcher_name(fn), err))

    def run_eval(self):
        assert self.eval
        self._run_eager()

    def run(self):
        run_captured(self)
