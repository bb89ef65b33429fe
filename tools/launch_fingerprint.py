"""Canonical fingerprint of the HIP step plans' launch lists, for host-side refactors of engine/hip_*.py.

    python tools/launch_fingerprint.py --out FILE [--device cpu|cuda] [--digest]

Builds a fixed set of train and eval plans of every HIP family (no kernel is launched: a plan is buffers plus a
launch list) and writes one line per launch: the launcher symbol or marker, every scalar argument, each non-pointer
field of every ctypes.Structure argument (zero fields are left out), and each pointer -- argument or field -- as the
index of that address's first appearance in the plan.  A pointer to an int32 work table or a byte job table reachable
from the plan carries, where it first appears, a hash of the table's contents (pointer words inside a job table are
canonicalised the same way).  Two trees that build the same plans give byte-identical files: run it on both and
diff.  ``--digest`` writes one line per plan instead -- its launch count and the SHA-1 of its lines -- which is what
profiles/ keeps; without it a differing plan can be read launch by launch.  The library is the one the environment
selects (DTF_DETERMINISTIC=1 / DTF_HALF=1).

A plan with no launch list (the bf16 MNIST plan before it moved onto HipPlan) is recorded instead: ``ops.lib()`` is
replaced by a stand-in that writes the same line for every launcher call of ``_run_eager`` and launches nothing.
The "rec" sections use it on every tree, so they compare.
"""
import argparse
import ctypes
import hashlib
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from distributedtf_amd import ops  # noqa: E402
from distributedtf_amd.engine.population import PopulationEngine  # noqa: E402
from distributedtf_amd.models.resnet import ResNetArch, cifar_config, imagenet_config  # noqa: E402


def _tensors(root):
    """Every tensor reachable from ``root`` through attributes, lists, tuples and dicts."""
    seen, out, todo = set(), [], [root]
    while todo:
        o = todo.pop()
        if id(o) in seen or isinstance(o, (str, bytes, int, float, type(None), ctypes.Structure, types.ModuleType)):
            continue
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            out.append(o)
        elif isinstance(o, dict):
            todo += list(o.values())
        elif isinstance(o, (list, tuple, set)):
            todo += list(o)
        elif hasattr(o, "__dict__") and not callable(o):
            todo += list(vars(o).values())
    return out


class Canon:
    """Pointer -> first-appearance index of one plan, with content hashes of its host-built tables."""

    def __init__(self, plan):
        self.idx, self.hashes = {}, {}
        self.tables, self.spans = {}, []
        for t in _tensors(plan):  # (the plan reaches its backend and engine)
            if not t.numel():
                continue
            if t.dtype == torch.int32 or (t.dtype == torch.uint8 and t.dim() == 1):
                self.tables.setdefault(t.data_ptr(), t)
            self.spans.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()))

    def ptr(self, v):
        v = getattr(v, "value", v)
        if not v:
            return "-"
        if v in self.idx:
            return "p%d" % self.idx[v]
        self.idx[v] = len(self.idx)
        return "p%d%s" % (self.idx[v], self._hash(v))  # (a table's hash where its pointer first appears)

    def _hash(self, addr):
        if addr not in self.tables:
            return ""
        if addr not in self.hashes:
            self.hashes[addr] = ""  # (a table that points at itself)
            t = self.tables[addr].detach().cpu().contiguous()
            if t.dtype == torch.int32:
                body = t.numpy().tobytes()
            else:  # job table: structs of 8-byte words, some of them pointers
                n = t.numel() // 8 * 8
                words = t[:n].view(torch.int64).tolist()
                body = " ".join(self.ptr(w) if any(a <= w < b for a, b in self.spans) else str(w)
                                for w in words).encode() + bytes(t[n:].tolist())
            self.hashes[addr] = "#" + hashlib.sha1(repr(tuple(t.shape)).encode() + body).hexdigest()[:12]
        return self.hashes[addr]

    @staticmethod
    def scalar(v):
        v = getattr(v, "value", v)
        return "-" if v is None else (repr(float(v)) if isinstance(v, float) else str(int(v)))

    def struct(self, s):
        parts = []
        for name, ty in s._fields_:
            v = getattr(s, name)
            if v:  # (a field left out is 0 / null)
                parts.append("%s=%s" % (name, self.ptr(v) if ty is ctypes.c_void_p else self.scalar(v)))
        return "%s{%s}" % (type(s).__name__, ",".join(parts))

    def launch(self, name, args, argtypes):
        out = [name]
        for i, a in enumerate(args):
            ty = argtypes[i] if argtypes is not None and i < len(argtypes) else None
            if hasattr(a, "_obj"):
                out.append(self.struct(a._obj))
            elif isinstance(a, torch.Tensor):
                out.append(self.ptr(a.data_ptr()))
            elif ty is ctypes.c_void_p or (ty is None and isinstance(a, int) and a >= 1 << 32):
                out.append(self.ptr(a))
            else:
                out.append(self.scalar(a))
        return " ".join(out)


def list_lines(plan):
    c = Canon(plan)
    lines = []
    for fn, args in plan.launches:
        if isinstance(fn, str):
            lines.append(c.launch(fn, [a for a in args if a is not None], None))
        else:
            lines.append(c.launch(ops.launcher_name(fn), args, fn.argtypes))
    return lines


class _RecFn:
    def __init__(self, name, real, sink):
        self.__name__, self.real, self.sink = name, real, sink

    @property
    def argtypes(self):
        return self.real.argtypes

    def __call__(self, *args):
        # the stream is not part of a launch; a struct is copied as it stands now (a plan may reuse and mutate one)
        snap = [types.SimpleNamespace(_obj=type(a._obj).from_buffer_copy(a._obj)) if hasattr(a, "_obj") else a
                for a in args[:-1]]
        self.sink.append((self.__name__, self.real.argtypes, snap))
        return 0


class _RecLib:
    """Stand-in for the kernel library: launchers (last parameter: the stream) are recorded, queries pass through."""

    def __init__(self, real, sink):
        self._real, self._sink = real, sink

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        at = getattr(fn, "argtypes", None)
        if at and at[-1] is ctypes.c_void_p:
            return _RecFn(name, fn, self._sink)
        return fn


def recorded_lines(make_plan, dev, run="_run_eager"):
    """Build a plan and run its ``_run_eager`` (or ``run_eval``) once against the recording library."""
    real_lib, real_stream, real_opt = ops.lib, ops.stream, ops.fused_optimizer
    sink, lines = [], []
    rec = _RecLib(real_lib(), sink)
    ops.lib = lambda: rec
    if dev.type != "cuda":  # no stream, and the optimizer wrapper insists on device tensors: record it one level up
        ops.stream = lambda: None
        ops.fused_optimizer = lambda state, grads, hyper, Pp, P, n_reg, shadow=None, zero_grads=True, grad_scale=1.0, \
            lscale=None: sink.append(("fused_optimizer", None, (state, grads, hyper, Pp, P, n_reg, shadow,
                                                                int(zero_grads), float(grad_scale), lscale)))
    try:
        plan = make_plan()
        del sink[:]
        getattr(plan, run)()
        c = Canon(plan)
        for name, argtypes, args in sink:
            lines.append(c.launch(name, [a for a in args], argtypes))
    finally:
        ops.lib, ops.stream, ops.fused_optimizer = real_lib, real_stream, real_opt
    return lines


def engine(arch, cap, dev, dtype, **kw):
    torch.manual_seed(0)
    return PopulationEngine(arch, cap, dev, backend="torch", compute_dtype=dtype, **kw)


def sections(dev):
    """(title, lines) per plan of the fixed set for this device and this process's kernel library."""
    from distributedtf_amd.engine import hip_f32, hip_imagenet, hip_imagenet_f32, hip_mnist, hip_mnist_f32, hip_resnet
    from distributedtf_amd.models.mnist import MnistArch
    half, gpu = ops.half_mode(), dev.type == "cuda"
    d16 = torch.float16 if half else torch.bfloat16
    kw16 = dict(loss_scale=128.0) if half else {}

    def plans(title, be, comps, evals, **pkw):
        for slots, sizes in comps:
            yield "%s train slots=%s sizes=%s" % (title, slots, sizes), list_lines(
                be._plan_cls(be, list(slots), list(sizes), **pkw))
        for slots, m in evals:
            yield "%s eval slots=%s m=%d" % (title, slots, m), list_lines(
                be._plan_cls(be, list(slots), [m] * len(slots), eval_mode=True))

    # ---- CIFAR ResNet: bf16 / fp16 and fp32
    small = [([0, 2], [3, 2]), ([0, 1, 2], [4, 4, 4])]
    small_ev = [([0, 2], 4), ([0, 1, 2], 4)]
    for version in (2, 1):
        for size in (8, 20):
            arch = ResNetArch(cifar_config(size, version=version))
            be = hip_resnet.HipResNetBackend(engine(arch, 3, dev, d16, **kw16))
            yield from plans("cifar%d v%d" % (size, version), be, small, small_ev)
            if not half:
                be = hip_f32.HipResNetF32Backend(engine(arch, 3, dev, torch.float32))
                yield from plans("cifar%d v%d fp32" % (size, version), be, small, small_ev)
    if gpu:
        arch = ResNetArch(cifar_config(20, version=2))
        be = hip_resnet.HipResNetBackend(engine(arch, 8, dev, d16, **kw16))
        for n in (1, 2, 4, 8):
            yield from plans("cifar20 v2 pop%d" % n, be, [(list(range(n)), [8] * n)],
                             [(list(range(n)), 8)] if n in (1, 8) else [])
        yield from plans("cifar20 v2 ragged", be, [([0, 1, 2], [8, 12, 6])], [])
        yield from plans("cifar20 v2 elastic", be, [([0, 1, 2], [8, 12, 6])], [], elastic_cap=16)
        yield from plans("cifar20 v2 index batches", be, [([0, 1, 2], [8, 8, 8])], [], src=object())
        be = hip_resnet.HipResNetBackend(engine(ResNetArch(cifar_config(20, version=1)), 3, dev, d16, **kw16))
        yield from plans("cifar20 v1 pop3", be, [([0, 1, 2], [8, 8, 8])], [([0, 1, 2], 8)])
        if half:
            be = hip_resnet.HipResNetBackend(engine(arch, 3, dev, d16, loss_scale="dynamic"))
            yield from plans("cifar20 v2 dynamic loss scale", be, [([0, 1, 2], [8, 8, 8])], [])
    # ---- MNIST: fp32 from its list, bf16 recorded
    if not half:
        comps = [([0, 2], [3, 2])] + ([([0, 1, 2, 3], [8, 8, 8, 8])] if gpu else [])
        be = hip_mnist_f32.HipMnistF32Backend(engine(MnistArch(), 4, dev, torch.float32))
        yield from plans("mnist fp32", be, comps, [([0, 2], 4)])
        be = hip_mnist.HipMnistBackend(engine(MnistArch(), 4, dev, torch.bfloat16))
        for slots, sizes in comps:
            yield "mnist bf16 rec train slots=%s sizes=%s" % (slots, sizes), recorded_lines(
                lambda: be._plan_cls(be, list(slots), list(sizes)), dev)
        for probs in (False, True):
            be.keep_probs = probs
            yield "mnist bf16 rec train keep_probs=%d" % probs, recorded_lines(
                lambda: be._plan_cls(be, [0, 2], [3, 2]), dev)
        be.keep_probs = False

        def eval_plan(logits):
            p = be._plan_cls(be, [0, 2], [4, 4], eval_mode=True)
            if logits:
                p.want_logits()
            return p
        for logits in (False, True):
            yield "mnist bf16 rec eval logits=%d" % logits, recorded_lines(lambda: eval_plan(logits), dev, "run_eval")
    # ---- ImageNet-shape ResNet-50
    for version in (2, 1):
        if half and version == 1:
            continue  # fp16: the v2 families
        arch = ResNetArch(imagenet_config(50, version, num_classes=1001, image_size=64))
        be = hip_imagenet.HipImageNetBackend(engine(arch, 2, dev, d16, **kw16))
        yield from plans("imagenet50 v%d" % version, be, [([0, 1], [2, 1])], [([0, 1], 2)])
        if not half:
            be = hip_imagenet_f32.HipImageNetF32Backend(engine(arch, 2, dev, torch.float32))
            yield from plans("imagenet50 v%d fp32" % version, be, [([0, 1], [2, 1])], [([0, 1], 2)])


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--digest", action="store_true", help="one line per plan: launch count and SHA-1 of its lines")
    a = ap.parse_args()
    dev = torch.device(a.device)
    lib = ops.lib()
    n = 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# device %s deterministic %d half %d\n" % (dev.type, ops.build_deterministic(), ops.build_half()))
        for title, lines in sections(dev):
            body = "".join(ln + "\n" for ln in lines)
            head = "== %s (%d launches)" % (title, len(lines))
            f.write("%s %s\n" % (head, hashlib.sha1(body.encode()).hexdigest()) if a.digest else head + "\n" + body)
            n += len(lines)
    print("launch_fingerprint: %d launches -> %s (%s)" % (n, a.out, getattr(getattr(lib, "_lib", lib), "_name", "")))


if __name__ == "__main__":
    main()
