"""Datasets: CIFAR-10 binary records, MNIST IDX, synthetic device batches, augmentation.

* CIFAR-10 (reference ``cifar10_main.py:34-135``): 3073-byte records (label +
  CHW uint8), ``data_batch_{1..5}.bin`` / ``test_batch.bin``; training
  preprocessing = pad to 40x40, random 32x32 crop, random horizontal flip, then
  ``per_image_standardization`` (mean / max(std, 1/sqrt(N))) for every image.
  The whole dataset is kept on the GPU as uint8 NHWC and batches are gathered
  and augmented on-device (no CPU input pipeline).
* MNIST (``mnist_model.py:131-138``): gz IDX files; pixels NOT normalised
  (0..255 floats, Appendix A5) unless ``normalize=True``.
* Synthetic (``model_helpers.py:59-86`` / ``resnet_run_loop.py:108-129``): the
  reference feeds constant zeros; here a fixed device-resident batch of
  standard-normal images and uniform labels (zeros would let DVFS inflate
  throughput numbers, and labels 0 make the loss trivial).
"""

from __future__ import annotations

import gzip
import os
from typing import Optional, Tuple

import numpy as np
import torch

CIFAR_TRAIN_FILES = ["data_batch_%d.bin" % i for i in range(1, 6)]
CIFAR_TEST_FILES = ["test_batch.bin"]
CIFAR_NUM_TRAIN, CIFAR_NUM_TEST = 50000, 10000
MNIST_NUM_TRAIN, MNIST_NUM_TEST = 60000, 10000


def _cifar_dir(data_dir: str) -> Optional[str]:
    for d in (os.path.join(data_dir, "cifar-10-batches-bin"), data_dir):
        if os.path.isfile(os.path.join(d, CIFAR_TEST_FILES[0])):
            return d
    return None


def cifar10_available(data_dir: Optional[str]) -> bool:
    return bool(data_dir) and _cifar_dir(data_dir) is not None


def load_cifar10(data_dir: str) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Returns uint8 NHWC images and int64 labels: (train_x, train_y, test_x, test_y)."""
    d = _cifar_dir(data_dir)
    if d is None:
        raise FileNotFoundError("CIFAR-10 binaries not found under %s" % data_dir)

    def read(files):
        raw = np.concatenate([np.fromfile(os.path.join(d, f), dtype=np.uint8) for f in files])
        rec = raw.reshape(-1, 3073)
        y = rec[:, 0].astype(np.int64)
        x = rec[:, 1:].reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1).copy()
        return x, y

    trx, tr_y = read(CIFAR_TRAIN_FILES)
    tex, te_y = read(CIFAR_TEST_FILES)
    return trx, tr_y, tex, te_y


def per_image_standardization(x: torch.Tensor) -> torch.Tensor:
    """tf.image.per_image_standardization over [B, H, W, C] float."""
    n = x[0].numel()
    flat = x.reshape(x.shape[0], -1)
    mean = flat.mean(dim=1, keepdim=True)
    std = flat.std(dim=1, unbiased=False, keepdim=True)
    adj = torch.clamp(std, min=1.0 / float(np.sqrt(n)))
    return ((flat - mean) / adj).reshape(x.shape)


def _mix32(h):
    h = h.astype(np.uint32)
    h ^= h >> np.uint32(16)
    h = (h * np.uint32(0x7FEB352D)).astype(np.uint32)
    h ^= h >> np.uint32(15)
    h = (h * np.uint32(0x846CA68B)).astype(np.uint32)
    h ^= h >> np.uint32(16)
    return h


def augment_params(seed: int, counter: int, n: int):
    """Crop offsets / flip bits drawn by the HIP augmentation kernel (data.hip) for batch positions 0..n-1."""
    with np.errstate(over="ignore"):
        pos = np.arange(n, dtype=np.uint32)
        inner = _mix32((np.uint32(counter & 0xFFFFFFFF) * np.uint32(0x9E3779B9)).astype(np.uint32) + pos)
        h = _mix32(np.uint32(seed & 0xFFFFFFFF) ^ inner)
    return (h % 9).astype(np.int64), ((h >> 8) % 9).astype(np.int64), ((h >> 16) & 1).astype(bool)


def augment_cifar_with(x_u8: torch.Tensor, oy, ox, flip) -> torch.Tensor:
    """pad 4 -> crop at (oy, ox) -> optional horizontal flip -> standardize (cifar10_main.py:98-108)."""
    b = x_u8.shape[0]
    dev = x_u8.device
    oy, ox, flip = (torch.as_tensor(t, device=dev) for t in (oy, ox, flip))
    x = x_u8.float()
    xp = torch.nn.functional.pad(x.permute(0, 3, 1, 2), (4, 4, 4, 4)).permute(0, 2, 3, 1)
    ar = torch.arange(32, device=dev)
    rows = (oy[:, None] + ar[None, :])  # [B, 32]
    cols = (ox[:, None] + ar[None, :])
    cols = torch.where(flip[:, None], cols.flip(1), cols)
    bi = torch.arange(b, device=dev)[:, None, None]
    out = xp[bi, rows[:, :, None], cols[:, None, :]]
    return per_image_standardization(out)


def augment_cifar(x_u8: torch.Tensor, gen: Optional[torch.Generator] = None) -> torch.Tensor:
    """pad 4 -> random crop 32 -> random flip -> standardize. [B,32,32,3] uint8 -> float32 (torch ops)."""
    b = x_u8.shape[0]
    dev = x_u8.device
    oy = torch.randint(0, 9, (b,), device=dev, generator=gen)
    ox = torch.randint(0, 9, (b,), device=dev, generator=gen)
    flip = torch.rand(b, device=dev, generator=gen) < 0.5
    return augment_cifar_with(x_u8, oy, ox, flip)


def eval_cifar(x_u8: torch.Tensor) -> torch.Tensor:
    return per_image_standardization(x_u8.float())


def synthetic_images(n: int, shape, num_classes: int, seed: int, device, dtype=torch.float32):
    g = torch.Generator().manual_seed(int(seed))
    x = torch.randn((n,) + tuple(shape), generator=g).to(dtype)
    y = torch.randint(0, num_classes, (n,), generator=g)
    return x.to(device), y.to(device)


def learnable_cifar(n_train: int = 10000, n_test: int = 2000, seed: int = 7, noise: float = 2.5,
                    num_classes: int = 10):
    """A learnable CIFAR-shaped dataset that needs no download (the real CIFAR-10 is not on these machines):
    uint8 NHWC 32x32x3 images with labels, so it runs through the real input path (on-device gather, pad-4 random
    crop, flip, per-image standardisation: data.hip / cifar10_main.py:98-108).

    Each class has a fixed smooth random template (an 8x8x3 Gaussian field upsampled bilinearly to 32x32, so a
    random crop and a flip keep most of it) and every image is ``template[label] * contrast + noise`` with a
    per-image random contrast in [0.6, 1.4], brightness shift and i.i.d. pixel noise of ``noise`` template
    standard deviations.  Chance accuracy is 1/num_classes; a ResNet-20 reaches well above it within a few hundred
    steps (ResNet-8 fp32 on CPU at noise 2.5: training loss 2.1 -> 0.05 in 500 steps of batch 64; eval accuracy with the
    reference's 0.997-momentum moving BN statistics 0.58 / 0.77 after 600 steps, still rising), so loss / accuracy
    trajectories of two implementations can be compared (tests/test_gpu_trajectory.py).
    Returns (train_x, train_y, test_x, test_y) as numpy arrays."""
    g = torch.Generator().manual_seed(int(seed))
    base = torch.randn(num_classes, 3, 8, 8, generator=g)
    tmpl = torch.nn.functional.interpolate(base, size=(32, 32), mode="bilinear", align_corners=False)
    tmpl = tmpl / tmpl.flatten(1).std(dim=1).view(-1, 1, 1, 1)

    def make(n):
        y = torch.randint(0, num_classes, (n,), generator=g)
        contrast = 0.6 + 0.8 * torch.rand(n, 1, 1, 1, generator=g)
        shift = 0.3 * torch.randn(n, 1, 1, 1, generator=g)
        x = tmpl[y] * contrast + shift + noise * torch.randn(n, 3, 32, 32, generator=g)
        x = (x * 40.0 + 128.0).round().clamp(0, 255).to(torch.uint8)
        return x.permute(0, 2, 3, 1).contiguous().numpy(), y.numpy().astype(np.int64)

    trx, tr_y = make(n_train)
    tex, te_y = make(n_test)
    return trx, tr_y, tex, te_y


# ------------------------------------------------------------------------------------------------- ImageNet arrays
IMAGENET_FILES = ("train_images.npy", "train_labels.npy", "val_images.npy", "val_labels.npy")
IMAGENET_MEAN = (123.68, 116.78, 103.94)  # upstream _CHANNEL_MEANS (RGB), subtracted after the resample; no division
# the random-resized-crop rule of augment_imagenet_kernel (data.hip), as integers
IMAGENET_RATIO_Q16 = (49152, 51074, 53071, 55146, 57303, 59543, 61872, 64291,
                      66805, 69417, 72132, 74952, 77883, 80929, 84093, 87381)  # 3/4 * (16/9)^(i/15) in Q16
IMAGENET_AREA_MIN_Q16 = 5243  # ceil(0.08 * 65536)
IMAGENET_ATTEMPTS = 10


def imagenet_arrays_available(data_dir: Optional[str]) -> bool:
    return bool(data_dir) and all(os.path.isfile(os.path.join(data_dir, f)) for f in IMAGENET_FILES)


def load_imagenet_arrays(data_dir: str, device=None, max_bytes: Optional[int] = None,
                         out_size: Optional[int] = None):
    """Pre-decoded ImageNet-style arrays: ``train_images.npy`` / ``val_images.npy`` uint8 [N, S, S, 3] (NHWC, one
    square stored side S for both) and ``train_labels.npy`` / ``val_labels.npy`` integer [N].  The files are memory
    mapped (``np.load(mmap_mode="r")``), so validation reads only their headers.  The arrays are meant to live on
    ``device`` (DeviceDataset): their bytes -- uint8 images, int64 labels and the fp32 evaluation cache of
    ``eval_set`` at ``out_size`` (the stored side if not given) -- are checked against the device's free memory (or
    ``max_bytes``) and a MemoryError is raised before anything is allocated.  The step's own buffers are not
    counted: the check catches a set that cannot fit at all, not one that leaves too little for a large batch.
    Returns (train_x, train_y, val_x, val_y) as memory-mapped numpy arrays."""
    if not imagenet_arrays_available(data_dir):
        raise FileNotFoundError("ImageNet arrays (%s) not found under %s" % (", ".join(IMAGENET_FILES), data_dir))
    arrs = [np.load(os.path.join(data_dir, f), mmap_mode="r") for f in IMAGENET_FILES]
    trx, tr_y, vax, va_y = arrs
    for f, x in ((IMAGENET_FILES[0], trx), (IMAGENET_FILES[2], vax)):
        if x.dtype != np.uint8:
            raise ValueError("%s: images must be uint8, not %s" % (f, x.dtype))
        if x.ndim != 4 or x.shape[3] != 3:
            raise ValueError("%s: images must be [N, S, S, 3] (NHWC), not %s" % (f, list(x.shape)))
        if x.shape[1] != x.shape[2]:
            raise ValueError("%s: stored images must be square, not %d x %d" % (f, x.shape[1], x.shape[2]))
    if vax.shape[1] != trx.shape[1]:
        raise ValueError("%s: stored side %d differs from %s's %d" % (IMAGENET_FILES[2], vax.shape[1],
                                                                      IMAGENET_FILES[0], trx.shape[1]))
    for f, y, x in ((IMAGENET_FILES[1], tr_y, trx), (IMAGENET_FILES[3], va_y, vax)):
        if not np.issubdtype(y.dtype, np.integer):
            raise ValueError("%s: labels must be integers, not %s" % (f, y.dtype))
        if y.ndim != 1:
            raise ValueError("%s: labels must be [N], not %s" % (f, list(y.shape)))
        if y.shape[0] != x.shape[0]:
            raise ValueError("%s: %d labels for %d images" % (f, y.shape[0], x.shape[0]))
        if y.shape[0] == 0:
            raise ValueError("%s: the set is empty" % f)
    side = int(out_size) if out_size else int(vax.shape[1])
    need = (int(trx.size) + int(vax.size) + 8 * (int(tr_y.size) + int(va_y.size))
            + 4 * int(vax.shape[0]) * side * side * 3)
    limit = max_bytes
    if limit is None and device is not None and torch.device(device).type == "cuda":
        limit = int(torch.cuda.mem_get_info(torch.device(device))[0])
    if limit is not None and need > limit:
        raise MemoryError("ImageNet arrays under %s need %.1f GB on the device (%d + %d images at %d x %d, with the "
                          "fp32 evaluation cache) but %.1f GB are free: store the images at a smaller side"
                          % (data_dir, need / 1e9, trx.shape[0], vax.shape[0], trx.shape[1], trx.shape[1],
                             limit / 1e9))
    return trx, tr_y, vax, va_y


def _isqrt(v):
    """floor(sqrt(v)) of a non-negative integer array (< 2^52), exactly."""
    v = np.asarray(v, dtype=np.int64)
    r = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > v, r - 1, r)
    return np.where((r + 1) * (r + 1) <= v, r + 1, r)


def imagenet_eval_box(side: int):
    """(y0, x0, h, w) of the evaluation crop: the central crop of side round(0.875 * side)."""
    c = (7 * int(side) + 4) >> 3
    o = (int(side) - c) >> 1
    return o, o, c, c


def imagenet_augment_params(seed: int, counter, n: int, side: int, rows=None, augment: bool = True):
    """Crop boxes / flip bits drawn by augment_imagenet_kernel (data.hip), reproduced exactly with integers.

    Keyed by (seed, counter, batch position 0..n-1); with ``rows`` (the images' dataset rows) by (seed, the image's
    member step counter -- ``counter``, a scalar or one value per image --, dataset row) as the per-member keys of the
    population step.  Returns (boxes int64 [n, 4] of (y0, x0, h, w), flip bool [n])."""
    S = int(side)
    if not augment:
        return np.tile(np.array(imagenet_eval_box(S), dtype=np.int64), (n, 1)), np.zeros(n, dtype=bool)
    with np.errstate(over="ignore"):
        cnt = (np.broadcast_to(np.asarray(counter, dtype=np.int64), (n,)) & 0xFFFFFFFF).astype(np.uint32)
        pos = (np.arange(n, dtype=np.uint32) if rows is None
               else (np.asarray(rows, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32))
        inner = _mix32((cnt * np.uint32(0x9E3779B9)).astype(np.uint32) + pos)
        h = _mix32(np.uint32(seed & 0xFFFFFFFF) ^ inner)
        flip = ((h >> np.uint32(20)) & np.uint32(1)).astype(bool)
        boxes = np.tile(np.array([0, 0, S, S], dtype=np.int64), (n, 1))  # no attempt fits: the whole image
        done = np.zeros(n, dtype=bool)
        table = np.array(IMAGENET_RATIO_Q16, dtype=np.int64)
        for _ in range(IMAGENET_ATTEMPTS):
            hi = h.astype(np.int64)
            f = IMAGENET_AREA_MIN_Q16 + (((hi & 0xFFFF) * (65536 - IMAGENET_AREA_MIN_Q16)) >> 16)
            area = (S * S * f) >> 16
            r = (hi >> 16) & 15
            w = _isqrt((area * table[r]) >> 16)
            hh = _isqrt((area * table[15 - r]) >> 16)
            ok = (w >= 1) & (hh >= 1) & (w <= S) & (hh <= S) & ~done
            g = _mix32(h ^ np.uint32(0x68E31DA4)).astype(np.int64)
            y0 = ((g & 0xFFFF) * (S - hh + 1)) >> 16
            x0 = ((g >> 16) * (S - w + 1)) >> 16
            boxes[ok] = np.stack([y0, x0, hh, w], axis=1)[ok]
            done |= ok
            h = _mix32(h + np.uint32(0x9E3779B9))
    return boxes, flip


def augment_imagenet_with(x_u8: torch.Tensor, boxes, flip, out_size: int) -> torch.Tensor:
    """Per image: crop the box (y0, x0, h, w), bilinear resample to ``out_size`` x ``out_size`` (half-pixel centres,
    clamped to the box: ``interpolate(mode="bilinear", align_corners=False)``), optional horizontal flip, subtract
    the channel means.  [B, S, S, 3] uint8 -> [B, out_size, out_size, 3] float32.  The torch reference of
    augment_imagenet_kernel (data.hip) and the CPU input path."""
    b, H = x_u8.shape[0], int(out_size)
    boxes = np.asarray(torch.as_tensor(boxes).cpu()).reshape(b, -1)
    flip = np.asarray(torch.as_tensor(flip).cpu()).reshape(b).astype(bool)
    out = torch.empty(b, H, H, 3, dtype=torch.float32, device=x_u8.device)
    mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32, device=x_u8.device)
    for i in range(b):
        y0, x0, h, w = (int(v) for v in boxes[i][:4])
        crop = x_u8[i, y0:y0 + h, x0:x0 + w].permute(2, 0, 1)[None].float()
        r = torch.nn.functional.interpolate(crop, size=(H, H), mode="bilinear", align_corners=False)[0]
        if flip[i]:
            r = r.flip(2)
        out[i] = r.permute(1, 2, 0) - mean
    return out


def augment_imagenet(x_u8: torch.Tensor, gen=None, out_size: int = 224, seed: int = 0, counter: int = 0):
    """Random-resized crop + flip + mean subtraction with the kernel's own draws for (seed, counter, position)."""
    boxes, flip = imagenet_augment_params(seed, counter, x_u8.shape[0], x_u8.shape[1])
    return augment_imagenet_with(x_u8, boxes, flip, out_size)


def eval_imagenet(x_u8: torch.Tensor, out_size: int = 224) -> torch.Tensor:
    """The evaluation transform: central crop of side round(0.875 S), resample to ``out_size``, subtract the means
    (upstream's resize-256 / crop-224 on square stored images)."""
    boxes, flip = imagenet_augment_params(0, 0, x_u8.shape[0], x_u8.shape[1], augment=False)
    return augment_imagenet_with(x_u8, boxes, flip, out_size)


def learnable_imagenet(n_train: int = 4000, n_test: int = 500, side: int = 64, num_classes: int = 10, seed: int = 11,
                       noise: float = 1.0):
    """A learnable ImageNet-shaped dataset that needs no download: uint8 NHWC ``side`` x ``side`` x 3 images with
    labels, so it runs through the real input path (on-device gather, random-resized crop, bilinear resample, flip,
    mean subtraction: data.hip).

    As ``learnable_cifar``: each class has a fixed smooth template, an 8x8x3 Gaussian field upsampled bilinearly to
    ``side``, plus a class colour; every image is ``template[label] * contrast + shift + noise`` with a per-image
    contrast in [0.6, 1.4], a brightness shift and i.i.d. pixel noise of ``noise`` template standard deviations.
    A random-resized crop keeps between 8 % and all of the image at an aspect ratio of 3/4 .. 4/3: the class colour
    survives every crop and the low-resolution field keeps most of its structure in a part of the image, so the set
    stays learnable under that augmentation.  Chance accuracy is 1 / num_classes.
    Returns (train_x, train_y, test_x, test_y) as numpy arrays."""
    g = torch.Generator().manual_seed(int(seed))
    side = int(side)
    base = torch.randn(num_classes, 3, 8, 8, generator=g)
    tmpl = torch.nn.functional.interpolate(base, size=(side, side), mode="bilinear", align_corners=False)
    tmpl = tmpl / tmpl.flatten(1).std(dim=1).view(-1, 1, 1, 1)
    tmpl = tmpl + 0.7 * torch.randn(num_classes, 3, 1, 1, generator=g)

    def make(n):
        y = torch.randint(0, num_classes, (n,), generator=g)
        xs = []
        for i in range(0, n, 512):  # in chunks: the float images of a large set do not fit at once
            m = min(512, n - i)
            contrast = 0.6 + 0.8 * torch.rand(m, 1, 1, 1, generator=g)
            shift = 0.3 * torch.randn(m, 1, 1, 1, generator=g)
            x = tmpl[y[i:i + m]] * contrast + shift + noise * torch.randn(m, 3, side, side, generator=g)
            xs.append((x * 40.0 + 128.0).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous())
        return torch.cat(xs).numpy(), y.numpy().astype(np.int64)

    trx, tr_y = make(n_train)
    tex, te_y = make(n_test)
    return trx, tr_y, tex, te_y


def _idx(path, offset, dtype=np.uint8):
    with gzip.open(path, "rb") as f:
        return np.frombuffer(f.read(), dtype, offset=offset)


def mnist_available(data_dir: Optional[str]) -> bool:
    return bool(data_dir) and os.path.isfile(os.path.join(data_dir, "t10k-images-idx3-ubyte.gz"))


def load_mnist(data_dir: str, normalize: bool = False):
    trx = _idx(os.path.join(data_dir, "train-images-idx3-ubyte.gz"), 16).astype(np.float32).reshape(-1, 28, 28, 1)
    tr_y = _idx(os.path.join(data_dir, "train-labels-idx1-ubyte.gz"), 8).astype(np.int64)
    tex = _idx(os.path.join(data_dir, "t10k-images-idx3-ubyte.gz"), 16).astype(np.float32).reshape(-1, 28, 28, 1)
    te_y = _idx(os.path.join(data_dir, "t10k-labels-idx1-ubyte.gz"), 8).astype(np.int64)
    if normalize:
        trx /= 255.0
        tex /= 255.0
    return trx, tr_y, tex, te_y


class IndexBatch:
    """A training batch named by dataset rows, materialised lazily.

    Engines with an on-device input path (the HIP ResNet step) consume the
    indices directly -- gather, augmentation and the bf16 stem packing run in
    one kernel inside the captured step graph; every other engine calls
    :meth:`materialize`.
    """

    def __init__(self, ds: "DeviceDataset", idx: torch.Tensor):
        self.ds, self.idx = ds, idx

    def __len__(self):
        return int(self.idx.numel())

    def materialize(self, gen=None):
        return self.ds.batch(self.idx, gen)


def batch_len(b) -> int:
    return len(b) if isinstance(b, IndexBatch) else int(b[1].shape[0])


class DeviceDataset:
    """Train/eval arrays resident on the device with per-member epoch shuffling.

    CIFAR-style uint8 32x32x3 data with ``augment=augment_cifar`` on a GPU uses
    the fused HIP kernel (data.hip) for gather + pad/crop/flip + standardize.
    Square uint8 [*, S, S, 3] data with ``augment=augment_imagenet`` and an
    ``out_size`` is the ImageNet-style set: on a GPU the second kernel of
    data.hip gathers, crops, resamples to ``out_size`` and subtracts the channel
    means; on a CPU the torch reference does, from the same draws.
    """

    def __init__(self, train_x, train_y, test_x, test_y, device, augment=None, eval_transform=None, seed=0,
                 out_size=None):
        self.train_x = torch.as_tensor(train_x).to(device).contiguous()
        self.train_y = torch.as_tensor(train_y).to(device).long().contiguous()
        self.test_x = torch.as_tensor(test_x).to(device).contiguous()
        self.test_y = torch.as_tensor(test_y).to(device).long().contiguous()
        self.augment = augment
        self.eval_transform = eval_transform
        self._eval_cache = None
        self.device = torch.device(device)
        self.hip_augment = (self.device.type == "cuda" and augment is augment_cifar
                            and self.train_x.dtype == torch.uint8 and tuple(self.train_x.shape[1:]) == (32, 32, 3))
        self.out_size = int(out_size) if out_size else None
        sq = self.train_x.dim() == 4 and self.train_x.shape[1] == self.train_x.shape[2] and self.train_x.shape[3] == 3
        self.imagenet = (augment is augment_imagenet and self.out_size is not None
                         and self.train_x.dtype == torch.uint8 and sq)
        if augment is augment_imagenet and not self.imagenet:
            raise ValueError("augment_imagenet needs square uint8 [N, S, S, 3] images and an out_size")
        if self.imagenet and self.device.type == "cuda":
            self.hip_augment = True
        self.rng_seed = int(seed) & 0x7FFFFFFF
        self.rng_counter = 0

    @property
    def num_train(self):
        return int(self.train_x.shape[0])

    def next_rng(self):
        """(seed, counter) for one augmentation launch; the counter advances per launch."""
        self.rng_counter = (self.rng_counter + 1) & 0x7FFFFFFF
        return self.rng_seed, self.rng_counter

    def batch(self, idx: torch.Tensor, gen=None):
        if self.imagenet:
            n, H = int(idx.numel()), self.out_size
            seed, counter = self.next_rng()
            if not self.hip_augment:
                x = augment_imagenet(self.train_x[idx], None, H, seed, counter)
                return x, self.train_y[idx]
            from .. import ops
            x = torch.empty(n, H, H, 3, dtype=torch.float32, device=self.device)
            y = torch.empty(n, dtype=torch.int64, device=self.device)
            rng = torch.tensor((seed, counter), dtype=torch.int32).to(self.device)
            ops.augment_imagenet(self.train_x, self.train_y, idx.long().contiguous(), rng, H, True, out32=x, lab64=y)
            return x, y
        if self.hip_augment:
            from .. import ops
            n = int(idx.numel())
            x = torch.empty(n, 32, 32, 3, dtype=torch.float32, device=self.device)
            y = torch.empty(n, dtype=torch.int64, device=self.device)
            rng = torch.tensor(self.next_rng(), dtype=torch.int32).to(self.device)
            ops.augment_cifar(self.train_x, self.train_y, idx.long().contiguous(), rng, True, out32=x, lab64=y)
            return x, y
        x = self.train_x[idx]
        x = self.augment(x, gen) if self.augment is not None else x.float()
        return x, self.train_y[idx]

    def eval_set(self):
        """The evaluation set as fp32 (cached).  The ImageNet-style set is materialised once through the kernel's
        ``augment = 0`` path (central crop, resample, means): 12 bytes per output pixel, 602 KB per image at 224 x
        224 -- 30 GB for 50 000 validation images, so size the validation file to what fits next to a step."""
        if self._eval_cache is None and self.imagenet and self.hip_augment:
            from .. import ops
            n, H = int(self.test_x.shape[0]), self.out_size
            x = torch.empty(n, H, H, 3, dtype=torch.float32, device=self.device)
            rng = torch.zeros(2, dtype=torch.int32, device=self.device)
            for i in range(0, n, 4096):
                rows = torch.arange(i, min(n, i + 4096), dtype=torch.int64, device=self.device)
                ops.augment_imagenet(self.test_x, self.test_y, rows, rng, H, False, out32=x[i:i + 4096])
            self._eval_cache = (x, self.test_y)
        if self._eval_cache is None and self.imagenet:
            self._eval_cache = (eval_imagenet(self.test_x, self.out_size), self.test_y)
        if self._eval_cache is None:
            x = self.test_x
            x = self.eval_transform(x) if self.eval_transform is not None else x.float()
            self._eval_cache = (x, self.test_y)
        return self._eval_cache


class SyntheticDataset:
    """Fixed device-resident batch reused every step (reference synthetic mode)."""

    def __init__(self, shape, num_classes, device, max_batch=256, n_eval=1000, seed=1234, dtype=torch.float32):
        self.x, self.y = synthetic_images(max_batch, shape, num_classes, seed, device, dtype)
        self.ex, self.ey = synthetic_images(n_eval, shape, num_classes, seed + 1, device, dtype)
        self.num_train = CIFAR_NUM_TRAIN if tuple(shape)[0] == 32 else 50000
        self.device = device

    def batch_slice(self, b: int):
        return self.x[:b], self.y[:b]

    def eval_set(self):
        return self.ex, self.ey
