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
                         out_size: Optional[int] = None, resident: bool = True, stage_rows: int = 1024):
    """Pre-decoded ImageNet-style arrays: ``train_images.npy`` / ``val_images.npy`` uint8 [N, S, S, 3] (NHWC, one
    square stored side S for both) and ``train_labels.npy`` / ``val_labels.npy`` integer [N].  The files are memory
    mapped (``np.load(mmap_mode="r")``), so validation reads only their headers.  The arrays are meant to live on
    ``device`` (DeviceDataset): their bytes -- uint8 images, int64 labels and the fp32 evaluation cache of
    ``eval_set`` at ``out_size`` (the stored side if not given) -- are checked against the device's free memory (or
    ``max_bytes``) and a MemoryError is raised before anything is allocated.  The step's own buffers are not
    counted: the check catches a set that cannot fit at all, not one that leaves too little for a large batch.
    ``resident=False`` (HostImageNetDataset): the training images stay in the memory-mapped file on the host and are
    not counted; the validation images, the labels, the evaluation cache and the two staging halves of ``stage_rows``
    images each (2 * stage_rows * S * S * 3 bytes, RowStager) are.
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
    if not resident:
        stage = 2 * int(stage_rows) * int(trx.shape[1]) * int(trx.shape[1]) * 3
        need = need - int(trx.size) + stage
        if limit is not None and need > limit:
            raise MemoryError("ImageNet arrays under %s with the training images on the host need %.1f GB on the "
                              "device (%d validation images at %d x %d with the fp32 evaluation cache, the labels and "
                              "%.1f GB of staging for %d rows per step) but %.1f GB are free: store fewer validation "
                              "images" % (data_dir, need / 1e9, vax.shape[0], trx.shape[1], trx.shape[1], stage / 1e9,
                                          int(stage_rows), limit / 1e9))
        return trx, tr_y, vax, va_y
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

    def __init__(self, ds: "DeviceDataset", idx: torch.Tensor, next_rows: Optional[torch.Tensor] = None):
        self.ds, self.idx = ds, idx
        # host-resident sets: the rows the member will ask for next (a hint the plan prefetches by and verifies on
        # the next step; None: nothing announced, e.g. at an epoch end)
        self.next_rows = next_rows

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
        self._init_rest(train_y, test_x, test_y, device, augment, eval_transform, seed, out_size)
        self.hip_augment = (self.device.type == "cuda" and augment is augment_cifar
                            and self.train_x.dtype == torch.uint8 and tuple(self.train_x.shape[1:]) == (32, 32, 3))
        sq = self.train_x.dim() == 4 and self.train_x.shape[1] == self.train_x.shape[2] and self.train_x.shape[3] == 3
        self.imagenet = (augment is augment_imagenet and self.out_size is not None
                         and self.train_x.dtype == torch.uint8 and sq)
        if augment is augment_imagenet and not self.imagenet:
            raise ValueError("augment_imagenet needs square uint8 [N, S, S, 3] images and an out_size")
        if self.imagenet and self.device.type == "cuda":
            self.hip_augment = True

    def _init_rest(self, train_y, test_x, test_y, device, augment, eval_transform, seed, out_size):
        """Everything but the training images, which a subclass may keep elsewhere (HostImageNetDataset): labels and
        the evaluation set on the device, the transforms, the evaluation cache, the augmentation rng."""
        self.train_y = torch.as_tensor(train_y).to(device).long().contiguous()
        self.test_x = torch.as_tensor(test_x).to(device).contiguous()
        self.test_y = torch.as_tensor(test_y).to(device).long().contiguous()
        self.augment = augment
        self.eval_transform = eval_transform
        self._eval_cache = None
        self.device = torch.device(device)
        self.out_size = int(out_size) if out_size else None
        self.rng_seed = int(seed) & 0x7FFFFFFF
        self.rng_counter = 0

    def close(self) -> None:
        """Release what the set holds besides memory (the gather threads of a host-resident set); idempotent."""

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


def _stager_worker(jobs):
    """A gather thread of a RowStager: runs queued callables until it reads None.  It holds the queue only, never
    the stager, so a dropped stager is collected and closes its threads."""
    while True:
        job = jobs.get()
        if job is None:
            return
        job()


class RowStager:
    """Rows of a host-resident uint8 image array [N, S, S, 3] -> one of two device staging halves.

    Holds two pinned host buffers [cap, S, S, 3], the device tensor ``dev`` [2, cap, S, S, 3], a copy stream and per
    half a "copied" and a "consumed" event.  ``stage(rows, half)`` returns at once: gather threads (at most
    ``min(8, torch.get_num_threads())``, daemons) copy ``images[rows]`` into the half's pinned buffer, one slice of
    the rows each (``np.take(..., out=...)``, which releases the interpreter lock); the thread that finishes last
    issues one non-blocking host-to-device copy on the copy stream -- after that stream has waited for the half's
    "consumed" event -- and records "copied".  The pinned buffer is not overwritten before the copy that last read
    it is done.  ``wait_copied(half)`` makes the current stream wait for the half, ``mark_consumed(half)`` records on
    the current stream that the half's reader is enqueued.  On a CPU device the same code runs without streams and
    events.  ``cap`` grows on demand (``ensure``: both halves are reallocated after one device synchronise and
    ``generation`` advances -- whoever baked ``dev``'s address into a captured graph must capture again)."""

    def __init__(self, images, device, threads: Optional[int] = None):
        import queue
        import threading
        assert isinstance(images, np.ndarray) and images.dtype == np.uint8 and images.ndim == 4
        self.images = images
        self.device = torch.device(device)
        self.cuda = self.device.type == "cuda"
        self.S = int(images.shape[1])
        self.cap, self.generation = 0, 0
        self.host, self.dev = [None, None], None
        self.copy_stream = torch.cuda.Stream(self.device) if self.cuda else None
        self.copied = self.consumed = (None, None)
        self.stages = 0  # stage() calls
        k = max(1, min(8, int(threads) if threads else torch.get_num_threads()))
        self._jobs = queue.SimpleQueue()
        self._threads = [threading.Thread(target=_stager_worker, args=(self._jobs,), daemon=True,
                                          name="dtf-row-stager-%d" % i) for i in range(k)]
        for t in self._threads:
            t.start()
        self._issued = [None, None]  # per half: the last job's (done Event, error list)
        self._closed = False

    # ---- buffers
    def ensure(self, cap: int) -> None:
        cap = int(cap)
        if cap <= self.cap:
            return
        self.drain()
        shape = (cap, self.S, self.S, 3)
        if self.cuda:
            torch.cuda.synchronize(self.device)  # once: nothing enqueued reads the old halves any more
            self.host = [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(2)]
            self.copied = tuple(torch.cuda.Event() for _ in range(2))
            self.consumed = tuple(torch.cuda.Event() for _ in range(2))
        else:
            self.host = [torch.empty(shape, dtype=torch.uint8) for _ in range(2)]
        self.dev = torch.empty((2,) + shape, dtype=torch.uint8, device=self.device)
        self.cap = cap
        self.generation += 1

    @property
    def nbytes(self) -> int:
        return 2 * self.cap * self.S * self.S * 3

    # ---- staging
    def stage(self, rows, half: int) -> None:
        import threading
        if self._closed:
            raise RuntimeError("RowStager is closed")
        rows = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.int64)
        n = int(rows.shape[0])
        assert 0 <= half <= 1 and 0 < n <= self.cap, (half, n, self.cap)
        assert int(rows.min()) >= 0 and int(rows.max()) < self.images.shape[0], "dataset row out of range"
        self.wait_issued(half)  # an earlier job of this half (an unused prefetch) is through
        self.stages += 1
        done, errors, lock = threading.Event(), [], threading.Lock()
        parts = min(len(self._threads), max(1, n // 8))
        left = [parts]
        images, host, dev = self.images, self.host[half], self.dev
        out = host.numpy()
        copied, consumed, stream, device = self.copied[half], self.consumed[half], self.copy_stream, self.device

        def part(lo, hi):
            try:
                if copied is not None:
                    copied.synchronize()  # the copy that last read this pinned buffer is done
                np.take(images, rows[lo:hi], axis=0, out=out[lo:hi], mode="clip")
            except BaseException as e:  # noqa: BLE001 -- re-raised on the staging thread's caller (wait_issued)
                errors.append(e)
            with lock:
                left[0] -= 1
                last = left[0] == 0
            if not last:
                return
            try:
                if errors:
                    return
                if stream is None:
                    dev[half, :n].copy_(host[:n])
                    return
                with torch.cuda.device(device), torch.cuda.stream(stream):
                    stream.wait_event(consumed)  # the half's last reader is through
                    dev[half, :n].copy_(host[:n], non_blocking=True)
                    copied.record(stream)
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
            finally:
                done.set()

        self._issued[half] = (done, errors)
        cut = [n * i // parts for i in range(parts + 1)]
        for i in range(parts):
            self._jobs.put(lambda lo=cut[i], hi=cut[i + 1]: part(lo, hi))

    def wait_issued(self, half: int) -> None:
        """Host wait until the half's last ``stage`` has gathered and issued its copy; re-raises its error."""
        job = self._issued[half]
        if job is None:
            return
        done, errors = job
        done.wait()
        self._issued[half] = None
        if errors:
            raise errors[0]

    def drain(self) -> None:
        for h in (0, 1):
            self.wait_issued(h)

    def wait_copied(self, half: int) -> None:
        self.wait_issued(half)
        if self.cuda:
            torch.cuda.current_stream(self.device).wait_event(self.copied[half])

    def mark_consumed(self, half: int) -> None:
        if self.cuda:
            self.consumed[half].record(torch.cuda.current_stream(self.device))

    # ---- shutdown
    def close(self) -> None:
        """Join the gather threads (idempotent).  They are daemons as well: a stager that is never closed does not
        keep the process alive."""
        if self._closed:
            return
        self._closed = True
        for _ in self._threads:
            self._jobs.put(None)
        for t in self._threads:
            t.join()

    def threads_alive(self) -> int:
        return sum(t.is_alive() for t in self._threads)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass


class HostFeed:
    """Which staging half holds which rows: the plan-side protocol over a RowStager (or anything with its
    ``ensure`` / ``stage`` / ``wait_copied`` / ``mark_consumed`` / ``cap`` / ``generation``).

    A step calls ``half = begin(rows)`` before it enqueues its reader and ``end(announced)`` after.  The halves
    alternate.  ``begin`` takes the other half as it is if the rows announced at the last ``end`` are exactly the rows
    now requested (``hits``), and stages the requested rows into it now otherwise (``syncs``): an announcement is a
    hint, and correctness never depends on it.  ``end`` marks the step's half consumed, then starts staging the
    announced rows into the other half -- whose own consumed mark dates from the step before."""

    def __init__(self, stager, prefetch: bool = True):
        self.stager = stager
        self.prefetch = prefetch  # False: every step is staged synchronously (measurements)
        self.half = 1  # the half of the last step
        self.ahead = None  # rows staged into the other half by the last end()
        self._gen = stager.generation
        self.hits = self.syncs = 0

    def begin(self, rows) -> int:
        st = self.stager
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        if rows.shape[0] > st.cap:
            st.ensure(rows.shape[0])
        if st.generation != self._gen:
            self._gen, self.ahead = st.generation, None  # reallocated halves hold nothing
        half = 1 - self.half
        if self.ahead is not None and np.array_equal(self.ahead, rows):
            self.hits += 1
        else:
            st.stage(rows, half)
            self.syncs += 1
        self.ahead = None
        st.wait_copied(half)
        self.half = half
        return half

    def end(self, announced=None) -> None:
        st = self.stager
        st.mark_consumed(self.half)
        if not self.prefetch or announced is None:
            return
        announced = np.array(announced, dtype=np.int64).reshape(-1)
        if 0 < announced.shape[0] <= st.cap:
            st.stage(announced, 1 - self.half)
            self.ahead = announced


class HostImageNetDataset(DeviceDataset):
    """The ImageNet-style set with the training images on the host: ``train_x`` is the (memory-mapped) numpy array
    [N, S, S, 3] uint8 and is never copied whole; the labels, the validation set and the evaluation cache live on the
    device exactly as in DeviceDataset.  A step's rows reach the device through the set's RowStager (``feed``), and
    the staged form of the input kernel reads them there (``ops.augment_imagenet_staged``): the same arithmetic and
    the same draws as the resident set for the same rows, seed and counter."""

    host_resident = True

    def __init__(self, train_x, train_y, test_x, test_y, device, out_size, seed=0):
        if not (isinstance(train_x, np.ndarray) and train_x.dtype == np.uint8 and train_x.ndim == 4
                and train_x.shape[1] == train_x.shape[2] and train_x.shape[3] == 3 and out_size):
            raise ValueError("HostImageNetDataset needs square uint8 [N, S, S, 3] numpy images and an out_size")
        self.train_x = train_x
        self._init_rest(train_y, test_x, test_y, device, augment_imagenet, eval_imagenet, seed, out_size)
        self.imagenet = True
        self.hip_augment = self.device.type == "cuda"
        self._feed = None

    @property
    def feed(self) -> HostFeed:
        if self._feed is None:
            self._feed = HostFeed(RowStager(self.train_x, self.device))
        return self._feed

    def batch(self, idx, gen=None):
        n, H = int(idx.numel()), self.out_size
        seed, counter = self.next_rng()
        rows = np.asarray(torch.as_tensor(idx).cpu(), dtype=np.int64).reshape(-1)
        if not self.hip_augment:
            x = augment_imagenet(torch.from_numpy(np.array(self.train_x[rows])), None, H, seed, counter)
            return x, self.train_y[torch.from_numpy(rows)]
        from .. import ops
        feed = self.feed
        half = feed.begin(rows)  # staged now: this path announces nothing
        x = torch.empty(n, H, H, 3, dtype=torch.float32, device=self.device)
        y = torch.empty(n, dtype=torch.int64, device=self.device)
        rng = torch.tensor((seed, counter), dtype=torch.int32).to(self.device)
        hw = torch.tensor([half], dtype=torch.int32).to(self.device)
        ops.augment_imagenet_staged(feed.stager.dev, hw, self.train_y, torch.from_numpy(rows).to(self.device), rng, H,
                                    True, out32=x, lab64=y)
        feed.end(None)
        return x, y

    def close(self) -> None:
        if self._feed is not None:
            self._feed.stager.close()


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
