"""The ImageNet input path without a device: array loader, the integer crop rule, the torch reference of the
resample, the constructions the GPU test relies on, and the model's choice of dataset."""
import math

import numpy as np
import pytest
import torch

from _imagenet_input_ref import resample_f64
from distributedtf_amd.data import datasets
from distributedtf_amd.data.datasets import (IMAGENET_MEAN, augment_imagenet_with, imagenet_augment_params,
                                             imagenet_eval_box, load_imagenet_arrays)


# ------------------------------------------------------------------------------------------------------ loader
def _write(d, n=6, nv=4, s=8, **over):
    rng = np.random.default_rng(0)
    arrs = {"train_images": rng.integers(0, 256, (n, s, s, 3), dtype=np.uint8),
            "train_labels": rng.integers(0, 5, (n,), dtype=np.int64),
            "val_images": rng.integers(0, 256, (nv, s, s, 3), dtype=np.uint8),
            "val_labels": rng.integers(0, 5, (nv,), dtype=np.int32)}
    arrs.update(over)
    for k, v in arrs.items():
        np.save(str(d / (k + ".npy")), v)
    return arrs


def test_loader_accepts_valid_dir(tmp_path):
    assert not datasets.imagenet_arrays_available(str(tmp_path))
    assert not datasets.imagenet_arrays_available(None)
    a = _write(tmp_path)
    assert datasets.imagenet_arrays_available(str(tmp_path))
    trx, tr_y, vax, va_y = load_imagenet_arrays(str(tmp_path))
    assert isinstance(trx, np.memmap) and trx.dtype == np.uint8 and trx.shape == (6, 8, 8, 3)
    assert np.array_equal(trx, a["train_images"]) and np.array_equal(va_y, a["val_labels"])
    assert np.array_equal(tr_y, a["train_labels"]) and np.array_equal(vax, a["val_images"])


@pytest.mark.parametrize("over,name", [
    (dict(train_images=np.zeros((6, 8, 8, 3), np.float32)), "train_images.npy"),       # wrong dtype
    (dict(val_images=np.zeros((4, 8, 8), np.uint8)), "val_images.npy"),                # wrong rank
    (dict(train_images=np.zeros((6, 8, 9, 3), np.uint8)), "train_images.npy"),         # not square
    (dict(train_labels=np.zeros((5,), np.int64)), "train_labels.npy"),                 # mismatched lengths
    (dict(val_labels=np.zeros((4,), np.float32)), "val_labels.npy"),                   # labels not integers
    (dict(val_images=np.zeros((4, 6, 6, 3), np.uint8)), "val_images.npy"),             # another stored side
])
def test_loader_rejects_by_file_name(tmp_path, over, name):
    _write(tmp_path, **over)
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):
        load_imagenet_arrays(str(tmp_path))


def test_loader_missing_and_too_large(tmp_path):
    with pytest.raises(FileNotFoundError):
        load_imagenet_arrays(str(tmp_path))
    _write(tmp_path)
    need = 6 * 192 + 4 * 192 + 8 * 10 + 4 * 4 * 192  # uint8 images, int64 labels, the fp32 evaluation cache
    load_imagenet_arrays(str(tmp_path), max_bytes=need)
    with pytest.raises(MemoryError, match="GB"):
        load_imagenet_arrays(str(tmp_path), max_bytes=need - 1)


# ---------------------------------------------------------------------------------------------------- box rule
# How far the integer rule moves a box from the real-valued one.  With A = S^2, f the Q16 area fraction in
# [0.08, 1) and r the Q16 table ratio (3/4 .. 4/3, each entry within 2^-17 of the real value, relative 2^-16):
#   T = floor(A f / 2^16)            in (0.08 A - 1, A)
#   w = floor(sqrt(floor(T r)))      so  w^2 <= T r  and  (w + 1)^2 > T r - 1
#   h = floor(sqrt(floor(T r')))     with r' the table's entry for 1 / r: r r' in 1 +- 2^-15
# hence  w h <= T sqrt(r r') < A (1 + 2^-15),  ((w + 1)^2 + 1)((h + 1)^2 + 1) > T^2 r r' > (0.08 A - 1)^2 (1 - 2^-15),
# and    w^2 / ((h + 1)^2 + 1) < r / r' <= (4/3)^2 (1 + 2^-14),  h^2 / ((w + 1)^2 + 1) < r' / r  likewise.
@pytest.mark.parametrize("side", [16, 37])
def test_box_rule_bounds(side):
    n = 4000
    boxes, flip = imagenet_augment_params(1234, 7, n, side)
    y0, x0, h, w = (boxes[:, i].astype(np.float64) for i in range(4))
    assert boxes.dtype == np.int64 and flip.dtype == bool
    assert (h >= 1).all() and (w >= 1).all() and (y0 >= 0).all() and (x0 >= 0).all()
    assert (y0 + h <= side).all() and (x0 + w <= side).all()
    A = float(side * side)
    whole = (h == side) & (w == side)  # the fallback (not expected in a few thousand draws) is outside the bounds
    assert whole.sum() == 0
    assert (w * h < A * (1 + 2.0 ** -15)).all()
    assert (((w + 1) ** 2 + 1) * ((h + 1) ** 2 + 1) > (0.08 * A - 1) ** 2 * (1 - 2.0 ** -15)).all()
    lim = (16.0 / 9.0) * (1 + 2.0 ** -14)
    assert (w ** 2 / ((h + 1) ** 2 + 1) < lim).all() and (h ** 2 / ((w + 1) ** 2 + 1) < lim).all()
    # the draws use the range: small and large areas, wide and tall boxes, every corner region
    assert (w * h < 0.2 * A).any() and (w * h > 0.7 * A).any() and (w > h).any() and (h > w).any()
    assert (y0 == 0).any() and (y0 + h == side).any() and (x0 == 0).any() and (x0 + w == side).any()
    assert 0.45 < flip.mean() < 0.55  # 4000 fair bits: 0.5 +- 0.008 (1 sigma)


def test_box_rule_fallback_keys_and_eval():
    # a 1 x 1 image: every attempt asks for floor(f) = 0 pixels, so all ten fail and the box is the whole image
    boxes, _ = imagenet_augment_params(5, 9, 50, 1)
    assert (boxes == np.array([0, 0, 1, 1])).all()
    # the isqrt is exact around squares
    v = np.array([0, 1, 3, 4, 8, 9, 15, 16, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 50 - 1, 2 ** 50])
    assert [int(r) for r in datasets._isqrt(v)] == [math.isqrt(int(x)) for x in v]
    a = imagenet_augment_params(11, 3, 300, 37)
    b = imagenet_augment_params(11, 3, 300, 37)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])  # equal keys: equal boxes
    c = imagenet_augment_params(11, 4, 300, 37)
    assert (a[0] != c[0]).any(axis=1).mean() > 0.9  # consecutive counters: other boxes
    d = imagenet_augment_params(12, 3, 300, 37)
    assert (a[0] != d[0]).any(axis=1).mean() > 0.9
    # per-member keys: (seed, the image's member step, dataset row) -- the batch position does not matter
    rows = np.array([5, 900, 5, 17, 900])
    steps = np.array([3, 3, 3, 4, 9])
    e, ef = imagenet_augment_params(11, steps, 5, 37, rows=rows)
    assert np.array_equal(e[0], e[2]) and ef[0] == ef[2]
    one, onef = imagenet_augment_params(11, 9, 1, 37, rows=np.array([900]))
    assert np.array_equal(one[0], e[4]) and onef[0] == ef[4]
    assert not np.array_equal(e[1], e[4])
    # evaluation: the central crop of side round(0.875 S), no flip
    assert imagenet_eval_box(16) == (1, 1, 14, 14) and imagenet_eval_box(32) == (2, 2, 28, 28)
    assert imagenet_eval_box(256) == (16, 16, 224, 224) and imagenet_eval_box(37) == (2, 2, 32, 32)
    ev, evf = imagenet_augment_params(1, 2, 3, 40, augment=False)
    assert (ev == np.array([2, 2, 35, 35])).all() and not evf.any()


# -------------------------------------------------------------------------------------------- resample reference
def _img(side, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (side, side, 3), dtype=np.uint8)


@pytest.mark.parametrize("side,H,box,flip", [
    (16, 14, (1, 1, 14, 14), False),   # crop equals output: the identity
    (16, 14, (1, 1, 14, 14), True),
    (32, 14, (2, 2, 28, 28), False),   # an exact 2x crop: every weight 1/2
    (20, 8, (7, 11, 1, 1), False),     # a 1-pixel box
    (20, 8, (0, 3, 5, 9), True),       # touching the top
    (20, 8, (13, 0, 7, 4), False),     # touching the bottom and the left
    (20, 8, (2, 14, 11, 6), True),     # touching the right
    (37, 16, (0, 0, 37, 37), False),   # the whole image (the fallback box)
    (37, 16, (5, 9, 3, 20), False),    # upsampled rows, downsampled columns
])
def test_torch_reference_matches_f64(side, H, box, flip):
    img = _img(side, seed=side + H)
    got = augment_imagenet_with(torch.from_numpy(img)[None], [list(box)], [flip], H)[0].numpy()
    ref = resample_f64(img, box, flip, H)
    assert got.shape == (H, H, 3) and got.dtype == np.float32
    # fp32 interpolation of values up to 255: a few ulp of 255 (2^-16 each) on weights and sums
    assert np.abs(got - ref).max() < 2e-4


def test_constructions_of_the_gpu_test():
    # S = 16, H = 14: the evaluation crop is the 14 x 14 centre, every weight exactly 0 or 1
    img = _img(16, 3)
    ref = resample_f64(img, imagenet_eval_box(16), False, 14)
    mean = np.array(IMAGENET_MEAN, dtype=np.float32).astype(np.float64)
    assert np.array_equal(ref, img[1:15, 1:15].astype(np.float64) - mean)
    # S = 32, H = 14: the crop is 28 = 2 H, positions 2 o + 1/2: every weight exactly 1/2, the value is the mean of
    # a 2 x 2 cell; in fp32 all of it is exact until the one rounding of (sum / 4 - mean)
    img = _img(32, 4)
    ref = resample_f64(img, imagenet_eval_box(32), False, 14)
    cell = img[2:30, 2:30].astype(np.float64).reshape(14, 2, 14, 2, 3).sum(axis=(1, 3)) / 4.0
    assert np.array_equal(ref, cell - mean)
    r32 = resample_f64(img, imagenet_eval_box(32), False, 14, dtype=np.float32)
    assert np.array_equal(r32, (cell.astype(np.float32) - np.array(IMAGENET_MEAN, dtype=np.float32)))
    # the learnable set: uint8, square, labelled, and separable by class means (so it can be learned)
    trx, tr_y, tex, te_y = datasets.learnable_imagenet(n_train=64, n_test=16, side=24, num_classes=4, seed=2)
    assert trx.shape == (64, 24, 24, 3) and trx.dtype == np.uint8 and tex.shape == (16, 24, 24, 3)
    assert tr_y.dtype == np.int64 and set(tr_y.tolist()) <= set(range(4)) and 20 < trx.std() < 110
    protos = np.stack([trx[tr_y == c].astype(np.float64).mean(axis=0) for c in range(4)])
    # nearest class prototype under a random-resized crop of both (the same box): far above chance (1/4)
    boxes, _ = imagenet_augment_params(3, 1, 16, 24)
    hit = 0
    for i in range(16):
        y0, x0, h, w = boxes[i]
        d = [np.abs(tex[i, y0:y0 + h, x0:x0 + w].astype(np.float64) - p[y0:y0 + h, x0:x0 + w]).mean() for p in protos]
        hit += int(np.argmin(d) == te_y[i])
    assert hit >= 12


# ------------------------------------------------------------------------------------------------------- model
def _hp():
    return {"opt_case": {"optimizer": "Momentum", "lr": 0.01, "momentum": 0.9}, "batch_size": 4,
            "regularizer": "l2_regularizer", "weight_decay": 1e-4, "initializer": "he_init", "decay_steps": 0,
            "decay_rate": 1.0}


def _model(tmp_path, **kw):
    from distributedtf_amd.models.imagenet_model import ImageNetModel
    return ImageNetModel(0, _hp(), str(tmp_path / "save" / "model_"), seed=1, resnet_size=50, image_size=32,
                         device="cpu", backend="torch", checkpoint_every_round=False, capacity=1, **kw)


@pytest.fixture
def fresh_engines():
    from distributedtf_amd.models.engine_model import EngineModel
    EngineModel.reset_engines()
    yield
    EngineModel.reset_engines()


def test_model_reads_arrays(tmp_path, fresh_engines):
    d = tmp_path / "data"
    d.mkdir()
    a = _write(d, n=12, nv=6, s=37)
    m = _model(tmp_path, data_dir=str(d))
    ds = m.make_dataset("cpu")
    assert isinstance(ds, datasets.DeviceDataset) and ds.imagenet and not ds.hip_augment and ds.out_size == 32
    assert np.array_equal(ds.train_x.numpy(), a["train_images"]) and ds.num_train == 12
    assert np.array_equal(ds.test_y.numpy(), a["val_labels"].astype(np.int64))
    assert m.num_classes == int(a["train_labels"].max()) + 1  # follows the labels: the caller set none
    assert m.steps_per_epoch() == 3  # 12 images / batch 4
    x, y = ds.batch(torch.tensor([3, 0, 3]))
    assert x.shape == (3, 32, 32, 3) and x.dtype == torch.float32 and y.tolist() == [int(a["train_labels"][i])
                                                                                     for i in (3, 0, 3)]
    boxes, flip = imagenet_augment_params(ds.rng_seed, ds.rng_counter, 3, 37)
    assert np.abs(x[1].numpy() - resample_f64(a["train_images"][0], boxes[1], flip[1], 32)).max() < 2e-4
    ex, ey = ds.eval_set()
    assert ex.shape == (6, 32, 32, 3) and ds.eval_set()[0] is ex
    assert np.abs(ex[2].numpy() - resample_f64(a["val_images"][2], imagenet_eval_box(37), False, 32)).max() < 2e-4
    m.release()


def test_model_num_classes_kept_when_set(tmp_path, fresh_engines):
    d = tmp_path / "data"
    d.mkdir()
    _write(d, n=12, nv=6, s=37)
    m = _model(tmp_path, data_dir=str(d), num_classes=9)
    assert m.num_classes == 9 and isinstance(m.make_dataset("cpu"), datasets.DeviceDataset)
    m.release()
    with pytest.raises(ValueError, match="classes"):
        _model(tmp_path, data_dir=str(d), num_classes=2).make_dataset("cpu")


def test_model_learnable_and_synthetic(tmp_path, fresh_engines):
    m = _model(tmp_path, use_synthetic_data="learnable")
    ds = m.make_dataset("cpu")
    assert isinstance(ds, datasets.DeviceDataset) and ds.imagenet and ds.train_x.dtype == torch.uint8
    assert tuple(ds.train_x.shape[1:]) == (36, 36, 3) and imagenet_eval_box(36)[2] == 32
    assert m.num_classes == 10 and int(ds.train_y.max()) < 10
    assert m.steps_per_epoch() == ds.num_train // 4
    m.release()
    from distributedtf_amd.models.imagenet_model import IMAGENET_NUM_TRAIN
    for kw in (dict(), dict(use_synthetic_data=True), dict(data_dir=str(tmp_path))):  # no arrays: as before
        s = _model(tmp_path, **kw)
        sd = s.make_dataset("cpu")
        assert isinstance(sd, datasets.SyntheticDataset) and tuple(sd.x.shape[1:]) == (32, 32, 3)
        assert s.num_classes == 1001 and s.steps_per_epoch() == IMAGENET_NUM_TRAIN // 4
        s.release()
