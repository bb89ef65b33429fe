"""ImageNet-shape ResNet population member (BASELINE config 5, SURVEY.md C12').

The reference's ResNet library supports bottleneck blocks and the first max-pool
(``resnet/resnet_model.py:215-320,487-529``) but ships no ImageNet entry point;
this family defines the upstream-standard config (7x7/2 stem, 3x3/2 max-pool,
[3,4,6,3] bottleneck stages, 2048 final) on 224x224x3 inputs.
LR: ``lr * B/256`` piecewise schedule with the same decay_steps/decay_rate rule
as the CIFAR family over the training set (1.28M images for synthetic data).

Data: pre-decoded uint8 arrays under ``data_dir`` (``datasets.load_imagenet_arrays``:
``train_images.npy`` [N, S, S, 3], ``train_labels.npy``, ``val_images.npy``,
``val_labels.npy``) resident on the device, cropped / resampled / flipped by the
HIP input kernel inside the step graph (data.hip); ``use_synthetic_data="learnable"``
is a class-template set through the same path; otherwise a fixed synthetic batch.
``imagenet_data="host"`` keeps the training images on the host instead and stages
every step's rows (``datasets.HostImageNetDataset``).
"""

from __future__ import annotations

import numpy as np
import torch

from .cifar10_model import Cifar10Model
from .resnet import ResNetArch, imagenet_config
from ..data import datasets
from ..engine import schedule

IMAGENET_NUM_TRAIN = 1281167
IMAGENET_NUM_CLASSES = 1001
LEARNABLE_NUM_CLASSES = 10


def _upload(arr, device, dtype, rows=1024):
    """A (memory-mapped) numpy array -> device tensor, ``rows`` rows at a time (the host never holds it whole)."""
    out = torch.empty(tuple(arr.shape), dtype=dtype, device=device)
    for i in range(0, arr.shape[0], rows):
        out[i:i + rows].copy_(torch.from_numpy(np.array(arr[i:i + rows])))
    return out


class ImageNetModel(Cifar10Model):
    def __init__(self, cluster_id, hparams, save_base_dir, seed=None, resnet_size=50, image_size=224,
                 num_classes=None, data_dir=None, use_synthetic_data=None, imagenet_data="device", **kw):
        self.image_size = int(image_size)
        if imagenet_data not in ("device", "host"):
            raise ValueError("imagenet_data must be device or host, not %r" % (imagenet_data,))
        self.imagenet_data = imagenet_data  # --imagenet_data: where the training images live
        if self.image_size < 32 or self.image_size % 32:
            raise ValueError("image_size must be a positive multiple of 32, not %d" % self.image_size)
        self._real = use_synthetic_data in (None, False) and datasets.imagenet_arrays_available(data_dir)
        self._learnable = use_synthetic_data == "learnable"
        if num_classes is None:  # not set by the caller: the labels' range for real / learnable data
            if self._real:
                labels = datasets.load_imagenet_arrays(data_dir)[1]  # validated: errors name the file
                num_classes = int(labels.max()) + 1
            else:
                num_classes = LEARNABLE_NUM_CLASSES if self._learnable else IMAGENET_NUM_CLASSES
        self.num_classes = int(num_classes)
        super().__init__(cluster_id, hparams, save_base_dir, seed=seed, resnet_size=resnet_size, data_dir=data_dir,
                         use_synthetic_data=use_synthetic_data, **kw)

    def make_arch(self):
        return ResNetArch(imagenet_config(self.resnet_size, self.resnet_version, self.num_classes, self.image_size))

    def make_dataset(self, device):
        H = self.image_size
        kw = dict(augment=datasets.augment_imagenet, eval_transform=datasets.eval_imagenet, out_size=H)
        host = self.imagenet_data == "host"
        if host and not (self._real or self._learnable):
            raise ValueError("imagenet_data=host needs the ImageNet arrays under data_dir or "
                             "use_synthetic_data='learnable'")
        if self._real:
            # staging is sized by the largest step: every slot of the engine at the largest batch size explore allows
            # (256), or this member's if --batch_size pins a larger one
            rows = self.engine.capacity * max(256, int(self.hparams["batch_size"]))
            trx, tr_y, vax, va_y = datasets.load_imagenet_arrays(self.data_dir, device, out_size=H, resident=not host,
                                                                 stage_rows=rows)
            hi = max(int(tr_y.max()), int(va_y.max()))
            if int(tr_y.min()) < 0 or hi >= self.num_classes:
                raise ValueError("%s: labels span 0..%d but the model has %d classes"
                                 % (self.data_dir, hi, self.num_classes))
            if host:  # the training images stay in the memory-mapped file; everything else as the resident set
                return datasets.HostImageNetDataset(trx, np.array(tr_y, dtype=np.int64),
                                                    _upload(vax, device, torch.uint8),
                                                    np.array(va_y, dtype=np.int64), device, out_size=H)
            return datasets.DeviceDataset(_upload(trx, device, torch.uint8), np.array(tr_y, dtype=np.int64),
                                          _upload(vax, device, torch.uint8), np.array(va_y, dtype=np.int64),
                                          device, **kw)
        if self._learnable:
            # class-template images through the real input path (--use_synthetic_data learnable): stored at the side
            # whose evaluation crop (0.875 S) is the model's input size, as 256 is for 224
            on_gpu = torch.device(device).type == "cuda"
            side = (8 * H + 2) // 7
            trx, tr_y, tex, te_y = datasets.learnable_imagenet(n_train=8000 if on_gpu else 256,
                                                               n_test=1000 if on_gpu else 64, side=side,
                                                               num_classes=min(self.num_classes, LEARNABLE_NUM_CLASSES))
            if host:  # the same set, kept as a numpy array on the host
                return datasets.HostImageNetDataset(trx, tr_y, tex, te_y, device, out_size=H)
            return datasets.DeviceDataset(trx, tr_y, tex, te_y, device, **kw)
        return datasets.SyntheticDataset((H, H, 3), self.num_classes, device, max_batch=256, n_eval=256)

    def dataset(self):
        """One dataset per (device, source, input size, classes): members of one population share it."""
        key = (type(self).__name__, str(self.device), self.data_dir, self.use_synthetic_data, self.image_size,
               self.num_classes) + (("host",) if self.imagenet_data == "host" else ())
        ds = Cifar10Model._datasets.get(key)
        if ds is None:
            ds = Cifar10Model._datasets[key] = self.make_dataset(self.device)
        return ds

    def _num_train(self):
        """Images per epoch: the dataset's own count for real / learnable data, ImageNet's for the synthetic batch."""
        if self._real or self._learnable:
            return int(self.dataset().num_train)
        return IMAGENET_NUM_TRAIN

    def learning_rate(self, step):
        b, v = schedule.cifar_boundaries(self.hparams, num_images=self._num_train(), batch_denom=256,
                                         total_epochs=90.0)
        return schedule.piecewise_constant(step, b, v)

    def steps_per_epoch(self):
        return max(1, int(self._num_train() / int(self.hparams["batch_size"])))
