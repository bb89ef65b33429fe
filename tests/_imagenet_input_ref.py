"""The ImageNet input kernel's resample written out with explicit taps and weights (numpy, any float type): the
float64 reference of tests/test_imagenet_input.py and tests/test_gpu_imagenet_input.py."""
import numpy as np

from distributedtf_amd.data.datasets import IMAGENET_MEAN


def resample_f64(img_u8, box, flip, H, dtype=np.float64):
    """The kernel's formula with explicit taps and weights, evaluated in ``dtype``: position relative to the box
    origin ((2 o + 1) crop - H) / (2 H) clamped to [0, crop - 1], taps i and min(i + 1, crop - 1)."""
    y0, x0, bh, bw = (int(v) for v in box)
    img = np.asarray(img_u8).astype(dtype)
    mean = np.array(IMAGENET_MEAN, dtype=np.float32).astype(dtype)

    def taps(o, crop):
        num = np.clip((2 * o + 1) * crop - H, 0, (crop - 1) * 2 * H)
        q = num.astype(dtype) / dtype(2 * H)
        i = np.floor(q).astype(np.int64)
        return i, np.minimum(i + 1, crop - 1), (q - i.astype(dtype)).astype(dtype)

    o = np.arange(H)
    iy0, iy1, fy = taps(o, bh)
    ix0, ix1, fx = taps(H - 1 - o if flip else o, bw)
    fy, fx = fy[:, None, None], fx[None, :, None]
    one = dtype(1)
    p = lambda iy, ix: img[y0 + iy][:, x0 + ix]  # noqa: E731
    top = (one - fx) * p(iy0, ix0) + fx * p(iy0, ix1)
    bot = (one - fx) * p(iy1, ix0) + fx * p(iy1, ix1)
    return ((one - fy) * top + fy * bot) - mean
