"""A numpy restatement of Pillow's antialiased resize (ImagingResample, 8 bits per channel) for BOX / BILINEAR / BICUBIC, of the two loader
recipes built on it, and the case builders shared by tests/test_image_transform_cpu.py and tests/test_hip_image_transform.py.

The arithmetic (Pillow's libImaging/Resample.c, restated; Pillow is the arbiter -- the CPU test compares this file with it byte for byte where it
is installed, and with tests/golden/image_transform.npz everywhere):
  * separable, HORIZONTAL first; the horizontal pass writes a uint8 image that the vertical pass reads; an axis whose size does not change is
    skipped;
  * per axis, in IEEE double with no fused multiply-add (numpy float64 scalars never fuse):  scale = in / out, fs = max(scale, 1),
    support = s * fs, ksize = (int)ceil(support) * 2 + 1;  for output xx: center = (xx + 0.5) * scale, xmin = max((int)(center - support + 0.5), 0),
    n = min((int)(center + support + 0.5), in) - xmin, w[x] = f((x + xmin - center + 0.5) * (1 / fs)), normalised by their sum in ascending x;
  * fixed point: k = (int)(w * 2^22 +- 0.5) with C truncation; output = clip((2^21 + sum pixel * k) >> 22) with an arithmetic shift.
Nothing here reads the code under test.
"""
import math

import numpy as np

BOX, BILINEAR, BICUBIC = 0, 1, 2
FILTER_NAMES = {BOX: "box", BILINEAR: "bilinear", BICUBIC: "bicubic"}
FILTERS_BY_NAME = {v: k for k, v in FILTER_NAMES.items()}
SUPPORT = {BOX: 0.5, BILINEAR: 1.0, BICUBIC: 2.0}
PRECISION_BITS = 22
F64 = np.float64


def _box(x):
    return F64(1.0) if (x > -0.5 and x <= 0.5) else F64(0.0)


def _bilinear(x):
    x = abs(x)
    return F64(1.0) - x if x < 1.0 else F64(0.0)


def _bicubic(x):
    a = F64(-0.5)
    x = abs(x)
    if x < 1.0:
        return ((a + F64(2.0)) * x - (a + F64(3.0))) * x * x + F64(1.0)
    if x < 2.0:
        return (((x - F64(5.0)) * x + F64(8.0)) * x - F64(4.0)) * a
    return F64(0.0)


_FILTERS = {BOX: _box, BILINEAR: _bilinear, BICUBIC: _bicubic}


def ksize_for(in_size, out_size, filt):
    scale = F64(in_size) / F64(out_size)
    fs = scale if scale > 1.0 else F64(1.0)
    return int(math.ceil(F64(SUPPORT[filt]) * fs)) * 2 + 1


def coeffs(in_size, out_size, filt):
    """-> (xmin int32 [out], n int32 [out], k int32 [out, ksize]) of one axis; taps beyond n are 0."""
    f = _FILTERS[filt]
    scale = F64(in_size) / F64(out_size)
    fs = scale if scale > 1.0 else F64(1.0)
    support = F64(SUPPORT[filt]) * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = F64(1.0) / fs
    xmins = np.zeros(out_size, np.int32)
    ns = np.zeros(out_size, np.int32)
    ks = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (F64(xx) + F64(0.5)) * scale
        xmin = max(int(center - support + F64(0.5)), 0)            # int(): C truncation
        xmax = min(int(center + support + F64(0.5)), in_size) - xmin
        w = [f((F64(x) + F64(xmin) - center + F64(0.5)) * ss) for x in range(xmax)]
        ww = F64(0.0)
        for v in w:
            ww = ww + v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            ks[xx, x] = int(v * F64(1 << PRECISION_BITS) - F64(0.5)) if v < 0 else int(v * F64(1 << PRECISION_BITS) + F64(0.5))
        xmins[xx], ns[xx] = xmin, xmax
    return xmins, ns, ks


def identity_coeffs(size):
    """The table of a skipped axis: one tap of weight 1 -- (2^21 + p 2^22) >> 22 = p."""
    return np.arange(size, dtype=np.int32), np.ones(size, np.int32), np.full((size, 1), 1 << PRECISION_BITS, np.int32)


def _pass(img, xmins, ns, ks, axis, clip_seen=None):
    """One pass along `axis` (0 rows, 1 columns) of a uint8 [H, W, C] image -> uint8."""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((len(xmins),) + src.shape[1:], np.int64)
    for i in range(len(xmins)):
        a, n = int(xmins[i]), int(ns[i])
        out[i] = (1 << (PRECISION_BITS - 1)) + np.tensordot(ks[i, :n].astype(np.int64), src[a:a + n], axes=(0, 0))
    assert np.abs(out).max() < 2 ** 31
    out >>= PRECISION_BITS                                          # arithmetic shift
    if clip_seen is not None and ((out < 0).any() or (out > 255).any()):
        clip_seen.append(axis)
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis)


def resize(img, out_h, out_w, filt, clip_seen=None, vertical_first=False):
    """uint8 [H, W, C] -> uint8 [out_h, out_w, C] as PIL.Image.resize((out_w, out_h), filt) gives it.  `vertical_first` is the WRONG order, kept
    so that a test can show it is told apart."""
    img = np.ascontiguousarray(img)
    H, W = img.shape[:2]
    steps = [(1, W, out_w), (0, H, out_h)]
    for axis, n_in, n_out in (steps[::-1] if vertical_first else steps):
        if n_in != n_out:
            img = _pass(img, *coeffs(n_in, n_out, filt), axis, clip_seen)
    return img


FLOAT_TABLE = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)       # ToTensor(): uint8 -> float32, .div(255)


def to_float_nchw(u8_hwc):
    return np.ascontiguousarray(FLOAT_TABLE[u8_hwc].transpose(2, 0, 1))


# ---- the two recipes: host arithmetic on sizes only ------------------------------------------------------------------------------------
def reference_sizes(H, W, R):
    """torchvision Resize(R) + CenterCrop(R) on a PIL image -> ((res_h, res_w), (top, left))."""
    if W <= H:
        res_w, res_h = R, int(R * H / W)
    else:
        res_h, res_w = R, int(R * W / H)
    return (res_h, res_w), (int(round((res_h - R) / 2.0)), int(round((res_w - R) / 2.0)))


def adm_sizes(H, W, R):
    """guided-diffusion's center_crop_arr -> (list of BOX halvings [(h, w), ...], (res_h, res_w), (top, left))."""
    halvings = []
    while min(H, W) >= 2 * R:
        H, W = H // 2, W // 2
        halvings.append((H, W))
    scale = R / min(H, W)
    res_h, res_w = round(H * scale), round(W * scale)
    return halvings, (res_h, res_w), ((res_h - R) // 2, (res_w - R) // 2)


def reference_transform(img, R, filt):
    (rh, rw), (top, left) = reference_sizes(img.shape[0], img.shape[1], R)
    return resize(img, rh, rw, filt)[top:top + R, left:left + R]


def adm_transform(img, R):
    halvings, (rh, rw), (top, left) = adm_sizes(img.shape[0], img.shape[1], R)
    for h, w in halvings:
        img = resize(img, h, w, BOX)
    return resize(img, rh, rw, BICUBIC)[top:top + R, left:left + R]


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
SIZE_CASES = [((37, 53), (16, 23)), ((53, 37), (23, 16)), ((16, 16), (16, 16)), ((16, 40), (16, 16)), ((9, 7), (32, 25)), ((100, 67), (16, 11)),
              ((33, 200), (16, 97)), ((5, 5), (16, 16)), ((17, 16), (16, 15)), ((1, 7), (16, 16)), ((7, 1), (16, 16)), ((1, 1), (16, 16)),
              ((300, 3), (16, 16))]
CONTENTS = ("random", "checker")


def make_image(H, W, content, seed=0):
    if content == "checker":
        yy, xx = np.mgrid[0:H, 0:W]
        return np.ascontiguousarray(np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2))
    rng = np.random.default_rng(1000 * H + W + 7919 * seed)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def ragged_batch(seed=3):
    """Eight sources of differing sizes and orientations, one with a side equal to 16 and 32, two that "adm" halves once and twice at R = 16."""
    sizes = [(37, 53), (53, 37), (16, 40), (32, 32), (70, 45), (131, 64), (9, 7), (20, 33)]
    return [make_image(h, w, "random", seed + i) for i, (h, w) in enumerate(sizes)]
