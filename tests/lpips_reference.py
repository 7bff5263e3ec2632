"""Float64 restatement of the reference's LPIPS (modeling/modules/lpips.py) for the tests, and the case tables of tests/golden/lpips.npz.

``lpips64(..., model=False)`` (`exact`): scaling layer ((2x - 1) - shift) / scale, thirteen 3x3 convolutions (zero padding 1) + bias + ReLU and four
2x2 max-pools in torchvision's VGG16-D order, taps after relu1_2 / 2_2 / 3_3 / 4_3 / 5_3, x / (sqrt(sum_c x^2) + 1e-10), sum_c w_c d_c^2, spatial
mean, summed over the taps -- all in float64 (tests/test_lpips_cpu.py holds it to the recorded float64 run of the reference itself).

``model=True``: the same with the HIP engine's documented roundings and nothing else: convolution weights rounded to fp16, the scaled input and
every stored activation rounded to fp16 (saturating at +-65504), arithmetic still float64.  |model - exact| is E_model, the unit of the GPU bounds.
"""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from convnet_reference import h16r
from maskbit_amd.synth import VGG16_CONVS, make_eval_images, make_vgg16_weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips.npz")
POOL_BEFORE = (5, 10, 17, 24)
TAP_AFTER = (2, 7, 14, 21, 28)
TAP_CHANNELS = (64, 128, 256, 512, 512)
VGG_SEED = 4100
SHIFT = (-0.030, -0.088, -0.188)          # ScalingLayer buffers (lpips.py:58-59)
SCALE = (0.458, 0.448, 0.450)

# name -> (family, err_sigma, B, H, W, image seed, weight style)
RESTATEMENT_CASES = {
    "he_64": ("noise", 0.05, 3, 64, 64, 4200, "he"),
    "grown_64": ("sin", 0.003, 3, 64, 64, 4201, "grown"),
    "he_37x50": ("bright", 0.003, 3, 37, 50, 4202, "he"),
    "grown_37x50": ("noise", 0.05, 3, 37, 50, 4203, "grown"),
}
ENGINE_CASES = {}
for _s, _style in enumerate(("he", "grown")):
    for _j, (_B, _H, _W) in enumerate(((2, 128, 256), (1, 256, 256))):
        for _k, _sig in enumerate((0.003, 0.05)):
            ENGINE_CASES[f"{_style}_{_H}x{_W}_{'lo' if _k == 0 else 'hi'}"] = ("noise", _sig, _B, _H, _W, 4300 + 100 * _s + 10 * _j + _k, _style)
CASES = {**RESTATEMENT_CASES, **ENGINE_CASES}


def scaling_buffers():
    return torch.tensor(SHIFT, dtype=torch.float32), torch.tensor(SCALE, dtype=torch.float32)


def vgg_taps64(x, vgg, model):
    """x float64 [N, 3, H, W] (scaled) -> the five taps, float64 NCHW"""
    taps = []
    h = h16r(x) if model else x
    for idx, _cin, _cout in VGG16_CONVS:
        if idx in POOL_BEFORE:
            h = F.max_pool2d(h, 2, 2)
        w = vgg[f"{idx}.weight"]
        w = w.to(torch.float16).double() if model else w.double()
        h = F.relu(F.conv2d(h, w, vgg[f"{idx}.bias"].double(), padding=1))
        if model:
            h = h16r(h)
        if idx in TAP_AFTER:
            taps.append(h)
    return taps


def distance64(a, b, w):
    """taps a, b float64 [B, C, h, w], w [C] -> [B]: spatial mean of sum_c w_c (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2"""
    na = a.pow(2).sum(1, keepdim=True).sqrt() + 1e-10
    nb = b.pow(2).sum(1, keepdim=True).sqrt() + 1e-10
    d = (a / na - b / nb).pow(2)
    return (d * w.double().view(1, -1, 1, 1)).sum(1).mean((1, 2))


def lpips64(real, fake, vgg, lins, model=False, clamp=False, return_taps=False):
    """-> float64 [B] (and the taps of the 2B images, real first)"""
    shift, scale = scaling_buffers()
    x = torch.cat([real, fake]).double()
    if clamp:
        x = x.clamp(0.0, 1.0)
    x = ((x * 2.0 - 1.0) - shift.double().view(1, 3, 1, 1)) / scale.double().view(1, 3, 1, 1)
    taps = vgg_taps64(x, vgg, model)
    B = real.shape[0]
    val = sum(distance64(t[:B], t[B:], torch.as_tensor(lins[k])) for k, t in enumerate(taps))
    return (val, taps) if return_taps else val


def golden():
    return np.load(GOLDEN)


def lin_vectors(z=None):
    z = golden() if z is None else z
    return [torch.from_numpy(z[f"lin{k}"].astype(np.float32)) for k in range(5)]


@functools.lru_cache(maxsize=None)
def vgg_weights(style):
    return make_vgg16_weights(VGG_SEED, style)


def case_images(name):
    fam, sig, B, H, W, seed, _style = CASES[name]
    return make_eval_images(fam, sig, B, H, W, seed)


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    """-> dict(exact [B], model [B], exact_taps, model_taps): computed once per case and shared (do not modify)"""
    real, fake = case_images(name)
    vgg, lins = vgg_weights(CASES[name][6]), lin_vectors()
    with torch.no_grad():
        exact, et = lpips64(real, fake, vgg, lins, model=False, return_taps=True)
        mod, mt = lpips64(real, fake, vgg, lins, model=True, return_taps=True)
    return dict(exact=exact, model=mod, exact_taps=et, model_taps=mt)


def reference_state_dict(vgg, lins, use_dropout=True):
    """the 33 entries of the reference's LPIPS state dict from bare VGG16 keys and the five lin vectors"""
    shift, scale = scaling_buffers()
    sd = {"scaling_layer.shift": shift.view(1, 3, 1, 1), "scaling_layer.scale": scale.view(1, 3, 1, 1)}
    bounds = (4, 9, 16, 23, 30)
    for idx, _cin, _cout in VGG16_CONVS:
        k = next(i for i, b in enumerate(bounds) if idx < b) + 1
        sd[f"net.slice{k}.{idx}.weight"], sd[f"net.slice{k}.{idx}.bias"] = vgg[f"{idx}.weight"], vgg[f"{idx}.bias"]
    for k in range(5):
        sd[f"lin{k}.model.{1 if use_dropout else 0}.weight"] = torch.as_tensor(lins[k]).float().view(1, -1, 1, 1)
    return sd
