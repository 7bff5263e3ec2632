"""A float64 restatement of the VQGAN+ discriminator's graph (DESIGN.md "Discriminator"), written from its description: what the tests of
maskbit_amd/csrc/discriminator.hip compare against.  ``forward64(..., emulate=True)`` is the same graph with fp16 rounding applied exactly where
the engine rounds (input, convolution weights, every stored map) and float64 everywhere the engine accumulates in fp32: its distance from the
plain float64 graph is what fp16 storage costs, whatever the order of the fp32 sums.
"""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

SLOPE = 0.1
GN_EPS = 1e-5
GROUPS = 32
SIDE = 16
BINOMIAL = {3: (1, 2, 1), 4: (1, 3, 3, 1), 5: (1, 4, 6, 4, 1)}


def h16(x: torch.Tensor) -> torch.Tensor:
    """round to fp16 (saturating at 65504, as the engine's stores do) and back to float64"""
    return x.clamp(-65504.0, 65504.0).to(torch.float16).double()


def blur_pad(n: int, k: int) -> Tuple[int, int]:
    """(front, back) zero padding of one axis of BlurBlock: the total max((ceil(n / 2) - 1) * 2 + k - n, 0), half of it rounded down in front"""
    pad = max((math.ceil(n / 2) - 1) * 2 + k - n, 0)
    return pad // 2, pad - pad // 2


def blur_kernel64(k: int) -> torch.Tensor:
    row = torch.tensor(BINOMIAL[k], dtype=torch.float64)
    w = row[:, None] * row[None, :]
    return w / w.sum()


def downsample64(x: torch.Tensor, k: int) -> torch.Tensor:
    """x float64 [B, C, H, W]; k = 3, 4, 5: the binomial blur with stride 2 and 'same' zero padding; k = 0: the 2 x 2 mean with stride 2"""
    B, C, H, W = x.shape
    if k == 0:
        Ho, Wo = H // 2, W // 2
        x = x[:, :, :2 * Ho, :2 * Wo]
        return 0.25 * (x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2] + x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2])
    (t, b), (l, r) = blur_pad(H, k), blur_pad(W, k)
    xp = F.pad(x, (l, r, t, b))
    Ho, Wo = (H + t + b - k) // 2 + 1, (W + l + r - k) // 2 + 1
    w = blur_kernel64(k)
    out = torch.zeros(B, C, Ho, Wo, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            out += w[ky, kx] * xp[:, :, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2]
    return out


def pool_windows(n: int) -> List[Tuple[int, int]]:
    """the 16 windows [floor(i n / 16), ceil((i + 1) n / 16)) of an axis of n"""
    return [(i * n // SIDE, -((-(i + 1) * n) // SIDE)) for i in range(SIDE)]


def adaptive_maxpool64(x: torch.Tensor) -> torch.Tensor:
    B, C, H, W = x.shape
    out = torch.empty(B, C, SIDE, SIDE, dtype=x.dtype)
    for i, (y0, y1) in enumerate(pool_windows(H)):
        for j, (x0, x1) in enumerate(pool_windows(W)):
            out[:, :, i, j] = x[:, :, y0:y1, x0:x1].amax(dim=(2, 3))
    return out


def leaky(x: torch.Tensor, slope: float = SLOPE) -> torch.Tensor:
    return torch.where(x >= 0, x, x * slope)


def conv_same(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """odd square kernel, stride 1, zero padding (k - 1) / 2"""
    return F.conv2d(x, w, b, padding=w.shape[-1] // 2)


def group_stats(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [B, C, H, W] -> per (image, group) the mean and the biased variance, float64 [B, 32]"""
    B, C = x.shape[:2]
    g = x.reshape(B, GROUPS, -1)
    return g.mean(2), g.var(2, unbiased=False)


def groupnorm_leaky64(x: torch.Tensor, mean: torch.Tensor, var: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = GN_EPS,
                      slope: float = SLOPE, emulate: bool = False) -> torch.Tensor:
    B, C = x.shape[:2]
    cpg = C // GROUPS
    m = mean.repeat_interleave(cpg, dim=1)[:, :, None, None]
    rstd = (1.0 / torch.sqrt(var + eps)).repeat_interleave(cpg, dim=1)[:, :, None, None]
    if emulate:                                  # the engine keeps mean, rstd, scale and shift in fp32
        m, rstd = m.float().double(), rstd.float().double()
        sc = (rstd * gamma[None, :, None, None]).float().double()
        sh = (beta[None, :, None, None] - (m * sc).float().double()).float().double()
        return leaky(x * sc + sh, slope)
    return leaky((x - m) * rstd * gamma[None, :, None, None] + beta[None, :, None, None], slope)


def num_stages(sd: Dict[str, torch.Tensor]) -> int:
    return len([k for k in sd if k.startswith("blocks.") and k.endswith(".0.weight")])


def forward64(sd: Dict[str, torch.Tensor], x: torch.Tensor, blur: int, emulate: bool = False) -> torch.Tensor:
    """the logits float64 [B, 1, 16, 16] of images x [B, 3, H, W]; blur = 3, 4, 5 or 0 (average pool)"""
    store = h16 if emulate else (lambda t: t)
    wq = h16 if emulate else (lambda t: t)       # the MFMA convolutions' weights are fp16; biases, GroupNorm and to_logits.2 stay fp32
    p = {k: v.double() for k, v in sd.items()}
    a = store(x.double())
    a = store(leaky(conv_same(a, wq(p["block_in.0.weight"]), p["block_in.0.bias"])))
    for i in range(num_stages(sd)):
        a = store(conv_same(a, wq(p[f"blocks.{i}.0.weight"]), p[f"blocks.{i}.0.bias"]))
        d = downsample64(a, blur)
        mean, var = group_stats(d)               # of the values before they are stored
        a = store(groupnorm_leaky64(store(d), mean, var, p[f"blocks.{i}.2.weight"], p[f"blocks.{i}.2.bias"], emulate=emulate))
    a = adaptive_maxpool64(a)
    a = store(leaky(conv_same(a, wq(p["to_logits.0.weight"]), p["to_logits.0.bias"])))
    return conv_same(a, p["to_logits.2.weight"], p["to_logits.2.bias"])


def softplus64(x: torch.Tensor) -> torch.Tensor:
    return x.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))


def stats64(logits: torch.Tensor) -> torch.Tensor:
    """logits [B, ...] -> float64 [B, 5]: per image the sums of l, relu(1 - l), relu(1 + l), softplus(-l), softplus(l)"""
    l = logits.double().reshape(logits.shape[0], -1)
    return torch.stack([l.sum(1), (1 - l).clamp(min=0).sum(1), (1 + l).clamp(min=0).sum(1), softplus64(-l).sum(1), softplus64(l).sum(1)], 1)


def losses64(real: torch.Tensor, fake: torch.Tensor) -> Dict[str, float]:
    """the five GAN losses on float64 logits, from their formulas: hinge / vanilla / non-saturating discriminator, hinge / non-saturating generator"""
    real, fake = real.double(), fake.double()
    return dict(
        hinge_d=float(0.5 * ((1 - real).clamp(min=0).mean() + (1 + fake).clamp(min=0).mean())),
        vanilla_d=float(0.5 * (softplus64(-real).mean() + softplus64(fake).mean())),
        non_saturating_d=float(softplus64(-real).mean() + softplus64(fake).mean()),      # -log sigmoid(real) - log(1 - sigmoid(fake))
        hinge_g=float(-fake.mean()),
        non_saturating_g=float(softplus64(-fake).mean()))


def lecam64(real_mean: float, fake_mean: float, ema_real: float, ema_fake: float) -> float:
    return max(real_mean - ema_fake, 0.0) ** 2 + max(ema_real - fake_mean, 0.0) ** 2
