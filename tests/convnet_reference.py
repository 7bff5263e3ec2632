"""What the float64 restatements of the feature networks (inception_reference.py, resnet_reference.py, lpips_reference.py) share: the fp16
rounding of the engines' stores, BatchNorm on running statistics as a scale and a shift, and one convolution + BatchNorm step."""
import torch
import torch.nn.functional as F


def h16r(t):
    """fp64 -> fp16 (nearest even, saturating at the fp16 range as the engine's stores do) -> fp64"""
    return t.clamp(-65504.0, 65504.0).to(torch.float16).double()


def bn_scale_shift(sd, prefix, eps, dtype=torch.float64):
    g, b = sd[prefix + ".weight"].to(dtype), sd[prefix + ".bias"].to(dtype)
    m, v = sd[prefix + ".running_mean"].to(dtype), sd[prefix + ".running_var"].to(dtype)
    scale = g / torch.sqrt(v + eps)
    return scale, b - m * scale


class Net:
    """one forward: the layers as methods on the state dict, `model` = with the engine's roundings"""

    def __init__(self, sd, model, eps, dtype=torch.float64):
        self.sd, self.model, self.eps, self.dtype = sd, model, eps, dtype

    def store(self, t):
        return h16r(t) if self.model else t

    def convbn(self, x, conv, bn, stride=1, padding=0):
        """the convolution `conv`.weight (no bias) and the BatchNorm `bn`.*, before any epilogue and unrounded"""
        w = self.sd[conv + ".weight"]
        w = w.to(torch.float16).to(self.dtype) if self.model else w.to(self.dtype)
        scale, shift = bn_scale_shift(self.sd, bn, self.eps, self.dtype)
        return F.conv2d(x, w, None, stride, padding) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
