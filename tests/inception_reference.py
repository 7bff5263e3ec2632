"""Float64 restatement of the FID Inception-v3 as DESIGN.md "Inception-v3" specifies it, for the tests, and the case tables.

``inception64(u8, sd, model=False)`` (`exact`): TF1-style bilinear resize to 299 x 299 (source coordinate dst * in / out, no half-pixel offset),
(v - 128) / 128, the 94 ``BasicConv2d`` layers (convolution without bias, BatchNorm on running statistics with eps 1e-3, ReLU), the pools, the
concatenations, the spatial means and the 1008-way head -- all in float64.  ``torch_fidelity`` and the real checkpoint are not available, so
nothing here is held against the real network; tests/test_inception_cpu.py holds the pieces to independent statements instead.

``model=True``: the same with the HIP engine's documented roundings and nothing else: convolution weights, the normalised input and every stored
activation (convolution and average-pool outputs) rounded to fp16, saturating at 65504; arithmetic still float64; the head on the fp32 weights.
|model - exact| is E_model, the unit of the GPU bounds.
"""
import functools

import torch
import torch.nn.functional as F

import convnet_reference
from convnet_reference import h16r  # noqa: F401  (part of this module's surface)
from maskbit_amd.synth import make_eval_images, make_inception_weights

SIDE = 299
BN_EPS = 1e-3
WEIGHT_SEED = 4400
MAP_NAMES = ("MaxPool_2", "Mixed_5d", "Mixed_6e", "Mixed_7c")
MAP_SHAPES = ((35, 192), (35, 288), (17, 768), (8, 2048))

# name -> (B, H, W, image seed, weight style)
CASES = {
    "he_64": (2, 64, 64, 4410, "he"),
    "tf_64": (2, 64, 64, 4411, "tf"),
    "he_256": (2, 256, 256, 4412, "he"),
    "tf_256": (2, 256, 256, 4413, "tf"),
}

# the per-launch convolution cases: name -> (B, H, W, Cin, Cout, (kh, kw), stride, (ph, pw))
CONV_CASES = {
    "3->32 k3 s2 19x19": (2, 19, 19, 3, 32, (3, 3), 2, (0, 0)),
    "32->32 k3 11x13": (2, 11, 13, 32, 32, (3, 3), 1, (0, 0)),
    "64->80 k1 9x7": (2, 9, 7, 64, 80, (1, 1), 1, (0, 0)),
    "80->192 k3 9x9": (2, 9, 9, 80, 192, (3, 3), 1, (0, 0)),
    "48->64 k5 p2 9x9": (2, 9, 9, 48, 64, (5, 5), 1, (2, 2)),
    "128->128 1x7 17x17": (2, 17, 17, 128, 128, (1, 7), 1, (0, 3)),
    "160->192 7x1 17x17": (3, 17, 17, 160, 192, (7, 1), 1, (3, 0)),
    "288->384 k3 s2 9x9": (2, 9, 9, 288, 384, (3, 3), 2, (0, 0)),
    "384->384 1x3 8x8": (2, 8, 8, 384, 384, (1, 3), 1, (0, 1)),
    "384->384 3x1 8x8": (2, 8, 8, 384, 384, (3, 1), 1, (1, 0)),
    "2048->320 k1 8x8": (2, 8, 8, 2048, 320, (1, 1), 1, (0, 0)),
    "448->384 k3 p1 8x8": (2, 8, 8, 448, 384, (3, 3), 1, (1, 1)),
}


def resize64(u8, out=SIDE, dtype=torch.float64):
    """uint8 [B, C, H, W] -> float64 [B, C, out, out]: i0 = floor(dst * in / out), i1 = min(i0 + 1, in - 1), t = dst * in / out - i0 (from the
    integers), v = a0 + (a1 - a0) * t along x for both rows, then along y"""
    x = u8.to(dtype)
    H, W = x.shape[-2:]

    def coords(n):
        d = torch.arange(out, dtype=torch.int64, device=u8.device) * n
        i0 = d // out
        return i0, (i0 + 1).clamp(max=n - 1), (d % out).to(dtype) / out

    y0, y1, ty = coords(H)
    x0, x1, tx = coords(W)

    def along_x(rows):
        a0, a1 = rows[..., x0], rows[..., x1]
        return a0 + (a1 - a0) * tx

    top, bot = along_x(x[..., y0, :]), along_x(x[..., y1, :])
    return top + (bot - top) * ty.view(-1, 1)


def input64(u8, dtype=torch.float64):
    return (resize64(u8, SIDE, dtype) - 128.0) / 128.0


class Net(convnet_reference.Net):
    def __init__(self, sd, model, dtype=torch.float64):
        super().__init__(sd, model, BN_EPS, dtype)
        self.used = []

    def conv(self, x, name, stride=1, padding=0):
        self.used.append(name)
        return self.store(F.relu(self.convbn(x, name + ".conv", name + ".bn", stride, padding)))

    def avg(self, x):
        return self.store(F.avg_pool2d(x, 3, 1, 1, count_include_pad=False))

    def a(self, x, n):
        b1 = self.conv(x, n + ".branch1x1")
        b5 = self.conv(self.conv(x, n + ".branch5x5_1"), n + ".branch5x5_2", padding=2)
        b3 = self.conv(self.conv(self.conv(x, n + ".branch3x3dbl_1"), n + ".branch3x3dbl_2", padding=1), n + ".branch3x3dbl_3", padding=1)
        return torch.cat([b1, b5, b3, self.conv(self.avg(x), n + ".branch_pool")], 1)

    def b(self, x, n):
        b3 = self.conv(x, n + ".branch3x3", stride=2)
        bd = self.conv(self.conv(self.conv(x, n + ".branch3x3dbl_1"), n + ".branch3x3dbl_2", padding=1), n + ".branch3x3dbl_3", stride=2)
        return torch.cat([b3, bd, F.max_pool2d(x, 3, 2)], 1)

    def c(self, x, n):
        b1 = self.conv(x, n + ".branch1x1")
        b7 = self.conv(x, n + ".branch7x7_1")
        b7 = self.conv(b7, n + ".branch7x7_2", padding=(0, 3))
        b7 = self.conv(b7, n + ".branch7x7_3", padding=(3, 0))
        bd = self.conv(x, n + ".branch7x7dbl_1")
        for k, pad in ((2, (3, 0)), (3, (0, 3)), (4, (3, 0)), (5, (0, 3))):
            bd = self.conv(bd, f"{n}.branch7x7dbl_{k}", padding=pad)
        return torch.cat([b1, b7, bd, self.conv(self.avg(x), n + ".branch_pool")], 1)

    def d(self, x, n):
        b3 = self.conv(self.conv(x, n + ".branch3x3_1"), n + ".branch3x3_2", stride=2)
        b7 = self.conv(x, n + ".branch7x7x3_1")
        b7 = self.conv(b7, n + ".branch7x7x3_2", padding=(0, 3))
        b7 = self.conv(b7, n + ".branch7x7x3_3", padding=(3, 0))
        b7 = self.conv(b7, n + ".branch7x7x3_4", stride=2)
        return torch.cat([b3, b7, F.max_pool2d(x, 3, 2)], 1)

    def e(self, x, n, use_max):
        b1 = self.conv(x, n + ".branch1x1")
        b3 = self.conv(x, n + ".branch3x3_1")
        b3 = torch.cat([self.conv(b3, n + ".branch3x3_2a", padding=(0, 1)), self.conv(b3, n + ".branch3x3_2b", padding=(1, 0))], 1)
        bd = self.conv(self.conv(x, n + ".branch3x3dbl_1"), n + ".branch3x3dbl_2", padding=1)
        bd = torch.cat([self.conv(bd, n + ".branch3x3dbl_3a", padding=(0, 1)), self.conv(bd, n + ".branch3x3dbl_3b", padding=(1, 0))], 1)
        pooled = F.max_pool2d(x, 3, 1, 1) if use_max else self.avg(x)
        return torch.cat([b1, b3, bd, self.conv(pooled, n + ".branch_pool")], 1)


def inception64(u8, sd, model=False, dtype=torch.float64):
    """uint8 [B, 3, H, W] -> dict: maps (the four of MAP_NAMES, float64 NCHW), relu (the five ReLU outputs whose zeros the weight conditions
    count), '64', '192', '768', '2048' [B, C], 'logits_unbiased', 'logits' [B, 1008], concat (block -> channels), used (layer names in order)"""
    net = Net(sd, model, dtype)      # dtype: the arithmetic (float64; tools/inception_timing.py also times float32)
    out = {"concat": {}, "relu": []}
    x = net.store(input64(u8, dtype))
    x = net.conv(x, "Conv2d_1a_3x3", stride=2)
    x = net.conv(x, "Conv2d_2a_3x3")
    x = net.conv(x, "Conv2d_2b_3x3", padding=1)
    out["relu"].append(x)
    x = F.max_pool2d(x, 3, 2)
    out["64"] = x.mean((2, 3))
    x = net.conv(x, "Conv2d_3b_1x1")
    x = net.conv(x, "Conv2d_4a_3x3")
    out["relu"].append(x)
    x = F.max_pool2d(x, 3, 2)
    out["192"] = x.mean((2, 3))
    maps = [x]
    for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        x = net.a(x, n)
        out["concat"][n] = x.shape[1]
    maps.append(x)
    x = net.b(x, "Mixed_6a")
    out["concat"]["Mixed_6a"] = x.shape[1]
    for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        x = net.c(x, n)
        out["concat"][n] = x.shape[1]
    out["768"] = x.mean((2, 3))
    maps.append(x)
    x = net.d(x, "Mixed_7a")
    out["concat"]["Mixed_7a"] = x.shape[1]
    x = net.e(x, "Mixed_7b", use_max=False)
    out["concat"]["Mixed_7b"] = x.shape[1]
    x = net.e(x, "Mixed_7c", use_max=True)
    out["concat"]["Mixed_7c"] = x.shape[1]
    maps.append(x)
    out["relu"] += maps[1:]
    out["maps"] = maps
    out["2048"] = x.mean((2, 3))
    out["logits_unbiased"] = out["2048"] @ sd["fc.weight"].to(dtype).T
    out["logits"] = out["logits_unbiased"] + sd["fc.bias"].to(dtype)
    out["used"] = net.used
    return out


@functools.lru_cache(maxsize=None)
def weights(style):
    return make_inception_weights(WEIGHT_SEED, style)


def images_u8(B, H, W, seed):
    real, _ = make_eval_images("noise", 0.05, B, H, W, seed)
    return (real * 255.0).to(torch.uint8)


def case_images(name):
    B, H, W, seed, _style = CASES[name]
    return images_u8(B, H, W, seed)


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    """-> (exact, model): the dicts of inception64, computed once per case and shared (do not modify)"""
    sd = weights(CASES[name][4])
    u8 = case_images(name)
    with torch.no_grad():
        return inception64(u8, sd, model=False), inception64(u8, sd, model=True)


def conv_case(name, seed):
    """the seeded operands of a per-launch convolution case: x fp16 NHWC (the output of a ReLU layer), w fp32 OIHW (He-normal), scale in [0.5, 2),
    shift N(0, 0.1)"""
    B, H, W, cin, cout, (kh, kw), _stride, _pad = CONV_CASES[name]
    g = torch.Generator().manual_seed(seed)
    x16 = torch.relu(torch.randn(B, H, W, cin, generator=g) * (0.5 + torch.rand(cin, generator=g))).to(torch.float16)
    if cin == 3:
        x16 = (torch.rand(B, H, W, cin, generator=g) * 2 - 1).to(torch.float16)                 # the normalised image
    w = torch.randn(cout, cin, kh, kw, generator=g) * (2.0 / (cin * kh * kw)) ** 0.5
    scale = 0.5 + 1.5 * torch.rand(cout, generator=g)
    shift = torch.randn(cout, generator=g) * 0.1
    return x16, w, scale, shift
