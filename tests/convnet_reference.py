"""What the float64 restatements of the feature networks (inception_reference.py, resnet_reference.py, lpips_reference.py) share: the fp16
rounding of the engines' stores, BatchNorm on running statistics as a scale and a shift, and one convolution + BatchNorm step; and the references
of the networks' fp32 tail -- the loaders' BatchNorm fold and the spatial mean operation by operation in fp32, the mean and the head in float64 with
the magnitude sums of their bounds -- with the per-launch cases both the CPU and the GPU tests of the tail use."""
import numpy as np
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


# ---- the networks' tail: the BatchNorm fold of the loaders, the spatial mean, the head (tests/test_convnet_tail_cpu.py, test_hip_convnet_tail.py)
U32 = 2.0 ** -24
INCEPTION_EPS, RESNET_EPS = 1e-3, 1e-5
MEAN_THREADS = 256


def _np32(t):
    return t.detach().cpu().to(torch.float32).contiguous().numpy()


def bn_fold32(g, b, m, v, eps):
    """the fold as bn_fold_kernel states it: five fp32 operations, each rounded to nearest (numpy's float32 add, sqrt, divide, multiply and
    subtract are; torch.sqrt on fp32 is not everywhere) -> (scale, shift) fp32 tensors"""
    g, b, m, v = _np32(g), _np32(b), _np32(m), _np32(v)
    a = v + np.float32(eps)
    q = np.sqrt(a)
    s = g / q
    t = m * s
    shift = b - t
    assert s.dtype == np.float32 and shift.dtype == np.float32
    return torch.from_numpy(s), torch.from_numpy(shift)


def bn_fold64(g, b, m, v, eps):
    """float64 of the same fp32 operands (eps as the fp32 value the kernel is handed) -> (scale, shift, |beta| + |mean scale|)"""
    g, b, m, v = (t.detach().cpu().float().double() for t in (g, b, m, v))
    scale = g / torch.sqrt(v + float(np.float32(eps)))
    return scale, b - m * scale, b.abs() + (m * scale).abs()


def bn_parts(sd, prefix):
    return tuple(sd[prefix + k] for k in (".weight", ".bias", ".running_mean", ".running_var"))


def spatial_mean32(x16):
    """spatial_mean_kernel's order in numpy float32: x16 fp16 [B, HW, C] -> fp32 [B, C].  Thread t of 256 adds pixels t, t + 256, .. in sequence
    from +0; red[:o] += red[o:2 o] for o = 128 .. 1; one division by fp32(HW).  A thread that runs out of pixels adds +0 here, which changes
    no bit: its sum starts at +0 and can therefore never be -0"""
    x = x16.detach().cpu().to(torch.float32).numpy()
    B, HW, C = x.shape
    rows = -(-HW // MEAN_THREADS)
    padded = np.zeros((B, rows * MEAN_THREADS, C), dtype=np.float32)
    padded[:, :HW] = x
    padded = padded.reshape(B, rows, MEAN_THREADS, C)
    red = np.zeros((B, MEAN_THREADS, C), dtype=np.float32)
    for r in range(rows):
        red = red + padded[:, r]
    o = MEAN_THREADS // 2
    while o > 0:
        red = red[:, :o] + red[:, o:2 * o]
        o //= 2
    out = red[:, 0] / np.float32(HW)
    assert out.dtype == np.float32
    return torch.from_numpy(np.ascontiguousarray(out))


def spatial_mean64(x16):
    """-> (mean, mean |x|) float64 [B, C]"""
    x = x16.detach().cpu().double()
    return x.mean(1), x.abs().mean(1)


def mean_bound(HW, mean_abs):
    """|fp32 mean - exact| <= (ceil(HW / 256) + 9) 2^-24 mean|x|: a thread's chain of at most ceil(HW / 256) adds, eight tree levels, the division"""
    return (-(-HW // MEAN_THREADS) + 9) * U32 * mean_abs


def fc_head64(pool, w, bias=None):
    """pool [B, D], w [N, D], bias [N] or None -> (unbiased, biased, sum |p w| + |bias|) float64 [B, N]"""
    p, wd = pool.detach().cpu().double(), w.detach().cpu().double()
    bd = bias.detach().cpu().double() if bias is not None else torch.zeros(wd.shape[0], dtype=torch.float64)
    unbiased = p @ wd.T
    return unbiased, unbiased + bd, p.abs() @ wd.abs().T + bd.abs()


def head_bound(D, S):
    """|fp32 head - exact| <= (D / 64 + 7) 2^-24 S: a lane's chain of D / 64 fmas, six butterfly levels, the bias add"""
    return (D / 64 + 7) * U32 * S


# the per-launch cases, shared by the CPU checks of the references and the GPU tests
FOLD_COUTS = (1, 32, 255, 256, 257, 2048)
MEAN_HW = (1, 4, 49, 64, 255, 256, 257, 289, 1225, 5329)         # the products' own sizes and the edges of the 256 threads
MEAN_C = (8, 72)
MEAN_B = (1, 3)
HEAD_D, HEAD_N, HEAD_B = (2048, 256, 1024), (1, 3, 5, 1000, 1008), (1, 7, 8, 9, 17)
# every (D, N), (D, B) and (N, B) pair occurs: D walks its three values along each row and each column of the N x B table
HEAD_CASES = tuple((HEAD_D[(i - j) % 3], n, b) for i, n in enumerate(HEAD_N) for j, b in enumerate(HEAD_B))


def fold_case(cout, seed=6100):
    """-> bn fp32 [4, cout]: gamma with zeros and negative values, beta, mean, variance over 1e-3 .. 10 with exact zeros"""
    g = torch.Generator().manual_seed(seed + cout)
    gamma, beta, mean = torch.randn(cout, generator=g), torch.randn(cout, generator=g), torch.randn(cout, generator=g) * 2
    var = torch.pow(10.0, torch.rand(cout, generator=g) * 4 - 3)
    gamma[3::7] = 0.0
    var[1::5] = 0.0
    return torch.stack([gamma, beta, mean, var]).float().contiguous()


def mean_case(kind, B, HW, C):
    """x fp16 [B, HW, C].  "integer": integers in [0, 64], every sum exact in fp32.  "seeded": ReLU-like values with per-channel spread, channel 1
    all negative, +65504 and -65504 in channels 0 and 2 of image 0"""
    g = torch.Generator().manual_seed(6200 + HW * 100 + C + B)
    if kind == "integer":
        return torch.randint(0, 65, (B, HW, C), generator=g).to(torch.float16)
    x = torch.relu(torch.randn(B, HW, C, generator=g) * (0.5 + torch.rand(C, generator=g)))
    x[..., 1] = -x[..., 1].abs() - 1.0
    x[0, 0, 0], x[0, HW - 1, 2] = 65504.0, -65504.0
    return x.to(torch.float16)


def head_case(kind, B, D, N):
    """-> (pool [B, D], w [N, D], bias [N]) fp32.  "integer": pool in [0, 8), w in [-4, 4], bias multiples of 1/2: every partial sum is an integer
    below 2^24 and both outputs are exact.  "seeded": pooled ReLU features, He-like weights, a small bias"""
    g = torch.Generator().manual_seed(6300 + D + N * 7 + B)
    if kind == "integer":
        return (torch.randint(0, 8, (B, D), generator=g).float(), torch.randint(-4, 5, (N, D), generator=g).float(),
                torch.randint(-8, 9, (N,), generator=g).float() * 0.5)
    return (torch.relu(torch.randn(B, D, generator=g)) * (0.25 + torch.rand(D, generator=g)), torch.randn(N, D, generator=g) * D ** -0.5,
            torch.randn(N, generator=g) * 0.1)


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
