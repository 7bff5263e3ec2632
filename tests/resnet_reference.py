"""Float64 restatement of the ResNet-50 perceptual loss as DESIGN.md "ResNet-50" specifies it, for the tests, and the case tables.

``resize_matrix(n)``: the antialiased bilinear resize of one axis to 224 as a [224, n] matrix (the formula of DESIGN.md; held against torch's own
CPU ``F.interpolate(..., antialias=True)`` in tests/test_perceptual_cpu.py).  ``input64``: both axes and ``(x - mean) / std``.  ``trunk64(img, sd,
model=False)`` (`exact`): torchvision's resnet50 (v1.5) from the normalised image on -- conv1 7x7 / 2, BatchNorm (running statistics, eps 1e-5),
ReLU, 3x3 / 2 max pool with padding 1, sixteen bottlenecks, the spatial mean and the 1000-way head -- all in float64.  torchvision and the ImageNet
checkpoint are not available, so nothing here is held against the real network or against the reference module.

``model=True``: the same with the HIP engine's documented roundings and nothing else: convolution weights and every stored activation (each
convolution's output after its epilogue, the downsample branch included; a bottleneck's sum is rounded once, after the ReLU) rounded to fp16,
saturating at 65504; arithmetic still float64; the head on the fp32 weights.  |model - exact| is E_model, the unit of the GPU bounds.
"""
import functools

import torch
import torch.nn.functional as F

import convnet_reference
from convnet_reference import h16r
from maskbit_amd.synth import make_resnet50_weights

SIDE = 224
BN_EPS = 1e-5
WEIGHT_SEED = 5200
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
BLOCKS = (3, 4, 6, 3)
LAYER_CHANNELS = (256, 512, 1024, 2048)
PARAMETERS = 25_557_032
RESIZE_SIZES = ((256, 256), (512, 512), (224, 224), (96, 160), (300, 257))

# the trunk cases: name -> (B, S, image seed)
TRUNK_CASES = {"s56": (3, 56, 5210), "s64": (3, 64, 5211)}
# the whole-path cases: name -> (H, W, image seed); one pair each: a base image and the base plus noise of sigma 0.02
PAIR_CASES = {"256": (256, 256, 5220), "96x160": (96, 160, 5221)}
PAIR_SIGMA = 0.02

# the per-launch convolution cases: name -> (B, H, W, Cin, Cout, k, stride, pad, epilogue) with epilogue 0 ReLU, 1 linear, 2 residual
EPI_RELU, EPI_LINEAR, EPI_RESIDUAL = 0, 1, 2
CONV_CASES = {
    "residual 64->256 k1 14x14": (3, 14, 14, 64, 256, 1, 1, 0, EPI_RESIDUAL),
    "linear 256->512 k1 s2 14x14": (2, 14, 14, 256, 512, 1, 2, 0, EPI_LINEAR),
    "relu 128->128 k3 s2 p1 14x14": (2, 14, 14, 128, 128, 3, 2, 1, EPI_RELU),
    "relu 512->512 k3 p1 7x7": (2, 7, 7, 512, 512, 3, 1, 1, EPI_RELU),
    "residual 512->2048 k1 7x7": (2, 7, 7, 512, 2048, 1, 1, 0, EPI_RESIDUAL),
}
STEM_SIDE = 32                            # the stem case: conv1 in its folded form on a 32 x 32 image


# ---- the written-out key list (independent of maskbit_amd.perceptual) ---------------------------------------------------------------------
def written_out_keys():
    """the reference module's state dict: its buffers, then torchvision's resnet50 under ``model.``, in order -> [(key, shape)]"""
    out = [("mean", (1, 3, 1, 1)), ("std", (1, 3, 1, 1))]

    def bn(p, c):
        return [(f"{p}.weight", (c,)), (f"{p}.bias", (c,)), (f"{p}.running_mean", (c,)), (f"{p}.running_var", (c,)), (f"{p}.num_batches_tracked", ())]

    net = [("conv1.weight", (64, 3, 7, 7))] + bn("bn1", 64)
    inplanes = 64
    for li, (blocks, planes) in enumerate(zip(BLOCKS, (64, 128, 256, 512))):
        for b in range(blocks):
            p = f"layer{li + 1}.{b}"
            net += [(p + ".conv1.weight", (planes, inplanes, 1, 1))] + bn(p + ".bn1", planes)
            net += [(p + ".conv2.weight", (planes, planes, 3, 3))] + bn(p + ".bn2", planes)
            net += [(p + ".conv3.weight", (planes * 4, planes, 1, 1))] + bn(p + ".bn3", planes * 4)
            if b == 0:
                net += [(p + ".downsample.0.weight", (planes * 4, inplanes, 1, 1))] + bn(p + ".downsample.1", planes * 4)
            inplanes = planes * 4
    net += [("fc.weight", (1000, 2048)), ("fc.bias", (1000,))]
    return out + [("model." + k, s) for k, s in net]


# ---- the input ------------------------------------------------------------------------------------------------------------------------------
def resize_taps(n, out=SIDE):
    """per output index: (first source index, the normalised float64 weights)"""
    scale = n / out
    support = max(scale, 1.0)
    inv = 1.0 / support
    taps = []
    for i in range(out):
        c = scale * (i + 0.5)
        lo, hi = max(int(c - support + 0.5), 0), min(int(c + support + 0.5), n)
        w = [max(0.0, 1.0 - abs((j - c + 0.5) * inv)) for j in range(lo, hi)]
        tot = sum(w)
        taps.append((lo, [v / tot for v in w]))
    return taps


@functools.lru_cache(maxsize=None)
def resize_matrix(n, out=SIDE):
    m = torch.zeros(out, n, dtype=torch.float64)
    for i, (lo, w) in enumerate(resize_taps(n, out)):
        m[i, lo:lo + len(w)] = torch.tensor(w, dtype=torch.float64)
    return m


def resize64(x):
    """[B, C, H, W] -> float64 [B, C, 224, 224]"""
    H, W = x.shape[-2:]
    return resize_matrix(H) @ x.double() @ resize_matrix(W).T


def input64(x, clamp=False):
    x = x.double()
    if clamp:
        x = x.clamp(0.0, 1.0)
    mean = torch.tensor(MEAN).double().view(1, 3, 1, 1)        # the fp32 buffers, as the module holds them
    std = torch.tensor(STD).double().view(1, 3, 1, 1)
    return (resize64(x) - mean) / std


def stem_cols64(img):
    """float64 [B, 3, S, S] -> [B, So, So, 147]: the 7x7 stride-2 padding-3 patches, channel ci * 49 + ky * 7 + kx"""
    B, _, S, _ = img.shape
    So = (S - 1) // 2 + 1
    return F.unfold(img, 7, padding=3, stride=2).view(B, 147, So, So).permute(0, 2, 3, 1)


# ---- the network ------------------------------------------------------------------------------------------------------------------------------
class Net(convnet_reference.Net):
    def __init__(self, sd, model):
        super().__init__(sd, model, BN_EPS)

    def bottleneck(self, x, p, stride, downsample):
        t = self.store(F.relu(self.convbn(x, p + ".conv1", p + ".bn1")))
        t = self.store(F.relu(self.convbn(t, p + ".conv2", p + ".bn2", stride, 1)))
        idn = self.store(self.convbn(x, p + ".downsample.0", p + ".downsample.1", stride)) if downsample else x
        return self.store(F.relu(self.convbn(t, p + ".conv3", p + ".bn3") + idn))


def trunk64(img, sd, model=False):
    """normalised image float64 [B, 3, S, S] (already on the fp16 grid when it came from the engine's input kernel) -> dict: maps (layer1 .. layer4,
    float64 NCHW), pool [B, 2048], logits [B, 1000]"""
    net = Net(sd, model)
    x = net.store(F.relu(net.convbn(img.double(), "conv1", "bn1", 2, 3)))
    x = F.max_pool2d(x, 3, 2, 1)
    maps = []
    for li, blocks in enumerate(BLOCKS):
        for b in range(blocks):
            x = net.bottleneck(x, f"layer{li + 1}.{b}", 2 if (b == 0 and li > 0) else 1, b == 0)
        maps.append(x)
    pool = x.mean((2, 3))
    logits = pool @ sd["fc.weight"].double().T + sd["fc.bias"].double()
    return {"maps": maps, "pool": pool, "logits": logits}


def loss64(out, B, on_logits):
    """the reference's value per pair from a trunk64 of 2B images (the first B against the last B): float64 [B]"""
    v = (out["logits"][:B] - out["logits"][B:]).pow(2).mean(1)
    if not on_logits:
        v = v + (out["maps"][3][:B] - out["maps"][3][B:]).pow(2).mean((1, 2, 3))
    return v


@functools.lru_cache(maxsize=None)
def weights():
    """torchvision layout (do not modify)"""
    return make_resnet50_weights(WEIGHT_SEED)


def reference_layout(sd):
    out = {"model." + k: v for k, v in sd.items()}
    out["mean"] = torch.tensor(MEAN)[None, :, None, None]
    out["std"] = torch.tensor(STD)[None, :, None, None]
    return out


def trunk_image(name):
    """the normalised image of a trunk case as the engine holds it: fp16 [B, S, S, 4], channel 3 NaN (it must not be read)"""
    B, S, seed = TRUNK_CASES[name]
    g = torch.Generator().manual_seed(seed)
    img = torch.full((B, S, S, 4), float("nan"), dtype=torch.float16)
    img[..., :3] = torch.randn(B, S, S, 3, generator=g).to(torch.float16)
    return img


@functools.lru_cache(maxsize=None)
def trunk_oracle(name):
    """-> (exact, model): the dicts of trunk64, computed once per case and shared (do not modify)"""
    img = trunk_image(name)[..., :3].double().permute(0, 3, 1, 2)
    with torch.no_grad():
        return trunk64(img, weights(), False), trunk64(img, weights(), True)


def pair_images(name):
    """-> (base, noisy) fp32 [1, 3, H, W] in [0, 1]"""
    H, W, seed = PAIR_CASES[name]
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    smooth = torch.stack([0.5 + 0.35 * torch.sin(6.0 * xx + 3.0 * yy + c) for c in range(3)])
    base = (smooth + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0.0, 1.0)[None]
    noisy = (base + PAIR_SIGMA * torch.randn(1, 3, H, W, generator=g)).clamp(0.0, 1.0)
    return base.float().contiguous(), noisy.float().contiguous()


@functools.lru_cache(maxsize=None)
def pair_oracle(name):
    """-> (exact, model): trunk64 dicts of the two images (base first) from the float64 input; the model's input is rounded to fp16"""
    base, noisy = pair_images(name)
    x = input64(torch.cat([base, noisy]))
    with torch.no_grad():
        return trunk64(x, weights(), False), trunk64(h16r(x), weights(), True)


def conv_case(name, seed):
    """the seeded operands of a per-launch case: x fp16 NHWC (the output of a ReLU layer), w fp32 OIHW (He-normal), scale in [0.5, 2), shift
    N(0, 0.1), identity fp16 [B, Ho, Wo, Cout] (a ReLU output; None unless the case is residual)"""
    B, H, W, cin, cout, k, stride, pad, epi = CONV_CASES[name]
    g = torch.Generator().manual_seed(seed)
    x16 = torch.relu(torch.randn(B, H, W, cin, generator=g) * (0.5 + torch.rand(cin, generator=g))).to(torch.float16)
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    scale = 0.5 + 1.5 * torch.rand(cout, generator=g)
    shift = torch.randn(cout, generator=g) * 0.1
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    idn = torch.relu(torch.randn(B, Ho, Wo, cout, generator=g)).to(torch.float16) if epi == EPI_RESIDUAL else None
    return x16, w, scale, shift, idn
