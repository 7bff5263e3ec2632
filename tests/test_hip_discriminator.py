"""GPU tests of the VQGAN+ discriminator (csrc/discriminator.hip; the LeakyReLU epilogue of csrc/inception.hip): every kernel through its
single-launch diagnostic entry against the float64 restatement of tests/discriminator_reference.py -- bit equality where the operands make the
arithmetic exact, a derived bound elsewhere -- then the whole network, the handle's invariances, and the Python surface on top of it.

Whole-network bound: twice the error of the restatement's fp16-storage emulation against the plain float64 restatement on the same input (max |.|
over the logits), measured in the test and not fixed in advance -- the engine's accumulation order and the point at which it takes the GroupNorm
statistics differ from any torch emulation; the measured figures are in profiles/discriminator.md.
GroupNorm mutant: with eps 1e-6 in place of 1e-5 (DISC_GN_EPS) test_groupnorm_apply fails in the constant group (tried once, not kept)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import discriminator_reference as R
import resnet_reference as RR
from conftest import load_golden
from convnet_helpers import DEV, EPI_LINEAR, U16, U32, _lib, _stream, bits, check_against_fp64, integer_case, ref_convbn
from maskbit_amd.synth import make_discriminator_weights

pytestmark = pytest.mark.gpu
EPI_LEAKY = 3


def nhwc16(x64):
    """float64 NCHW -> fp16 NHWC"""
    return x64.permute(0, 2, 3, 1).contiguous().to(torch.float16)


# ------------------------------------------------------------------------------------------------ downsample + partials
def run_down(x16, K, partials=True):
    L, lib = _lib()
    B, H, W, Cc = x16.shape
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if K else (H // 2, W // 2)
    nchunk = lib.mb_disc_down_chunks(Ho, Wo, Cc)
    xd = x16.to(DEV).contiguous()
    y = torch.full((B, Ho, Wo, Cc), float("nan"), dtype=torch.float16, device=DEV)
    part = torch.full((B, nchunk, 32, 2), float("nan"), dtype=torch.float32, device=DEV) if partials else None
    L.check(lib.mb_disc_downsample(xd.data_ptr(), y.data_ptr(), part.data_ptr() if partials else None, B, H, W, Cc, K, _stream()), "mb_disc_downsample")
    torch.cuda.synchronize()
    return y.cpu(), (part.cpu() if partials else None), nchunk


def check_partials(part, exact, nchunk, K):
    """exact float64 [B, C, Ho, Wo], the values the kernel summed.  Per (image, chunk, group): a thread adds ceil(pixels / lanes) terms in fp32 (one
    rounding each, the square by fma), two float64 levels are rounded to fp32 once each: (n1 + 2) 2^-24 times the sum of the magnitudes"""
    B, Cc, Ho, Wo = exact.shape
    HWo, cpg = Ho * Wo, Cc // 32
    per = -(-HWo // nchunk)
    npl = 256 // (Cc // 8)
    v = exact.reshape(B, 32, cpg, HWo)
    worst = 0.0
    for k in range(nchunk):
        seg = v[..., k * per:min(HWo, (k + 1) * per)]
        n1 = -(-seg.shape[-1] // npl)
        for j, t in enumerate((seg, seg * seg)):
            want, mag = t.sum((2, 3)), t.abs().sum((2, 3))
            err = (part[:, k, :, j].double() - want).abs()
            bound = (n1 + 2) * U32 * mag
            assert bool((err <= bound).all()), (k, j, float((err - bound).max()))
            worst = max(worst, float((err / bound.clamp(min=1e-300)).max()))
    return worst


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Cc", [32, 40, 128])
@pytest.mark.parametrize("H,W", [(8, 16), (6, 10), (7, 9)])
@pytest.mark.parametrize("K", [3, 4, 5, 0])
def test_downsample_integer_operands_are_bit_exact(K, H, W, Cc, B):
    g = torch.Generator().manual_seed(7000 + K * 100 + H * 10 + Cc + B)
    x16 = torch.randint(-3, 4, (B, H, W, Cc), generator=g).to(torch.float16)
    exact = R.downsample64(x16.double().permute(0, 3, 1, 2), K)            # every product and partial sum is a multiple of 2^-8 below 2^3: exact in fp32
    partials = Cc % 32 == 0
    got, part, nchunk = run_down(x16, K, partials)
    assert torch.equal(bits(got), bits(nhwc16(exact))) and bool((exact != exact.round()).any())
    if partials:
        assert nchunk == 1
        check_partials(part, exact, nchunk, K)


@pytest.mark.parametrize("K", [4, 0])
def test_downsample_several_chunks_vs_fp64(K):
    """64 x 96 x 32 -> three pixel chunks an image; random fp16 operands: 2^-11 |y| for the store + K^2 fma roundings on the magnitude sum"""
    g = torch.Generator().manual_seed(7100 + K)
    x16 = torch.randn(2, 64, 96, 32, generator=g).to(torch.float16)
    a = x16.double().permute(0, 3, 1, 2)
    exact, S = R.downsample64(a, K), R.downsample64(a.abs(), K)
    got, part, nchunk = run_down(x16, K)
    assert nchunk == 3
    err = (got.double().permute(0, 3, 1, 2) - exact).abs()
    bound = U16 * exact.abs() + max(K * K, 4) * U32 * S
    assert bool((err <= bound).all()), float((err / bound).max())
    # the partials are of the fp32 values before the store: within the accumulation's error of the float64 ones
    worst = check_partials_loose(part, exact, S, nchunk, K)
    print(f"downsample K {K}: worst partial err / bound {worst:.3f}")


def check_partials_loose(part, exact, S, nchunk, K):
    """as check_partials, for inexact accumulation: each summed value carries up to K^2 2^-24 S of its own error (twice that, relatively, squared)"""
    B, Cc, Ho, Wo = exact.shape
    HWo, cpg = Ho * Wo, Cc // 32
    per, npl, terms = -(-HWo // nchunk), 256 // (Cc // 8), max(K * K, 4)
    v, s = exact.reshape(B, 32, cpg, HWo), S.reshape(B, 32, cpg, HWo)
    worst = 0.0
    for k in range(nchunk):
        sl = slice(k * per, min(HWo, (k + 1) * per))
        seg, mag = v[..., sl], s[..., sl]
        n1 = -(-seg.shape[-1] // npl)
        dv = terms * U32 * mag                                                # a value's own error
        for j, (t, tmag, dt) in enumerate(((seg, seg.abs(), dv), (seg * seg, seg * seg, 2 * seg.abs() * dv + dv * dv))):
            err = (part[:, k, :, j].double() - t.sum((2, 3))).abs()
            bound = (n1 + 2) * U32 * (tmag + dt).sum((2, 3)) + dt.sum((2, 3))
            assert bool((err <= bound).all()), (k, j)
            worst = max(worst, float((err / bound).max()))
    return worst


# ------------------------------------------------------------------------------------------------ GroupNorm + LeakyReLU
@pytest.mark.parametrize("Cc,nchunk", [(32, 1), (64, 3), (128, 1), (512, 2)])          # group widths 1, 2, 4, 16
def test_groupnorm_apply(Cc, nchunk):
    L, lib = _lib()
    B, HW, cpg, slope = 2, 24, Cc // 32, 0.1
    g = torch.Generator().manual_seed(7200 + Cc)
    v32 = (torch.randn(B, HW, Cc, generator=g) * 1.5 + torch.randn(1, 1, Cc, generator=g)).float()
    # group 5 of image 1 is constant in fp32 at a value fp16 cannot hold (1 + 2^-12 -> 1): variance 0, and (x - mean) rstd is set by eps alone
    v32[1, :, 5 * cpg:6 * cpg] = 1.0 + 2.0 ** -12
    x16 = v32.to(torch.float16)
    gr = v32.double().reshape(B, HW, 32, cpg)
    # the partials as the downsample leaves them: fp32 sums of the fp32 values, here split over `nchunk` chunks of pixels
    edges = [HW * k // nchunk for k in range(nchunk + 1)]
    part = torch.stack([torch.stack([gr[:, a:b].sum((1, 3)), gr[:, a:b].pow(2).sum((1, 3))], -1) for a, b in zip(edges, edges[1:])], 1).float()
    gamma = (0.6 + 0.8 * torch.rand(Cc, generator=g)).float()
    beta = (torch.randn(Cc, generator=g) * 0.2).float()
    xd, pd, gd, bd = x16.to(DEV).contiguous(), part.to(DEV).contiguous(), gamma.to(DEV), beta.to(DEV)
    sat = C.c_uint(7)
    L.check(lib.mb_disc_groupnorm(xd.data_ptr(), pd.data_ptr(), nchunk, gd.data_ptr(), bd.data_ptr(), C.byref(sat), B, HW, Cc, slope, _stream()), "mb_disc_groupnorm")
    got = xd.cpu().double()
    # float64 from the same fp32 partials
    n = HW * cpg
    ts, tq = part.double().sum(1)[..., 0], part.double().sum(1)[..., 1]
    mean = ts / n
    var = (tq / n - mean * mean).clamp(min=0)
    assert float(var[1, 5]) < 1e-6                                            # (what rounding the partials to fp32 leaves) against eps 1e-5
    m = mean.repeat_interleave(cpg, 1)[:, None, :]
    sc = (1.0 / torch.sqrt(var + R.GN_EPS)).repeat_interleave(cpg, 1)[:, None, :] * gamma.double()
    t = x16.double() * sc - m * sc + beta.double()
    slope32 = float(torch.tensor(slope, dtype=torch.float32))
    want = torch.where(t >= 0, t, t * slope32)
    # roundings: mean, rstd, scale (2 on x sc and mean sc), shift (product, subtraction), the fma, the slope: 8 2^-24 on the magnitudes; the store
    T = x16.double().abs() * sc.abs() + m.abs() * sc.abs() + beta.double().abs()
    bound = U16 * want.abs() + 8 * U32 * T
    err = (got - want).abs()
    print(f"groupnorm C {Cc}: worst err / bound {float((err / bound).max()):.3f}; constant group: got {float(got[1, 0, 5 * cpg]):.5f}, "
          f"want {float(want[1, 0, 5 * cpg]):.5f}, with eps 1e-6 {float(-2.0 ** -12 * 1e3 * gamma[5 * cpg] + beta[5 * cpg]):.5f}")
    assert bool((err <= bound).all()) and sat.value == 0
    assert bool((got < 0).any()) and bool((got > 0).any())


# ------------------------------------------------------------------------------------------------ adaptive pool
@pytest.mark.parametrize("H,W", [(4, 6), (16, 16), (24, 16), (32, 32), (64, 64)])
@pytest.mark.parametrize("negative", [False, True])
def test_adaptive_pool_bit_equal(H, W, negative):
    L, lib = _lib()
    B, Cc = 2, 40
    x16 = torch.randn(B, H, W, Cc, generator=torch.Generator().manual_seed(7300 + H + W)).to(torch.float16)
    if negative:
        x16 = -x16.abs() - 1
    xd = x16.to(DEV).contiguous()
    y = torch.full((B, 16, 16, Cc), float("nan"), dtype=torch.float16, device=DEV)
    L.check(lib.mb_disc_pool(xd.data_ptr(), y.data_ptr(), B, H, W, Cc, _stream()), "mb_disc_pool")
    want = R.adaptive_maxpool64(x16.double().permute(0, 3, 1, 2))
    assert torch.equal(bits(y.cpu()), bits(nhwc16(want)))
    if (H, W) == (16, 16):
        assert torch.equal(bits(y.cpu()), bits(x16))


# ------------------------------------------------------------------------------------------------ the LeakyReLU epilogue
def run_leaky(x16, w, scale, shift, pad, slope, variant=0):
    L, lib = _lib()
    B, H, W, cin = x16.shape
    cout, _, kh, kw = w.shape
    out = torch.full((B, H + 2 * pad - kh + 1, W + 2 * pad - kw + 1, cout), float("nan"), dtype=torch.float16, device=DEV)
    xd, wd, sc, sh = x16.to(DEV).contiguous(), w.float().to(DEV).contiguous(), scale.float().to(DEV), shift.float().to(DEV)
    sat = C.c_uint(0)
    L.check(lib.mb_convbn_layer_leaky(xd.data_ptr(), wd.data_ptr(), sc.data_ptr(), sh.data_ptr(), out.data_ptr(), C.byref(sat), B, H, W, cin, cout, kh, kw, 1,
                                      pad, pad, 0, cin, 0, cout, variant, EPI_LEAKY, slope, None, 0, 0, _stream()), "mb_convbn_layer_leaky")
    return out.cpu(), int(sat.value)


def leaky32(v64, slope):
    """v (exact in fp32) -> fp32(v * fp32(slope)) below zero, as the kernel's one multiplication rounds"""
    s = float(torch.tensor(slope, dtype=torch.float32))
    return torch.where(v64 >= 0, v64, (v64 * s).float().double())


LEAKY_CASES = {"1x1 96->32 9x9": (2, 9, 9, 96, 32, 1, 0), "3x3 32->64 7x10": (1, 7, 10, 32, 64, 3, 1), "1x1 128->128 16x16": (3, 16, 16, 128, 128, 1, 0),
               "5x5 8->32 6x6": (1, 6, 6, 8, 32, 5, 2)}


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("slope", [0.1, 0.25])
@pytest.mark.parametrize("name", list(LEAKY_CASES))
def test_leaky_epilogue_integer_operands_are_bit_exact(name, slope, variant):
    B, H, W, cin, cout, k, pad = LEAKY_CASES[name]
    x16, w, scale, shift, _ = integer_case(7400 + cin, B, H, W, cin, cout, k, 1, pad)
    v, _ = ref_convbn(x16, w, scale, shift, 1, pad, epi=EPI_LINEAR)
    want = leaky32(v, slope)
    assert bool((v < 0).any()) and bool((v > 0).any())
    got, sat = run_leaky(x16, w, scale, shift, pad, slope, variant)
    assert torch.equal(bits(got), bits(nhwc16(want))) and sat == 0


@pytest.mark.parametrize("name", list(LEAKY_CASES))
def test_leaky_epilogue_vs_fp64(name):
    B, H, W, cin, cout, k, pad = LEAKY_CASES[name]
    g = torch.Generator().manual_seed(7500 + cin)
    x16 = torch.randn(B, H, W, cin, generator=g).to(torch.float16)
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    scale, shift = torch.ones(cout), torch.randn(cout, generator=g) * 0.1
    v, S = ref_convbn(x16, w, scale, shift, 1, pad, epi=EPI_LINEAR)
    s32 = float(torch.tensor(0.1, dtype=torch.float32))
    exact = torch.where(v >= 0, v, v * s32)
    got, sat = run_leaky(x16, w, scale, shift, pad, 0.1)
    check_against_fp64("leaky " + name, got, exact, S, cin * k * k + 2, epi=EPI_LINEAR)         # + the epilogue's fma and the slope
    assert sat == 0
    assert torch.equal(bits(got), bits(run_leaky(x16, w, scale, shift, pad, 0.1, 1)[0])) and torch.equal(bits(got), bits(run_leaky(x16, w, scale, shift, pad, 0.1, 2)[0]))
    big, sat = run_leaky(x16, w, scale * 3e5, shift, pad, 0.1)
    assert sat > 0 and float(big.double().abs().max()) == 65504.0 and bool((big.double() < -6550).any())     # both signs clamp and are counted


# ------------------------------------------------------------------------------------------------ the logits kernel
def run_logits(x16, w, bias, stats=True, total=None):
    L, lib = _lib()
    B, _, _, Cc = x16.shape
    xd, wd, bd = x16.to(DEV).contiguous(), w.float().to(DEV).contiguous(), bias.float().to(DEV)
    lo = torch.full((B, 256), float("nan"), dtype=torch.float32, device=DEV)
    st = torch.full((B, 5), float("nan"), dtype=torch.float64, device=DEV) if stats else None
    L.check(lib.mb_disc_logits(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), lo.data_ptr(), st.data_ptr() if stats else None,
                               total.data_ptr() if total is not None else None, B, Cc, _stream()), "mb_disc_logits")
    return lo.cpu(), (st.cpu() if stats else None)


def check_stats(st, logits32):
    want = R.stats64(logits32)
    mag = want.clone()
    mag[:, 0] = logits32.double().reshape(want.shape[0], -1).abs().sum(1)     # the sum of the logits is taken relative to the sum of their magnitudes
    rel = ((st - want).abs() / mag.clamp(min=1e-300)).max()
    assert float(rel) <= 1e-12, float(rel)


@pytest.mark.parametrize("Cc,B", [(32, 1), (128, 3), (512, 2)])
def test_logits_kernel_vs_fp64(Cc, B):
    g = torch.Generator().manual_seed(7600 + Cc)
    x16 = torch.randn(B, 16, 16, Cc, generator=g).to(torch.float16)
    w = torch.randn(1, Cc, 5, 5, generator=g) * 1.5 / (25 * Cc) ** 0.5
    bias = torch.tensor([0.1])
    a = x16.double().permute(0, 3, 1, 2)
    want = F.conv2d(a, w.double(), bias.double(), padding=2)
    S = F.conv2d(a.abs(), w.double().abs(), None, padding=2) + 0.1
    total = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0], dtype=torch.float64, device=DEV)
    lo, st = run_logits(x16, w, bias, total=total)
    err = (lo.double().view(B, 1, 16, 16) - want).abs()
    bound = 25 * Cc * U32 * S
    print(f"logits C {Cc}: worst err / bound {float((err / bound).max()):.4f}, logits in [{float(lo.min()):.2f}, {float(lo.max()):.2f}]")
    assert bool((err <= bound).all()) and float(lo.min()) < -1 and float(lo.max()) > 1
    check_stats(st, lo)
    t = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0], dtype=torch.float64)
    for b in range(B):
        t = t + st[b]
    assert torch.equal(total.cpu(), t)                                        # the running sum: the images added in order
    assert torch.equal(run_logits(x16, w, bias, stats=False)[0], lo)


def test_logits_kernel_at_the_kinks_and_the_ends():
    """a centre-tap weight of 1 on channel 0 passes the map through: logits of exactly +-1, 0 and +-40"""
    Cc = 32
    vals = torch.tensor([1.0, -1.0, 0.0, 40.0, -40.0, 0.5, -0.5, 3.0])
    x16 = torch.zeros(1, 16, 16, Cc, dtype=torch.float16)
    x16[0, :, :, 0] = vals.repeat(32).view(16, 16).to(torch.float16)
    x16[0, :, :, 1:] = torch.randn(16, 16, Cc - 1, generator=torch.Generator().manual_seed(7700)).to(torch.float16)     # met by zero weights
    w = torch.zeros(1, Cc, 5, 5)
    w[0, 0, 2, 2] = 1.0
    lo, st = run_logits(x16, w, torch.zeros(1))
    assert torch.equal(lo.view(16, 16), vals.repeat(32).view(16, 16))
    check_stats(st, lo)
    assert bool(torch.isfinite(st).all()) and abs(float(st[0, 4]) - 32 * float(R.softplus64(vals.double()).sum())) <= 1e-9
    assert float(st[0, 1]) == 32 * float((1 - vals).clamp(min=0).sum()) and float(st[0, 2]) == 32 * float((1 + vals).clamp(min=0).sum())


# ------------------------------------------------------------------------------------------------ the whole network
@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("discriminator.npz")


def images(seed, shape):
    return torch.rand(*[int(v) for v in shape], generator=torch.Generator().manual_seed(int(seed)))


@functools.lru_cache(maxsize=None)
def hip_model(hidden=32, blur=4):
    from maskbit_amd import NLayerDiscriminatorv2
    m = NLayerDiscriminatorv2(hidden_channels=hidden, num_stages=3, blur_resample=blur != 0, blur_kernel_size=blur or 4)
    m.load_state_dict(make_discriminator_weights(int(golden()["seed"]), hidden, 3, blur), strict=True)
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """-> (float64 restatement, its fp16-storage emulation) of a hidden-32 case, computed once (do not modify)"""
    z = golden()
    blur = int(z[name + ".blur"])
    sd, x = make_discriminator_weights(int(z["seed"]), 32, 3, blur), images(z[name + ".image_seed"], z[name + ".shape"])
    with torch.no_grad():
        return R.forward64(sd, x, blur), R.forward64(sd, x, blur, emulate=True)


def check_network(name, got, ref, emu, m):
    E = float((emu - ref).abs().max())
    d = float((got.double() - ref).abs().max())
    print(f"network {name}: emulation error {E:.3e}, engine error {d:.3e}, ratio {d / E:.3f}; logits in [{float(ref.min()):.2f}, {float(ref.max()):.2f}]")
    assert tuple(got.shape) == tuple(ref.shape) and got.dtype == torch.float32 and E > 0
    assert d <= 2 * E
    assert m.saturation_count() == 0


@pytest.mark.parametrize("name", ["blur4_128", "blur4_32x48", "blur4_192x128", "avg_64", "blur3_64", "blur5_64"])
def test_network_hidden32_vs_fp64(name):
    z = golden()
    m = hip_model(32, int(z[name + ".blur"]))
    m.saturation_count()
    x = images(z[name + ".image_seed"], z[name + ".shape"]).to(DEV)
    got = m(x).cpu()
    ref, emu = oracle(name)
    check_network(name, got, ref, emu, m)
    assert float((got.double() - torch.from_numpy(z[name + ".logits"]).double()).abs().max()) <= 2 * float((emu - ref).abs().max()) + 1e-5     # the reference's own fp32 run
    check_stats(m.logit_stats(x).cpu(), got.view(got.shape[0], -1))


@pytest.mark.parametrize("name", ["h128_256", "h128_512x256"])
def test_network_hidden128_vs_fp64(name):
    """the restatement's and the emulation's logits are recorded (tools/make_golden_discriminator.py h128): minutes of float64 convolutions"""
    z = load_golden("discriminator_h128.npz")
    m = hip_model(128, 4)
    m.saturation_count()
    got = m(images(z[name + ".image_seed"], z[name + ".shape"]).to(DEV)).cpu()
    check_network(name, got, torch.from_numpy(z[name + ".ref64"]), torch.from_numpy(z[name + ".emu64"]), m)


def test_an_image_does_not_depend_on_the_batch_or_the_chunking():
    from maskbit_amd import NLayerDiscriminatorv2
    m = hip_model()
    x = images(7800, (5, 3, 64, 96)).to(DEV)
    lo, st = m(x), m.logit_stats(x)
    assert torch.equal(lo, m(x)) and torch.equal(st, m.logit_stats(x))        # two runs: bit-identical
    assert st.dtype == torch.float64 and tuple(st.shape) == (5, 5) and tuple(lo.shape) == (5, 1, 16, 16)
    for i in (0, 2, 4):
        assert torch.equal(m(x[i:i + 1]), lo[i:i + 1]) and torch.equal(m.logit_stats(x[i:i + 1]), st[i:i + 1]), i
    # a handle whose workspace takes one 512 x 512 image walks five 512 x 256 images in chunks of two
    big = images(7801, (5, 3, 512, 256)).to(DEV)
    small = NLayerDiscriminatorv2(hidden_channels=32, num_stages=3, blur_resample=True)
    small.load_state_dict(m.state_dict(), strict=True)
    small = small.to(DEV)
    small.max_images_per_call = 2
    whole = small(big)
    assert small._engine_key[1] == 2
    for i in range(5):
        assert torch.equal(m(big[i:i + 1]), whole[i:i + 1]), i
    clamped = m.logit_stats(x * 1.5 - 0.25, clamp=True)
    assert torch.equal(clamped, m.logit_stats((x * 1.5 - 0.25).clamp(0, 1)))


def test_reload_after_an_in_place_weight_change():
    from maskbit_amd import NLayerDiscriminatorv2
    m = NLayerDiscriminatorv2(hidden_channels=32, num_stages=3, blur_resample=True)
    m.load_state_dict(hip_model().state_dict(), strict=True)
    m = m.to(DEV)
    x = images(7802, (1, 3, 64, 64)).to(DEV)
    before = m(x).clone()
    assert torch.equal(before, hip_model()(x))
    with torch.no_grad():
        m.state_dict()["to_logits.2.bias"].add_(0.5)
        m.state_dict()["blocks.1.2.weight"].mul_(1.25)
    after = m(x)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    ref = R.forward64(sd, x.cpu(), 4)
    assert not torch.equal(after, before) and float((after.cpu().double() - ref).abs().max()) <= 0.01
    with torch.no_grad():
        m.state_dict()["blocks.0.1.kernel"][0, 0, 0, 0] += 0.01               # no longer the binomial kernel: the handle refuses it
    with pytest.raises(RuntimeError, match="binomial"):
        m(x)


def test_refusals_come_before_any_device_work():
    from maskbit_amd import NLayerDiscriminatorv2
    L, lib = _lib()
    m = hip_model()
    for bad in ((1, 3, 40, 64), (1, 3, 16, 64), (1, 3, 64, 528), (1, 1, 64, 64)):
        with pytest.raises(ValueError):
            m(torch.zeros(*bad, device=DEV))
    empty = NLayerDiscriminatorv2(hidden_channels=32).to(DEV)
    h = C.c_void_p()
    L.check(lib.mb_disc_create(1, 32, 3, 4, C.byref(h)), "mb_disc_create")
    x = torch.zeros(1, 3, 64, 64, device=DEV)
    out = torch.full((256,), float("nan"), device=DEV)
    try:
        assert lib.mb_disc_forward(h, x.data_ptr(), 1, 64, 64, 0, out.data_ptr(), None, None, _stream()) == -1 and b"not complete" in lib.mb_last_error()
        w = torch.zeros(32, 3, 5, 5, device=DEV)
        shape = (C.c_int64 * 4)(32, 3, 5, 5)
        assert lib.mb_disc_load(h, b"block_in.1.weight", w.data_ptr(), shape, 4, _stream()) == -2
        assert lib.mb_disc_load(h, b"blocks.0.0.weight", w.data_ptr(), shape, 4, _stream()) == -4
        assert lib.mb_disc_load(h, b"block_in.0.weight", w.data_ptr(), shape, 4, _stream()) == 0
        for H, W in ((48, 40), (16, 64), (64, 1024)):
            assert lib.mb_disc_forward(h, x.data_ptr(), 1, H, W, 0, out.data_ptr(), None, None, _stream()) == -1
    finally:
        lib.mb_disc_destroy(h)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    del empty


# ------------------------------------------------------------------------------------------------ the product on top
def test_tokenizer_evaluator_takes_the_model():
    from maskbit_amd import TokenizerEvaluator
    z = golden()
    m = hip_model()
    both = images(z["blur4_128.image_seed"], z["blur4_128.shape"])
    real, fake = both.to(DEV), both.flip(0).contiguous().to(DEV)
    plain = TokenizerEvaluator(DEV, enable_mae_error=True)
    plain.update(real, fake)
    ev = TokenizerEvaluator(DEV, enable_mae_error=True)
    ev.use_discriminator(m, loss="hinge")
    ev.update(real[:1], fake[:1])
    ev.update(real[1:], fake[1:])
    r = ev.result()
    assert set(r) - set(plain.result()) == {"LogitsReal", "LogitsFake", "DiscriminatorLoss", "GeneratorLoss"} and r["MAE"] == plain.result()["MAE"]
    ref, emu = oracle("blur4_128")
    E = float((emu - ref).abs().max())
    want = R.losses64(ref, ref.flip(0))
    assert abs(r["LogitsReal"] - float(ref.mean())) <= 2 * E and abs(r["LogitsFake"] - float(ref.mean())) <= 2 * E
    assert abs(r["DiscriminatorLoss"] - want["hinge_d"]) <= 2 * E and abs(r["GeneratorLoss"] - want["hinge_g"]) <= 2 * E     # the losses are 1-Lipschitz in the logits
    st = m.logit_stats(real).cpu()
    assert r["LogitsReal"] == float((st[0, 0] + st[1, 0]) / 2 / 256)          # the device sums: image order, no other arithmetic
    ev.use_discriminator(m, loss="non-saturating")
    ev.reset_metrics()
    ev.update(real, fake)
    r = ev.result()
    assert abs(r["DiscriminatorLoss"] - want["non_saturating_d"]) <= 2 * E and abs(r["GeneratorLoss"] - want["non_saturating_g"]) <= 2 * E
    ev.use_discriminator(None)
    assert "LogitsReal" not in ev.result()
    with pytest.raises(TypeError):
        ev.use_discriminator(object())
    with pytest.raises(ValueError):
        ev.use_discriminator(m, loss="wgan")


class Cfg(dict):
    __getattr__ = dict.__getitem__


@functools.lru_cache(maxsize=None)
def vqgan_case():
    """a seeded tiny tokenizer's forward() on one image and everything of the restatement that does not depend on the loss kind, computed once"""
    from test_hip_evaluator import tiny_tokenizers
    tok = dict((n, t) for n, t, _ in tiny_tokenizers())["vq"]
    x = images(7900, (1, 3, 64, 64)).to(DEV)
    rec, extra = tok(x)
    dsd = make_discriminator_weights(int(golden()["seed"]), 32, 3, 4)
    xc, rc = x.cpu(), rec.cpu().float()
    with torch.no_grad():
        lr, lf = R.forward64(dsd, xc, 4), R.forward64(dsd, rc, 4)
        E = max(float((R.forward64(dsd, t, 4, emulate=True) - l).abs().max()) for t, l in ((xc, lr), (rc, lf)))
        trunk = RR.trunk64(RR.input64(torch.cat([xc, rc])), RR.weights(), False)
        model = RR.trunk64(R.h16(RR.input64(torch.cat([xc, rc]))), RR.weights(), True)
    perc = float(RR.loss64(trunk, 1, True))
    Ep = float((model["logits"] - trunk["logits"]).abs().max())
    dp = (trunk["logits"][:1] - trunk["logits"][1:]).abs()
    perc_bound = float((2 * dp * 4 * Ep + (4 * Ep) ** 2).mean())               # the bound of tests/test_hip_perceptual.py's whole path
    return x, rec, extra, dsd, lr, lf, E, perc, perc_bound


@pytest.mark.parametrize("kind", ["hinge", "non-saturating"])
def test_vqganloss_on_a_tokenizers_output(kind):
    """both modes on a seeded tiny tokenizer's forward(), against the float64 discriminator, tests/resnet_reference.py and the formulas"""
    from maskbit_amd import VQGANLoss
    x, rec, extra, dsd, lr, lf, E, perc, perc_bound = vqgan_case()
    loss = VQGANLoss(Cfg(name="VQGAN+Discriminator", num_channels=3, num_stages=3, hidden_channels=32, blur_resample=True, blur_kernel_size=4),
                     Cfg(discriminator_loss=kind, reconstruction_loss="l2", discriminator_gradient_penalty="none", quantizer_weight=1.0,
                         perceptual_loss="resnet50", perceptual_weight=0.1, lecam_regularization_weight=0.001, discriminator_start=0,
                         discriminator_factor=1.0, discriminator_weight=0.1, discriminator_penalty_cost=10.0, ema_decay=0.9))
    state = {"discriminator." + k: v for k, v in dsd.items()}
    state.update({"perceptual_loss." + k: v for k, v in RR.reference_layout(RR.weights()).items()})
    state.update(ema_real_logits_mean=torch.tensor([0.2]), ema_fake_logits_mean=torch.tensor([-0.1]))
    loss.load_state_dict(state, strict=True)                                  # the layout of a training run's loss-module checkpoint
    loss = loss.to(DEV)
    total_g, dg = loss(x, rec, extra, 10, None, mode="gen")
    total_d, dd = loss(x, rec, extra, 10, mode="disc", update_ema=False)
    assert float(loss.ema_real_logits_mean) == float(torch.tensor(0.2)) and float(dg["entropy_loss"]) == 0.0
    xc, rc = x.cpu(), rec.cpu().float()
    l64 = R.losses64(lr, lf)
    gan = l64["hinge_g" if kind == "hinge" else "non_saturating_g"]
    mse = float((xc.double() - rc.double()).pow(2).mean())
    quant = float(extra["quantizer_loss"])
    want_g = mse + 0.1 * perc + quant + 0.1 * gan
    tol_g = 0.1 * perc_bound + 0.1 * 2 * E + 1e-6 * max(1.0, abs(want_g))
    print(f"VQGANLoss {kind}: gen {float(total_g):.6f} want {want_g:.6f} (tol {tol_g:.2e}); gan {float(dg['gan_loss']):.5f} want {gan:.5f}; E {E:.2e}")
    assert abs(float(total_g) - want_g) <= tol_g and abs(float(dg["gan_loss"]) - gan) <= 2 * E
    assert abs(float(dg["perceptual_loss"]) - 0.1 * perc) <= 0.1 * perc_bound + 1e-7 and abs(float(dg["reconstruction_loss"]) - mse) <= 1e-6 * max(mse, 1e-3)
    assert float(dg["quantizer_loss"]) == quant and "codebook_loss" in dg and float(dg["weighted_gan_loss"]) == pytest.approx(0.1 * float(dg["gan_loss"]), rel=1e-6)
    mr, mf = float(lr.mean()), float(lf.mean())
    lecam = 0.001 * R.lecam64(mr, mf, 0.2, -0.1)
    want_d = l64["hinge_d" if kind == "hinge" else "non_saturating_d"] + lecam
    assert abs(float(dd["logits_real"]) - mr) <= 2 * E and abs(float(dd["logits_fake"]) - mf) <= 2 * E
    assert abs(float(total_d) - want_d) <= 2 * 2 * E + 1e-6 and abs(float(dd["lecam_loss"]) - lecam) <= 0.001 * 8 * E + 1e-8
    loss(x, rec, extra, 10, mode="disc")                                      # the training step's call moves the EMA
    assert abs(float(loss.ema_real_logits_mean) - (0.2 * 0.9 + mr * 0.1)) <= 0.1 * 2 * E + 1e-6
    assert loss.discriminator.saturation_count() == 0
