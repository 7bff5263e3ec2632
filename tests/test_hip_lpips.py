"""LPIPS on the HIP path (maskbit_amd/csrc/lpips.hip, the ReLU convolution and the max-pool of conv.hip): every kernel alone on its smallest
shapes through the diagnostic entries of include/maskbit_hip_diag.h, the whole network against the float64 restatement of the reference
(tests/lpips_reference.py) and the reference's own recorded float64 run (tests/golden/lpips.npz), and the state of ``TokenizerEvaluator.use_lpips``.

Tolerances are derived, none is tuned to what the kernels give:

* convolution + bias + ReLU: tests/test_hip_conv.py's criterion and constants -- per element 2^-11 |y| (the fp16 store) + K 2^-24 sum|w a| (fp32
  accumulation of K = Cin k k products); rms error against the exact layer <= 1.25 x the rms error of the same layer with the output rounded to fp16.
* max-pool and the input kernel: bit-equal (the maximum of fp16 values is exact; the scaling layer is three IEEE fp32 operations and one rounding).
* distance kernel: 1e-5 relative against float64 on the same fp16 features: a dozen fp32 operations per channel and a log2(C)-deep fp32 butterfly,
  of order 1e-6, all terms non-negative; sums across pixels are fp64.
* whole network: E_model = |model - exact| of the case, where `model` is the float64 restatement with fp16 weights and fp16 stored activations.
  Taps: rms error <= 1.5 x the model's, largest error <= 2 x the model's largest.  Per image |hip - exact| <= 2 E, and the same against the
  reference's own float64 value.  The weights are seeded (He-normal and "grown"), not ImageNet VGG16.
"""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import lpips_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U16 = 2.0 ** -11
U32 = 2.0 ** -24


def _lib():
    from maskbit_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def h16r(t):
    return t.to(torch.float16).double()


# ------------------------------------------------------------------------------------------------ convolution + bias + ReLU
def run_conv_relu(x16, w, bias, ks):
    """mb_conv_relu_layer: x16 fp16 NHWC (CPU), w fp32 OIHW -> (out fp16 NHWC on the CPU, saturation count)"""
    L, lib = _lib()
    B, H, W, cin = x16.shape
    cout = w.shape[0]
    xd, wd = x16.to(DEV).contiguous(), w.float().to(DEV).contiguous()
    bd = bias.float().to(DEV).contiguous() if bias is not None else None
    out = torch.full((B, H, W, cout), float("nan"), dtype=torch.float16, device=DEV)
    sat = C.c_uint(0)
    L.check(lib.mb_conv_relu_layer(xd.data_ptr(), wd.data_ptr(), bd.data_ptr() if bd is not None else None, out.data_ptr(), C.byref(sat), B, H, W, cin, cout,
                                   ks, _stream()), "mb_conv_relu_layer")
    torch.cuda.synchronize()
    return out.cpu(), int(sat.value)


def ref_conv_relu(x16, w, bias, ks, rounded):
    a = x16.double().permute(0, 3, 1, 2)
    wq = w.to(torch.float16).double()
    y = F.relu(F.conv2d(a, wq, bias.double() if bias is not None else None, padding=(ks - 1) // 2))
    S = F.conv2d(a.abs(), wq.abs(), None, padding=(ks - 1) // 2)
    return (h16r(y) if rounded else y), S


def check_conv_relu(x16, w, bias, ks, what):
    got16, sat = run_conv_relu(x16, w, bias, ks)
    got = got16.double().permute(0, 3, 1, 2)
    exact, S = ref_conv_relu(x16, w, bias, ks, rounded=False)
    model, _ = ref_conv_relu(x16, w, bias, ks, rounded=True)
    assert got.shape == exact.shape and bool(torch.isfinite(got).all()) and bool((got >= 0).all())
    K = w.shape[1] * ks * ks
    bound = U16 * exact.abs() + K * U32 * S
    err = (got - exact).abs()
    worst = (err / bound.clamp(min=1e-300)).max().item()
    e_kernel, e_model = err.pow(2).mean().sqrt().item(), (model - exact).pow(2).mean().sqrt().item()
    print(f"conv+relu {what}: max err / bound {worst:.3f}; rms err {e_kernel:.3e}, E_model {e_model:.3e}, ratio {e_kernel / e_model:.3f}; "
          f"zeros {float((exact == 0).double().mean()):.2f}")
    assert worst <= 1.0
    assert e_model > 0.0 and e_kernel <= 1.25 * e_model
    assert bool((got[exact == 0] == 0).all())                  # what ReLU cuts is exactly 0
    assert sat == 0


@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128), (512, 512)])
@pytest.mark.parametrize("H,W", [(8, 16), (32, 32)])
def test_conv_relu_layer_vs_fp64(H, W, cin, cout):
    """one 8-row tile per image / four 16-row tiles; a partial (Cout 64) and whole 128-channel output tiles, one and eight input chunks"""
    g = torch.Generator().manual_seed(100 * H + cin + cout)
    x16 = torch.relu(torch.randn(2, H, W, cin, generator=g) * (0.5 + torch.rand(cin, generator=g))).to(torch.float16)       # the output of a ReLU layer
    w = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (cin * 9))
    bias = torch.randn(cout, generator=g) * 0.05
    check_conv_relu(x16, w, bias, 3, f"{cin}->{cout} {H}x{W}")


def lpips_input(real, fake, clamp):
    """mb_lpips_input -> fp16 [2B, H, W, 64] on the CPU"""
    L, lib = _lib()
    B, _, H, W = real.shape
    shift, scale = R.scaling_buffers()
    sc = torch.cat([shift, scale]).to(DEV)
    out = torch.full((2 * B, H, W, 64), float("nan"), dtype=torch.float16, device=DEV)
    rd, fd = real.to(DEV).contiguous(), fake.to(DEV).contiguous()
    L.check(lib.mb_lpips_input(rd.data_ptr(), fd.data_ptr(), sc.data_ptr(), out.data_ptr(), B, H, W, int(clamp), _stream()), "mb_lpips_input")
    torch.cuda.synchronize()
    return out.cpu()


def ref_input_patches(real, fake, clamp):
    """the fp32 expression of the scaling layer (lpips.py:62-63), zero padding after it, the 27 patch values per pixel, rounded to fp16"""
    shift, scale = R.scaling_buffers()
    x = torch.cat([real, fake]).float()
    if clamp:
        x = x.clamp(0.0, 1.0)
    x = x * 2.0 - 1.0
    x = (x - shift.view(1, 3, 1, 1)) / scale.view(1, 3, 1, 1)
    N, _, H, W = x.shape
    p = F.unfold(x, 3, padding=1).reshape(N, 27, H, W).permute(0, 2, 3, 1)          # channel ci * 9 + ky * 3 + kx
    return torch.cat([p, torch.zeros(N, H, W, 37)], dim=-1).to(torch.float16)


@pytest.mark.parametrize("H,W", [(8, 16), (32, 32)])
def test_first_layer_as_1x1_on_patches(H, W):
    """conv1_1 as built: the input kernel's 27-in-64 patches through a ks = 1 convolution whose weight is the OIHW tensor read as [64, 27, 1, 1],
    against the float64 3x3 convolution (zero padding 1) of the fp16-rounded scaled image"""
    from maskbit_amd.synth import make_eval_images
    real, fake = make_eval_images("noise", 0.05, 1, H, W, 31 + H)
    patches = lpips_input(real, fake, False)
    w = R.vgg_weights("he")["0.weight"]
    bias = R.vgg_weights("he")["0.bias"]
    got16, sat = run_conv_relu(patches, torch.cat([w.reshape(64, 27, 1, 1), torch.zeros(64, 37, 1, 1)], 1), bias, 1)
    x16 = patches[..., [4, 13, 22]]                            # the centre taps: the scaled image itself, fp16 NHWC
    exact, S = ref_conv_relu(x16, w, bias, 3, rounded=False)
    model, _ = ref_conv_relu(x16, w, bias, 3, rounded=True)
    got = got16.double().permute(0, 3, 1, 2)
    err = (got - exact).abs()
    worst = (err / (U16 * exact.abs() + 27 * U32 * S).clamp(min=1e-300)).max().item()
    e_kernel, e_model = err.pow(2).mean().sqrt().item(), (model - exact).pow(2).mean().sqrt().item()
    print(f"conv1_1 {H}x{W}: max err / bound {worst:.3f}, rms ratio {e_kernel / e_model:.3f}")
    assert worst <= 1.0 and e_kernel <= 1.25 * e_model and sat == 0


def test_conv_relu_all_negative_gives_exact_zero():
    g = torch.Generator().manual_seed(5)
    x16 = torch.rand(2, 8, 16, 64, generator=g).add(0.1).to(torch.float16)
    w = -torch.rand(128, 64, 3, 3, generator=g) - 0.01
    out, sat = run_conv_relu(x16, w, -torch.rand(128, generator=g), 3)
    assert torch.equal(out, torch.zeros_like(out)) and not bool(torch.signbit(out).any()) and sat == 0


def test_conv_relu_saturation_is_counted():
    """exact outputs of +120000 in known (pixel, 4-channel group) cells are stored as 65504 and counted; -120000 is cut by the ReLU first: not counted"""
    H, W, cin, cout = 16, 32, 64, 128
    pix = [(0, 0), (7, 15), (8, 16), (15, 31), (3, 20)]
    x16 = torch.zeros(2, H, W, cin, dtype=torch.float16)
    for b in range(2):
        for (y, x) in pix:
            x16[b, y, x, 0] = 60000.0
    w = torch.zeros(cout, cin, 1, 1)
    w[:, 0] = 1.0
    for c, v in {0: 2.0, 1: 2.0, 5: 2.0, 64: -2.0, 127: 2.0}.items():       # channels 0 and 1 share a group: 3 positive groups per hot pixel
        w[c, 0] = v
    out, sat = run_conv_relu(x16, w, None, 1)
    assert sat == 2 * len(pix) * 3
    exact, _ = ref_conv_relu(x16, w, None, 1, rounded=False)
    assert torch.equal(out.double().permute(0, 3, 1, 2), exact.clamp(max=65504.0))
    assert float(out[0, 0, 0, 64]) == 0.0 and float(out[0, 0, 0, 2]) == 60000.0


# ------------------------------------------------------------------------------------------------ max-pool, input kernel
@pytest.mark.parametrize("C_", [8, 64])
@pytest.mark.parametrize("H,W", [(2, 2), (8, 16), (6, 10)])
def test_maxpool2_bit_equal(H, W, C_):
    L, lib = _lib()
    g = torch.Generator().manual_seed(H * W + C_)
    x16 = (torch.randn(3, H, W, C_, generator=g) * 8).to(torch.float16)
    x16[0, 0, 0, 0], x16[0, 0, 1, 0] = 65504.0, -65504.0
    xd = x16.to(DEV)
    y = torch.full((3, H // 2, W // 2, C_), float("nan"), dtype=torch.float16, device=DEV)
    L.check(lib.mb_maxpool2(xd.data_ptr(), y.data_ptr(), 3, H, W, C_, _stream()), "mb_maxpool2")
    want = F.max_pool2d(x16.float().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).to(torch.float16)
    assert torch.equal(y.cpu().view(torch.int16), want.contiguous().view(torch.int16))
    assert lib.mb_maxpool2(xd.data_ptr(), y.data_ptr(), 3, H + 1, W, C_, _stream()) != 0 and lib.mb_maxpool2(xd.data_ptr(), y.data_ptr(), 3, H, W, 12, _stream()) != 0


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("H,W", [(8, 16), (5, 7)])
def test_input_kernel_equals_the_fp32_expression(H, W, clamp):
    from maskbit_amd.synth import make_eval_images
    real, fake = make_eval_images("noise", 0.3, 2, H, W, 17 + H)                    # sigma 0.3: the fake images leave [0, 1], the clamp matters
    assert float(fake.min()) < 0.0 and float(fake.max()) > 1.0
    got, want = lpips_input(real, fake, clamp), ref_input_patches(real, fake, clamp)
    assert torch.equal(got.view(torch.int16), want.contiguous().view(torch.int16))
    assert not torch.equal(want, ref_input_patches(real, fake, not clamp))          # the clamp matters on these inputs


# ------------------------------------------------------------------------------------------------ distance kernel
def run_distance(a16, b16, w):
    """mb_lpips_distance: a16 / b16 fp16 [B, HW, C] (CPU), w fp32 [C] -> float64 [B] on the CPU"""
    L, lib = _lib()
    B, HW, C_ = a16.shape
    ad, bd, wd = a16.to(DEV).contiguous(), b16.to(DEV).contiguous(), w.float().to(DEV).contiguous()
    out = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
    L.check(lib.mb_lpips_distance(ad.data_ptr(), bd.data_ptr(), wd.data_ptr(), B, HW, C_, out.data_ptr(), _stream()), "mb_lpips_distance")
    torch.cuda.synchronize()
    return out.cpu()


def ref_distance(a16, b16, w):
    to = lambda t: t.double().permute(0, 2, 1).unsqueeze(-1)                          # [B, C, HW, 1]
    return R.distance64(to(a16), to(b16), w)


def _features(B, HW, C_, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.relu(torch.randn(B, HW, C_, generator=g) + 0.3) * 3.0
    b = torch.relu(a + 0.2 * torch.randn(B, HW, C_, generator=g))
    return a.to(torch.float16), b.to(torch.float16), torch.rand(C_, generator=g)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (8, 16)])
@pytest.mark.parametrize("C_", [64, 128, 256, 512])
def test_distance_vs_fp64(C_, H, W, B):
    HW = H * W
    a16, b16, w = _features(B, HW, C_, 1000 * C_ + 10 * HW + B)
    want = ref_distance(a16, b16, w)
    got = run_distance(a16, b16, w)
    rel = ((got - want).abs() / want).max().item()
    print(f"distance C {C_} {H}x{W} B {B}: value {want.tolist()}, relative error {rel:.2e}")
    assert bool((want > 0).all()) and rel <= 1e-5
    # identical maps: exactly 0
    assert torch.equal(run_distance(a16, a16.clone(), w), torch.zeros(B, dtype=torch.float64))
    # all-zero pixels (in both maps; in one map only): the eps path, no NaN, the value of the float64 expression
    az, bz = a16.clone(), b16.clone()
    az[:, 0], bz[:, 0] = 0, 0
    if HW > 1:
        az[:, 1] = 0
    got, want = run_distance(az, bz, w), ref_distance(az, bz, w)
    assert bool(torch.isfinite(got).all())
    if HW > 1:
        assert ((got - want).abs() / want).max().item() <= 1e-5
    else:
        assert torch.equal(got, torch.zeros(B, dtype=torch.float64)) and bool((want.abs() < 1e-300).all())


@pytest.mark.parametrize("C_", [64, 128, 256, 512])
def test_distance_of_one_ulp_in_one_channel(C_):
    """the cancellation case: maps that differ in one fp16 ulp of one channel of one pixel -- a value of the order of 1e-9, within the same bound"""
    B, HW = 1, 15
    a16, _, w = _features(B, HW, C_, 7 * C_)
    w = w + 0.1
    c = int(torch.argmax(a16[0, 7].float()))
    assert float(a16[0, 7, c]) > 1.0
    small = a16[0, 14].float()
    small[small == 0] = float("inf")
    for (p, ch) in ((7, c), (14, int(torch.argmin(small)))):   # the pixel's largest channel; another pixel's smallest positive one
        b16 = a16.clone()
        bits = b16.view(torch.int16)
        bits[0, p, ch] += 1
        assert int((b16 != a16).sum()) == 1
        got, want = run_distance(a16, b16, w), ref_distance(a16, b16, w)
        rel = ((got - want).abs() / want).max().item()
        print(f"one ulp, C {C_} pixel {p}: value {want.item():.3e}, relative error {rel:.2e}")
        assert float(want) > 0 and rel <= 1e-5


# ------------------------------------------------------------------------------------------------ whole network
@functools.lru_cache(maxsize=None)
def hip_model(style):
    from maskbit_amd import LPIPS
    m = LPIPS()
    m.load_state_dict(R.reference_state_dict(R.vgg_weights(style), R.lin_vectors()), strict=True)
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def hip_case(name):
    """one mb_lpips_features + one per_image of the case -> (taps float64 NCHW [2B, ...] on the CPU, per image float64 [B], saturation count)"""
    L, lib = _lib()
    fam, sig, B, H, W, seed, style = R.CASES[name]
    m = hip_model(style)
    real, fake = R.case_images(name)
    rd, fd = real.to(DEV), fake.to(DEV)
    m.saturation_count()
    val = m.per_image(rd, fd)
    taps = [torch.full((2 * B, H >> k, W >> k, c), float("nan"), dtype=torch.float16, device=DEV) for k, c in enumerate(R.TAP_CHANNELS)]
    L.check(lib.mb_lpips_features(m._engine, rd.data_ptr(), fd.data_ptr(), B, H, W, 0, *[t.data_ptr() for t in taps], _stream()), "mb_lpips_features")
    sat = m.saturation_count()
    return [t.cpu().double().permute(0, 3, 1, 2) for t in taps], val.cpu(), sat


@pytest.mark.parametrize("name", list(R.ENGINE_CASES))
def test_network_taps_and_value(name):
    o = R.case_oracle(name)
    taps, val, sat = hip_case(name)
    z = R.golden()
    for k, (got, exact, model) in enumerate(zip(taps, o["exact_taps"], o["model_taps"])):
        assert got.shape == exact.shape and bool(torch.isfinite(got).all())
        e_hip, e_mod = (got - exact), (model - exact)
        r_rms = (e_hip.pow(2).mean().sqrt() / e_mod.pow(2).mean().sqrt()).item()
        r_max = (e_hip.abs().max() / e_mod.abs().max()).item()
        print(f"{name} tap {k}: rms error / model's {r_rms:.3f}, max error / model's {r_max:.3f}")
        assert r_rms <= 1.5 and r_max <= 2.0
    E = float((o["model"] - o["exact"]).abs().max())
    ref64 = torch.from_numpy(z[name + ".ref64"])
    d_exact, d_ref = (val - o["exact"]).abs(), (val - ref64).abs()
    print(f"{name}: hip {val.tolist()} exact {o['exact'].tolist()} E {E:.3e}; |hip - exact| / E {(d_exact / E).tolist()}, |hip - ref64| / E {(d_ref / E).tolist()}")
    assert E > 0 and bool((d_exact <= 2 * E).all()) and bool((d_ref <= 2 * E).all())
    assert sat == 0


# ------------------------------------------------------------------------------------------------ state and invariance (bit-exact)
def _pairs(n, seed=9):
    from maskbit_amd.synth import make_eval_images
    real, fake = make_eval_images("noise", 0.05, n, 128, 256, seed)
    return real.to(DEV), fake.to(DEV)


def _evaluator(model):
    from maskbit_amd import TokenizerEvaluator
    ev = TokenizerEvaluator(DEV, enable_mae_error=True)
    ev.use_lpips(model)
    return ev


def test_evaluator_state_is_bit_exact():
    m = hip_model("he")
    real, fake = _pairs(5)
    ev = _evaluator(m)
    ev.update(real, fake)
    v5, s5 = ev.last_lpips.clone(), ev._lpips_sum.clone()
    assert ev.last_per_image.shape == (5, 3) and v5.shape == (5,) and v5.dtype == torch.float64
    # forward == per_image == last_lpips
    assert torch.equal(m.per_image(real, fake), v5) and torch.equal(m(real, fake), v5.float().view(5, 1, 1, 1))
    # the running sum is the in-order float64 sum of the per-image values
    t = 0.0
    for v in v5.tolist():
        t += v
    assert float(s5) == t and ev.result()["LPIPS"] == t / 5 and list(ev.result()) == ["MAE", "LPIPS"]
    # B = 1 equals the same pair inside the batch of 5
    for b in (0, 3, 4):
        assert torch.equal(m.per_image(real[b:b + 1], fake[b:b + 1]), v5[b:b + 1])
    # 5 = 2 + 3
    ev.reset_metrics()
    assert float(ev._lpips_sum) == 0.0 and ev.last_lpips is None
    ev.update(real[:2], fake[:2])
    first = ev.last_lpips.clone()
    ev.update(real[2:], fake[2:])
    assert torch.equal(torch.cat([first, ev.last_lpips]), v5) and torch.equal(ev._lpips_sum, s5) and ev.result()["LPIPS"] == t / 5
    # the same update twice doubles the sum (one pair: s + s is exact; five: the in-order sum continued)
    ev.reset_metrics()
    ev.update(real[:1], fake[:1])
    ev.update(real[:1], fake[:1])
    assert float(ev._lpips_sum) == 2.0 * float(v5[0])
    ev.reset_metrics()
    ev.update(real, fake)
    ev.update(real, fake)
    for v in v5.tolist():
        t += v
    assert float(ev._lpips_sum) == t and ev._num_examples == 10
    # detached: no LPIPS any more
    ev.use_lpips(None)
    ev.reset_metrics()
    ev.update(real[:1], fake[:1])
    assert list(ev.result()) == ["MAE"] and ev.last_lpips is None


def test_batch_beyond_the_capacity_equals_its_chunks():
    from maskbit_amd import LPIPS
    real, fake = _pairs(5, seed=10)
    whole = hip_model("he").per_image(real, fake)
    m = LPIPS()
    m.load_state_dict(hip_model("he").state_dict(), strict=True)
    m = m.to(DEV)
    m.max_pairs_per_call = 1                                   # 128 x 256 images are half the area the bound is stated for: chunks of 2 pairs
    ev = _evaluator(m)
    ev.update(real, fake)
    assert m._engine_key[1] == 2
    assert torch.equal(ev.last_lpips, whole)
    t = 0.0
    for v in whole.tolist():
        t += v
    assert float(ev._lpips_sum) == t
    # clamp is honoured: images that leave [0, 1]
    real2, fake2 = real * 1.3 - 0.15, fake * 1.3 - 0.15
    a = m.per_image(real2, fake2, clamp=True)
    assert torch.equal(a, m.per_image(real2.clamp(0, 1), fake2.clamp(0, 1))) and not torch.equal(a, m.per_image(real2, fake2))


# ------------------------------------------------------------------------------------------------ integration
def test_eval_reconstruction_reports_lpips():
    from maskbit_amd import eval_reconstruction
    from hip_helpers import hip_tokenizer
    from oracle import maskbit_oracle as O
    tc = O.TokCfg(token_size=12, hidden_channels=64, channel_mult=(1, 1, 2), num_resolutions=3, num_res_blocks=1)
    tok = hip_tokenizer(tc, O.make_tokenizer_weights(tc, seed=21, with_encoder=True), DEV)
    g = torch.Generator().manual_seed(78)
    loader = [{"image": torch.rand(2, 3, 256, 256, generator=g) * 1.2 - 0.1} for _ in range(2)]
    m = hip_model("he")
    ev = _evaluator(m)
    r = eval_reconstruction(tok, loader, ev)
    assert list(r) == ["MAE", "LPIPS"] and ev._num_examples == 4
    vals = []
    for batch in loader:
        img = batch["image"].to(DEV)
        rec, _ = tok(img)
        vals.append(m.per_image(img, rec, clamp=True))
    vals = torch.cat(vals).cpu()
    t = 0.0
    for v in vals.tolist():
        t += v
    print(f"eval_reconstruction: LPIPS {r['LPIPS']:.6f} per image {vals.tolist()}")
    assert r["LPIPS"] == t / 4 and 0.0 < r["LPIPS"] < 10.0 and m.saturation_count() == 0


def test_unsupported_sizes_raise_before_any_device_work():
    m = hip_model("he")
    ev = _evaluator(m)
    ok = torch.rand(1, 3, 128, 256, device=DEV)
    ev.update(ok, ok)
    state = (ev._lpips_sum.clone(), ev._sums.clone(), ev._num_examples, ev._num_updates, ev.last_lpips)
    for shape in ((3, 3, 64, 64), (3, 3, 37, 50), (1, 3, 256, 128), (1, 1, 128, 256), (1, 4, 128, 256)):
        x = torch.rand(*shape, device=DEV)
        with pytest.raises(ValueError):
            ev.update(x, x)
        with pytest.raises(ValueError):
            m.per_image(x, x)
        with pytest.raises(ValueError):
            m(x, x)
    assert torch.equal(ev._lpips_sum, state[0]) and torch.equal(ev._sums, state[1]) and (ev._num_examples, ev._num_updates) == state[2:4]
    assert ev.last_lpips is state[4]
    # the C entry refuses them too, with the constraint in the message
    L, lib = _lib()
    out = torch.zeros(1, dtype=torch.float64, device=DEV)
    assert lib.mb_lpips_forward(m._engine, ok.data_ptr(), ok.data_ptr(), 1, 64, 64, 0, out.data_ptr(), None, _stream()) != 0
    assert b"multiple of 128" in lib.mb_last_error()
    assert lib.mb_lpips_forward(m._engine, ok.data_ptr(), ok.data_ptr(), 0, 128, 256, 0, out.data_ptr(), None, _stream()) != 0
    from maskbit_amd import LPIPS
    empty = LPIPS().to(DEV)
    with pytest.raises(RuntimeError, match="load_vgg16"):
        empty(ok, ok)
