"""The Inception-v3 feature extractor on the HIP path (maskbit_amd/csrc/inception.hip): the convolution, pool and input kernels alone on their
smallest shapes through the diagnostic entries of include/maskbit_hip_diag.h (``repack_convbn_kernel`` runs inside ``mb_convbn_layer``; the fp32
tail -- ``bn_fold_kernel``, ``spatial_mean_kernel``, ``fc_head_kernel``, ``channel_tap_kernel`` -- has its per-launch tests in
tests/test_hip_convnet_tail.py), the whole network against the float64 restatement of the specification (tests/inception_reference.py) on
seeded weights, and the product surface (``InceptionV3``, the evaluators' ``use_inception``).

Tolerances are derived, none is tuned to what the kernels give:

* convolution + BatchNorm + ReLU: tests/test_hip_lpips.py's criterion and constants -- per element 2^-11 |y| (the fp16 store) + K 2^-24 S with
  S = |scale| sum |w a| + |shift| (fp32 accumulation of K = Cin kh kw products and the fp32 epilogue); rms error against the exact layer
  <= 1.25 x the rms error of the same layer with the output rounded to fp16; what ReLU cuts is exactly 0.
* integer-valued operands (sums exact in fp32, power-of-two scales): bit-equal to float64 rounded once to fp16, for both tile shapes.
* pools: the maximum of fp16 values is exact; the average is the stated fp32 expression (sequential adds in row-major tap order, one division,
  one rounding): bit-equal.
* input kernel: 2^-11 |exact| (the fp16 store) + 8 x 2^-24 (the fp32 evaluation of two nested interpolations of values up to 255, over 128).
* whole network: the four fp16 maps have error rms <= 1.5 x and max <= 2 x the model's (`model` = the float64 restatement with fp16 weights
  and fp16 stored activations); every fp32 output is within 2 E of exact, E = max |model - exact|.  The weights are seeded, not the checkpoint.
* the network's fp32 tail, on the same run's buffers: ``192``, ``768`` and ``2048`` are bit-equal to the stated fp32 mean
  (convnet_reference.spatial_mean32) of the run's own fp16 maps; both logits are within (2048 / 64 + 7) 2^-24 (sum |p w| + |bias|) of the float64
  head of the run's own fp32 pooled features; ``logits`` is ``logits_unbiased`` plus the bias in one fp32 add.
"""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import convnet_reference as CR
import inception_reference as R
from convnet_helpers import DEV, U16, U32, _lib, _stream, bits, bits32, check_against_fp64, integer_case, ref_convbn, run_convbn, run_pool

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ convolution + BatchNorm + ReLU
# run_convbn, ref_convbn, check_against_fp64 and integer_case live in tests/convnet_helpers.py (imported above), shared with the ResNet tests
def pad_channels(x16, fill=float("nan")):
    """the 3-channel image as the engine holds it: in 8-channel pixels; the pad channels hold `fill`, which must never be read into a product"""
    B, H, W, cin = x16.shape
    cs = (cin + 7) // 8 * 8
    if cs == cin:
        return x16
    buf = torch.full((B, H, W, cs), fill, dtype=torch.float16)
    buf[..., :cin] = x16
    return buf


@pytest.mark.parametrize("name", list(R.CONV_CASES))
def test_convbn_layer_vs_fp64(name):
    B, H, W, cin, cout, k, stride, pad = R.CONV_CASES[name]
    x16, w, scale, shift = R.conv_case(name, seed=4500 + cin + cout)
    got16, sat = run_convbn(pad_channels(x16), w, scale, shift, stride, pad)
    exact, S = ref_convbn(x16, w, scale, shift, stride, pad)
    check_against_fp64(f"{name} B {B}", got16, exact, S, cin * k[0] * k[1])        # K 2^-24 S: the K products' accumulation
    assert sat == 0


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("name", list(R.CONV_CASES))
def test_convbn_layer_integer_operands_are_bit_exact(name, variant):
    """every kernel shape, both wave tiles: the tile walk, the tap geometry and the K tail decide every bit here"""
    B, H, W, cin, cout, k, stride, pad = R.CONV_CASES[name]
    x16, w, scale, shift, _ = integer_case(4600 + cin, B, H, W, cin, cout, k)
    exact, _ = ref_convbn(x16, w, scale, shift, stride, pad)
    assert float(exact.max()) > 0 and cin * k[0] * k[1] * 6 < 2 ** 24
    got16, sat = run_convbn(pad_channels(x16), w, scale, shift, stride, pad, variant=variant)
    want16 = R.h16r(exact).permute(0, 2, 3, 1).to(torch.float16)
    assert torch.equal(bits(got16), bits(want16)) and sat == 0


def test_convbn_tile_shapes_give_the_same_bits():
    name = "160->192 7x1 17x17"                                # B = 3: 867 pixels, tiles straddle the images
    B, H, W, cin, cout, k, stride, pad = R.CONV_CASES[name]
    x16, w, scale, shift = R.conv_case(name, seed=4700)
    a, _ = run_convbn(x16, w, scale, shift, stride, pad, variant=1)
    b, _ = run_convbn(x16, w, scale, shift, stride, pad, variant=2)
    assert torch.equal(bits(a), bits(b))
    # an image alone gives its part of the batch: a pixel's bits do not depend on its tile, its image index or the batch
    for i in range(B):
        for variant in (1, 2):
            one, _ = run_convbn(x16[i:i + 1], w, scale, shift, stride, pad, variant=variant)
            assert torch.equal(bits(one), bits(a[i:i + 1]))


def test_convbn_output_slice_leaves_the_rest_untouched():
    """a branch writes channels [64, 160) of the 288-wide concatenation: every other byte keeps the sentinel"""
    g = torch.Generator().manual_seed(4800)
    x16 = torch.relu(torch.randn(2, 9, 9, 64, generator=g)).to(torch.float16)
    w = torch.randn(96, 64, 3, 3, generator=g) * (2.0 / 576) ** 0.5
    scale, shift = 0.5 + torch.rand(96, generator=g), torch.randn(96, generator=g) * 0.1
    dense, _ = run_convbn(x16, w, scale, shift, 1, (1, 1))
    sentinel = torch.full((2, 9, 9, 288), -1234.0, dtype=torch.float16)
    for variant in (1, 2):
        out, sat = run_convbn(x16, w, scale, shift, 1, (1, 1), out=sentinel.clone(), out_off=64, variant=variant)
        assert torch.equal(bits(out[..., 64:160]), bits(dense)) and sat == 0
        assert bool((out[..., :64] == -1234.0).all()) and bool((out[..., 160:] == -1234.0).all())


@pytest.mark.parametrize("cin,cout,k,pad", [(80, 192, (3, 3), (0, 0)), (48, 64, (5, 5), (2, 2)), (160, 192, (7, 1), (3, 0))])
def test_convbn_input_slice_beside_nan(cin, cout, k, pad):
    """the input is a channel slice whose neighbours hold NaN, the slice ends where the buffer ends, and Cin is no multiple of the 32-channel step:
    the K tail and the taps outside the image are masked on the load (a NaN times a zero weight would be NaN) -- finite, and the dense result
    bit for bit"""
    g = torch.Generator().manual_seed(4900 + cin)
    B, H, W = 2, 9, 9
    x16 = torch.relu(torch.randn(B, H, W, cin, generator=g)).to(torch.float16)
    w = torch.randn(cout, cin, *k, generator=g) * (2.0 / (cin * k[0] * k[1])) ** 0.5
    scale, shift = 0.5 + torch.rand(cout, generator=g), torch.randn(cout, generator=g) * 0.1
    dense, _ = run_convbn(x16, w, scale, shift, 1, pad)
    assert bool(torch.isfinite(dense).all())
    off = 32
    buf = torch.full((B, H, W, off + cin), float("nan"), dtype=torch.float16)          # the last pixel's slice ends with the buffer
    buf[..., off:] = x16
    wide = torch.full((B, H, W, off + cin + 64), float("nan"), dtype=torch.float16)     # NaN on both sides
    wide[..., off:off + cin] = x16
    for variant in (1, 2):
        for b in (buf, wide):
            got, sat = run_convbn(b, w, scale, shift, 1, pad, in_off=off, variant=variant)
            assert bool(torch.isfinite(got).all()) and torch.equal(bits(got), bits(dense)) and sat == 0


def test_convbn_saturation_is_counted():
    """exact outputs of +120000 in known (pixel, 4-channel group) cells are stored as 65504 and counted; -120000 is cut by the ReLU first: not counted"""
    H, W, cin, cout = 9, 11, 32, 128
    pix = [(0, 0), (4, 5), (8, 10), (3, 7), (8, 0)]
    x16 = torch.zeros(2, H, W, cin, dtype=torch.float16)
    for b in range(2):
        for (y, x) in pix:
            x16[b, y, x, 0] = 60000.0
    w = torch.zeros(cout, cin, 1, 1)
    w[:, 0] = 1.0
    for c, v in {0: 2.0, 1: 2.0, 5: 2.0, 64: -2.0, 127: 2.0}.items():       # channels 0 and 1 share a group: 3 positive groups per hot pixel
        w[c, 0] = v
    for variant in (1, 2):
        out, sat = run_convbn(x16, w, torch.ones(cout), torch.zeros(cout), 1, (0, 0), variant=variant)
        assert sat == 2 * len(pix) * 3
        exact, _ = ref_convbn(x16, w, torch.ones(cout), torch.zeros(cout), 1, (0, 0))
        assert torch.equal(out.double().permute(0, 3, 1, 2), exact.clamp(max=65504.0))
        assert float(out[0, 0, 0, 64]) == 0.0 and float(out[0, 0, 0, 2]) == 60000.0


def test_convbn_refuses_what_it_does_not_take():
    L, lib = _lib()
    x = torch.zeros(1, 9, 9, 32, dtype=torch.float16, device=DEV)
    w = torch.zeros(32, 32, 3, 3, device=DEV)
    v = torch.zeros(32, device=DEV)
    out = torch.zeros(1, 9, 9, 32, dtype=torch.float16, device=DEV)
    sat = C.c_uint(0)

    def call(**kw):
        a = dict(B=1, H=9, W=9, cin=32, cout=32, kh=3, kw=3, stride=1, ph=1, pw=1, in_off=0, in_cs=32, out_off=0, out_cs=32, variant=0)
        a.update(kw)
        return lib.mb_convbn_layer(x.data_ptr(), w.data_ptr(), v.data_ptr(), v.data_ptr(), out.data_ptr(), C.byref(sat), *a.values(), _stream())

    assert call() == 0
    for bad in (dict(stride=3), dict(kh=9), dict(ph=3), dict(in_off=4), dict(in_cs=24), dict(out_off=2), dict(out_cs=16), dict(cout=30), dict(H=2, ph=0),
                dict(variant=3), dict(B=0)):
        assert call(**bad) != 0, bad
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ pools
def ref_avgpool(x16):
    """the stated fp32 expression: the in-image taps added one after the other in row-major order, divided by their number, rounded once"""
    x = x16.float().permute(0, 3, 1, 2)
    B, C_, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    ones = F.pad(torch.ones(1, 1, H, W), (1, 1, 1, 1))
    s, n = torch.zeros_like(x), torch.zeros(1, 1, H, W)
    for dy in range(3):
        for dx in range(3):
            s = s + xp[:, :, dy:dy + H, dx:dx + W]             # a padded tap adds +0.0: the sum's bits are those of the in-image taps alone
            n = n + ones[:, :, dy:dy + H, dx:dx + W]
    return (s / n).permute(0, 2, 3, 1).to(torch.float16), n


def pool_input(H, W, C_):
    g = torch.Generator().manual_seed(H * W + C_)
    x16 = (torch.randn(3, H, W, C_, generator=g) * 8).to(torch.float16)
    x16[..., 1] = -x16[..., 1].abs() - 1.0                     # an all-negative channel: a padded border must not win with 0
    x16[0, 0, 0, 0], x16[0, 0, 1, 0] = 65504.0, -65504.0
    return x16


@pytest.mark.parametrize("C_", [48, 288])
@pytest.mark.parametrize("H,W", [(9, 9), (17, 17), (8, 8)])
def test_pools_bit_equal(H, W, C_):
    x16 = pool_input(H, W, C_)
    x = x16.float().permute(0, 3, 1, 2)
    want0 = F.max_pool2d(x, 3, 2).permute(0, 2, 3, 1).to(torch.float16)
    want1 = F.max_pool2d(x, 3, 1, 1).permute(0, 2, 3, 1).to(torch.float16)
    got0, got1, got2 = run_pool(x16, 0), run_pool(x16, 1), run_pool(x16, 2)
    assert got0.shape == want0.shape and torch.equal(bits(got0), bits(want0))
    assert torch.equal(bits(got1), bits(want1)) and bool(torch.isfinite(got1).all()) and bool((got1[..., 1] < 0).all())
    want2, n = ref_avgpool(x16)
    assert sorted(set(n.flatten().tolist())) == [4.0, 6.0, 9.0]
    assert torch.equal(bits(got2), bits(want2)) and bool((got2[..., 1] < 0).all())
    # into a channel slice, as Mixed_6a / Mixed_7a place the pooled input in the concatenation
    sentinel = torch.full((3, got0.shape[1], got0.shape[2], C_ + 72), -1234.0, dtype=torch.float16)
    out = run_pool(x16, 0, out=sentinel.clone(), out_off=40)
    assert torch.equal(bits(out[..., 40:40 + C_]), bits(want0)) and bool((out[..., :40] == -1234.0).all()) and bool((out[..., 40 + C_:] == -1234.0).all())


def test_pool_refuses_what_it_does_not_take():
    L, lib = _lib()
    x = torch.zeros(1, 9, 9, 48, dtype=torch.float16, device=DEV)
    y = torch.zeros(1, 9, 9, 48, dtype=torch.float16, device=DEV)
    args = lambda **kw: list({**dict(B=1, H=9, W=9, C=48, mode=1, in_off=0, in_cs=48, out_off=0, out_cs=48), **kw}.values())
    assert lib.mb_pool3(x.data_ptr(), y.data_ptr(), *args(), _stream()) == 0
    for bad in (dict(mode=3), dict(C=44), dict(in_cs=40), dict(out_off=4), dict(mode=0, H=2), dict(B=0)):
        assert lib.mb_pool3(x.data_ptr(), y.data_ptr(), *args(**bad), _stream()) != 0, bad
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ input kernel
def run_input(u8):
    L, lib = _lib()
    B, _, H, W = u8.shape
    ud = u8.to(DEV).contiguous()
    out = torch.full((B, R.SIDE, R.SIDE, 8), float("nan"), dtype=torch.float16, device=DEV)
    L.check(lib.mb_inception_input(ud.data_ptr(), out.data_ptr(), B, H, W, _stream()), "mb_inception_input")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("H,W", [(4, 4), (37, 50), (256, 256)])
def test_input_kernel_vs_fp64(H, W):
    u8 = torch.randint(0, 256, (2, 3, H, W), generator=torch.Generator().manual_seed(H + W), dtype=torch.uint8)
    got = run_input(u8)
    exact = R.input64(u8).permute(0, 2, 3, 1)
    err = (got[..., :3].double() - exact).abs()
    bound = U16 * exact.abs() + 8 * U32
    print(f"input {H}x{W}: max err / bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(got[..., 3:], torch.zeros_like(got[..., 3:]))


def test_input_kernel_of_the_network_size_is_exact():
    u8 = torch.randint(0, 256, (2, 3, 299, 299), generator=torch.Generator().manual_seed(299), dtype=torch.uint8)
    u8[0, :, 0, 0], u8[0, :, 0, 1] = 0, 255
    got = run_input(u8)
    want = ((u8.double() - 128.0) / 128.0).permute(0, 2, 3, 1).to(torch.float16)
    assert torch.equal(bits(got[..., :3]), bits(want))


# ------------------------------------------------------------------------------------------------ whole network
@functools.lru_cache(maxsize=None)
def hip_model(style):
    from maskbit_amd import InceptionV3
    m = InceptionV3(["64", "192", "768", "2048", "logits_unbiased", "logits"])
    m.load_weights(R.weights(style))
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def hip_case(name):
    """one mb_inception_taps of the case -> (the four maps float64 NCHW on the CPU, dict of the fp32 outputs as float64, saturation count)"""
    L, lib = _lib()
    B, H, W, _seed, style = R.CASES[name]
    m = hip_model(style)
    u8 = R.case_images(name).to(DEV)
    h = m.engine(B)
    m.saturation_count()
    maps = [torch.full((B, s, s, c), float("nan"), dtype=torch.float16, device=DEV) for s, c in R.MAP_SHAPES]
    keys = ("64", "192", "768", "2048", "logits_unbiased", "logits")
    outs = {k: torch.full((B, w), float("nan"), dtype=torch.float32, device=DEV) for k, w in zip(keys, (64, 192, 768, 2048, 1008, 1008))}
    L.check(lib.mb_inception_taps(h, u8.data_ptr(), B, H, W, *[t.data_ptr() for t in maps], *[outs[k].data_ptr() for k in keys], _stream()), "mb_inception_taps")
    sat = m.saturation_count()
    return [t.cpu().double().permute(0, 3, 1, 2) for t in maps], {k: v.cpu().double() for k, v in outs.items()}, sat


@pytest.mark.parametrize("name", list(R.CASES))
def test_network_maps_and_features(name):
    exact, model = R.case_oracle(name)
    maps, outs, sat = hip_case(name)
    for k, (got, ex, mo) in enumerate(zip(maps, exact["maps"], model["maps"])):
        assert got.shape == ex.shape and bool(torch.isfinite(got).all())
        e_hip, e_mod = (got - ex), (mo - ex)
        r_rms = (e_hip.pow(2).mean().sqrt() / e_mod.pow(2).mean().sqrt()).item()
        r_max = (e_hip.abs().max() / e_mod.abs().max()).item()
        print(f"{name} {R.MAP_NAMES[k]}: rms error / model's {r_rms:.3f}, max error / model's {r_max:.3f}")
        assert r_rms <= 1.5 and r_max <= 2.0
    for k, got in outs.items():
        E = float((model[k] - exact[k]).abs().max())
        d = float((got - exact[k]).abs().max())
        print(f"{name} {k}: E {E:.3e}, |hip - exact| / E {d / E:.3f}")
        assert got.shape == exact[k].shape and E > 0 and d <= 2 * E
    assert sat == 0
    # the fp32 tail on the run's own buffers, in its own unit: the taps and the pooled features are the stated fp32 mean of the fp16 maps the same
    # run handed out (map 0: the 192-channel pool, 2: Mixed_6e, 3: Mixed_7c), the logits the head of the run's own fp32 pooled features
    nhwc16 = lambda m: m.permute(0, 2, 3, 1).reshape(m.shape[0], -1, m.shape[1]).to(torch.float16)
    for key, k in (("192", 0), ("768", 2), ("2048", 3)):
        assert torch.equal(bits32(outs[key].float()), bits32(CR.spatial_mean32(nhwc16(maps[k])))), key
    sd = R.weights(R.CASES[name][4])
    pool32 = outs["2048"].float()
    head_u, head_b, S = CR.fc_head64(pool32, sd["fc.weight"], sd["fc.bias"])
    bound = CR.head_bound(2048, S)
    for key, want in (("logits_unbiased", head_u), ("logits", head_b)):
        err = (outs[key] - want).abs()
        print(f"{name} {key} against the float64 head of its own pool: worst err / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())
    assert torch.equal(bits32(outs["logits"].float()), bits32(outs["logits_unbiased"].float() + sd["fc.bias"].float()))


# ------------------------------------------------------------------------------------------------ the product
def _images(n, seed=9, side=64):
    return R.images_u8(n, side, side, seed).to(DEV)


def _fresh(style="he", features=None):
    from maskbit_amd import InceptionV3
    m = InceptionV3(features) if features else InceptionV3()
    m.load_weights(R.weights(style))
    return m.to(DEV)


def test_forward_keys_dtypes_and_devices():
    x = _images(2)
    out = _fresh()(x)
    assert list(out) == ["2048", "logits_unbiased"]
    assert tuple(out["2048"].shape) == (2, 2048) and tuple(out["logits_unbiased"].shape) == (2, 1008)
    assert all(v.dtype == torch.float32 and v.device.type == "cuda" and bool(torch.isfinite(v).all()) for v in out.values())
    every = hip_model("he")(x)
    assert list(every) == ["64", "192", "768", "2048", "logits_unbiased", "logits"]
    assert [tuple(v.shape) for v in every.values()] == [(2, 64), (2, 192), (2, 768), (2, 2048), (2, 1008), (2, 1008)]
    assert torch.equal(every["2048"], out["2048"]) and torch.equal(every["logits_unbiased"], out["logits_unbiased"])      # the same forward behind both entries
    bias = R.weights("he")["fc.bias"].to(DEV)
    assert torch.equal(every["logits"], every["logits_unbiased"] + bias)


def test_rows_do_not_depend_on_the_batch_or_the_chunking():
    x = _images(5, seed=10)
    m = hip_model("he")
    whole = m(x)
    again = m(x)
    assert all(torch.equal(whole[k], again[k]) for k in whole)                     # two runs: bit-identical
    small = _fresh(features=list(whole))
    small.max_images_per_call = 2                                                  # 5 = 2 + 2 + 1
    chunked = small(x)
    assert small._engine_key[1] == 2
    assert all(torch.equal(whole[k], chunked[k]) for k in whole)
    for b in range(5):
        one = m(x[b:b + 1])
        assert all(torch.equal(one[k], whole[k][b:b + 1]) for k in whole), b
    assert m.saturation_count() == 0


def test_generator_evaluator_takes_the_network():
    from maskbit_amd import GeneratorEvaluator, get_inception_model
    net = get_inception_model(R.weights("tf")).to(DEV)
    stats = (torch.zeros(2048, dtype=torch.float64), torch.eye(2048, dtype=torch.float64))
    x = _images(6, seed=11)
    a = GeneratorEvaluator(DEV, enable_fid=True, enable_inception_score=True)
    a.use_inception(net, stats)
    a.update_uint8(x[:4])
    a.update_uint8(x[4:])
    feats = net(x)
    b = GeneratorEvaluator(DEV, enable_fid=True, enable_inception_score=True)
    b.use_inception(net, stats)
    b.update_features(feats["2048"][:4], feats["logits_unbiased"][:4])
    b.update_features(feats["2048"][4:], feats["logits_unbiased"][4:])
    ra, rb = a.result(), b.result()
    print(f"GeneratorEvaluator on the HIP network: {ra}")
    assert ra == rb and len(ra) >= 2 and all(v == v for v in ra.values())


def test_tokenizer_evaluator_takes_the_network():
    from maskbit_amd import TokenizerEvaluator
    net = _fresh("he")
    ev = TokenizerEvaluator(DEV, enable_mae_error=True)
    ev.use_inception(net)
    g = torch.Generator().manual_seed(12)
    real = torch.rand(3, 3, 64, 64, generator=g).to(DEV)
    fake = (real + 0.05 * torch.randn(3, 3, 64, 64, generator=g).to(DEV)).clamp(0, 1)
    ev.update(real, fake)
    r = ev.result()
    print(f"TokenizerEvaluator on the HIP network: {r}")
    assert "MAE" in r and len(r) >= 2 and all(v == v for v in r.values())


def test_forward_refuses_before_any_device_work():
    from maskbit_amd import InceptionV3
    m = hip_model("he")
    ok = _images(1)
    for bad in (ok.float(), ok[:, :1], ok[0]):
        with pytest.raises(ValueError):
            m(bad)
    with pytest.raises(RuntimeError, match="load_weights"):
        InceptionV3().to(DEV)(ok)
    # the C entry refuses what the handle does not take, with no launch
    L, lib = _lib()
    h = m.engine(1)
    out = torch.zeros(1, 2048, device=DEV)
    assert lib.mb_inception_forward(h, ok.data_ptr(), 0, 64, 64, out.data_ptr(), None, None, _stream()) != 0
    assert lib.mb_inception_forward(h, ok.data_ptr(), 1, 1, 64, out.data_ptr(), None, None, _stream()) != 0
    assert lib.mb_inception_forward(h, ok.data_ptr(), m._engine_key[1] + 1, 64, 64, out.data_ptr(), None, None, _stream()) != 0
    hh = C.c_void_p()
    L.check(lib.mb_inception_create(1, C.byref(hh)), "mb_inception_create")
    assert lib.mb_inception_forward(hh, ok.data_ptr(), 1, 64, 64, out.data_ptr(), None, None, _stream()) != 0
    assert b"not complete" in lib.mb_last_error()
    lib.mb_inception_destroy(hh)
