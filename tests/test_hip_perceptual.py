"""The ResNet-50 perceptual loss on the HIP path (maskbit_amd/csrc/resnet.hip and the epilogues of csrc/inception.hip): every kernel resnet.hip
adds and every new epilogue alone on its smallest shapes through the diagnostic entries of include/maskbit_hip_diag.h (the fp32 tail it shares
with Inception-v3 -- ``bn_fold_kernel`` at eps 1e-5, ``spatial_mean_kernel``, ``fc_head_kernel`` -- has its per-launch tests, and the fold of
each of the 53 BatchNorms, in tests/test_hip_convnet_tail.py), the trunk against the float64 restatement of the specification
(tests/resnet_reference.py) on seeded weights at two small sides, the whole path at two image sizes, and the product surface (``PerceptualLoss``,
``TokenizerEvaluator.use_perceptual``).

Tolerances are derived, none is tuned to what the kernels give:

* input kernel: 2^-11 |exact| (the fp16 store) + 2^-24 |exact| (the division) + (ny + nx + 4) 2^-24 max|x| / min(std) -- the fp32 weights, one
  rounding per fma over the ny + nx taps of a pixel's row and column sums (weights sum to 1), the subtraction; at 224 x 224 bit-equal to torch's fp32.
* convolution + BatchNorm + epilogue: tests/test_hip_inception.py's criterion -- per element 2^-11 |y| + (K + 1) 2^-24 S with S = |scale| sum |w a| +
  |shift| (+ |identity|); rms error <= 1.25 x the rms error of the same layer with the output rounded to fp16.
* integer-valued operands: bit-equal to float64 rounded once to fp16, for both tile shapes.
* pool: the maximum of fp16 values is exact: bit-equal.
* trunk: the four fp16 layer maps have error rms <= 1.5 x and max <= 2 x the model's (`model` = the float64 restatement with fp16 weights and
  fp16 stored activations); pooled features and logits within 2 E of exact, E = max |model - exact|.
* the trunk's fp32 tail, on the same run's buffers: the pooled features are bit-equal to the stated fp32 mean (convnet_reference.spatial_mean32)
  of the run's own layer4 map; the logits are within (2048 / 64 + 7) 2^-24 (sum |p w| + |bias|) of the float64 head of the run's own pool.
* whole path: each logit within 2 E, so each difference within 4 E: |loss - exact| <= mean(2 |a - b| 4 E + (4 E)^2), and the same with the layer4
  model error for the features term.
"""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import convnet_reference as CR
import resnet_reference as R
from convnet_helpers import DEV, U16, U32, _lib, _stream, bits, bits32, check_against_fp64, integer_case, ref_convbn, run_convbn, run_pool

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ input kernel
def run_input(real, fake, clamp=False, cols=False):
    L, lib = _lib()
    B, _, H, W = real.shape
    ms = torch.tensor(R.MEAN + R.STD, dtype=torch.float32, device=DEV)
    img = torch.full((2 * B, R.SIDE, R.SIDE, 4), float("nan"), dtype=torch.float16, device=DEV)
    col = torch.full((2 * B, 112, 112, 160), float("nan"), dtype=torch.float16, device=DEV) if cols else None
    rd, fd = real.to(DEV).contiguous(), fake.to(DEV).contiguous()
    L.check(lib.mb_resnet_input(rd.data_ptr(), fd.data_ptr(), ms.data_ptr(), img.data_ptr(), col.data_ptr() if cols else None, B, H, W, 1 if clamp else 0,
                                _stream()), "mb_resnet_input")
    torch.cuda.synchronize()
    return img.cpu(), (col.cpu() if cols else None)


def input_bound(exact, H, W, vmax):
    ny = max(len(w) for _lo, w in R.resize_taps(H))
    nx = max(len(w) for _lo, w in R.resize_taps(W))
    return (U16 + U32) * exact.abs() + (ny + nx + 4) * U32 * vmax / min(R.STD)


@pytest.mark.parametrize("H,W", R.RESIZE_SIZES)
def test_input_kernel_vs_fp64(H, W):
    g = torch.Generator().manual_seed(H * 3 + W)
    real, fake = torch.rand(2, 3, H, W, generator=g), torch.rand(2, 3, H, W, generator=g)
    cols = (H, W) in ((224, 224), (96, 160))
    got, col = run_input(real, fake, cols=cols)
    x = torch.cat([real, fake])
    exact = R.input64(x).permute(0, 2, 3, 1)
    err = (got[..., :3].double() - exact).abs()
    bound = input_bound(exact, H, W, 1.0)
    print(f"input {H}x{W}: max err / bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(got[..., 3], torch.zeros_like(got[..., 3]))
    if (H, W) == (224, 224):                                       # one tap of weight 1: torch's fp32 formula bit for bit
        mean, std = torch.tensor(R.MEAN).view(1, 3, 1, 1), torch.tensor(R.STD).view(1, 3, 1, 1)
        want = ((x - mean) / std).permute(0, 2, 3, 1).to(torch.float16)
        assert torch.equal(bits(got[..., :3]), bits(want))
    if cols:                                                       # the im2col holds the image's own values, zeros outside it and in the pad channels
        want = R.stem_cols64(got[..., :3].double().permute(0, 3, 1, 2))
        assert torch.equal(col[..., :147].double(), want)
        assert torch.equal(col[..., 147:], torch.zeros_like(col[..., 147:]))


def test_input_kernel_clamps():
    g = torch.Generator().manual_seed(77)
    real, fake = torch.rand(2, 3, 96, 160, generator=g) * 1.5 - 0.25, torch.rand(2, 3, 96, 160, generator=g) * 1.5 - 0.25
    x = torch.cat([real, fake])
    assert float(x.min()) < -0.2 and float(x.max()) > 1.2
    for clamp in (True, False):
        got, _ = run_input(real, fake, clamp=clamp)
        exact = R.input64(x, clamp=clamp).permute(0, 2, 3, 1)
        assert bool(((got[..., :3].double() - exact).abs() <= input_bound(exact, 96, 160, 1.25)).all())
    assert float((R.input64(x, True) - R.input64(x, False)).abs().max()) > 0.5


# ------------------------------------------------------------------------------------------------ the epilogues, per launch
# run_convbn, ref_convbn, check_against_fp64 and integer_case live in tests/convnet_helpers.py (imported above), shared with the Inception tests
@pytest.mark.parametrize("name", list(R.CONV_CASES))
def test_epilogue_layer_vs_fp64(name):
    B, H, W, cin, cout, k, stride, pad, epi = R.CONV_CASES[name]
    x16, w, scale, shift, idn = R.conv_case(name, seed=5300 + cin + cout)
    got16, sat = run_convbn(x16, w, scale, shift, stride, pad, epi=epi, idn=idn)
    exact, S = ref_convbn(x16, w, scale, shift, stride, pad, epi, idn)
    check_against_fp64(name, got16, exact, S, cin * k * k + 1, epi)             # (K + 1) 2^-24 S: the K products and the epilogue
    assert sat == 0


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("name", list(R.CONV_CASES))
def test_epilogue_integer_operands_are_bit_exact(name, variant):
    B, H, W, cin, cout, k, stride, pad, epi = R.CONV_CASES[name]
    x16, w, scale, shift, idn = integer_case(5400 + cin, B, H, W, cin, cout, k, stride, pad, epi == R.EPI_RESIDUAL)
    exact, _ = ref_convbn(x16, w, scale, shift, stride, pad, epi, idn)
    assert float(exact.max()) > 0 and cin * k * k * 6 < 2 ** 24
    if epi == R.EPI_LINEAR:
        assert float(exact.min()) < -4
    got16, sat = run_convbn(x16, w, scale, shift, stride, pad, epi=epi, idn=idn, variant=variant)
    want16 = R.h16r(exact).permute(0, 2, 3, 1).to(torch.float16)
    assert torch.equal(bits(got16), bits(want16)) and sat == 0


@pytest.mark.parametrize("name", list(R.CONV_CASES))
def test_epilogue_tile_shapes_give_the_same_bits(name):
    B, H, W, cin, cout, k, stride, pad, epi = R.CONV_CASES[name]
    x16, w, scale, shift, idn = R.conv_case(name, seed=5500)
    a, _ = run_convbn(x16, w, scale, shift, stride, pad, epi=epi, idn=idn, variant=1)
    b, _ = run_convbn(x16, w, scale, shift, stride, pad, epi=epi, idn=idn, variant=2)
    assert torch.equal(bits(a), bits(b))
    one, _ = run_convbn(x16[1:2], w, scale, shift, stride, pad, epi=epi, idn=idn[1:2] if idn is not None else None)
    assert torch.equal(bits(one), bits(a[1:2]))                  # an image alone: a pixel's bits do not depend on its tile or the batch


@pytest.mark.parametrize("name", ["relu 128->128 k3 s2 p1 14x14", "relu 512->512 k3 p1 7x7"])
def test_relu_epilogue_through_the_new_entry_is_the_old_one(name):
    B, H, W, cin, cout, k, stride, pad, epi = R.CONV_CASES[name]
    x16, w, scale, shift, _ = R.conv_case(name, seed=5600)
    for variant in (1, 2):
        new, s1 = run_convbn(x16, w, scale, shift, stride, pad, epi=R.EPI_RELU, variant=variant)
        old, s0 = run_convbn(x16, w, scale, shift, stride, pad, epi=None, variant=variant)
        assert torch.equal(bits(new), bits(old)) and s0 == s1 == 0


def test_identity_is_read_only_inside_its_slice():
    name = "residual 64->256 k1 14x14"
    B, H, W, cin, cout, k, stride, pad, epi = R.CONV_CASES[name]
    x16, w, scale, shift, idn = R.conv_case(name, seed=5700)
    dense, _ = run_convbn(x16, w, scale, shift, stride, pad, epi=epi, idn=idn)
    assert bool(torch.isfinite(dense).all())
    wide = torch.full((B, H, W, 64 + cout + 32), float("nan"), dtype=torch.float16)          # NaN on both sides
    wide[..., 64:64 + cout] = idn
    tight = torch.full((B, H, W, 64 + cout), float("nan"), dtype=torch.float16)              # the last pixel's slice ends with the buffer
    tight[..., 64:] = idn
    for variant in (1, 2):
        for buf in (wide, tight):
            got, sat = run_convbn(x16, w, scale, shift, stride, pad, epi=epi, idn=buf, idn_off=64, variant=variant)
            assert torch.equal(bits(got), bits(dense)) and sat == 0


def test_saturation_is_counted_on_both_signs():
    """exact outputs of +-120000 in known (pixel, 4-channel group) cells.  Linear: stored as +-65504, both counted.  Residual: 60000 from the
    convolution + 60000 from the identity is stored as 65504 and counted, -120000 is cut by the ReLU first"""
    H, W, cin, cout = 7, 9, 32, 128
    pix = [(0, 0), (3, 4), (6, 8), (2, 7)]
    x16 = torch.zeros(2, H, W, cin, dtype=torch.float16)
    idn = torch.zeros(2, H, W, cout, dtype=torch.float16)
    for b in range(2):
        for (y, x) in pix:
            x16[b, y, x, 0] = 60000.0
            idn[b, y, x, 0] = idn[b, y, x, 5] = 60000.0
    w = torch.zeros(cout, cin, 1, 1)
    for c, v in {0: 2.0, 1: 2.0, 5: 2.0, 64: -2.0, 127: 2.0}.items():       # channels 0 and 1 share a group
        w[c, 0] = v
    one, zero = torch.ones(cout), torch.zeros(cout)
    for variant in (1, 2):
        out, sat = run_convbn(x16, w, one, zero, 1, 0, epi=R.EPI_LINEAR, variant=variant)
        assert sat == 2 * len(pix) * 4                            # groups 0, 1, 31 positive and 16 negative
        exact, _ = ref_convbn(x16, w, one, zero, 1, 0, R.EPI_LINEAR)
        assert torch.equal(out.double().permute(0, 3, 1, 2), exact.clamp(-65504.0, 65504.0))
        assert float(out[0, 0, 0, 64]) == -65504.0 and float(out[0, 0, 0, 0]) == 65504.0
        w1 = w / 2                                                # the convolution gives +-60000, the identity adds 60000 to channels 0 and 5
        out, sat = run_convbn(x16, w1, one, zero, 1, 0, epi=R.EPI_RESIDUAL, idn=idn, variant=variant)
        assert sat == 2 * len(pix) * 2                            # groups 0 and 1 reach 120000; group 31 stays at 60000; -60000 is cut
        exact, _ = ref_convbn(x16, w1, one, zero, 1, 0, R.EPI_RESIDUAL, idn)
        assert torch.equal(out.double().permute(0, 3, 1, 2), exact.clamp(max=65504.0))
        assert float(out[0, 0, 0, 64]) == 0.0 and float(out[0, 0, 0, 127]) == 60000.0 and float(out[0, 0, 0, 5]) == 65504.0


def test_stem_in_its_folded_form():
    """conv1 as the network runs it on a 32 x 32 image: the im2col kernel, then the general convolution as a 1x1 over 147 of 160 channels with the
    weight read as [64, 147] -- against the 7x7 stride-2 padding-3 convolution itself"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(5800)
    B, S = 3, R.STEM_SIDE
    img = torch.full((B, S, S, 4), float("nan"), dtype=torch.float16)
    img[..., :3] = torch.randn(B, S, S, 3, generator=g).to(torch.float16)
    w = torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5
    scale, shift = 0.5 + 1.5 * torch.rand(64, generator=g), torch.randn(64, generator=g) * 0.1
    cols = torch.full((B, S // 2, S // 2, 160), float("nan"), dtype=torch.float16, device=DEV)
    imd = img.to(DEV)
    L.check(lib.mb_resnet_stem_cols(imd.data_ptr(), cols.data_ptr(), B, S, _stream()), "mb_resnet_stem_cols")
    torch.cuda.synchronize()
    cols = cols.cpu()
    assert torch.equal(cols[..., :147].double(), R.stem_cols64(img[..., :3].double().permute(0, 3, 1, 2)))
    assert torch.equal(cols[..., 147:], torch.zeros_like(cols[..., 147:]))
    cols[..., 147:] = float("nan")                                 # the convolution's K tail must mask the pad channels itself
    exact, Smag = ref_convbn(img[..., :3], w, scale, shift, 2, 3, R.EPI_RELU)
    outs = []
    for variant in (1, 2):
        got16, sat = run_convbn(cols, w.reshape(64, 147, 1, 1), scale, shift, 1, 0, epi=R.EPI_RELU, variant=variant)
        assert sat == 0
        outs.append(got16)
    check_against_fp64("stem 3->64 k7 s2 p3 32x32 folded", outs[0], exact, Smag, 147 + 1, R.EPI_RELU)
    assert torch.equal(bits(outs[0]), bits(outs[1]))


# ------------------------------------------------------------------------------------------------ pool
@pytest.mark.parametrize("H,W", [(14, 14), (9, 9)])
def test_padded_stride2_pool_bit_equal(H, W):
    g = torch.Generator().manual_seed(H * W)
    x16 = (torch.randn(2, H, W, 64, generator=g) * 8).to(torch.float16)
    x16[..., 1] = -x16[..., 1].abs() - 1.0                        # an all-negative channel: a padded border must not win with 0
    x16[0, 0, 0, 0], x16[0, 0, 1, 0] = 65504.0, -65504.0
    want = F.max_pool2d(x16.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).to(torch.float16)
    got = run_pool(x16, 3, ex=True)
    assert got.shape == want.shape and torch.equal(bits(got), bits(want)) and bool((got[..., 1] < 0).all())
    sentinel = torch.full((2, got.shape[1], got.shape[2], 64 + 72), -1234.0, dtype=torch.float16)
    out = run_pool(x16, 3, out=sentinel.clone(), out_off=40, ex=True)
    assert torch.equal(bits(out[..., 40:104]), bits(want)) and bool((out[..., :40] == -1234.0).all()) and bool((out[..., 104:] == -1234.0).all())


def test_pool_refuses_what_it_does_not_take():
    L, lib = _lib()
    x = torch.zeros(1, 9, 9, 64, dtype=torch.float16, device=DEV)
    y = torch.zeros(1, 5, 5, 64, dtype=torch.float16, device=DEV)
    args = lambda **kw: list({**dict(B=1, H=9, W=9, C=64, mode=3, in_off=0, in_cs=64, out_off=0, out_cs=64), **kw}.values())
    assert lib.mb_pool3_ex(x.data_ptr(), y.data_ptr(), *args(), _stream()) == 0
    for bad in (dict(mode=4), dict(C=60), dict(in_cs=56), dict(out_off=4), dict(B=0), dict(H=0)):
        assert lib.mb_pool3_ex(x.data_ptr(), y.data_ptr(), *args(**bad), _stream()) != 0, bad
    assert lib.mb_pool3(x.data_ptr(), y.data_ptr(), *args(), _stream()) != 0            # the Inception entry keeps its three modes
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ distance
def test_distance_kernel_vs_fp64():
    L, lib = _lib()
    g = torch.Generator().manual_seed(5900)
    B, N, Fe = 3, 1000, 4 * 2048
    logits = torch.randn(2 * B, N, generator=g)
    feat = torch.relu(torch.randn(2 * B, Fe, generator=g)).to(torch.float16)
    logits[B + 1], feat[B + 1] = logits[1], feat[1]               # an identical pair
    ld, fd = logits.to(DEV), feat.to(DEV)
    for with_feat in (False, True):
        out = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
        total = torch.full((1,), 10.0, dtype=torch.float64, device=DEV)
        L.check(lib.mb_resnet_distance(ld.data_ptr(), fd.data_ptr() if with_feat else None, B, N, Fe if with_feat else 0, out.data_ptr(), total.data_ptr(),
                                       _stream()), "mb_resnet_distance")
        want = (logits[:B].double() - logits[B:].double()).pow(2).mean(1)
        if with_feat:
            want = want + (feat[:B].double() - feat[B:].double()).pow(2).mean(1)
        got = out.cpu()
        assert bool(((got - want).abs() <= 1e-13 * want).all()) and float(got[1]) == 0.0
        t = 10.0
        for v in got.tolist():
            t += v
        assert float(total.cpu()) == t                             # the running sum: the pairs added in order


# ------------------------------------------------------------------------------------------------ trunk
@functools.lru_cache(maxsize=None)
def hip_model(on_logits=True):
    from maskbit_amd import PerceptualLoss
    m = PerceptualLoss(compute_perceptual_loss_on_logits=on_logits)
    m.load_resnet50(R.weights())
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def hip_trunk(name):
    """one mb_resnet_taps of the case -> (the four maps float64 NCHW on the CPU, pool, logits as float64, saturation count)"""
    L, lib = _lib()
    B, S, _seed = R.TRUNK_CASES[name]
    m = hip_model()
    h = m.engine(2)
    m.saturation_count()
    img = R.trunk_image(name).to(DEV)
    exact, _ = R.trunk_oracle(name)
    maps = [torch.full((B, e.shape[2], e.shape[3], e.shape[1]), float("nan"), dtype=torch.float16, device=DEV) for e in exact["maps"]]
    pool = torch.full((B, 2048), float("nan"), dtype=torch.float32, device=DEV)
    logits = torch.full((B, 1000), float("nan"), dtype=torch.float32, device=DEV)
    L.check(lib.mb_resnet_taps(h, img.data_ptr(), B, S, *[t.data_ptr() for t in maps], pool.data_ptr(), logits.data_ptr(), _stream()), "mb_resnet_taps")
    sat = m.saturation_count()
    return [t.cpu().double().permute(0, 3, 1, 2) for t in maps], pool.cpu().double(), logits.cpu().double(), sat


@pytest.mark.parametrize("name", list(R.TRUNK_CASES))
def test_trunk_maps_and_features(name):
    exact, model = R.trunk_oracle(name)
    maps, pool, logits, sat = hip_trunk(name)
    S = R.TRUNK_CASES[name][1]
    assert [m.shape[2] for m in maps] == ([14, 7, 4, 2] if S == 56 else [16, 8, 4, 2])
    for k, (got, ex, mo) in enumerate(zip(maps, exact["maps"], model["maps"])):
        assert got.shape == ex.shape and bool(torch.isfinite(got).all())
        e_hip, e_mod = (got - ex), (mo - ex)
        r_rms = (e_hip.pow(2).mean().sqrt() / e_mod.pow(2).mean().sqrt()).item()
        r_max = (e_hip.abs().max() / e_mod.abs().max()).item()
        print(f"{name} layer{k + 1}: rms error / model's {r_rms:.3f}, max error / model's {r_max:.3f}")
        assert r_rms <= 1.5 and r_max <= 2.0
    for key, got in (("pool", pool), ("logits", logits)):
        E = float((model[key] - exact[key]).abs().max())
        d = float((got - exact[key]).abs().max())
        print(f"{name} {key}: E {E:.3e}, |hip - exact| / E {d / E:.3f}")
        assert got.shape == exact[key].shape and E > 0 and d <= 2 * E
    assert sat == 0
    # the fp32 tail on the run's own buffers, in its own unit: the pooled features are the stated fp32 mean of the layer4 map the same run handed
    # out, the logits the head of the run's own fp32 pooled features
    l4 = maps[3]
    l4_16 = l4.permute(0, 2, 3, 1).reshape(l4.shape[0], -1, l4.shape[1]).to(torch.float16)
    assert torch.equal(bits32(pool.float()), bits32(CR.spatial_mean32(l4_16)))
    sd = R.weights()
    _unbiased, want, Smag = CR.fc_head64(pool.float(), sd["fc.weight"], sd["fc.bias"])
    err, bound = (logits - want).abs(), CR.head_bound(2048, Smag)
    print(f"{name} logits against the float64 head of its own pool: worst err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


# ------------------------------------------------------------------------------------------------ whole path
@pytest.mark.parametrize("on_logits", [True, False])
@pytest.mark.parametrize("name", list(R.PAIR_CASES))
def test_whole_path_vs_fp64(name, on_logits):
    exact, model = R.pair_oracle(name)
    base, noisy = R.pair_images(name)
    m = hip_model(on_logits)
    got = float(m.per_image(base.to(DEV), noisy.to(DEV)).cpu())
    want = float(R.loss64(exact, 1, on_logits))
    E = float((model["logits"] - exact["logits"]).abs().max())
    d = (exact["logits"][:1] - exact["logits"][1:]).abs()
    bound = float((2 * d * 4 * E + (4 * E) ** 2).mean())
    if not on_logits:
        E4 = float((model["maps"][3] - exact["maps"][3]).abs().max())
        d4 = (exact["maps"][3][:1] - exact["maps"][3][1:]).abs()
        bound += float((2 * d4 * 4 * E4 + (4 * E4) ** 2).mean())
    print(f"whole path {name} on_logits {on_logits}: loss {got:.6e}, exact {want:.6e}, model {float(R.loss64(model, 1, on_logits)):.6e}, "
          f"|err| {abs(got - want):.3e}, bound {bound:.3e}, E {E:.3e}")
    assert want > 0 and abs(got - want) <= bound
    assert m.saturation_count() == 0


# ------------------------------------------------------------------------------------------------ exactness
def _pairs(n, seed=21, H=64, W=64):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(n, 3, H, W, generator=g)
    b = (a + 0.05 * torch.randn(n, 3, H, W, generator=g)).clamp(0, 1)
    return a.to(DEV), b.to(DEV)


@pytest.mark.parametrize("on_logits", [True, False])
def test_identical_images_give_exactly_zero(on_logits):
    a, _ = _pairs(2)
    assert torch.equal(hip_model(on_logits).per_image(a, a).cpu(), torch.zeros(2, dtype=torch.float64))


@pytest.mark.parametrize("on_logits", [True, False])
def test_a_pair_does_not_depend_on_the_batch_or_the_chunking(on_logits):
    from maskbit_amd import PerceptualLoss
    a, b = _pairs(3, seed=22)
    m = hip_model(on_logits)
    whole = m.per_image(a, b)
    assert torch.equal(whole, m.per_image(a, b))                  # two runs: bit-identical
    assert whole.dtype == torch.float64 and whole.device.type == "cuda" and bool((whole > 0).all())
    for i in range(3):
        assert torch.equal(m.per_image(a[i:i + 1], b[i:i + 1]), whole[i:i + 1]), i
    small = PerceptualLoss(compute_perceptual_loss_on_logits=on_logits)
    small.load_resnet50(R.weights())
    small = small.to(DEV)
    small.max_pairs_per_call = 1
    assert torch.equal(small.per_image(a, b), whole) and small._engine_key[1] == 1


# ------------------------------------------------------------------------------------------------ the product
def test_forward_is_the_mean_and_strict_loading_works():
    from maskbit_amd import PerceptualLoss
    a, b = _pairs(3, seed=23)
    m = PerceptualLoss()
    with pytest.raises(RuntimeError, match="load_resnet50"):
        m.to(DEV)(a, b)
    m.load_state_dict(R.reference_layout(R.weights()), strict=True)
    m = m.to(DEV)
    loss = m(a, b)
    per = m.per_image(a, b)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device.type == "cuda"
    assert torch.equal(loss, per.mean().to(torch.float32)) and torch.equal(per, hip_model().per_image(a, b))
    clamped = m.per_image(a * 1.5 - 0.25, b * 1.5 - 0.25, clamp=True)
    assert torch.equal(clamped, m.per_image((a * 1.5 - 0.25).clamp(0, 1), (b * 1.5 - 0.25).clamp(0, 1)))


def test_tokenizer_evaluator_takes_the_model():
    from maskbit_amd import TokenizerEvaluator
    m = hip_model()
    a, b = _pairs(5, seed=24)
    plain = TokenizerEvaluator(DEV, enable_mae_error=True)
    plain.update(a, b)
    ev = TokenizerEvaluator(DEV, enable_mae_error=True)
    ev.use_perceptual(m)
    ev.update(a[:3], b[:3])
    first = ev.last_perceptual
    ev.update(a[3:], b[3:])
    r = ev.result()
    assert set(r) - set(plain.result()) == {"PerceptualLoss"} and set(plain.result()) <= set(r) and abs(r["MAE"] - plain.result()["MAE"]) < 1e-12
    assert torch.equal(first, m.per_image(a[:3], b[:3])) and torch.equal(ev.last_perceptual, m.per_image(a[3:], b[3:]))
    t = 0.0
    for v in m.per_image(a, b).cpu().tolist():
        t += v
    assert r["PerceptualLoss"] == t / 5
    ev.reset_metrics()
    ev.update(a[:1], b[:1])
    assert ev.result()["PerceptualLoss"] == float(m.per_image(a[:1], b[:1]).cpu())
    ev.use_perceptual(None)
    assert "PerceptualLoss" not in ev.result()
    with pytest.raises(TypeError):
        ev.use_perceptual(object())


def test_refusals_come_before_any_device_work():
    L, lib = _lib()
    m = hip_model()
    a, b = _pairs(1, seed=25)
    for bad in (a[:, :1], a[0], a[:, :, :31], torch.zeros(1, 3, 64, 1025, device=DEV)):
        with pytest.raises(ValueError):
            m(bad, bad)
    with pytest.raises(ValueError):
        m(a, torch.cat([b, b]))
    h = m.engine(1)
    out = torch.zeros(4, dtype=torch.float64, device=DEV)
    call = lambda hh, B, H, W: lib.mb_resnet_forward(hh, a.data_ptr(), b.data_ptr(), B, H, W, 0, 1, out.data_ptr(), None, _stream())
    assert call(h, 1, 64, 64) == 0
    assert call(h, 0, 64, 64) != 0 and call(h, 1, 31, 64) != 0 and call(h, 1, 64, 1025) != 0 and call(h, m._engine_key[1] + 1, 64, 64) != 0
    img = torch.zeros(1, 40, 40, 4, dtype=torch.float16, device=DEV)
    taps = lambda B, S: lib.mb_resnet_taps(h, img.data_ptr(), B, S, None, None, None, None, None, None, _stream())
    assert taps(1, 40) == 0 and taps(1, 36) != 0 and taps(1, 24) != 0 and taps(1, 232) != 0 and taps(2 * m._engine_key[1] + 1, 40) != 0
    hh = C.c_void_p()
    L.check(lib.mb_resnet_create(1, C.byref(hh)), "mb_resnet_create")
    assert call(hh, 1, 64, 64) != 0
    assert b"not complete" in lib.mb_last_error()
    lib.mb_resnet_destroy(hh)
    torch.cuda.synchronize()
