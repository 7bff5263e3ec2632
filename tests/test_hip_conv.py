"""The tokenizer's kernels (maskbit_amd/csrc/conv.hip) layer by layer against an fp64 reference of the same operation.

Every case runs ONE layer through the diagnostic entries of include/maskbit_hip_diag.h (mb_conv_layer, mb_groupnorm_stats, mb_avgpool2, mb_s2d), which
call the product's own launch_conv / launch_gn / weight repack on a scratch context.  The reference is torch on the CPU in float64, fed the same
fp16-representable inputs and the weights after fp16 rounding: conv2d, group_norm(eps 1e-6), SiLU, nearest upsampling and the asymmetric TF-"same"
padding of the stride-2 conv.  Nothing in it comes from the code under test.

Tolerances are derived, none is tuned to what the kernels give:

* bound (worst case, per output element)  2^-11 sum|w a| (fp16 rounding of the prologue's output; 0 without a prologue)
  + 2^-11 |y| (the fp16 store; not for the final layer, which writes fp32) + K 2^-24 sum|w a| (fp32 accumulation of K = Cin k k products).
  A correct kernel cannot leave it; a missing or shifted tap is far outside.
* E_model = rms(exact reference - the same reference with the design's documented roundings applied in fp64: prologue output -> fp16, output ->
  fp16).  The kernel's rms error against the exact reference must stay below 1.25 E_model: one more independent rounding of the same size would give
  sqrt(2).  Every case has >= 1e5 outputs (sampling noise of an rms < 1 %).  A layer without any documented rounding (a final layer without
  prologue) has E_model = 0 and is held to the bound alone.
* GroupNorm (scale, shift): |d scale| <= 2^-11 |scale| and |d shift| <= 2^-11 (|beta| + |mean scale|) against fp64 statistics of the same fp16
  values -- the precision at which the consumer rounds the normalised value anyway.
* GroupNorm partial sums of a tile: any-order fp32 summation of n terms, n 2^-24 sum|x| resp. n 2^-24 sum x^2.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from taming_blocks_reference import U16, U32, check_scale_shift, h16r, ref_conv, ref_gn

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _lib():
    from maskbit_amd import _lib
    return _lib, _lib.load()


def _ptr(t):
    return t.data_ptr() if t is not None else None


def run_conv(x, w, bias=None, gamma=None, beta=None, res=None, *, H, W, ks, up=False, final=False, out_norm=None, want_u8=False):
    """mb_conv_layer: x fp16 NHWC on the GPU, w fp32 OIHW, -> dict(out | img (+ u8), sat, tiles, part, ss)."""
    L, lib = _lib()
    B, cin, cout = x.shape[0], x.shape[-1], w.shape[0]
    dev = lambda t: t.to(DEV).contiguous() if t is not None else None
    w, bias, gamma, beta = dev(w.float()), dev(bias), dev(gamma), dev(beta)
    out = img = u8 = ss = og = ob = None
    if final:
        img = torch.full((B, cout, H, W), float("nan"), device=DEV)
        u8 = torch.zeros((B, H, W, cout), dtype=torch.uint8, device=DEV) if want_u8 else None
    else:
        out = torch.full((B, H, W, cout), float("nan"), dtype=torch.float16, device=DEV)
    part = torch.full((B * (H // 8) * (W // 16) * 64,), float("nan"), device=DEV)
    if out_norm is not None:
        og, ob = dev(out_norm[0]), dev(out_norm[1])
        ss = torch.full((B, cout, 2), float("nan"), device=DEV)
    tiles, sat = C.c_int(-1), C.c_uint(0)
    L.check(lib.mb_conv_layer(_ptr(x), _ptr(w), _ptr(bias), _ptr(gamma), _ptr(beta), _ptr(res), _ptr(out), _ptr(img), _ptr(u8), _ptr(og), _ptr(ob),
                              _ptr(ss), _ptr(part), C.byref(tiles), C.byref(sat), B, H, W, cin, cout, ks, int(up), int(final),
                              torch.cuda.current_stream().cuda_stream), "mb_conv_layer")
    torch.cuda.synchronize()
    return dict(out=out, img=img, u8=u8, sat=int(sat.value), tiles=int(tiles.value), part=part, ss=ss)


def gn_stats(x, gamma, beta):
    """mb_groupnorm_stats (the sweep path): x fp16 [B, HW, C] on the GPU -> (scale, shift) [B, C, 2]."""
    L, lib = _lib()
    B, HW, Cc = x.shape
    ss = torch.full((B, Cc, 2), float("nan"), device=DEV)
    g, b = gamma.to(DEV).contiguous(), beta.to(DEV).contiguous()
    L.check(lib.mb_groupnorm_stats(x.data_ptr(), g.data_ptr(), b.data_ptr(), ss.data_ptr(), B, HW, Cc, torch.cuda.current_stream().cuda_stream),
            "mb_groupnorm_stats")
    torch.cuda.synchronize()
    return ss


# ------------------------------------------------------------------------------------------------ fp64 reference
# h16r, ref_conv, ref_gn and check_scale_shift live in tests/taming_blocks_reference.py (imported above), shared with the block tests


def check_partials(r, out16, H, W):
    """the epilogue's per-tile GroupNorm partials against fp64 sums of the kernel's own fp16 output"""
    B, cout = out16.shape[0], out16.shape[-1]
    tiles = r["tiles"]
    th = 8 if tiles == (H // 8) * (W // 16) else 16
    assert tiles == (H // th) * (W // 16)
    cpg = cout // 32
    v = out16.double().cpu().reshape(B, H // th, th, W // 16, 16, 32, cpg).permute(0, 1, 3, 5, 2, 4, 6).reshape(B, tiles, 32, -1)
    n = v.shape[-1]
    got = r["part"][: B * tiles * 64].double().cpu().reshape(B, tiles, 32, 2)
    es = (got[..., 0] - v.sum(-1)).abs() - n * U32 * v.abs().sum(-1)
    eq = (got[..., 1] - v.pow(2).sum(-1)).abs() - n * U32 * v.pow(2).sum(-1)
    assert es.max().item() <= 0 and eq.max().item() <= 0, (es.max().item(), eq.max().item())


# ------------------------------------------------------------------------------------------------ shape matrix
# (Cin, Cout, H, W, B, ks, up, final, prologue, residual, bias): every launch_conv branch -- final / ks 1 / ks 2 / UP x {8, 16}-row tiles / plain x
# {8, 16}-row tiles --, the four epilogue bodies (residual or not x full or partial 128-channel tile), GroupNorm partials from the epilogue (Cout 128 / 256 /
# 512 = 4 / 8 / 16 channels per group) or none (Cout 64, 192, 12), Cin padded to 64 (3, 12) and more than one chunk (192, 512, 4 x 64 .. 4 x 512).
CASES = [
    (12, 512, 16, 16, 1, 3, 0, 0, 0, 0, 1),       # decoder.conv_in: 12 -> 64 channel padding, 8-row tiles
    (3, 128, 64, 64, 1, 3, 0, 0, 0, 0, 0),        # encoder.conv_in: 3 -> 64 channel padding, 16-row tiles
    (512, 256, 16, 16, 3, 3, 0, 0, 1, 1, 0),      # 8 chunks, 8-row tiles, residual, full tiles, 8 channels per group
    (64, 64, 32, 32, 3, 3, 0, 0, 1, 1, 0),        # partial tile with residual, 2 channels per group: no epilogue partials
    (192, 128, 48, 48, 1, 3, 0, 0, 1, 0, 0),      # 3 chunks, 16-row tiles on a 48 x 48 map, 4 channels per group
    (512, 512, 32, 32, 1, 3, 0, 0, 1, 1, 1),      # 16-row tiles, 4 channel tiles, 16 channels per group
    (64, 128, 64, 64, 1, 3, 0, 0, 1, 1, 0),       # 64 x 64
    (64, 128, 16, 32, 3, 3, 0, 0, 1, 0, 0),       # non-square, 8-row tiles
    (256, 256, 16, 16, 3, 3, 1, 0, 0, 0, 1),      # UP, 8-row tiles (8 x 8 -> 16 x 16)
    (128, 128, 64, 64, 1, 3, 1, 0, 0, 0, 1),      # UP, 16-row tiles (32 x 32 -> 64 x 64)
    (64, 64, 48, 48, 1, 3, 1, 0, 0, 1, 1),        # UP, 16-row tiles, partial tile, residual
    (128, 128, 32, 32, 1, 1, 0, 0, 0, 1, 0),      # nin_shortcut: 1x1, residual = its own input
    (512, 12, 64, 64, 3, 1, 0, 0, 1, 0, 1),       # encoder.conv_out: 1x1 with prologue, 12 stored channels
    (64, 64, 32, 32, 3, 2, 0, 0, 0, 0, 1),        # down_conv 64 (64 x 64 -> 32 x 32)
    (192, 192, 16, 16, 3, 2, 0, 0, 0, 0, 1),      # down_conv 192: a full and a partial channel tile
    (512, 512, 16, 16, 1, 2, 0, 0, 0, 0, 1),      # down_conv 512: 32 chunks
    (128, 3, 128, 128, 3, 3, 0, 1, 1, 0, 1),      # decoder.conv_out, 3 channels
    (64, 4, 96, 96, 3, 3, 0, 1, 1, 0, 1),         # final layer, 4 channels
    (64, 3, 128, 128, 3, 3, 0, 1, 0, 0, 1),       # final layer without prologue: no documented rounding, bound only
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "cin{}_cout{}_{}x{}_b{}_ks{}_up{}_fin{}_gn{}_res{}_bias{}".format(*c))
def test_conv_layer_vs_fp64(case):
    cin, cout, H, W, B, ks, up, final, prologue, residual, has_bias = case
    g = torch.Generator().manual_seed(1000 + CASES.index(case))
    hin, win = (2 * H, 2 * W) if ks == 2 else ((H // 2, W // 2) if up else (H, W))
    k = 3 if ks == 2 else ks
    # inputs with per-channel offsets and gains, so that the prologue's GroupNorm has something to do
    x16 = ((torch.randn(B, hin, win, cin, generator=g) * (0.5 + torch.rand(cin, generator=g)) + torch.randn(cin, generator=g))).to(torch.float16)
    w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    bias = torch.randn(cout, generator=g) * 0.3 if has_bias else None
    gamma = 1.0 + 0.3 * torch.randn(cin, generator=g) if prologue else None
    beta = 0.3 * torch.randn(cin, generator=g) if prologue else None
    res16 = None
    if residual:
        res16 = x16 if (ks == 1 and cin == cout) else torch.randn(B, H, W, cout, generator=g).to(torch.float16)
    og, ob = 1.0 + 0.3 * torch.randn(cout, generator=g), 0.3 * torch.randn(cout, generator=g)
    want_norm = not final and cout % 32 == 0
    xd = x16.to(DEV)
    rd = xd if res16 is x16 else (res16.to(DEV) if res16 is not None else None)
    r = run_conv(xd, w, bias, gamma, beta, rd, H=H, W=W, ks=ks, up=bool(up), final=bool(final), out_norm=(og, ob) if want_norm else None)

    exact, S = ref_conv(x16, w, bias, gamma, beta, res16, ks, up, final, rounded=False)
    model, _ = ref_conv(x16, w, bias, gamma, beta, res16, ks, up, final, rounded=True)
    got = (r["img"] if final else r["out"].permute(0, 3, 1, 2)).double().cpu()
    assert got.shape == exact.shape and bool(torch.isfinite(got).all())
    assert got.numel() >= 100_000
    K = cin * k * k
    bound = (U16 * S if prologue else 0.0) + (0.0 if final else U16 * exact.abs()) + K * U32 * S
    err = (got - exact).abs()
    worst = (err / bound).max().item()
    e_kernel = err.pow(2).mean().sqrt().item()
    e_model = (model - exact).pow(2).mean().sqrt().item()
    print(f"conv {case}: max err / bound {worst:.3f}; rms err {e_kernel:.3e}, E_model {e_model:.3e}, ratio {e_kernel / e_model if e_model else float('nan'):.3f}")
    assert worst <= 1.0
    if e_model > 0.0:
        assert e_kernel <= 1.25 * e_model
    assert r["sat"] == 0
    cpg = cout // 32
    expect_part = not final and cout % 128 == 0 and cpg in (4, 8, 16)
    assert (r["tiles"] > 0) == expect_part
    if expect_part:
        check_partials(r, r["out"], H, W)
    if want_norm:                                             # the next layer's GroupNorm (epilogue partials, or the sweep) of the kernel's own output
        flat = r["out"].cpu().reshape(B, H * W, cout)
        check_scale_shift(r["ss"], flat, og, ob, "output GroupNorm (" + ("epilogue" if expect_part else "sweep") + ")")


# ------------------------------------------------------------------------------------------------ impulse: layout
def _impulse_positions(hin, win):
    ys = sorted({y for y in (0, 3, 4, 7, 8, 15, 16, 31, 32, hin - 1) if y < hin})
    xs = sorted({x for x in (0, 7, 8, 15, 16, 31, 32, 33, win - 1) if x < win})
    images = []                                               # within an image the 3x3 (UP: 4x4) footprints of two impulses never overlap
    for p in [(y, x) for y in ys for x in xs]:
        for im in images:
            if all(abs(p[0] - q[0]) >= 3 or abs(p[1] - q[1]) >= 3 for q in im):
                im.append(p)
                break
        else:
            images.append([p])
    return images


@pytest.mark.parametrize("mode", ["ks3", "ks2", "up"])
@pytest.mark.parametrize("H,W", [(16, 32), (32, 32)])
def test_conv_impulse_detects_layout_bugs(mode, H, W):
    """One-hot inputs at corners and tile seams (x = 15 / 16, y = 7 / 8 on 8-row tiles, 15 / 16 on 16-row tiles), integer taps that differ by tap and by
    (input, output) channel: all products and sums are small integers, so every output pixel, tap and channel must match the fp64 convolution EXACTLY.
    What test_gemm_identity_detects_layout_bugs is to the GEMM."""
    cin, cout = 128, 128
    ks = 2 if mode == "ks2" else 3
    up = mode == "up"
    hin, win = (2 * H, 2 * W) if ks == 2 else ((H // 2, W // 2) if up else (H, W))
    images = _impulse_positions(hin, win)
    B = len(images)
    chans = [0, 7, 8, 63, 64, 69, 127, 33]
    x16 = torch.zeros(B, hin, win, cin, dtype=torch.float16)
    n = 0
    for b, im in enumerate(images):
        for (y, x) in im:
            x16[b, y, x, chans[n % len(chans)]] = 1.0
            n += 1
    co, ci, tap = torch.meshgrid(torch.arange(cout), torch.arange(cin), torch.arange(9), indexing="ij")
    w = (1 + tap + 9 * ((co * 5 + ci * 11) % 56)).float().reshape(cout, cin, 3, 3)      # <= 504: sums of up to 4 taps (UP) stay exact in fp16
    r = run_conv(x16.to(DEV), w, H=H, W=W, ks=ks, up=up)
    want, _ = ref_conv(x16, w, None, None, None, None, ks, up, False, rounded=False)
    got = r["out"].permute(0, 3, 1, 2).double().cpu()
    assert float(want.abs().max()) <= 2048 and int((want != 0).sum()) >= n * cout
    bad = (got != want)
    assert not bool(bad.any()), f"{int(bad.sum())} outputs differ, first at (b, c, y, x) = {bad.nonzero()[0].tolist()}"
    assert r["sat"] == 0 and r["tiles"] > 0
    check_partials(r, r["out"], H, W)


# ------------------------------------------------------------------------------------------------ GroupNorm statistics
@pytest.mark.parametrize("side", [16, 64])
@pytest.mark.parametrize("C_", [128, 256, 512])
@pytest.mark.parametrize("ratio", [0, 8, 32, 64])
def test_groupnorm_stats_offset_inputs(ratio, C_, side):
    """(scale, shift) on inputs whose per-group |mean| / std is 0 / 8 / 32 / 64 (trained VQGAN decoders show such groups; at 64 fp16 still resolves the
    std to 3 %), 4 / 8 / 16 channels per group, by the sweep (gn_partial_kernel) and by the conv epilogue's per-tile partials -- through a 1x1 (8-row
    tiles) and a 3x3 (16-row tiles from 32 x 32 on) identity convolution, whose output must equal its input bit for bit -- against fp64 statistics
    of the same fp16 values, and against each other."""
    B, HW, cpg = 3, side * side, C_ // 32
    g = torch.Generator().manual_seed(7 * ratio + C_ + side)
    sign = torch.where(torch.rand(B, 1, 32, 1, generator=g) < 0.5, -1.0, 1.0)
    x16 = (torch.randn(B, HW, 32, cpg, generator=g) + ratio * sign).reshape(B, HW, C_).to(torch.float16)
    gamma, beta = 1.0 + 0.5 * torch.randn(C_, generator=g), torch.randn(C_, generator=g)
    xd = x16.to(DEV)
    paths = {"sweep": gn_stats(xd, gamma, beta)}
    for ks in (1, 3):
        w = torch.zeros(C_, C_, ks, ks)
        w[torch.arange(C_), torch.arange(C_), ks // 2, ks // 2] = 1.0
        r = run_conv(xd.reshape(B, side, side, C_), w, H=side, W=side, ks=ks, out_norm=(gamma, beta))
        assert torch.equal(r["out"].reshape(B, HW, C_), xd) and r["tiles"] == (side // (16 if ks == 3 and side >= 32 else 8)) * (side // 16)
        check_partials(r, r["out"], side, side)
        paths[f"epilogue ks{ks}"] = r["ss"]
    for name, ss in paths.items():
        check_scale_shift(ss, x16, gamma, beta, f"ratio {ratio} C {C_} {side}x{side} {name}")
    scale, shift, mean = ref_gn(x16, gamma, beta)
    for name in ("epilogue ks1", "epilogue ks3"):                # the two paths agree with each other within the same bound
        d = (paths[name].double() - paths["sweep"].double()).abs().cpu()
        assert bool((d[..., 0] <= U16 * scale.abs()).all()) and bool((d[..., 1] <= U16 * (beta.double().abs() + (mean * scale).abs())).all()), name


# ------------------------------------------------------------------------------------------------ final layer: uint8 epilogue
def test_final_layer_uint8_at_the_quantisation_steps():
    """fp32 outputs placed exactly on k / 255, one fp32 step below and above, below 0 and above 1 (each target is the sum of three fp16 inputs times
    the taps 1, 2^-11, 2^-22: exact in fp32): uint8 = trunc(clamp(v, 0, 1) * 255) of the kernel's OWN fp32 output, and that output inside the bound."""
    H = W = 32
    k = torch.arange(256, dtype=torch.float32) / 255.0
    t = torch.cat([k, torch.nextafter(k, torch.tensor(2.0)), torch.nextafter(k, torch.tensor(-2.0)),
                   torch.tensor([-1.0, -1e-3, -1e-8, 1.0 + 2 ** -23, 1.5, 7.0])])
    t = torch.cat([t, torch.linspace(-0.25, 1.25, H * W - t.numel())]).double()
    parts, rest = [], t.clone()
    for j in range(3):
        p = h16r(rest * 2.0 ** (11 * j))
        parts.append(p)
        rest = rest - p * 2.0 ** (-11 * j)
    x16 = torch.zeros(1, H, W, 64, dtype=torch.float16)
    for j in range(3):
        x16[0, :, :, 5 + 9 * j] = parts[j].reshape(H, W).to(torch.float16)
    w = torch.zeros(3, 64, 3, 3)
    for j in range(3):
        w[:, 5 + 9 * j, 1, 1] = 2.0 ** (-11 * j)
    bias = torch.tensor([0.0, 0.5, -0.5])
    r = run_conv(x16.to(DEV), w, bias, H=H, W=W, ks=3, final=True, want_u8=True)
    v = r["img"]
    want = (torch.clamp(v, 0.0, 1.0) * 255.0).permute(0, 2, 3, 1).to(torch.uint8)
    assert torch.equal(r["u8"], want)
    exact, S = ref_conv(x16, w, bias, None, None, None, 3, False, True, rounded=False)
    # (here the bias is the largest addend of the fp32 sum at most pixels -- the taps only carry the target --, so it is counted among the |w a|)
    assert bool(((v.double().cpu() - exact).abs() <= 64 * 9 * U32 * (S + bias.double().abs().view(1, 3, 1, 1))).all())
    hit = (v[0, 0].reshape(-1)[:256].cpu() == k)
    assert float(hit.float().mean()) > 0.99 and len(torch.unique(r["u8"])) == 256       # the steps themselves were reached


# ------------------------------------------------------------------------------------------------ saturation
def test_saturation_is_counted_exactly_and_stored_at_the_fp16_limit():
    """A 1x1 layer whose exact outputs are +-120000 in a known set of (pixel, 4-channel group) cells and 60000 (inside the range) elsewhere."""
    H, W, cin, cout = 16, 32, 64, 128
    pix = [(0, 0), (7, 15), (8, 16), (15, 31), (3, 20)]
    x16 = torch.zeros(2, H, W, cin, dtype=torch.float16)
    for b in range(2):
        for (y, x) in pix:
            x16[b, y, x, 0] = 60000.0
    w = torch.zeros(cout, cin, 1, 1)
    w[:, 0] = 1.0
    hot = {0: 2.0, 1: -2.0, 5: 2.0, 64: -2.0, 127: 2.0}                 # channels 0 and 1 share a group: 4 groups per hot pixel
    for c, v in hot.items():
        w[c, 0] = v
    r = run_conv(x16.to(DEV), w, H=H, W=W, ks=1)
    assert r["sat"] == 2 * len(pix) * 4
    exact, _ = ref_conv(x16, w, None, None, None, None, 1, False, False, rounded=False)
    assert int(((exact.abs() > 65504).reshape(2, 32, 4, H, W).any(2)).sum()) == r["sat"]
    got = r["out"].permute(0, 3, 1, 2).double().cpu()
    assert torch.equal(got, exact.clamp(-65504.0, 65504.0))


# ------------------------------------------------------------------------------------------------ pooling kernels
@pytest.mark.parametrize("C_", [64, 192])
def test_s2d_exact_and_avgpool2_within_half_ulp(C_):
    L, lib = _lib()
    B, H, W = 3, 32, 48
    g = torch.Generator().manual_seed(C_)
    mag = 0.25 * 2.0 ** (4.0 * torch.rand(B, H, W, C_, generator=g))               # |x| in [0.25, 4): the four-term sum is exact in fp32
    x16 = (mag * torch.where(torch.rand(B, H, W, C_, generator=g) < 0.5, -1.0, 1.0)).to(torch.float16)
    xd = x16.to(DEV)
    y = torch.full((B, H // 2, W // 2, 4 * C_), float("nan"), dtype=torch.float16, device=DEV)
    L.check(lib.mb_s2d(xd.data_ptr(), y.data_ptr(), B, H, W, C_, torch.cuda.current_stream().cuda_stream), "mb_s2d")
    want = x16.reshape(B, H // 2, 2, W // 2, 2, C_).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4 * C_)   # channel (py * 2 + px) * C + c
    assert torch.equal(y.cpu(), want)
    p = torch.full((B, H // 2, W // 2, C_), float("nan"), dtype=torch.float16, device=DEV)
    L.check(lib.mb_avgpool2(xd.data_ptr(), p.data_ptr(), B, H, W, C_, torch.cuda.current_stream().cuda_stream), "mb_avgpool2")
    m = F.avg_pool2d(x16.double().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    ulp = 2.0 ** (torch.floor(torch.log2(m.abs().clamp(min=2.0 ** -14))) - 10)
    assert bool(((p.double().cpu() - m).abs() <= 0.5 * ulp).all())


def test_layer_entries_reject_bad_arguments():
    L, lib = _lib()
    x = torch.zeros(1, 16, 16, 64, dtype=torch.float16, device=DEV)
    w = torch.zeros(64, 64, 3, 3, device=DEV)
    o = torch.zeros(1, 16, 16, 64, dtype=torch.float16, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    n, u = C.c_int(0), C.c_uint(0)
    call = lambda H, W, cin, cout, ks, up, fin: lib.mb_conv_layer(x.data_ptr(), w.data_ptr(), None, None, None, None, o.data_ptr(), None, None, None, None, None,
                                                                  None, C.byref(n), C.byref(u), 1, H, W, cin, cout, ks, up, fin, s)
    assert call(16, 16, 64, 64, 4, 0, 0) != 0 and call(12, 16, 64, 64, 3, 0, 0) != 0 and call(16, 8, 64, 64, 3, 0, 0) != 0
    assert call(16, 16, 64, 6, 3, 0, 0) != 0 and call(16, 16, 64, 64, 1, 1, 0) != 0 and call(16, 16, 64, 64, 3, 0, 1) != 0
    assert call(16, 16, 64, 64, 3, 0, 0) == 0
    assert lib.mb_groupnorm_stats(x.data_ptr(), w.data_ptr(), w.data_ptr(), o.data_ptr(), 1, 256, 48, s) != 0
    assert lib.mb_s2d(x.data_ptr(), o.data_ptr(), 1, 15, 16, 64, s) != 0 and lib.mb_avgpool2(x.data_ptr(), o.data_ptr(), 1, 16, 16, 60, s) != 0
