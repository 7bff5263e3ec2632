"""GPU checks of the tokenizers' blocks ONE LAUNCH AT A TIME: the no-SiLU convolution and the stats = false switch of launch_conv
(mb_conv_layer_ex), the three wirings of run_block (mb_autoenc_block), run_attn of the Taming handle (mb_taming_attn_block), load_param's row slices
and folded final convolution (mb_taming_load + mb_taming_attn_block / mb_taming_final) and the +-1 image packer (mb_taming_pack_image).

References and criteria are tests/taming_blocks_reference.py: every launch is compared against float64 of the kernel's OWN fp16 input to that
launch, with the derived bounds of test_hip_conv.py / test_hip_spatial_attention.py and nothing wider; tests/test_taming_blocks_cpu.py proves on the
CPU that those criteria reject the wrong wirings.  Each case prints its error-to-bound and rms-to-E_model ratios."""
import ctypes as C
import math

import pytest
import torch

import taming_blocks_reference as R
import taming_reference as TR

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = R.T_ATT


def _lib():
    from maskbit_amd import _lib
    return _lib, _lib.load()


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t):
    return t.to(DEV).contiguous() if t is not None else None


def _nan16(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float16, device=DEV)


# ------------------------------------------------------------------------------------------------ handles
class Handle:
    def __init__(self, max_batch, latent):
        L, lib = _lib()
        self.h = C.c_void_p()
        L.check(lib.mb_taming_create(max_batch, latent, C.byref(self.h)), "mb_taming_create")

    def load(self, name, t):
        """-> the return code of mb_taming_load for one checkpoint entry (fp32, any shape)"""
        _, lib = _lib()
        t = t.float().to(DEV).contiguous()
        shape = (C.c_int64 * t.dim())(*t.shape)
        rc = lib.mb_taming_load(self.h, name.encode(), t.data_ptr(), shape, t.dim(), _stream())
        torch.cuda.synchronize()
        return rc

    def load_attn(self, block, P, order=("norm", "q", "k", "v", "proj_out")):
        for n in order:
            for leaf in ("weight", "bias"):
                assert self.load(f"{TR.ATTN[block]}.{n}.{leaf}", P[f"{n}.{leaf}"]) == 0

    def saturation(self):
        L, lib = _lib()
        n = C.c_uint(0)
        L.check(lib.mb_taming_saturation_count(self.h, C.byref(n), 1, _stream()), "mb_taming_saturation_count")
        return int(n.value)

    def close(self):
        _lib()[1].mb_taming_destroy(self.h)


@pytest.fixture(scope="module")
def handle16():
    h = Handle(2, 16)
    yield h
    h.close()


@pytest.fixture(scope="module")
def handle32():
    h = Handle(1, 32)
    yield h
    h.close()


# ------------------------------------------------------------------------------------------------ mb_conv_layer_ex
def run_conv_ex(x, w, bias, gamma, beta, *, H, W, ks, flags, out_norm=None):
    """mb_conv_layer_ex without residual: x fp16 NHWC on the GPU, w fp32 OIHW -> dict(out, sat, tiles, ss, rc)"""
    L, lib = _lib()
    B, cin, cout = x.shape[0], x.shape[-1], w.shape[0]
    w, bias, gamma, beta = _dev(w.float()), _dev(bias), _dev(gamma), _dev(beta)
    out = _nan16(B, H, W, cout)
    og = ob = ss = None
    if out_norm is not None:
        og, ob = _dev(out_norm[0]), _dev(out_norm[1])
        ss = torch.full((B, cout, 2), float("nan"), device=DEV)
    part = torch.full((B * (H // 8) * (W // 16) * 64,), float("nan"), device=DEV)
    tiles, sat = C.c_int(-1), C.c_uint(0)
    rc = lib.mb_conv_layer_ex(_ptr(x), _ptr(w), _ptr(bias), _ptr(gamma), _ptr(beta), None, _ptr(out), None, None, _ptr(og), _ptr(ob), _ptr(ss),
                              _ptr(part), C.byref(tiles), C.byref(sat), B, H, W, cin, cout, ks, 0, 0, flags, _stream())
    torch.cuda.synchronize()
    return dict(out=out, sat=int(sat.value), tiles=int(tiles.value), ss=ss, part=part, rc=rc)


# (cin, cout, H, W, B): the product's q / k / v projection with its 12 channel tiles (48 channels per group: never epilogue partials); one channel
# tile of 4 channels per group, whose epilogue writes partials unless stats = false, with >= 1e5 outputs
NOSILU_CASES = [(512, 1536, 16, 16, 2), (64, 128, 8, 16, 7)]


@pytest.mark.parametrize("case", NOSILU_CASES, ids=lambda c: "cin{}_cout{}_{}x{}_b{}".format(*c))
def test_conv_no_silu_and_stats_off(case):
    cin, cout, H, W, B = case
    g = torch.Generator().manual_seed(300 + cin)
    r = lambda *s: torch.randn(*s, generator=g)
    x16 = (r(B, H, W, cin) * (0.5 + torch.rand(cin, generator=g)) + r(cin)).to(torch.float16)
    w, bias = r(cout, cin, 1, 1) / math.sqrt(cin), 0.3 * r(cout)
    gamma, beta = 1.0 + 0.3 * r(cin), 0.3 * r(cin)
    og, ob = 1.0 + 0.3 * r(cout), 0.3 * r(cout)
    xd = x16.to(DEV)
    runs = {f: run_conv_ex(xd, w, bias, gamma, beta, H=H, W=W, ks=1, flags=f, out_norm=(og, ob)) for f in (0, 1, 2, 3)}
    assert all(v["rc"] == 0 and v["sat"] == 0 for v in runs.values())
    assert B * H * W * cout >= 100_000
    for f, v in runs.items():                                                   # bit 0 picks the prologue, with and without the statistics
        R.check_conv(v["out"], x16, w, bias, gamma, beta, None, 1, silu=not (f & 1), what=f"conv {case} flags {f}")
        flat = v["out"].cpu().reshape(B, H * W, cout)
        # bit 1: no partials from the epilogue whatever Cout, and the output's statistics come from the sweep
        assert (v["tiles"] > 0) == (not (f & 2) and cout // 32 in (4, 8, 16)), (f, v["tiles"])
        if f & 2:
            assert v["tiles"] == 0 and bool(torch.isnan(v["part"]).all())
        R.check_scale_shift(v["ss"], flat, og, ob, f"conv {case} flags {f} output GroupNorm ({'epilogue' if v['tiles'] else 'sweep'})")
    assert torch.equal(runs[0]["out"], runs[2]["out"]) and torch.equal(runs[1]["out"], runs[3]["out"])      # stats off changes no output
    assert not torch.equal(runs[0]["out"], runs[1]["out"])
    differ = float((runs[0]["out"] != runs[1]["out"]).float().mean())
    print(f"conv {case}: outputs differing between the SiLU and the no-SiLU prologue {differ:.3f}")
    assert differ > 0.9


def test_conv_layer_ex_refusals():
    x = torch.zeros(1, 16, 16, 64, dtype=torch.float16, device=DEV)
    w3, w1 = torch.zeros(64, 64, 3, 3), torch.zeros(64, 64, 1, 1)
    gb = torch.ones(64)
    assert run_conv_ex(x, w3, None, gb, gb, H=16, W=16, ks=3, flags=1)["rc"] == -1          # no-SiLU prologue with ks 3
    assert run_conv_ex(x, w1, None, None, None, H=16, W=16, ks=1, flags=1)["rc"] == -1      # ... without a prologue
    for flags in (4, 8, 5, -1, 1 << 16):
        assert run_conv_ex(x, w1, None, gb, gb, H=16, W=16, ks=1, flags=flags)["rc"] == -1  # unknown bits
    ok = run_conv_ex(x, w1, None, gb, gb, H=16, W=16, ks=1, flags=3)
    assert ok["rc"] == 0 and bool(torch.isfinite(ok["out"]).all())
    bad = run_conv_ex(x, w3, None, gb, gb, H=16, W=16, ks=3, flags=1)
    assert bool(torch.isnan(bad["out"]).all())                                               # refused before anything was launched


# ------------------------------------------------------------------------------------------------ ResBlock
def run_block(case, image=None):
    """mb_autoenc_block on a case of R.make_block (image: that image of the batch alone) -> dict(h1, mid, out, ss) on the CPU, sat"""
    L, lib = _lib()
    P, form, cin, cout, H, W = case["P"], case["form"], case["cin"], case["cout"], case["H"], case["W"]
    x16 = case["x16"] if image is None else case["x16"][image:image + 1]
    B = x16.shape[0]
    d = {k: _dev(v) for k, v in P.items()}
    p = lambda k: _ptr(d.get(k))
    x = x16.to(DEV).contiguous()
    out, h1, mid = _nan16(B, H, W, cout), _nan16(B, H, W, cout), _nan16(B, H, W, cout)
    og, ob = _dev(case["og"]), _dev(case["ob"])
    ss = torch.full((B, cout, 2), float("nan"), device=DEV)
    sat = C.c_uint(77)
    L.check(lib.mb_autoenc_block(_ptr(x), p("norm1.weight"), p("norm1.bias"), p("conv1.weight"), p("conv1.bias"), p("norm2.weight"), p("norm2.bias"),
                                 p("conv2.weight"), p("conv2.bias"), p("nin_shortcut.weight"), p("nin_shortcut.bias"), form, int("conv1.bias" in P),
                                 _ptr(out), _ptr(h1), _ptr(mid) if form else None, _ptr(og), _ptr(ob), _ptr(ss), C.byref(sat), B, H, W, cin, cout,
                                 _stream()), "mb_autoenc_block")
    torch.cuda.synchronize()
    got = dict(h1=h1.cpu(), out=out.cpu(), ss=ss.cpu(), sat=int(sat.value))
    if form:
        got["mid"] = mid.cpu()
    return got


@pytest.mark.parametrize("bias", [1, 0], ids=["bias", "nobias"])
@pytest.mark.parametrize("H,W", R.BLOCK_SIZES)
@pytest.mark.parametrize("form,cin,cout", R.BLOCK_FORMS)
def test_res_block_per_launch(form, cin, cout, H, W, bias):
    case = R.make_block(form, cin, cout, H, W, bool(bias), seed=1000 * form + cin + 2 * cout + H + bias)
    got = run_block(case)
    assert got["sat"] == 0
    R.check_block(case, got, what=f"block form {form} {cin}->{cout} {H}x{W} bias {bias}:")
    one = run_block(case, image=1)                                              # batch invariance: image 1 alone gives the same bits
    assert one["sat"] == 0
    for k in ("h1", "mid", "out"):
        if k in got:
            assert torch.equal(one[k], got[k][1:2]), k
    assert torch.equal(one["ss"], got["ss"][1:2])


def test_autoenc_block_refusals():
    _, lib = _lib()
    case = R.make_block(1, 128, 256, 16, 32, True, seed=3)
    d = {k: _dev(v) for k, v in case["P"].items()}
    x = case["x16"].to(DEV)
    o = _nan16(2, 16, 32, 256)
    sat = C.c_uint(0)

    def call(form=1, bias=1, H=16, W=32, cin=128, cout=256, x_=x, mid=o, scw="nin_shortcut.weight", c1b="conv1.bias"):
        return lib.mb_autoenc_block(_ptr(x_), _ptr(d["norm1.weight"]), _ptr(d["norm1.bias"]), _ptr(d["conv1.weight"]), _ptr(d.get(c1b)),
                                    _ptr(d["norm2.weight"]), _ptr(d["norm2.bias"]), _ptr(d["conv2.weight"]), _ptr(d["conv2.bias"]), _ptr(d.get(scw)),
                                    _ptr(d["nin_shortcut.bias"]), form, bias, _ptr(o), _ptr(o), _ptr(mid), None, None, None, C.byref(sat), 2, H, W,
                                    cin, cout, _stream())
    assert call(form=0) == -1 and call(form=3) == -1 and call(form=2, cin=256) == -1      # the form goes with (cin, cout)
    assert call(H=12) == -1 and call(W=24) == -1 and call(cin=96) == -1 and call(cout=4096) == -1
    assert call(x_=None) == -1 and call(mid=None) == -1 and call(scw="none") == -1 and call(c1b="none") == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all())                                           # nothing was launched


# ------------------------------------------------------------------------------------------------ AttnBlock
def run_attn(hd, case, tap=True):
    """mb_taming_attn_block of the case's block on handle hd -> dict(qkv, attn, out, ss) on the CPU; the mb_taming_set_tap copy must equal out"""
    L, lib = _lib()
    B, H, W, block = case["B"], case["H"], case["W"], case["block"]
    N = H * W
    x = case["x16"].to(DEV).contiguous()
    qkv, att, out, tapbuf = _nan16(B * N, 3 * T), _nan16(B * N, T), _nan16(B, H, W, T), _nan16(B, N, T)
    og, ob = _dev(case["og"]), _dev(case["ob"])
    ss = torch.full((B, T, 2), float("nan"), device=DEV)
    if tap:
        L.check(lib.mb_taming_set_tap(hd.h, block, tapbuf.data_ptr()), "mb_taming_set_tap")
    try:
        L.check(lib.mb_taming_attn_block(hd.h, block, _ptr(x), _ptr(qkv), _ptr(att), _ptr(out), _ptr(og), _ptr(ob), _ptr(ss), B, H, W, _stream()),
                "mb_taming_attn_block")
        torch.cuda.synchronize()
    finally:
        L.check(lib.mb_taming_set_tap(hd.h, block, None), "mb_taming_set_tap")
    if tap:
        assert torch.equal(tapbuf.reshape(B, H, W, T), out)
    assert hd.saturation() == 0
    return dict(qkv=qkv.cpu(), attn=att.cpu(), out=out.cpu(), ss=ss.cpu())


@pytest.mark.parametrize("case", R.ATTN_CASES, ids=lambda c: "block{}_{}x{}_b{}_latent{}".format(*c))
def test_attn_block_per_launch(case, request):
    block, H, W, B, latent = case
    hd = request.getfixturevalue("handle16" if latent == 16 else "handle32")
    c = R.make_attn(block, H, W, B, seed=R.attn_seed(case))
    assert 0.3 < c["mp"] < 0.7
    hd.load_attn(block, c["P"])
    got = run_attn(hd, c)
    R.check_attn_block(c, got, what=f"attn block {block} {H}x{W} B {B}:")
    if B == 2:                                                                  # image 1 alone gives the same bits
        one = run_attn(hd, dict(c, B=1, x16=c["x16"][1:2]))
        N = H * W
        assert torch.equal(one["qkv"], got["qkv"][N:]) and torch.equal(one["attn"], got["attn"][N:]) and torch.equal(one["out"], got["out"][1:2])


def test_attn_block_refusals(handle16):
    _, lib = _lib()
    x, o = torch.zeros(2, 16, 16, T, dtype=torch.float16, device=DEV), _nan16(2 * 256, 3 * T)
    call = lambda block, B, H, W, xp=x.data_ptr(): lib.mb_taming_attn_block(handle16.h, block, xp, _ptr(o), _ptr(o), _ptr(o), None, None, None, B, H, W,
                                                                            _stream())
    assert call(7, 1, 16, 16) == -1 and call(-1, 1, 16, 16) == -1 and call(0, 3, 16, 16) == -1 and call(0, 0, 16, 16) == -1
    assert call(0, 1, 12, 16) == -1 and call(0, 1, 16, 8) == -1 and call(0, 1, 16, 32) == -1 and call(0, 1, 16, 16, None) == -1
    assert lib.mb_taming_final(handle16.h, x.data_ptr(), None, None, 1, 16, 16, _stream()) == -1
    assert lib.mb_taming_final(handle16.h, x.data_ptr(), o.data_ptr(), None, 1, 16, 24, _stream()) == -1
    assert lib.mb_taming_final(handle16.h, x.data_ptr(), o.data_ptr(), None, 3, 16, 16, _stream()) == -1
    assert lib.mb_taming_final(handle16.h, x.data_ptr(), o.data_ptr(), None, 1, 512, 256, _stream()) == -1
    assert lib.mb_taming_pack_image(None, o.data_ptr(), 1, 4, 4, _stream()) == -1 and lib.mb_taming_pack_image(x.data_ptr(), o.data_ptr(), 1, 0, 4, _stream()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all())


# ------------------------------------------------------------------------------------------------ sliced loads
def test_sliced_loads_are_exact(handle16):
    """load_param's row slices of the stacked q / k / v weight: any load order gives the canonical stacking; reloading one slice touches no other
    row; a slice of the wrong size is refused with -4 and changes nothing."""
    block, H, W, B = 1, 8, 16, 2
    c = R.make_attn(block, H, W, B, seed=77)
    P = c["P"]
    name = TR.ATTN[block]
    handle16.load_attn(block, P, order=("norm", "proj_out", "v", "q", "k"))
    first = run_attn(handle16, c)
    R.check_attn_block(c, first, what="sliced load v, q, k:")
    g = torch.Generator().manual_seed(78)
    k_new = {"k.weight": torch.randn(T, T, 1, 1, generator=g) / T ** 0.5, "k.bias": 0.3 * torch.randn(T, generator=g)}
    for leaf, t in k_new.items():
        assert handle16.load(f"{name}.{leaf}", t) == 0
    second = run_attn(handle16, c)["qkv"]
    assert torch.equal(second[:, :T], first["qkv"][:, :T]) and torch.equal(second[:, 2 * T:], first["qkv"][:, 2 * T:])
    assert not torch.equal(second[:, T:2 * T], first["qkv"][:, T:2 * T])
    c2 = dict(c, P=dict(P, **k_new))
    fresh = Handle(2, 16)
    try:
        fresh.load_attn(block, c2["P"])
        canonical = run_attn(fresh, c2)
    finally:
        fresh.close()
    assert torch.equal(second, canonical["qkv"])
    R.check_attn_block(c2, canonical, what="sliced load, k reloaded:")
    # wrong sizes: refused, and the stacked weight and bias are as before
    assert handle16.load(f"{name}.q.weight", torch.ones(T // 2, T, 1, 1)) == -4
    assert handle16.load(f"{name}.v.weight", torch.ones(3 * T, T, 1, 1)) == -4
    assert handle16.load(f"{name}.k.bias", torch.ones(3 * T)) == -4
    assert handle16.load(f"{name}.q.bias", torch.ones(T - 1)) == -4
    assert handle16.load(f"{name}.norm.weight", torch.ones(T // 2)) == -4
    assert torch.equal(run_attn(handle16, c)["qkv"], second)


# ------------------------------------------------------------------------------------------------ folded final layer
@pytest.mark.parametrize("H,W", [(32, 48), (64, 64)])
def test_folded_final_layer(handle16, H, W):
    L, lib = _lib()
    B = 2
    c = R.make_final(H, W, B, seed=H + W)
    for name, t in (("decoder.norm_out.weight", c["gamma"]), ("decoder.norm_out.bias", c["beta"]), ("decoder.conv_out.weight", c["w"]),
                    ("decoder.conv_out.bias", c["b"])):
        assert handle16.load(name, t) == 0
    x = c["x16"].to(DEV).contiguous()
    img = torch.full((B, 3, H, W), float("nan"), device=DEV)
    u8 = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=DEV)
    L.check(lib.mb_taming_final(handle16.h, _ptr(x), _ptr(img), _ptr(u8), B, H, W, _stream()), "mb_taming_final")
    torch.cuda.synchronize()
    assert handle16.saturation() == 0
    R.check_final(c, img, what=f"folded final layer {H}x{W}")
    assert torch.equal(u8, (img.clamp(0.0, 1.0) * 255.0).permute(0, 2, 3, 1).to(torch.uint8))
    # the same kernels on pre-folded operands: w * 0.5 (exact) and float32((float64(b) + 1) / 2) -- fmaf(b, 0.5, 0.5) rounds once, as that does
    w2, b2 = R.prefolded(c)
    img2 = torch.full((B, 3, H, W), float("nan"), device=DEV)
    u82 = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=DEV)
    tiles, sat = C.c_int(-1), C.c_uint(0)
    w2d, b2d, gd, bd = _dev(w2), _dev(b2), _dev(c["gamma"]), _dev(c["beta"])
    L.check(lib.mb_conv_layer(_ptr(x), _ptr(w2d), _ptr(b2d), _ptr(gd), _ptr(bd), None, None, _ptr(img2), _ptr(u82), None, None, None, None,
                              C.byref(tiles), C.byref(sat), B, H, W, 128, 3, 3, 0, 1, _stream()), "mb_conv_layer")
    torch.cuda.synchronize()
    assert int(sat.value) == 0
    assert torch.equal(img, img2) and torch.equal(u8, u82)


# ------------------------------------------------------------------------------------------------ packer
@pytest.mark.parametrize("H,W", R.PACK_SHAPES)
@pytest.mark.parametrize("B", [1, 3])
def test_pack_image_pm1_exact(B, H, W):
    L, lib = _lib()
    GUARD = 64
    img = R.make_pack(B, H, W, seed=B * 100 + H)
    out = torch.full((B * H * W + GUARD, 64), -7.0, dtype=torch.float16, device=DEV)
    imd = img.to(DEV).contiguous()
    L.check(lib.mb_taming_pack_image(_ptr(imd), _ptr(out), B, H, W, _stream()), "mb_taming_pack_image")
    torch.cuda.synchronize()
    R.check_pack(out[:B * H * W], img)
    want = (img.float() * 2 - 1).half().clamp(-65504.0, 65504.0)                # the issue's formula, on the CPU
    assert torch.equal(out[:B * H * W, :3].cpu(), want.permute(0, 2, 3, 1).reshape(-1, 3))
    assert bool((out[:B * H * W, 3:] == 0).all()) and bool((out[B * H * W:] == -7.0).all())
