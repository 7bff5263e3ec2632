"""Float64 references and pass / fail criteria for the single launches of the tokenizers' blocks (csrc/mb_autoenc.h run_block and load_param,
csrc/taming.hip run_attn, the folded final layer and the +-1 image packer), for tests/test_hip_taming_blocks.py (GPU) and
tests/test_taming_blocks_cpu.py (which proves on the CPU that the criteria reject wrong wirings).  Torch on the CPU only; nothing of the product is
imported.  The convolution / GroupNorm reference and its criteria are those of tests/test_hip_conv.py, which imports them from here.

Every launch is compared against float64 of the KERNEL'S OWN fp16 input to that launch (x, h1, mid, qkv, attn): a stage's reference never takes
another stage's reference as input, so single-launch bounds are never multiplied through a chain, and the wiring is pinned by which tensors the
reference of each stage takes.

Criteria (derived in test_hip_conv.py and test_hip_spatial_attention.py; none is new, none is tuned to what the kernels give):

* convolution launches (check_conv): the per-element bound 2^-11 sum|w a| (fp16 rounding of the prologue's output; 0 without a prologue)
  + 2^-11 |y| (the fp16 store; not for the final layer) + K 2^-24 sum|w a| (fp32 accumulation of K products); and rms error <= 1.25 E_model,
  E_model = rms(exact - the reference with the design's documented roundings: prologue output -> fp16, stored output -> fp16).  The rms is a
  sample statistic: test_hip_conv.py takes >= 1e5 outputs per case (sampling noise below 1 %).  The shapes that the tests here are given have
  >= 65 536 outputs per block launch and 9 216 for the smaller final layer: the noise of an rms, 1 / sqrt(2 n), is 0.3 % resp. 0.7 %, still below
  1 % against a margin of 25 %.
* GroupNorm (scale, shift) (check_scale_shift): |d scale| <= 2^-11 |scale|, |d shift| <= 2^-11 (|beta| + |mean scale|) against float64
  statistics of the same fp16 values.
* the attention launch (check_attention): |out - ref| <= 2^-9 max|v|; documented roundings: probabilities -> fp16 for P V, output -> fp16.
"""
import math

import torch
import torch.nn.functional as F

import taming_reference as TR

U16 = 2.0 ** -11          # unit roundoff of fp16
U32 = 2.0 ** -24          # ... of fp32
T_ATT = 512


def h16r(t):
    """round an fp64 tensor to fp16 (nearest even) and back"""
    return t.to(torch.float16).double()


def nchw(t16):
    """fp16 NHWC -> float64 NCHW"""
    return t16.double().permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ convolution / GroupNorm
def ref_gn(x16, gamma, beta):
    """fp64 GroupNorm(32, eps 1e-6) statistics of fp16 values x16 [B, HW, C] -> scale, shift, mean, each [B, C]"""
    B, HW, Cc = x16.shape
    cpg = Cc // 32
    v = x16.double().reshape(B, HW, 32, cpg)
    mean = v.mean(dim=(1, 3))
    var = (v - mean[:, None, :, None]).pow(2).mean(dim=(1, 3))
    rstd = (var + 1e-6).rsqrt()
    mean, rstd = mean.repeat_interleave(cpg, 1), rstd.repeat_interleave(cpg, 1)
    scale = rstd * gamma.double()
    return scale, beta.double() - mean * scale, mean


def ref_conv(x16, w, bias, gamma, beta, res16, ks, up, final, rounded, silu=True, stats_of=None, fold=None):
    """-> (y fp64 NCHW, S = sum|w a| per output).  x16 fp16 NHWC (CPU).  rounded: the design's documented roundings applied in fp64.
    silu = False: the prologue is the GroupNorm alone (the AttnBlock's q / k / v projection).  stats_of (fp16 NHWC, for mutants): the prologue
    normalises x16 with the GroupNorm statistics of THAT tensor.  fold: the final layer carrying decode's (y + 1) / 2 -- "full" = weight x 0.5
    and bias -> (b + 1) / 2, i.e. (conv + 1) / 2; for mutants "weight" = the weight alone halved; None = no fold."""
    a = x16.double().permute(0, 3, 1, 2)
    if gamma is not None:
        if stats_of is None:
            a = F.group_norm(a, 32, gamma.double(), beta.double(), 1e-6)
        else:
            B, C_ = stats_of.shape[0], stats_of.shape[-1]
            scale, shift, _ = ref_gn(stats_of.reshape(B, -1, C_), gamma, beta)
            a = a * scale[:, :, None, None] + shift[:, :, None, None]
        if silu:
            a = F.silu(a)
        if rounded:
            a = h16r(a)
    if up:
        a = F.interpolate(a, scale_factor=2.0, mode="nearest")
    wq = w.to(torch.float16).double()
    if ks == 2:                                                # 3x3, stride 2, TF "same": the odd pixel goes to the bottom / right
        a = F.pad(a, [0, 1, 0, 1])
        conv = lambda t, ww, bb: F.conv2d(t, ww, bb, stride=2)
    else:
        conv = lambda t, ww, bb: F.conv2d(t, ww, bb, padding=(ks - 1) // 2)
    y = conv(a, wq, bias.double() if bias is not None else None)
    S = conv(a.abs(), wq.abs(), None)
    if fold == "full":
        y, S = (y + 1.0) / 2.0, S / 2.0
    elif fold == "weight":
        y, S = conv(a, wq / 2.0, bias.double() if bias is not None else None), S / 2.0
    if res16 is not None:
        y = y + res16.double().permute(0, 3, 1, 2)
    if rounded and not final:
        y = h16r(y)
    return y, S


def scale_shift_errors(ss, x16, gamma, beta):
    """-> (scale error / |scale|, shift error / (|beta| + |mean scale|)), the maxima, of ss [B, C, 2] against fp64 statistics of x16 [B, HW, C]"""
    scale, shift, mean = ref_gn(x16, gamma, beta)
    got = ss.double().cpu()
    e_sc = ((got[..., 0] - scale).abs() / scale.abs()).max().item()
    e_sh = ((got[..., 1] - shift).abs() / (beta.double().abs() + (mean * scale).abs())).max().item()
    return e_sc, e_sh


def check_scale_shift(ss, x16, gamma, beta, what):
    e_sc, e_sh = scale_shift_errors(ss, x16, gamma, beta)
    print(f"{what}: scale rel err {e_sc / U16:.3f} x 2^-11, shift err {e_sh / U16:.3f} x 2^-11 (|beta| + |mean scale|)")
    assert e_sc <= U16 and e_sh <= U16, (what, e_sc / U16, e_sh / U16)
    return max(e_sc, e_sh) / U16


def ref_scale_shift(x16, gamma, beta):
    """the (scale, shift) [B, C, 2] a correct launch_gn gives for x16 fp16 [B, HW, C], as fp32 (what the CPU test feeds in as "got")"""
    scale, shift, _ = ref_gn(x16, gamma, beta)
    return torch.stack([scale, shift], dim=-1).float()


def check_conv(got, x16, w, bias, gamma, beta, res16, ks, *, silu=True, final=False, fold=None, what=""):
    """The three criteria of test_conv_layer_vs_fp64 minus the statistics (check_scale_shift): got = fp16 NHWC output of the launch (final: the fp32
    NCHW image) against float64 of the launch's own inputs.  -> (max error / bound, rms error / E_model)."""
    exact, S = ref_conv(x16, w, bias, gamma, beta, res16, ks, False, final, False, silu=silu, fold=fold)
    model, _ = ref_conv(x16, w, bias, gamma, beta, res16, ks, False, final, True, silu=silu, fold=fold)
    got = (got if final else got.permute(0, 3, 1, 2)).double().cpu()
    assert got.shape == exact.shape and bool(torch.isfinite(got).all()), what
    K = x16.shape[-1] * ks * ks
    bound = (U16 * S if gamma is not None else 0.0) + (0.0 if final else U16 * exact.abs()) + K * U32 * S
    err = (got - exact).abs()
    worst = (err / bound).max().item()
    e_kernel = err.pow(2).mean().sqrt().item()
    e_model = (model - exact).pow(2).mean().sqrt().item()
    ratio = e_kernel / e_model if e_model else float("nan")
    print(f"{what}: max err / bound {worst:.3f}; rms err {e_kernel:.3e}, E_model {e_model:.3e}, ratio {ratio:.3f} ({got.numel()} outputs)")
    assert worst <= 1.0, (what, worst)
    if e_model > 0.0:
        assert e_kernel <= 1.25 * e_model, (what, ratio)
    return worst, ratio


# ------------------------------------------------------------------------------------------------ ResBlock (mb_autoenc.h run_block)
# (form, cin, cout): 0 no shortcut; 1 Taming's nin_shortcut(x) + h; 2 the conv-VQGAN h + nin_shortcut(h).  64 output channels = 2 channels per
# group: the next GroupNorm must sweep instead of reading epilogue partials.
BLOCK_FORMS = [(0, 128, 128), (1, 128, 256), (1, 256, 128), (1, 128, 64), (2, 128, 256), (2, 64, 128)]
BLOCK_SIZES = [(16, 32), (32, 32)]                             # 8-row and 16-row tiles
BLOCK_B = 2


def make_block(form, cin, cout, H, W, bias, seed, B=BLOCK_B):
    """Seeded inputs of one ResBlock case: x16 fp16 NHWC with per-channel offsets and gains, fp32 parameters under the checkpoint's names, and
    (og, ob) for the GroupNorm that would read the block's output."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    x16 = (r(B, H, W, cin) * (0.5 + torch.rand(cin, generator=g)) + r(cin)).to(torch.float16)
    P = {"norm1.weight": 1.0 + 0.3 * r(cin), "norm1.bias": 0.3 * r(cin), "conv1.weight": r(cout, cin, 3, 3) / math.sqrt(cin * 9),
         "norm2.weight": 1.0 + 0.3 * r(cout), "norm2.bias": 0.3 * r(cout), "conv2.weight": r(cout, cout, 3, 3) / math.sqrt(cout * 9)}
    if form:
        sc_in = cin if form == 1 else cout
        P["nin_shortcut.weight"] = 1.5 * r(cout, sc_in, 1, 1) / math.sqrt(sc_in)
    if bias:
        for k in ("conv1", "conv2") + (("nin_shortcut",) if form else ()):
            P[k + ".bias"] = 0.3 * r(cout)
    return dict(form=form, cin=cin, cout=cout, H=H, W=W, B=B, x16=x16, P=P, og=1.0 + 0.3 * r(cout), ob=0.3 * r(cout))


def _fit_cin(w, cin):
    """a 1x1 weight made to read cin channels (truncated / zero-padded): only for the mutants that run a block in the other form's wiring"""
    if w.shape[1] == cin:
        return w
    out = torch.zeros(w.shape[0], cin, 1, 1)
    n = min(cin, w.shape[1])
    out[:, :n] = w[:, :n]
    return out


def block_stages(case, x16, h1, mid, form=None, residual="x", stats_from="h1"):
    """The launches of run_block as (name, ref_conv arguments) from the fp16 tensors each one READS.  form / residual / stats_from override the
    wiring for the mutants of the CPU test: another form's wiring, the residual of form 0's conv2 ("x" / "h1"), the tensor whose statistics
    conv2's prologue uses ("h1" / "mid")."""
    P, form = case["P"], case["form"] if form is None else form
    b = lambda k: P.get(k + ".bias")
    st = [("h1", dict(x16=x16, w=P["conv1.weight"], bias=b("conv1"), gamma=P["norm1.weight"], beta=P["norm1.bias"], res16=None, ks=3))]
    c2 = dict(x16=h1, w=P["conv2.weight"], bias=b("conv2"), gamma=P["norm2.weight"], beta=P["norm2.bias"], ks=3)
    if stats_from == "mid":
        c2["stats_of"] = mid
    sc = dict(w=P.get("nin_shortcut.weight"), bias=b("nin_shortcut"), gamma=None, beta=None, ks=1)
    if form == 0:
        st.append(("out", dict(c2, res16=h1 if residual == "h1" else x16)))
    elif form == 1:
        st.append(("mid", dict(sc, x16=x16, w=_fit_cin(sc["w"], case["cin"]), res16=None)))
        st.append(("out", dict(c2, res16=mid)))
    else:
        st.append(("mid", dict(c2, res16=None)))
        st.append(("out", dict(sc, x16=mid, w=_fit_cin(sc["w"], case["cout"]), res16=mid)))
    return st


def _run_stage(a, rounded):
    a = dict(a)
    y, _ = ref_conv(a.pop("x16"), a.pop("w"), a.pop("bias"), a.pop("gamma"), a.pop("beta"), a.pop("res16"), a.pop("ks"), False, False, rounded, **a)
    return y.permute(0, 2, 3, 1).to(torch.float16).contiguous()


def ref_block(case, rounded=True, **wiring):
    """The block as a chain of float64 launches, each stage's fp16 output feeding the next -> dict(h1, mid (forms 1, 2), out, ss) as the entry
    returns them.  With rounded = True this is what a correct engine computes up to its fp32 accumulation; **wiring as for block_stages."""
    x16, got = case["x16"], {}
    form = wiring.get("form", case["form"])
    stage = lambda name: _run_stage(dict(block_stages(case, x16, got.get("h1"), got.get("mid"), **wiring))[name], rounded)
    got["h1"] = stage("h1")
    if form:
        got["mid"] = stage("mid")
    got["out"] = stage("out")
    B, cout = case["B"], case["cout"]
    got["ss"] = ref_scale_shift(got["out"].reshape(B, -1, cout), case["og"], case["ob"])
    return got


def check_block(case, got, what=""):
    """Every launch of the block against float64 of its own fp16 inputs (got["h1"], got["mid"], the case's x16), and the next GroupNorm's
    (scale, shift) against float64 statistics of got["out"].  -> dict stage -> (max error / bound, rms / E_model), "ss" -> error / 2^-11."""
    res = {}
    for name, a in block_stages(case, case["x16"], got["h1"], got.get("mid")):
        a = dict(a)
        res[name] = check_conv(got[name], a.pop("x16"), a.pop("w"), a.pop("bias"), a.pop("gamma"), a.pop("beta"), a.pop("res16"), a.pop("ks"),
                               what=f"{what} {name}")
    B, cout = case["B"], case["cout"]
    res["ss"] = check_scale_shift(got["ss"], got["out"].reshape(B, -1, cout), case["og"], case["ob"], f"{what} output GroupNorm")
    return res


# ------------------------------------------------------------------------------------------------ AttnBlock (taming.hip run_attn)
# (block, H, W, B, latent side of the handle): N = 128 / 256 on the latent-16 handle, N = 1024 on a latent-32 one
ATTN_CASES = [(0, 8, 16, 1, 16), (0, 8, 16, 2, 16), (0, 16, 16, 1, 16), (0, 16, 16, 2, 16), (6, 16, 16, 2, 16), (3, 32, 32, 1, 32)]
_ATTN_CACHE = {}


def attn_seed(case):
    return 500 + ATTN_CASES.index(case)


def ref_attention(q16, k16, v16, rounded, scale=T_ATT ** -0.5):
    """q, k, v fp16 [B, N, 512] -> (out fp64 [B, N, 512], probabilities).  Exact: taming_reference.attention's softmax(q k^T 512^-0.5) v.  rounded:
    the kernel's documented roundings -- the unnormalised probabilities exp(s - max) to fp16 for P V, normalised by the sum of the unrounded ones,
    the output to fp16."""
    q, k, v = q16.double(), k16.double(), v16.double()
    if not rounded and scale == T_ATT ** -0.5:
        return TR.attention(q, k, v), torch.softmax(torch.bmm(q, k.transpose(1, 2)) * scale, dim=2)
    s = torch.bmm(q, k.transpose(1, 2)) * scale
    e = torch.exp(s - s.max(dim=2, keepdim=True).values)
    den = e.sum(dim=2, keepdim=True)
    if not rounded:
        return torch.bmm(e / den, v), e / den
    return h16r(torch.bmm(h16r(e), v) / den), e / den


def make_attn(block, H, W, B, seed):
    """Seeded inputs of one AttnBlock case (cached): x16 fp16 [B, H, W, 512] and the block's fp32 parameters under their checkpoint names
    (norm, q, k, v, proj_out).  The gain of q.weight is chosen by bisection on the float64 reference so that the mean maximum probability is about
    0.5: with the plain draw the softmax over N keys is nearly uniform and a wrong score would not show.  -> dict, "mp" = the mean maximum probability
    of the float64 reference with the final (fp16-rounded) weights."""
    key = (block, H, W, B, seed)
    if key in _ATTN_CACHE:
        return _ATTN_CACHE[key]
    C_ = T_ATT
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    x16 = (r(B, H, W, C_) * (0.5 + torch.rand(C_, generator=g)) + r(C_)).to(torch.float16)
    P = {"norm.weight": 1.0 + 0.3 * r(C_), "norm.bias": 0.3 * r(C_)}
    for n in ("q", "k", "v", "proj_out"):
        P[n + ".weight"] = r(C_, C_, 1, 1) / math.sqrt(C_)
        P[n + ".bias"] = 0.3 * r(C_)
    P["v.weight"] = P["v.weight"] * 1.5
    case = dict(block=block, H=H, W=W, B=B, x16=x16, P=P, og=1.0 + 0.3 * r(C_), ob=0.3 * r(C_))

    def mean_max_prob():
        q, k, v = split_qkv(ref_qkv(case, rounded=True), B)
        return float(ref_attention(q, k, v, False)[1].max(dim=2).values.mean())

    # the bisection works on the scores' two parts, gain * (Wq a) . k + bq . k, of the float64 projection; the result is measured with the real weights
    a = h16r(F.group_norm(nchw(x16), 32, P["norm.weight"].double(), P["norm.bias"].double(), 1e-6)).permute(0, 2, 3, 1).reshape(B, H * W, C_)
    wq, wk = P["q.weight"].double().reshape(C_, C_), P["k.weight"].double().reshape(C_, C_)
    kk = (a @ wk.t() + P["k.bias"].double()).transpose(1, 2)
    s_w, s_b = torch.bmm(a @ wq.t(), kk) * C_ ** -0.5, (P["q.bias"].double() @ kk)[:, None, :] * C_ ** -0.5
    lo, hi = 1e-2, 256.0
    for _ in range(16):
        f = (lo * hi) ** 0.5
        mp = float(torch.softmax(f * s_w + s_b, dim=2).max(dim=2).values.mean())
        lo, hi = (f, hi) if mp < 0.5 else (lo, f)
    P["q.weight"] = P["q.weight"] * lo
    case["mp"] = mean_max_prob()
    _ATTN_CACHE[key] = case
    return case


def qkv_params(P):
    """the stacked 512 -> 1536 projection in canonical order q, k, v"""
    return torch.cat([P[n + ".weight"] for n in ("q", "k", "v")]), torch.cat([P[n + ".bias"] for n in ("q", "k", "v")])


def ref_qkv(case, rounded, silu=False):
    """-> qkv fp16 [B N, 1536]: GroupNorm (no SiLU) -> the stacked 1x1 projection of x16"""
    w, b = qkv_params(case["P"])
    y, _ = ref_conv(case["x16"], w, b, case["P"]["norm.weight"], case["P"]["norm.bias"], None, 1, False, False, rounded, silu=silu)
    return y.permute(0, 2, 3, 1).reshape(-1, 3 * T_ATT).to(torch.float16).contiguous()


def split_qkv(qkv16, B):
    """qkv [B N, 1536] -> the column blocks q, k, v, each [B, N, 512]"""
    t = qkv16.reshape(B, -1, 3 * T_ATT)
    return t[..., :T_ATT], t[..., T_ATT:2 * T_ATT], t[..., 2 * T_ATT:]


def ref_attn_block(case, rounded=True, silu=False, rotate=0, scale=T_ATT ** -0.5, residual="x"):
    """run_attn as a chain of float64 launches, each stage's fp16 output feeding the next -> dict(qkv [B N, 1536], attn [B N, 512],
    out [B, H, W, 512], ss) as the entry returns them.  The keyword arguments are the CPU test's mutants: SiLU in the q / k / v prologue, the
    column blocks of qkv rotated by `rotate` blocks, another score scale, proj_out's residual ("x", "attn" or None)."""
    B, H, W, P = case["B"], case["H"], case["W"], case["P"]
    qkv = ref_qkv(case, rounded, silu=silu)
    if rotate:
        qkv = torch.roll(qkv, rotate * T_ATT, dims=1).contiguous()
    att, _ = ref_attention(*split_qkv(qkv, B), rounded, scale=scale)
    att = att.reshape(B * H * W, T_ATT).to(torch.float16)
    att_img = att.reshape(B, H, W, T_ATT)
    res = {"x": case["x16"], "attn": att_img, None: None}[residual]
    y, _ = ref_conv(att_img, P["proj_out.weight"], P["proj_out.bias"], None, None, res, 1, False, False, rounded)
    out = y.permute(0, 2, 3, 1).to(torch.float16).contiguous()
    return dict(qkv=qkv, attn=att, out=out, ss=ref_scale_shift(out.reshape(B, -1, T_ATT), case["og"], case["ob"]))


def check_attention(got, q16, k16, v16, what=""):
    """The bound of test_hip_spatial_attention.py: |out - ref| <= 2^-9 max|v| against float64 of the given fp16 q, k, v.  -> error / bound"""
    ref, _ = ref_attention(q16, k16, v16, False)
    err = float((got.double().cpu().reshape(ref.shape) - ref).abs().max())
    bound = 2.0 ** -9 * float(v16.float().abs().max())
    print(f"{what}: max |out - ref| {err:.3g}, bound {bound:.3g}, ratio {err / bound:.3f}")
    assert err <= bound, (what, err / bound)
    return err / bound


def check_attn_block(case, got, what=""):
    """Every launch of run_attn against float64 of its own fp16 inputs: qkv from x16 (no-SiLU prologue, canonical q, k, v order), the attention
    from the slices of got["qkv"], proj_out + x16 from got["attn"], the next GroupNorm's (scale, shift) from got["out"].
    -> dict(qkv, out -> (max error / bound, rms / E_model), attn -> error / bound, ss -> error / 2^-11)."""
    B, H, W, P = case["B"], case["H"], case["W"], case["P"]
    w, b = qkv_params(P)
    res = {"qkv": check_conv(got["qkv"].reshape(B, H, W, 3 * T_ATT), case["x16"], w, b, P["norm.weight"], P["norm.bias"], None, 1, silu=False,
                             what=f"{what} qkv")}
    res["attn"] = check_attention(got["attn"], *split_qkv(got["qkv"].cpu(), B), what=f"{what} attention")
    res["out"] = check_conv(got["out"], got["attn"].cpu().reshape(B, H, W, T_ATT), P["proj_out.weight"], P["proj_out.bias"], None, None,
                            case["x16"], 1, what=f"{what} proj_out")
    res["ss"] = check_scale_shift(got["ss"], got["out"].cpu().reshape(B, -1, T_ATT), case["og"], case["ob"], f"{what} output GroupNorm")
    return res


# ------------------------------------------------------------------------------------------------ the folded final layer, the +-1 packer
def make_final(H, W, B, seed):
    """decoder.norm_out + decoder.conv_out (128 -> 3): x16 fp16 [B, H, W, 128]; weights fp16-representable NORMAL numbers of at least 2^-13, so
    that halving them is exact in fp16; |bias| log-uniform in [2^-20, 4] with random signs."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    x16 = (r(B, H, W, 128) * (0.5 + torch.rand(128, generator=g)) + r(128)).to(torch.float16)
    w = (r(3, 128, 3, 3) / math.sqrt(128 * 9)).to(torch.float16).float()
    w = torch.where(w.abs() < 2.0 ** -13, torch.full_like(w, 2.0 ** -13), w)
    mag = 2.0 ** (torch.rand(3, generator=g) * 22.0 - 20.0)
    mag[0], mag[1] = 2.0 ** -20, 4.0                                                    # both ends of the range are present
    bias = mag * torch.tensor([1.0, -1.0, 1.0])
    return dict(H=H, W=W, B=B, x16=x16, w=w, b=bias, gamma=1.0 + 0.3 * r(128), beta=0.3 * r(128))


def ref_final(case, rounded=True, fold="full"):
    """-> img fp32 NCHW: (conv(silu(gn(x))) + 1) / 2 in float64; fold = None / "weight": the mutants without the fold / with the weight's half only"""
    y, _ = ref_conv(case["x16"], case["w"], case["b"], case["gamma"], case["beta"], None, 3, False, True, rounded, fold=fold)
    return y.float()


def check_final(case, img, what=""):
    """the final layer's criteria (no fp16 store) against float64 of (conv(silu(gn(x))) + 1) / 2"""
    return check_conv(img, case["x16"], case["w"], case["b"], case["gamma"], case["beta"], None, 3, final=True, fold="full", what=what)


def prefolded(case):
    """the operands a loader without fold support would be handed: w * 0.5 and float32((float64(b) + 1) / 2), one rounding as fmaf(b, 0.5, 0.5)"""
    return case["w"] * 0.5, ((case["b"].double() + 1.0) / 2.0).float()


PACK_SHAPES = [(1, 1), (5, 7), (16, 16)]


def make_pack(B, H, W, seed):
    """img fp32 [B, 3, H, W]: the grid 0, 0.5, 1 with one fp32 step either side, -3, 1e5 (2 x - 1 beyond the fp16 range), then uniform [0, 1)"""
    g = torch.Generator().manual_seed(seed)
    one = torch.tensor(4.0)
    base = torch.tensor([0.0, 0.5, 1.0])
    grid = torch.cat([base, torch.nextafter(base, one), torch.nextafter(base, -one), torch.tensor([-3.0, 1e5, -1e5, 0.25, 0.75])])
    n = B * 3 * H * W
    v = torch.rand(n, generator=g)
    m = min(n, grid.numel())
    v[torch.randperm(n, generator=g)[:m]] = grid[:m]
    return v.reshape(B, 3, H, W)


def ref_pack(img, scaled=True):
    """-> fp16 [B H W, 64]: channels 0 .. 2 = fp16(x * 2 - 1) of the fp32 product, clamped at +-65504; 0 beyond.  scaled = False: the mutant x"""
    B, _, H, W = img.shape
    v = (img.float() * 2.0 - 1.0) if scaled else img.float()
    out = torch.zeros(B * H * W, 64, dtype=torch.float16)
    out[:, :3] = v.clamp(-65504.0, 65504.0).permute(0, 2, 3, 1).reshape(-1, 3).half()
    return out


def check_pack(got, img):
    assert torch.equal(got.cpu(), ref_pack(img)), "the packed image differs from fp16(2 x - 1)"
