"""What the per-launch GPU tests of the Conv+BatchNorm networks (test_hip_inception.py, test_hip_perceptual.py) share: the library handle, one
runner of the convolution's two diagnostic entries, its float64 reference with the magnitude sum of the bound, the error criterion, the
integer-operand case maker and the pool runner; and the runners of the fp32 tail's entries (mb_bn_fold, mb_spatial_mean, mb_fc_head,
mb_channel_tap, mb_*_folded_bn), each on a window of a NaN-filled buffer (tests/test_hip_convnet_tail.py)."""
import ctypes as C

import torch
import torch.nn.functional as F

from convnet_reference import h16r

DEV = "cuda"
U16 = 2.0 ** -11
U32 = 2.0 ** -24
EPI_RELU, EPI_LINEAR, EPI_RESIDUAL = 0, 1, 2


def _lib():
    from maskbit_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(torch.int16)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def run_convbn(xbuf, w, scale, shift, stride, pad, in_off=0, out=None, out_off=0, variant=0, epi=None, idn=None, idn_off=0):
    """``epi`` None: mb_convbn_layer; an epilogue (EPI_*): mb_convbn_layer_ex.  xbuf fp16 [B, H, W, in_cs] (CPU) of which channels
    [in_off, in_off + Cin) are read, w fp32 OIHW, pad an int or (ph, pw); `out` (CPU, optional) is the pre-filled output buffer, written at
    channels [out_off, out_off + Cout); idn fp16 [B, Ho, Wo, idn_cs] of which channels [idn_off, idn_off + Cout) are the identity
    -> (the output buffer on the CPU, saturation count)"""
    L, lib = _lib()
    B, H, W, in_cs = xbuf.shape
    cout, cin, kh, kw = w.shape
    ph, pw = _pair(pad)
    Ho, Wo = (H + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1
    if out is None:
        out = torch.full((B, Ho, Wo, cout), float("nan"), dtype=torch.float16)
    assert tuple(out.shape[:3]) == (B, Ho, Wo)
    xd, wd, od = xbuf.to(DEV).contiguous(), w.float().to(DEV).contiguous(), out.to(DEV).contiguous()
    sc, sh = scale.float().to(DEV).contiguous(), shift.float().to(DEV).contiguous()
    idd = idn.to(DEV).contiguous() if idn is not None else None
    sat = C.c_uint(0)
    head = (xd.data_ptr(), wd.data_ptr(), sc.data_ptr(), sh.data_ptr(), od.data_ptr(), C.byref(sat), B, H, W, cin, cout, kh, kw, stride, ph, pw, in_off, in_cs,
            out_off, out.shape[3], variant)
    if epi is None:
        L.check(lib.mb_convbn_layer(*head, _stream()), "mb_convbn_layer")
    else:
        L.check(lib.mb_convbn_layer_ex(*head, epi, idd.data_ptr() if idd is not None else None, idn_off, idn.shape[3] if idn is not None else 0, _stream()),
                "mb_convbn_layer_ex")
    torch.cuda.synchronize()
    return od.cpu(), int(sat.value)


def ref_convbn(x16, w, scale, shift, stride, pad, epi=EPI_RELU, idn16=None):
    """-> (exact float64 NCHW with fp16 weights, the magnitude sum S of the bound)"""
    a = x16.double().permute(0, 3, 1, 2)
    wq = w.to(torch.float16).double()
    sc, sh = scale.float().double().view(1, -1, 1, 1), shift.float().double().view(1, -1, 1, 1)
    y = F.conv2d(a, wq, None, stride, pad) * sc + sh
    S = F.conv2d(a.abs(), wq.abs(), None, stride, pad) * sc.abs() + sh.abs()
    if epi == EPI_RESIDUAL:
        i = idn16.double().permute(0, 3, 1, 2)
        y, S = y + i, S + i.abs()
    return (y if epi == EPI_LINEAR else F.relu(y)), S


def check_against_fp64(tag, got16, exact, S, terms, epi=EPI_RELU):
    """per element 2^-11 |y| (the fp16 store) + `terms` 2^-24 S (the fp32 accumulation and epilogue: the caller's count of roundings); rms error
    <= 1.25 x the rms error of the same layer with the output rounded to fp16; what ReLU cuts is exactly 0"""
    got = got16.double().permute(0, 3, 1, 2)
    model = h16r(exact)
    assert got.shape == exact.shape and bool(torch.isfinite(got).all())
    bound = U16 * exact.abs() + terms * U32 * S
    err = (got - exact).abs()
    worst = (err / bound.clamp(min=1e-300)).max().item()
    e_kernel, e_model = err.pow(2).mean().sqrt().item(), (model - exact).pow(2).mean().sqrt().item()
    print(f"convbn {tag}: max err / bound {worst:.3f}; rms err {e_kernel:.3e}, E_model {e_model:.3e}, ratio {e_kernel / e_model:.3f}; "
          f"zeros {float((exact == 0).double().mean()):.2f}, negative {float((exact < 0).double().mean()):.2f}")
    assert worst <= 1.0
    assert e_model > 0.0 and e_kernel <= 1.25 * e_model
    if epi == EPI_LINEAR:
        assert bool((got < 0).any())
    else:
        assert bool((got >= 0).all()) and bool((got[exact == 0] == 0).all())       # what ReLU cuts is exactly 0


def integer_case(seed, B, H, W, cin, cout, k, stride=1, pad=0, residual=False):
    """operands whose every partial sum is an integer below 2^24 (exact in fp32), scale a power of two, shift and (`residual`) identity multiples
    of 1/2 -> (x16, w, scale, shift, idn or None); k and pad an int or a pair"""
    (kh, kw), (ph, pw) = _pair(k), _pair(pad)
    g = torch.Generator().manual_seed(seed)
    x16 = torch.randint(0, 4, (B, H, W, cin), generator=g).to(torch.float16)
    w = torch.randint(-2, 3, (cout, cin, kh, kw), generator=g).float()
    scale = torch.pow(2.0, torch.randint(-3, 1, (cout,), generator=g).float())
    shift = torch.randint(-8, 9, (cout,), generator=g).float() * 0.5
    Ho, Wo = (H + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1
    idn = (torch.randint(0, 64, (B, Ho, Wo, cout), generator=g).float() * 0.5).to(torch.float16) if residual else None
    return x16, w, scale, shift, idn


# ---- the networks' tail (tests/test_hip_convnet_tail.py and the network tests): every runner hands the entry a window of a larger buffer filled
# with NaN and returns (the window, whether everything outside it still holds the sentinel), both on the CPU
GUARD = 64


def bits32(t):
    return t.contiguous().view(torch.int32)


def _guarded(n):
    return torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)


def _window(buf, n):
    host = buf.cpu()
    return host[GUARD:GUARD + n].clone(), bool(torch.isnan(host[:GUARD]).all()) and bool(torch.isnan(host[GUARD + n:]).all())


def run_bn_fold(bn, eps):
    """mb_bn_fold on bn fp32 [4, cout] -> (scale, shift, untouched)"""
    L, lib = _lib()
    cout = bn.shape[1]
    bd = bn.float().to(DEV).contiguous()
    sc, sh = _guarded(cout), _guarded(cout)
    L.check(lib.mb_bn_fold(bd.data_ptr(), sc[GUARD:].data_ptr(), sh[GUARD:].data_ptr(), cout, eps, _stream()), "mb_bn_fold")
    torch.cuda.synchronize()
    (s, ok_s), (t, ok_t) = _window(sc, cout), _window(sh, cout)
    return s, t, ok_s and ok_t


def run_spatial_mean(x16):
    """mb_spatial_mean on x16 fp16 [B, HW, C] -> (mean fp32 [B, C], untouched)"""
    L, lib = _lib()
    B, HW, C_ = x16.shape
    xd = x16.to(DEV).contiguous()
    out = _guarded(B * C_)
    L.check(lib.mb_spatial_mean(xd.data_ptr(), out[GUARD:].data_ptr(), B, HW, C_, _stream()), "mb_spatial_mean")
    torch.cuda.synchronize()
    got, ok = _window(out, B * C_)
    return got.view(B, C_), ok


def run_fc_head(pool, w, bias=None, unbiased=True, biased=True):
    """mb_fc_head -> (unbiased or None, biased or None, untouched); pool [B, D], w [N, D], bias [N] or None"""
    L, lib = _lib()
    (B, D), N = pool.shape, w.shape[0]
    pd, wd = pool.float().to(DEV).contiguous(), w.float().to(DEV).contiguous()
    bd = bias.float().to(DEV).contiguous() if bias is not None else None
    ou, ob = (_guarded(B * N) if unbiased else None), (_guarded(B * N) if biased else None)
    ptr = lambda t: t[GUARD:].data_ptr() if t is not None else None
    L.check(lib.mb_fc_head(pd.data_ptr(), wd.data_ptr(), bd.data_ptr() if bd is not None else None, ptr(ou), ptr(ob), B, D, N, _stream()), "mb_fc_head")
    torch.cuda.synchronize()
    got, ok = [], True
    for t in (ou, ob):
        if t is None:
            got.append(None)
        else:
            v, fine = _window(t, B * N)
            got.append(v.view(B, N))
            ok = ok and fine
    return got[0], got[1], ok


def run_channel_tap(buf16, C_, off):
    """mb_channel_tap on channels [off, off + C_) of buf16 fp16 [B, HW, cs] -> (out fp32 [B, HW, C_], untouched)"""
    L, lib = _lib()
    B, HW, cs = buf16.shape
    xd = buf16.to(DEV).contiguous()
    n = B * HW * C_
    out = _guarded(n)
    L.check(lib.mb_channel_tap(xd.data_ptr(), out[GUARD:].data_ptr(), B, HW, C_, off, cs, _stream()), "mb_channel_tap")
    torch.cuda.synchronize()
    got, ok = _window(out, n)
    return got.view(B, HW, C_), ok


def folded_bns(abi, h, layers):
    """mb_{abi}_folded_bn of every (BatchNorm prefix, cout) in `layers` on handle h -> {prefix: (scale, shift)} fp32 on the CPU"""
    L, lib = _lib()
    entry = getattr(lib, f"mb_{abi}_folded_bn")
    total = sum(c for _p, c in layers)
    buf = torch.full((2, total), float("nan"), dtype=torch.float32, device=DEV)
    at = 0
    for prefix, cout in layers:
        L.check(entry(h, prefix.encode(), buf[0, at:].data_ptr(), buf[1, at:].data_ptr(), cout, _stream()), f"mb_{abi}_folded_bn({prefix})")
        at += cout
    torch.cuda.synchronize()
    host, out, at = buf.cpu(), {}, 0
    for prefix, cout in layers:
        out[prefix] = (host[0, at:at + cout].clone(), host[1, at:at + cout].clone())
        at += cout
    return out


def run_pool(x16, mode, out=None, out_off=0, ex=False):
    """mb_pool3 (`ex`: mb_pool3_ex, which also takes mode 3) on x16 fp16 [B, H, W, C] -> the (optionally pre-filled) output buffer on the CPU"""
    L, lib = _lib()
    B, H, W, C_ = x16.shape
    size = {0: lambda n: (n - 3) // 2 + 1, 3: lambda n: (n - 1) // 2 + 1}.get(mode, lambda n: n)
    if out is None:
        out = torch.full((B, size(H), size(W), C_), float("nan"), dtype=torch.float16)
    xd, od = x16.to(DEV).contiguous(), out.to(DEV).contiguous()
    entry = "mb_pool3_ex" if ex else "mb_pool3"
    L.check(getattr(lib, entry)(xd.data_ptr(), od.data_ptr(), B, H, W, C_, mode, 0, C_, out_off, out.shape[3], _stream()), entry)
    torch.cuda.synchronize()
    return od.cpu()
