"""GPU tests of the head path of gemm.hip, per launch: the two head GEMMs as engine.hip head_gemms fills them (three sweeps with the weights' lo plane and
the power-of-two scale; Bert's two-sweep form with the per-position bias) and the kernels that run once per checkpoint load (split_f32_to_h16_planes,
cast_f32_to_h16, w4_from_f32, w4lo_from_f32), against the float64 statements of tests/head_reference.py.

Exact operands (small integers, power-of-two scales): the logits epilogue must EQUAL float64 bit for bit, the GELU epilogue lies within 2e-4 of max |ref|.
Split planes, cast and the e2m1 copy of the rounding errors: every bit / byte equals the statement.  The e2m1 value copy: every code equals
e2m1(fp16(w) 2^r) for the r of its scale byte, and r is the float64 argmin wherever float64 decides it (head_reference.w4_check).  Outputs live in NaN /
0xA5-filled buffers with guard bands that must stay untouched.  tests/test_head_cpu.py proves what this net catches; profiles/head_kernels.md records
what was measured.  Weights beyond fp16's range are out of scope for the e2m1 copies: no checkpoint has them, their output is not defined."""
import pytest
import torch

import head_reference as H

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 288                                  # guard rows around a GEMM output: more than two 128-row tiles
PAD = 4096                                   # guard elements around a flat output


def _L():
    from maskbit_amd import _lib
    return _lib


def _lib():
    return _L().load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _guarded_rows(rows, cols):
    buf = torch.full((rows + 2 * GUARD, cols), float("nan"), device=DEV, dtype=torch.float32)
    return buf, buf[GUARD:GUARD + rows]


def _guarded_flat(n, dtype):
    """-> (whole buffer, the n output elements in its middle; 16-byte aligned); fill: NaN, bytes 0xA5."""
    fill = 0xA5 if dtype == torch.uint8 else float("nan")
    buf = torch.full((n + 2 * PAD,), fill, device=DEV, dtype=dtype)
    return buf, buf[PAD:PAD + n]


def _untouched(buf, lo, hi):
    g = torch.cat([buf[:lo].reshape(-1), buf[hi:].reshape(-1)])
    return bool((g == 0xA5).all()) if buf.dtype == torch.uint8 else bool(torch.isnan(g).all())


def _to(c, dev):
    mv = lambda t: t.to(dev) if t is not None else None
    return mv(c.A), mv(c.A2), mv(c.W), mv(c.W2), mv(c.bias)


def _head(lib, c, ops, out, scale_t, *, epi=None, M=None, N=None, kw=None, period=None, per_pos=None):
    A, A2, W, W2, bias = ops
    return lib.mb_gemm_head(c.epi if epi is None else epi, _ptr(A), _ptr(A2), _ptr(W), _ptr(W2), _ptr(scale_t), _ptr(bias),
                            int(c.per_pos if per_pos is None else per_pos), _ptr(out), c.M if M is None else M, c.N if N is None else N,
                            c.kw if kw is None else kw, c.period if period is None else period, _stream())


def _run_head(lib, c):
    """One launch of an exact case -> (got [out rows, N] on the CPU, GELU error relative to max |ref| or 0)."""
    ops = _to(c, DEV)
    scale_t = torch.tensor([c.scale], device=DEV, dtype=torch.float32) if c.W2 is not None else None
    rows = H.head_out_rows(c)
    buf, view = _guarded_rows(rows, c.N)
    _L().check(_head(lib, c, ops, view, scale_t), "mb_gemm_head")
    torch.cuda.synchronize()
    assert _untouched(buf, GUARD, GUARD + rows), f"{c.label}: guard band written"
    got = view.cpu()
    assert not bool(torch.isnan(got).any()), f"{c.label}: {int(torch.isnan(got).sum())} output elements were not written"
    want = H.head_expected(c)
    if c.epi == 4:
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            raise AssertionError(f"{c.label}: {len(bad)} elements differ from float64, first at (row, column) {bad[0].tolist()}: "
                                 f"{float(got[tuple(bad[0])])} != {float(want[tuple(bad[0])])}; rows {sorted(set(bad[:, 0].tolist()))[:8]}")
        return got, 0.0
    top = float(want.abs().max())
    err = float((got.double() - want).abs().max())
    assert err < H.GELU_BOUND * top, f"{c.label}: GELU error {err:.3e} = {err / top:.2e} max |ref| (bound {H.GELU_BOUND:.0e})"
    return got, err / top


_CASES = None


def _cases(pred):
    global _CASES
    if _CASES is None:
        _CASES = H.head_cases()
    return [c for c in _CASES if pred(c)]


# ---- head GEMMs, exact operands ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", H.HEAD_M)
def test_head_gemm_gelu_three_and_two_sweeps(M):
    lib = _lib()
    cases = _cases(lambda c: c.epi == 3 and c.M == M)
    assert len(cases) == 2 * len(H.HEAD_N) * len(H.HEAD_KW)
    worst = max(_run_head(lib, c)[1] for c in cases)
    print(f"head GEMM epi 3 M {M}: largest GELU error {worst:.2e} of max |ref| (bound {H.GELU_BOUND:.0e}) over {len(cases)} launches")


@pytest.mark.parametrize("M,period", [mp for mp in H.LOGITS_SHAPES if mp[0] % mp[1] == 0])
def test_head_gemm_logits_equal_float64(M, period):
    lib = _lib()
    cases = _cases(lambda c: c.epi == 4 and (c.M, c.period) == (M, period))
    assert {(c.per_pos, c.W2 is not None) for c in cases} == {(a, b) for a in (False, True) for b in (False, True)}
    for c in cases:
        got, _ = _run_head(lib, c)
        assert got.shape[0] == M - M // period


def test_head_gemm_refusals_launch_nothing():
    lib = _lib()
    c = H.make_head_case(4, 10, 8, 64, period=5, three=True, per_pos=True, scale=1.0, seed=9)
    A, A2, W, W2, bias = _to(c, DEV)
    s = torch.ones(1, device=DEV)
    buf, view = _guarded_rows(10, 8)
    ok = (A, A2, W, W2, bias)
    refused = {
        "A_hi NULL": dict(ops=(None, A2, W, W2, bias)), "A_lo NULL": dict(ops=(A, None, W, W2, bias)), "W_hi NULL": dict(ops=(A, A2, None, W2, bias)),
        "bias NULL": dict(ops=(A, A2, W, W2, None)), "out NULL": dict(out=None), "kw 0": dict(kw=0), "kw -64": dict(kw=-64), "kw 32": dict(kw=32),
        "kw 96": dict(kw=96), "N 6": dict(N=6), "N 0": dict(N=0), "M 0": dict(M=0), "epilogue 2": dict(epi=2, per_pos=0), "epilogue 0": dict(epi=0, per_pos=0),
        "epilogue 5": dict(epi=5, per_pos=0), "period 1": dict(period=1), "period 0": dict(period=0), "M % period": dict(period=4),
        "600 rows of period 257": dict(M=600, period=257), "bias_per_pos with epilogue 3": dict(epi=3), "W_lo without scale": dict(scale=None),
        "scale without W_lo": dict(ops=(A, A2, W, None, bias)),
    }
    for name, kw in refused.items():
        kw = dict(kw)
        rc = _head(lib, c, kw.pop("ops", ok), kw.pop("out", view), kw.pop("scale", s), **kw)
        assert rc in (-1, -3), f"{name}: returned {rc}"
        assert lib.mb_last_error(), name
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()), "a refused call wrote to the output"
    _L().check(_head(lib, c, ok, view, s), "mb_gemm_head")                                # ... and the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert torch.equal(view[:8].cpu(), H.head_expected(c)) and _untouched(buf, GUARD, GUARD + 8)


# ---- head GEMMs on real-valued data ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", [3, 4])
def test_head_gemm_real_valued_is_as_good_as_fp32(epi):
    """LayerNorm rows split by mb_layernorm against a Gaussian weight split by mb_split_f32_planes, reference float64 (x_hi + x_lo) . W32^T + bias.
    Condition 1: the kernel's error is below 1 / 8 of E_hi, the error of the float64 product with the hi plane alone (the lo sweep does its work).
    Condition 2: it is within max(F E_ref, 2 ulp32(max |ref|)), E_ref the error of a plain fp32 CPU matmul of the same operands (F: head_reference.F_REF)."""
    L, lib = _L(), _lib()
    M, N, kw = H.REAL_SHAPE
    y, gamma, beta, W32, bias = (t.to(DEV) for t in H.real_inputs())
    x_hi, x_lo = torch.empty(M, kw, device=DEV, dtype=torch.float16), torch.empty(M, kw, device=DEV, dtype=torch.float16)
    L.check(lib.mb_layernorm(_ptr(y), _ptr(gamma), _ptr(beta), 1e-12, None, _ptr(x_hi), _ptr(x_lo), None, M, kw, _stream()), "mb_layernorm")
    w_hi, w_lo = torch.empty(N, kw, device=DEV, dtype=torch.float16), torch.empty(N, kw, device=DEV, dtype=torch.float16)
    scale, tmp = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV, dtype=torch.int32)
    L.check(lib.mb_split_f32_planes(_ptr(W32), _ptr(w_hi), _ptr(w_lo), N, kw, _ptr(scale), _ptr(tmp), _stream()), "mb_split_f32_planes")
    period = 257 if epi == 4 else 0
    rows = M - M // period if epi == 4 else M
    buf, view = _guarded_rows(rows, N)
    L.check(lib.mb_gemm_head(epi, _ptr(x_hi), _ptr(x_lo), _ptr(w_hi), _ptr(w_lo), _ptr(scale), _ptr(bias), 0, _ptr(view), M, N, kw, period, _stream()), "mb_gemm_head")
    torch.cuda.synchronize()
    assert _untouched(buf, GUARD, GUARD + rows)
    got = view.cpu()
    assert not bool(torch.isnan(got).any())
    keep = torch.arange(M)
    keep = keep[keep % period != period - 1] if epi == 4 else keep
    ref, e_hi, e_ref = H.real_reference(epi, x_hi.cpu(), x_lo.cpu(), W32.cpu(), bias.cpu(), w_hi.cpu(), scale.cpu(), rows=keep)
    err = float((got.double() - ref).abs().max())
    ulp = H.ulp32(float(ref.abs().max()))
    print(f"head GEMM epi {epi} real-valued M {M} N {N} kw {kw}: kernel error {err:.3e}, E_hi {e_hi:.3e} (ratio {err / e_hi:.3f}, bound 1/{H.HI_ONLY_FACTOR:.0f}), "
          f"E_ref {e_ref:.3e} (ratio {err / e_ref:.3f}, F {H.F_REF}), ulp32(max |ref|) {ulp:.3e}, max |ref| {float(ref.abs().max()):.3f}")
    assert e_hi > 0 and err < e_hi / H.HI_ONLY_FACTOR, f"epi {epi}: the lo sweep does not do its work: error {err:.3e} against {e_hi:.3e} with the hi plane alone"
    assert err <= max(H.F_REF * e_ref, 2 * ulp), f"epi {epi}: error {err:.3e} beyond {H.F_REF} x the fp32 matmul's {e_ref:.3e}"


# ---- split planes -------------------------------------------------------------------------------------------------------------------------------------------
def _split(lib, w, tmp):
    """One mb_split_f32_planes on guarded planes -> (hi buffer, lo buffer, scale buffer [3]) still on the device (no synchronisation)."""
    n = w.numel()
    hb, lb = _guarded_flat(n, torch.float16), _guarded_flat(n, torch.float16)
    sc = torch.full((3,), float("nan"), device=DEV)
    _L().check(lib.mb_split_f32_planes(_ptr(w), _ptr(hb[1]), _ptr(lb[1]), w.shape[0], w.shape[1], sc[1:].data_ptr(), _ptr(tmp), _stream()), "mb_split_f32_planes")
    return hb, lb, sc


def _split_check(w_cpu, res, label):
    (hbuf, hi), (lbuf, lo), sc = res
    n = w_cpu.numel()
    assert _untouched(hbuf, PAD, PAD + n) and _untouched(lbuf, PAD, PAD + n), f"{label}: a plane's guard band was written"
    assert bool(torch.isnan(sc[0])) and bool(torch.isnan(sc[2])), f"{label}: written beside the scale"
    whi, wlo, wsc = H.split_planes(w_cpu)
    assert float(sc[1]) == float(wsc), f"{label}: scale {float(sc[1])} != {float(wsc)}"
    for name, got, want in (("hi", hi.cpu(), whi.reshape(-1)), ("lo", lo.cpu(), wlo.reshape(-1))):
        bad = (got.view(torch.int16) != want.view(torch.int16)).nonzero()
        assert not len(bad), f"{label}: {len(bad)} elements of the {name} plane differ, first at {int(bad[0])}: {float(got[bad[0]])} != {float(want[bad[0]])}"


@pytest.mark.parametrize("N,K", H.SPLIT_SHAPES)
def test_split_planes_equal_the_statement(N, K):
    lib = _lib()
    tmp = torch.full((1,), 0x7F7FFFFF, device=DEV, dtype=torch.int32)                    # stale scratch: the launcher clears it
    inputs = H.split_inputs(N, K)
    assert ("single in the second pass" in [n for n, _, _ in inputs]) == (N * K > H.GRID_PASS)
    for name, w, _ in inputs:
        res = _split(lib, w.to(DEV), tmp)
        torch.cuda.synchronize()
        _split_check(w, res, f"split {N} x {K} '{name}'")


def test_split_planes_back_to_back_share_one_scratch_word():
    """As mb_gen_load runs the two head weights: one tmp, one stream, no synchronisation in between -- the same bits as each alone."""
    lib = _lib()
    g = torch.Generator().manual_seed(3)
    small, large = torch.randn(96, 128, generator=g) * 0.01, torch.randn(64, 192, generator=g) * 5.0
    tmp = torch.zeros(1, device=DEV, dtype=torch.int32)
    ws = [w.to(DEV) for w in (large, small, large)]                                         # a larger maximum before a smaller one, and back
    torch.cuda.synchronize()
    res = [_split(lib, w, tmp) for w in ws]
    torch.cuda.synchronize()
    for w, r, name in zip((large, small, large), res, ("first (large)", "second (small)", "third (large)")):
        _split_check(w, r, f"back to back, {name}")
    assert float(res[0][2][1]) != float(res[1][2][1])


# ---- cast ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", H.CAST_N)
def test_cast_equals_round_to_nearest_even(n):
    lib = _lib()
    x = H.cast_values(n)
    src = torch.cat([x, torch.full((8,), 7.0)]).to(DEV)                                      # (readable slack behind the source)
    buf, view = _guarded_flat(n, torch.float16)
    dst = buf.data_ptr() + PAD * buf.element_size()                                          # (n = 0: an empty view has no pointer to speak of)
    _L().check(lib.mb_cast_f32_to_h16(_ptr(src), dst, n, _stream()), "mb_cast_f32_to_h16")
    torch.cuda.synchronize()
    assert _untouched(buf, PAD, PAD + n), f"n {n}: written outside dst[0, n)"
    got, want = view.cpu(), H.cast_reference(x)
    if not H.same_f16(got, want):
        bad = ((got.view(torch.int16) != want.view(torch.int16)) & ~(torch.isnan(got) & torch.isnan(want))).nonzero()
        raise AssertionError(f"n {n}: {len(bad)} elements differ, first at {int(bad[0])}: fp16({float(x[bad[0]])!r}) = {float(got[bad[0]])} != {float(want[bad[0]])}")
    if n >= 29:
        assert bool(torch.isinf(got).any()) and bool(torch.isnan(got).any()) and bool(((got.float().abs() < 2.0 ** -14) & (got != 0)).any())


def test_cast_refusals():
    lib = _lib()
    x = torch.ones(8, device=DEV)
    buf, view = _guarded_flat(8, torch.float16)
    assert lib.mb_cast_f32_to_h16(None, _ptr(view), 8, _stream()) == -1 and lib.mb_cast_f32_to_h16(_ptr(x), None, 8, _stream()) == -1
    assert lib.mb_cast_f32_to_h16(_ptr(x), _ptr(view), -1, _stream()) == -1
    t = torch.zeros(1, device=DEV, dtype=torch.int32)
    for args in ((None, view, view, 2, 4, x, t), (x, None, view, 2, 4, x, t), (x, view, None, 2, 4, x, t), (x, view, view, 2, 4, None, t),
                 (x, view, view, 2, 4, x, None), (x, view, view, 0, 4, x, t), (x, view, view, 2, 0, x, t), (x, view, view, -2, 4, x, t)):
        assert lib.mb_split_f32_planes(*[_ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args], _stream()) == -1, args[3:5]
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()) and bool((x == 1).all())


# ---- e2m1 copies of a weight --------------------------------------------------------------------------------------------------------------------------------------
def _w4_run(lib, entry, w):
    N, K = w.shape
    b4, v4 = _guarded_flat(N * K // 2, torch.uint8)
    bs, vs = _guarded_flat(N * K // 128, torch.uint8)
    wd = w.to(DEV)
    _L().check(getattr(lib, entry)(_ptr(wd), N, K, _ptr(v4), _ptr(vs), _stream()), entry)
    torch.cuda.synchronize()
    assert _untouched(b4, PAD, PAD + N * K // 2) and _untouched(bs, PAD, PAD + N * K // 128), f"{entry} {N} x {K}: guard band written"
    return v4.cpu(), vs.cpu()


@pytest.mark.parametrize("N,K", H.W4_SHAPES)
def test_w4lo_equals_the_statement_byte_for_byte(N, K):
    lib = _lib()
    for name, w, use in H.w4_inputs(N, K):
        if use != "w4":
            H.w4lo_check(w, *_w4_run(lib, "mb_w4lo_from_f32", w), label=f"w4lo {N} x {K} '{name}'")


@pytest.mark.parametrize("N,K", H.W4_SHAPES)
def test_w4_codes_are_exact_and_the_scale_is_the_float64_choice(N, K):
    lib = _lib()
    for name, w, use in H.w4_inputs(N, K):
        if use == "w4lo":
            continue
        w4, ws = _w4_run(lib, "mb_w4_from_f32", w)
        ref4, refs = H.w4_emulate(w)
        share, moved = H.w4_check(w, w4, ws, label=f"w4 {N} x {K} '{name}'")
        print(f"w4 {N} x {K} '{name}': {N * K // 128} blocks, undecided share {share:.4f} (cap {H.MAX_UNDECIDED}), blocks whose r is not the float64 argmin "
              f"{moved}, bytes equal to the float64 emulation: codes {bool(torch.equal(w4, ref4))} scales {bool(torch.equal(ws, refs))}")
