"""The quantizer kernels one launch sequence at a time, against the plain restatements of tests/quantizer_reference.py (anchored without a GPU by
tests/test_quantizer_cpu.py): the lookup search with its row and codebook preparation (mb_vq_encode_rows), the code gather and the latent pack
(mb_vq_gather, mb_vq_pack_latent), the LFQ sign / pack and its inverse (mb_lfq_pack, mb_lfq_latent) and the image pack (mb_pack_image).

Every comparison is bit equality over ALL rows, pixels and elements: the kernels select, copy or round once, and the search cases have integer
operands whose scores fp32 computes exactly in any order.  Output buffers are pre-filled with a sentinel (NaN, -1234) and followed by a guard region
that must stay untouched."""
import pytest
import torch

import quantizer_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 320
INT_OF = {2: torch.int16, 4: torch.int32, 8: torch.int64}


def lib():
    from maskbit_amd import _lib
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def sentinel_buffer(n, dtype):
    return torch.full((n + GUARD,), -1234 if dtype in (torch.int64, torch.int32) else float("nan"), dtype=dtype, device=DEV)


def untouched(buf, n=0):
    fresh = sentinel_buffer(buf.numel() - GUARD, buf.dtype)
    w = INT_OF[buf.element_size()]
    return torch.equal(buf[n:].view(w), fresh[n:].view(w))


def same(got, want):
    """bit equality (so +0 is not -0); a NaN equals a NaN"""
    want = want.to(got.device)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if not got.dtype.is_floating_point:
        return torch.equal(got, want)
    w = INT_OF[got.element_size()]
    return bool(((got.contiguous().view(w) == want.contiguous().view(w)) | (got.isnan() & want.isnan())).all())


def ptr(t):
    return t.data_ptr() if t is not None else None


# ------------------------------------------------------------------------------------------------------------------ lookup search
def encode_rows(cb, B, HW, splits, z32=None, z16=None, l2=0, want=("idx", "zq", "zraw", "dist")):
    """-> {name: output}, after checking the guard regions"""
    N, (C, K) = B * HW, cb.shape
    sizes = {"idx": (N, torch.int64), "zq": (N * K, torch.float32), "zraw": (N * K, torch.float32), "dist": (N, torch.float32)}
    buf = {k: sentinel_buffer(*sizes[k]) for k in want}
    rc = lib().mb_vq_encode_rows(ptr(z16), z16.shape[1] if z16 is not None else 0, ptr(z32), cb.data_ptr(), B, HW, C, K, l2, splits,
                                 ptr(buf.get("idx")), ptr(buf.get("zq")), ptr(buf.get("zraw")), ptr(buf.get("dist")), stream())
    assert rc == 0, lib().mb_last_error()
    torch.cuda.synchronize()
    out = {}
    for k, b in buf.items():
        n = sizes[k][0]
        assert untouched(b, n), f"{k}: written beyond its {n} elements"
        out[k] = b[:n].reshape(B, K, HW) if k in ("zq", "zraw") else b[:n]
    return out


_REF = {}


def search_ref(case):
    if case not in _REF:
        z, cb, want = R.search_case(case)
        idx, dist, zq, zraw = R.lookup_search(z, cb, case.B, case.HW)
        assert want is None or torch.equal(idx, want)
        _REF[case] = (z.to(DEV), cb.to(DEV), dict(idx=idx.to(DEV), dist=dist.float().to(DEV), zq=zq.to(DEV), zraw=zraw.to(DEV)))
    return _REF[case]


@pytest.mark.parametrize("case", R.SEARCH_CASES, ids=lambda c: c.name)
def test_search_equals_the_restatement_for_every_split_count(case):
    z, cb, ref = search_ref(case)
    for splits in R.SPLITS:
        out = encode_rows(cb, case.B, case.HW, splits, z32=z)
        for k in ("idx", "dist", "zq", "zraw"):
            assert same(out[k], ref[k]), f"{case.name} splits={splits}: {k} differs in {int((out[k] != ref[k]).sum())} of {ref[k].numel()} elements"


@pytest.mark.parametrize("case", R.SEARCH_CASES, ids=lambda c: c.name)
def test_search_from_strided_fp16_rows(case):
    z, cb, ref = search_ref(case)
    for stride in R.strides16(case.K):
        z16 = R.fp16_rows(z.cpu(), stride).to(DEV)
        out = encode_rows(cb, case.B, case.HW, 0, z16=z16)
        for k in ("idx", "dist", "zq", "zraw"):
            assert same(out[k], ref[k]), f"{case.name} stride16={stride}: {k} differs"


def test_search_outputs_are_optional():
    case = next(c for c in R.SEARCH_CASES if (c.K, c.C, c.B, c.HW) == (100, 65, 3, 25))
    z, cb, ref = search_ref(case)
    for want in (("idx",), ("dist",), ("zq",), ("zraw",), ("idx", "zraw"), ()):
        out = encode_rows(cb, case.B, case.HW, 3, z32=z, want=want)
        assert all(same(out[k], ref[k]) for k in want)


def test_search_with_non_finite_rows():
    """A row of NaN and a row of +inf among ordinary rows: every score of both is NaN, nothing compares, and vq_finalize_kernel's clamp gives index 0
    (torch.argmin over the reference's expression gives 0 as well).  dist is sum_k (z_k - e_0k)^2 as it stands: NaN, and +inf for the +inf row."""
    z, cb, bad = R.nonfinite_case()
    idx, dist, zq, zraw = R.lookup_search(z, cb, 1, z.shape[0])
    assert idx[list(bad)].tolist() == [0, 0]
    for splits in (1, 0, 3):
        out = encode_rows(cb.to(DEV), 1, z.shape[0], splits, z32=z.to(DEV))
        assert same(out["idx"], idx) and same(out["dist"], dist.float()) and same(out["zq"], zq) and same(out["zraw"], zraw)


@pytest.mark.parametrize("C,K", R.ARGMIN_L2_ADDED + ((1000, 48),))
def test_normalised_search_is_the_argmin_entry_and_feeds_the_gather(C, K):
    """l2 = 1 is not exact arithmetic, so no restatement is compared here; but the three entries run the same launchers on the same prepared
    codebook: mb_vq_encode_rows gives mb_vq_argmin's bits, and mb_vq_gather of its indices stores the fp16 of its zq."""
    cb, rows = R.argmin_inputs(C, K, True)
    cb, z = cb.to(DEV), rows[255].to(DEV)
    out = encode_rows(cb, 5, 51, 0, z32=z, l2=1)
    idx, dist = sentinel_buffer(255, torch.int64), sentinel_buffer(255, torch.float32)
    assert lib().mb_vq_argmin(z.data_ptr(), cb.data_ptr(), 255, C, K, 1, 0, idx.data_ptr(), dist.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out["idx"], idx[:255]) and same(out["dist"], dist[:255]) and same(out["zraw"], z.reshape(5, 51, K).permute(0, 2, 1).contiguous())
    assert float((out["zq"].pow(2).sum(1) - 1).abs().max()) < 1e-5
    pad = R.cin_pad_of(K)
    got, sat = run_h16(lambda o, s: lib().mb_vq_gather(out["idx"].data_ptr(), cb.data_ptr(), 255, C, K, 1, pad, o, s, stream()), 255 * pad)
    got = got.reshape(5, 51, pad)
    assert same(got[..., :K].permute(0, 2, 1).contiguous(), out["zq"].half()) and sat == 0
    assert same(got[..., K:].contiguous(), torch.zeros(5, 51, pad - K, dtype=torch.float16))


# ------------------------------------------------------------------------------------------------------------------ gather / latent pack
def run_h16(call, n):
    """call(out pointer, sat pointer) -> (fp16 output [n], saturation count added to a counter that held 7)"""
    out = sentinel_buffer(n, torch.float16)
    sat = torch.full((9,), 7, dtype=torch.int32, device=DEV)
    rc = call(out.data_ptr(), sat.data_ptr())
    assert rc == 0, lib().mb_last_error()
    torch.cuda.synchronize()
    assert untouched(out, n) and sat[1:].tolist() == [7] * 8
    return out[:n], int(sat[0]) - 7


@pytest.mark.parametrize("K,C,npix", R.GATHER_CASES)
def test_gather(K, C, npix):
    codes, cb = R.gather_case(K, C, npix)
    pad = R.cin_pad_of(K)
    want, nsat = R.gather_latent(codes, cb, pad)
    cd, cbd = codes.to(DEV), cb.to(DEV)
    got, sat = run_h16(lambda o, s: lib().mb_vq_gather(cd.data_ptr(), cbd.data_ptr(), npix, C, K, 0, pad, o, s, stream()), npix * pad)
    assert same(got.reshape(npix, pad), want)
    assert sat == nsat
    assert float(got.float().abs().max()) == R.H16_MAX


@pytest.mark.parametrize("B,K,HW", R.PACK_LATENT_CASES)
def test_pack_latent(B, K, HW):
    z = R.pack_latent_case(B, K, HW)
    pad = R.cin_pad_of(K)
    want, nsat = R.pack_latent(z, pad)
    zd = z.to(DEV)
    got, sat = run_h16(lambda o, s: lib().mb_vq_pack_latent(zd.data_ptr(), B, K, HW, pad, o, s, stream()), B * HW * pad)
    assert same(got.reshape(B * HW, pad), want)
    assert sat == nsat


# ------------------------------------------------------------------------------------------------------------------ LFQ
def lfq_pack(z16, B, HW, K, want=("zq", "zraw")):
    N = B * HW
    idx = sentinel_buffer(N, torch.int64)
    buf = {k: sentinel_buffer(N * K, torch.float32) for k in want}
    rc = lib().mb_lfq_pack(z16.data_ptr(), B, HW, K, z16.shape[1], idx.data_ptr(), ptr(buf.get("zq")), ptr(buf.get("zraw")), stream())
    assert rc == 0, lib().mb_last_error()
    torch.cuda.synchronize()
    assert untouched(idx, N) and all(untouched(b, N * K) for b in buf.values())
    return idx[:N], {k: b[:N * K].reshape(B, K, HW) for k, b in buf.items()}


@pytest.mark.parametrize("K,Kp,B,HW", R.lfq_pack_cases())
def test_lfq_pack(K, Kp, B, HW):
    z = R.lfq_pack_case(K, Kp, B, HW)
    idx, zq, zraw = R.lfq_pack(z, B, HW, K)
    got, maps = lfq_pack(z.to(DEV), B, HW, K)
    assert torch.equal(got, idx.to(DEV)), f"{int((got.cpu() != idx).sum())} of {idx.numel()} codes differ"
    assert same(maps["zq"], zq) and same(maps["zraw"], zraw)
    if (B, HW) == (3, 25):
        got2, none = lfq_pack(z.to(DEV), B, HW, K, want=())
        assert torch.equal(got2, got) and not none


def lfq_latent(tokens, K):
    n = tokens.numel()
    out = sentinel_buffer(n * 64, torch.float16)
    rc = lib().mb_lfq_latent(tokens.data_ptr(), n, K, out.data_ptr(), stream())
    assert rc == 0, lib().mb_last_error()
    torch.cuda.synchronize()
    assert untouched(out, n * 64)
    return out[:n * 64].reshape(n, 64)


@pytest.mark.parametrize("K,n", [(K, 777) for K in R.LFQ_K] + [(12, R.LATENT_BIG)])
def test_lfq_latent_and_round_trip(K, n):
    t = R.lfq_tokens(K, n)
    lat = lfq_latent(t.to(DEV), K)
    assert same(lat, R.lfq_latent(t, K))
    back, _ = lfq_pack(lat, 1, t.numel(), K, want=())
    assert torch.equal(back, t.to(DEV))


# ------------------------------------------------------------------------------------------------------------------ image pack
@pytest.mark.parametrize("B,C,H,W", R.pack_image_cases())
def test_pack_image(B, C, H, W):
    img = R.pack_image_case(B, C, H, W)
    n = B * H * W * 64
    out = sentinel_buffer(n, torch.float16)
    imgd = img.to(DEV)
    rc = lib().mb_pack_image(imgd.data_ptr(), B, C, H, W, out.data_ptr(), stream())
    assert rc == 0, lib().mb_last_error()
    torch.cuda.synchronize()
    assert untouched(out, n)
    assert same(out[:n].reshape(-1, 64), R.pack_image(img))


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing():
    L, s = lib(), stream()
    f32, h16, i64 = (sentinel_buffer(4096, d) for d in (torch.float32, torch.float16, torch.int64))
    sat = torch.zeros(1, dtype=torch.int32, device=DEV)
    p32, p16, p64, ps = f32.data_ptr(), h16.data_ptr(), i64.data_ptr(), sat.data_ptr()

    def enc(z16=None, stride=0, z32=p32, cb=p32, B=1, HW=4, C=8, K=4, idx=p64):
        return L.mb_vq_encode_rows(z16, stride, z32, cb, B, HW, C, K, 0, 0, idx, None, None, None, s)
    refused = [enc(z32=None), enc(z16=p16, stride=4), enc(cb=None), enc(B=0), enc(B=-1), enc(HW=0), enc(C=1), enc(C=65537), enc(K=0), enc(K=257),
               enc(z16=p16, stride=3, z32=None), enc(B=1 << 15, HW=1 << 15)]

    def gat(codes=p64, cb=p32, npix=4, C=8, K=4, pad=64, out=p16, st=ps):
        return L.mb_vq_gather(codes, cb, npix, C, K, 0, pad, out, st, s)
    refused += [gat(codes=None), gat(cb=None), gat(out=None), gat(st=None), gat(npix=0), gat(npix=-3), gat(C=1), gat(C=65537), gat(K=0), gat(K=257),
                gat(K=65, pad=64), gat(pad=96), gat(pad=0)]

    def pak(z=p32, B=1, K=4, HW=4, pad=64, out=p16, st=ps):
        return L.mb_vq_pack_latent(z, B, K, HW, pad, out, st, s)
    refused += [pak(z=None), pak(out=None), pak(st=None), pak(B=0), pak(HW=0), pak(HW=-1), pak(K=0), pak(K=257), pak(K=65, pad=64), pak(pad=100)]

    def lfq(z=p16, B=1, HW=4, K=4, Kp=4, idx=p64):
        return L.mb_lfq_pack(z, B, HW, K, Kp, idx, None, None, s)
    refused += [lfq(z=None), lfq(idx=None), lfq(B=0), lfq(HW=0), lfq(K=0), lfq(K=65, Kp=68), lfq(K=8, Kp=4), lfq(K=4, Kp=3)]

    def lat(t=p64, npix=4, K=4, out=p16):
        return L.mb_lfq_latent(t, npix, K, out, s)
    refused += [lat(t=None), lat(out=None), lat(npix=0), lat(npix=-1), lat(K=0), lat(K=65)]

    def img(x=p32, B=1, C=3, H=2, W=2, out=p16):
        return L.mb_pack_image(x, B, C, H, W, out, s)
    refused += [img(x=None), img(out=None), img(B=0), img(C=0), img(C=5), img(H=0), img(W=0)]

    assert all(rc == -1 for rc in refused), refused
    assert b"mb_pack_image" in L.mb_last_error()
    torch.cuda.synchronize()
    assert untouched(f32) and untouched(h16) and untouched(i64) and int(sat) == 0
    # the same helpers with their defaults are accepted: the refusals above are about the argument that was changed
    f32[:64] = 1.0
    i64[:4] = 0
    assert [enc(), gat(), pak(), lfq(), lat(), img()] == [0] * 6
    torch.cuda.synchronize()
