"""The fp32 reference mode's GEMM (maskbit_amd/csrc/gemm_f32.hip, mb_gemm_f32) per launch.  Its contract is exact: every output element is ONE
ascending-k fmaf chain, one bias add, the epilogue -- so integer data must come out exactly (any error is an indexing error), random data must equal
the CPU's correctly rounded fmaf chain bit for bit, and an output must not depend on where its row sits in M.  Only the GELU epilogue is compared
with a tolerance, against float64, with torch's own fp32 GELU on the same pre-activations as the yardstick."""
import ctypes
import ctypes.util
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE, BK = 128, 32                      # gemm_f32.hip: FB x FB output tiles, FBK-wide K-tiles
PLAIN, GELU, RES, LOGITS = 0, 1, 2, 3


def _ptr(t):
    return t.data_ptr() if t is not None else None


def gemm_f32(epi, A, W, bias, res=None, period=0, bias_per_pos=0, out=None):
    from maskbit_amd import _lib
    M, K = A.shape
    N = W.shape[0]
    rows = (M // period) * (period - 1) if epi == LOGITS else M
    if out is None:
        out = torch.full((rows, N), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().mb_gemm_f32(epi, _ptr(A), _ptr(W), _ptr(bias), _ptr(res), _ptr(out), M, N, K, period, bias_per_pos,
                                       torch.cuda.current_stream().cuda_stream), "mb_gemm_f32")
    return out


def _ints(gen, shape, lim):
    return torch.randint(-lim, lim + 1, shape, generator=gen)


EDGES = (1, TILE - 1, TILE + 1, 2 * TILE + 3)
KS = (4, BK - 4, BK, BK + 4, 3 * BK + 8)


@pytest.mark.parametrize("K", KS)
def test_integer_data_is_exact_at_every_tile_edge_plain_and_residual(K):
    """|A|, |W| <= 8, K <= 104: every partial sum is below 2^24, so fp32 holds each exactly, as it does the integer bias and residual."""
    gen = torch.Generator().manual_seed(100 + K)
    for M in EDGES:
        for N in EDGES:
            A, W = _ints(gen, (M, K), 8), _ints(gen, (N, K), 8)
            b, r = _ints(gen, (N,), 100), _ints(gen, (M, N), 100)
            want = A @ W.T + b                                                   # int64
            Ad, Wd, bd, rd = A.float().to(DEV), W.float().to(DEV), b.float().to(DEV), r.float().to(DEV)
            got = gemm_f32(PLAIN, Ad, Wd, bd)
            assert torch.equal(got.cpu().long(), want) and torch.equal(got.cpu(), want.float()), (M, N, K, "plain")
            got = gemm_f32(RES, Ad, Wd, bd, rd)
            assert torch.equal(got.cpu(), (want + r).float()), (M, N, K, "residual")
            rd2 = rd.clone()                                                     # in place: out aliases residual
            gemm_f32(RES, Ad, Wd, bd, rd2, out=rd2)
            assert torch.equal(rd2.cpu(), (want + r).float()), (M, N, K, "residual in place")


@pytest.mark.parametrize("period,Ms", [(5, (5, 125, 130, 260)), (257, (257, 514))])
@pytest.mark.parametrize("bias_per_pos", [0, 1])
def test_integer_data_is_exact_logits_epilogue(period, Ms, bias_per_pos):
    """Rows with m % period == period - 1 are dropped and the rest compacted; the bias is [N] or one row per position.  M is a whole number of periods
    (the epilogue's own condition), chosen on both sides of the 128-row tile edges."""
    gen = torch.Generator().manual_seed(7 * period + bias_per_pos)
    for M in Ms:
        for N in EDGES:
            for K in (4, BK + 4, 3 * BK + 8):
                A, W = _ints(gen, (M, K), 8), _ints(gen, (N, K), 8)
                b = _ints(gen, (period - 1, N) if bias_per_pos else (N,), 100)
                full = (A @ W.T).reshape(M // period, period, N)[:, : period - 1]
                want = (full + b).reshape(-1, N)
                got = gemm_f32(LOGITS, A.float().to(DEV), W.float().to(DEV), b.float().to(DEV), period=period, bias_per_pos=bias_per_pos)
                assert got.shape == want.shape and torch.equal(got.cpu(), want.float()), (M, N, K)


def _fmaf():
    """A correctly rounded single-precision fma on the CPU: libm's fmaf through ctypes (one rounding, in fp32).  math.fma works on doubles -- rounding its
    result to fp32 is a second rounding -- and serves only where libm cannot be loaded."""
    name = ctypes.util.find_library("m")
    if name:
        f = ctypes.CDLL(name).fmaf
        f.restype = ctypes.c_float
        f.argtypes = [ctypes.c_float] * 3
        return f
    return lambda a, b, c: float(np.float32(math.fma(a, b, c)))


def _chain(A, W, bias):
    """out[m, n] = fp32(chain(m, n) + bias[n]) with chain = the ascending-k fmaf chain from 0."""
    fmaf = _fmaf()
    A, W = A.tolist(), W.tolist()                                                # (fp32 values as Python floats: exact)
    out = np.empty((len(A), len(W)), dtype=np.float32)
    for m, ar in enumerate(A):
        for n, wr in enumerate(W):
            acc = 0.0
            for a, w in zip(ar, wr):
                acc = fmaf(a, w, acc)
            out[m, n] = acc
    return torch.from_numpy(out) + bias


@pytest.mark.parametrize("M,N,K", [(33, 40, 68), (3, 5, 4096)])
def test_random_data_equals_the_cpu_fmaf_chain_bit_for_bit(M, N, K):
    gen = torch.Generator().manual_seed(K)
    A, W, b = torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen), torch.randn(N, generator=gen)
    want = _chain(A, W, b)
    got = gemm_f32(PLAIN, A.to(DEV), W.to(DEV), b.to(DEV)).cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"{int((got != want).sum())} of {M * N} elements differ"
    # and it is NOT what a blocked sum gives: the test can tell the orders apart
    assert not torch.equal(want, (A.double() @ W.double().T + b).float())


def test_gelu_epilogue_against_float64():
    """gelu_erf(v) with an accurate erff against float64 on the SAME pre-activations v (the plain epilogue's bits).  Yardstick: the max abs error of
    torch's own fp32 F.gelu on the CPU over those v; the kernel's erff is another implementation of the same function: at most 2 x that.
    Measured (MI355X): kernel 4.5e-07, torch fp32 1.1e-06."""
    gen = torch.Generator().manual_seed(9)
    M, N, K = 200, 300, 64
    A, W, b = torch.randn(M, K, generator=gen) * 0.35, torch.randn(N, K, generator=gen), torch.randn(N, generator=gen) * 0.5
    Ad, Wd, bd = A.to(DEV), W.to(DEV), b.to(DEV)
    v = gemm_f32(PLAIN, Ad, Wd, bd).cpu()
    got = gemm_f32(GELU, Ad, Wd, bd).cpu()
    assert float(v.abs().max()) > 6.0 and float(v.abs().min()) < 1e-3             # the pre-activations cover both tails and the origin
    exact = torch.nn.functional.gelu(v.double())
    e_kernel = float((got.double() - exact).abs().max())
    e_torch = float((torch.nn.functional.gelu(v).double() - exact).abs().max())
    print(f"GELU epilogue max abs error against float64: kernel {e_kernel:.3e}, torch fp32 CPU {e_torch:.3e}")
    assert e_kernel <= 2.0 * e_torch


def test_rows_do_not_depend_on_their_place_in_m_and_runs_repeat():
    gen = torch.Generator().manual_seed(21)
    K, N = 200, 150
    A, W, b = torch.randn(300, K, generator=gen).to(DEV), torch.randn(N, K, generator=gen).to(DEV), torch.randn(N, generator=gen).to(DEV)
    big = gemm_f32(PLAIN, A, W, b)
    assert torch.equal(big, gemm_f32(PLAIN, A, W, b))                              # deterministic
    for lo, hi in ((137, 170), (0, 1), (299, 300), (120, 260)):
        assert torch.equal(gemm_f32(PLAIN, A[lo:hi].contiguous(), W, b), big[lo:hi]), (lo, hi)
    sub = gemm_f32(PLAIN, A, W[17:140].contiguous(), b[17:140].contiguous())       # ... nor on the column's place in N
    assert torch.equal(sub, big[:, 17:140])


def test_shapes_outside_the_contract_are_refused_with_a_message():
    A, W, b = torch.zeros(4, 8, device=DEV), torch.zeros(4, 8, device=DEV), torch.zeros(4, device=DEV)
    from maskbit_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    out = torch.zeros(4, 4, device=DEV)
    for (M, N, K) in ((4, 4, 6), (4, 4, 0), (0, 4, 8), (4, 0, 8)):
        assert lib.mb_gemm_f32(PLAIN, A.data_ptr(), W.data_ptr(), b.data_ptr(), None, out.data_ptr(), M, N, K, 0, 0, st) == -3
        assert b"K % 4 == 0" in lib.mb_last_error()
    assert lib.mb_gemm_f32(LOGITS, A.data_ptr(), W.data_ptr(), b.data_ptr(), None, out.data_ptr(), 4, 4, 8, 3, 0, st) == -3      # M % period
    assert lib.mb_gemm_f32(RES, A.data_ptr(), W.data_ptr(), b.data_ptr(), None, out.data_ptr(), 4, 4, 8, 0, 0, st) == -1          # no residual
