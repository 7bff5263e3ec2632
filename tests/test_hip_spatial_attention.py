"""GPU checks of the spatial self-attention kernel (csrc/spatial_attention.hip) per launch, through the diagnostic entry mb_spatial_attention:
against float64 on the fp16-rounded inputs, exact cases at every length, batch invariance and run-to-run determinism.

Bound of the comparison, derived: the output row is a convex combination of the rows of v, so every error term scales with max |v|.  The
probabilities are rounded to fp16 for the P V product (relative 2^-11 each, so at most 2^-11 max|v| on the combination), the row sum that
normalises them is the fp32 sum of the unrounded probabilities (the rounded ones sum to it within 2^-11: another 2^-11 max|v|), the output is
rounded to fp16 once (2^-11 max|v|), and the fp32 accumulation of scores (512 terms) and of P V (up to 1 024 terms) with the exp of a score
that is itself off by a few fp32 ulp stays below the remaining 2^-11: |out - ref| <= 4 * 2^-11 = 2^-9 max|v| per element.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = 512
SHAPES = [(16, 1), (16, 3), (48, 1), (48, 3), (256, 1), (256, 3), (1024, 1)]          # (N, B)
GUARD = 64                                                                              # guard rows behind the output, checked untouched


def run(q, k, v, packed=True):
    """q, k, v fp16 [B, N, 512] on the device -> out fp16 [B, N, 512]; packed: as slices of one [B N, 1536] buffer (the engine's layout)."""
    from maskbit_amd import _lib
    B, N, _ = q.shape
    if packed:
        qkv = torch.cat([q, k, v], dim=2).contiguous()
        qp, kp, vp, ld = qkv.data_ptr(), qkv.data_ptr() + 2 * C, qkv.data_ptr() + 4 * C, 3 * C
    else:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        qp, kp, vp, ld = q.data_ptr(), k.data_ptr(), v.data_ptr(), C
    out = torch.full((B * N + GUARD, C), -7.0, dtype=torch.float16, device=DEV)
    sat = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().mb_spatial_attention(qp, kp, vp, out.data_ptr(), sat.data_ptr(), B, N, ld, C, torch.cuda.current_stream().cuda_stream),
               "mb_spatial_attention")
    assert bool((out[B * N:] == -7.0).all()) and int(sat) == 0
    return out[:B * N].reshape(B, N, C)


def ref64(q, k, v):
    w = torch.softmax(torch.bmm(q.double(), k.double().transpose(1, 2)) * C ** -0.5, dim=2)
    return torch.bmm(w, v.double()), w


def inputs(N, B, seed, target):
    """Random fp16 q, k, v with q scaled (bisection on the float64 softmax of the inputs themselves) so that the mean maximum probability is
    about `target`."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = torch.randn(B, N, C, device=DEV, generator=g)
    k = torch.randn(B, N, C, device=DEV, generator=g)
    v = (torch.randn(B, N, C, device=DEV, generator=g) * 1.5).half()
    k = k.half()
    lo, hi = 1e-3, 64.0
    for _ in range(16):
        f = (lo * hi) ** 0.5
        mp = float(ref64((q * f).half(), k, v)[1].max(dim=2).values.mean())
        lo, hi = (f, hi) if mp < target else (lo, f)
    return (q * lo).half(), k, v


def check(q, k, v, packed=True):
    out = run(q, k, v, packed)
    ref, w = ref64(q, k, v)
    err = float((out.double() - ref).abs().max())
    bound = 2.0 ** -9 * float(v.float().abs().max())
    mp = float(w.max(dim=2).values.mean())
    print(f"N {q.shape[1]} B {q.shape[0]}: mean max probability {mp:.3f}, max |out - ref| {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    return mp


@pytest.mark.parametrize("N,B", SHAPES)
def test_against_fp64(N, B):
    mp = check(*inputs(N, B, 10 + N + B, 0.5), packed=B == 1)
    assert 0.3 < mp < 0.7


@pytest.mark.parametrize("N,B", [(48, 3), (256, 1), (1024, 1)])
def test_near_uniform_and_near_one_hot(N, B):
    assert check(*inputs(N, B, 77 + N, 1.5 / N)) < 3.0 / N
    assert check(*inputs(N, B, 78 + N, 0.97)) > 0.9


@pytest.mark.parametrize("N,B", SHAPES)
def test_exact_mean(N, B):
    """k = 0: every score is 0, every probability exactly 1, the row sum N.  N a power of two: v holds small integers, the output is the exact
    column mean (an integer multiple of 1 / N below 2^11: exact in fp16).  N = 48: every key carries the same row of v, which is the output."""
    g = torch.Generator(device=DEV).manual_seed(N + B)
    q = torch.randn(B, N, C, device=DEV, generator=g).half()
    k = torch.zeros(B, N, C, device=DEV, dtype=torch.float16)
    if N & (N - 1) == 0:
        v = torch.randint(-8, 9, (B, N, C), device=DEV, generator=g).half()
        want = v.double().mean(dim=1, keepdim=True).expand(B, N, C)
    else:
        v = torch.randint(-8, 9, (B, 1, C), device=DEV, generator=g).half().expand(B, N, C).contiguous()
        want = v.double()
    out = run(q, k, v)
    assert torch.equal(out.double(), want)
    assert torch.equal(want.half().double(), want)                      # (the expectation itself is an fp16 number)


@pytest.mark.parametrize("N,B", SHAPES)
def test_dominant_key_returns_its_value_row(N, B):
    """Key j carries 32 in channels j % 32 and 32 + j // 32, query i carries 32 in the two channels of its target key pi(i): the target scores
    2 * 1024, every other key at most 1024, i.e. at least 1024 * 512^-0.5 = 45.3 below in the exponent.  exp(-45.3) rounds to 0 in fp16 and
    N of them vanish against 1 in the fp32 row sum: the output is v[pi(i)] bit for bit."""
    g = torch.Generator(device=DEV).manual_seed(3 * N + B)
    j = torch.arange(N, device=DEV)
    k = torch.zeros(B, N, C, device=DEV, dtype=torch.float16)
    k[:, j, j % 32] = 32.0
    k[:, j, 32 + j // 32] = 32.0
    pi = torch.stack([torch.randperm(N, device=DEV, generator=g) for _ in range(B)])
    q = torch.gather(k, 1, pi[:, :, None].expand(B, N, C))
    v = torch.randn(B, N, C, device=DEV, generator=g).half()
    out = run(q, k, v, packed=N != 256)
    assert torch.equal(out, torch.gather(v, 1, pi[:, :, None].expand(B, N, C)))


@pytest.mark.parametrize("N", [16, 48, 256])
def test_batch_invariance_and_determinism(N):
    q, k, v = inputs(N, 3, 5 + N, 0.5)
    out3 = run(q, k, v)
    assert torch.equal(run(q[1:2], k[1:2], v[1:2]), out3[1:2])         # image 1 of the batch of 3, run alone
    assert torch.equal(run(q, k, v), out3)                              # run to run
    assert torch.equal(run(q, k, v, packed=False), out3)                # the layout of the inputs does not matter


def test_determinism_1024():
    q, k, v = inputs(1024, 1, 9, 0.5)
    assert torch.equal(run(q, k, v), run(q, k, v))


def test_refusals():
    from maskbit_amd import _lib
    lib = _lib.load()
    x = torch.zeros(1024 + 16, 3 * C, dtype=torch.float16, device=DEV)
    out = torch.zeros(1024 + 16, C, dtype=torch.float16, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    for (B, N, ld, ldo) in ((1, 24, 3 * C, C), (1, 0, 3 * C, C), (1, 1040, 3 * C, C), (0, 16, 3 * C, C), (1, 16, 256, C), (1, 16, 3 * C + 4, C),
                            (1, 16, 3 * C, C - 4), (1, 16, 3 * C, C + 2)):
        assert lib.mb_spatial_attention(x.data_ptr(), x.data_ptr() + 2 * C, x.data_ptr() + 4 * C, out.data_ptr(), None, B, N, ld, ldo, s) == -1
    assert lib.mb_spatial_attention(None, x.data_ptr(), x.data_ptr(), out.data_ptr(), None, 1, 16, 3 * C, C, s) == -1
    torch.cuda.synchronize()
    assert bool((out == 0).all())
