"""The fp32 reference mode's attention (maskbit_amd/csrc/gemm_f32.hip, mb_attention_f32) per launch: fp32 qkv [nb, N, 3d] -> fp32 out [nb, N, d],
softmax(Q K^T / sqrt(dh)) V per (sequence, head), keys streamed in tiles of 16 with a running max and sum.
Exact case: one key per query leads by >= 120 after scaling, so every other exp underflows to 0 in fp32 and the output IS that key's V row, bit for
bit, wherever the key sits.  Random case: against float64, with torch's fp32 CPU evaluation of the same formula as the yardstick."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEY_TILE = 16                           # gemm_f32.hip AKT


def attention_f32(qkv, heads):
    from maskbit_amd import _lib
    nb, N, d3 = qkv.shape
    out = torch.full((nb, N, d3 // 3), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().mb_attention_f32(qkv.data_ptr(), out.data_ptr(), nb, N, d3 // 3, heads, torch.cuda.current_stream().cuda_stream),
               "mb_attention_f32")
    return out


def attention_torch(qkv, heads):
    """nn.MultiheadAttention's arithmetic (the oracle's attention, oracle/maskbit_oracle.py) in qkv's own dtype."""
    nb, N, d3 = qkv.shape
    d = d3 // 3
    dh = d // heads
    q, k, v = (t.reshape(nb, N, heads, dh).transpose(1, 2) for t in qkv.split(d, dim=-1))
    w = torch.softmax((q * (1.0 / math.sqrt(dh))) @ k.transpose(-1, -2), dim=-1)
    return (w @ v).transpose(1, 2).reshape(nb, N, d)


def _winner_case(N, dh, nb, heads, seed):
    """qkv whose query i of every (sequence, head) has ONE key w[i] leading every other key's scaled score by >= 125 (checked here in float64 on the
    fp32 values): keys are distinct unit vectors u_j, query i is c u_w[i], so the lead is c (1 - max cosine) / sqrt(dh)."""
    gen = torch.Generator().manual_seed(seed)
    d = heads * dh
    cands = sorted({j for j in (0, N - 1, KEY_TILE - 1, KEY_TILE, KEY_TILE + 1, 4 * KEY_TILE, N // 2) if 0 <= j < N})   # first, last, both sides of a key-tile boundary
    w = torch.tensor([cands[i % len(cands)] for i in range(N)])
    qkv = torch.empty(nb, N, 3 * d, dtype=torch.float64)
    for b in range(nb):
        for h in range(heads):
            u = torch.randn(N, dh, generator=gen, dtype=torch.float64)
            u = u / u.norm(dim=1, keepdim=True)
            cos = u @ u.T
            cos.fill_diagonal_(-1.0)
            rho = float(cos.max()) if N > 1 else 0.0
            c = 140.0 * math.sqrt(dh) / (1.0 - rho)
            sl = slice(h * dh, (h + 1) * dh)
            qkv[b, :, sl] = c * u[w]
            qkv[b, :, d + h * dh: d + (h + 1) * dh] = u
            qkv[b, :, 2 * d + h * dh: 2 * d + (h + 1) * dh] = torch.randn(N, dh, generator=gen, dtype=torch.float64)
    qkv = qkv.float()
    # the lead, on the values the kernel reads
    q, k, _ = (t.double().reshape(nb, N, heads, dh).transpose(1, 2) for t in qkv.split(d, dim=-1))
    s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)                               # [nb, heads, N, N]
    win = s.gather(-1, w.view(1, 1, N, 1).expand(nb, heads, N, 1))
    others = s.scatter(-1, w.view(1, 1, N, 1).expand(nb, heads, N, 1), float("-inf"))
    lead = float((win.squeeze(-1) - others.max(-1).values).min()) if N > 1 else float("inf")
    assert lead >= 125.0, lead
    return qkv, w


@pytest.mark.parametrize("dh", [32, 64])
@pytest.mark.parametrize("N", [1, 2, 17, 257, 1025])
def test_one_dominant_key_gives_its_value_row_bit_for_bit(N, dh):
    nb, heads = 2, 2
    qkv, w = _winner_case(N, dh, nb, heads, seed=N * 100 + dh)
    got = attention_f32(qkv.to(DEV), heads).cpu()
    want = qkv[:, :, 2 * heads * dh:][:, w]                                     # V rows of the winners, every head's slice at once
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"{int((got != want).sum())} elements differ"


@pytest.mark.parametrize("N,dh", [(257, 64), (100, 32), (1025, 64)])
def test_random_data_against_float64(N, dh):
    """Yardstick: torch's fp32 CPU evaluation of the same attention against float64.  The kernel rescales a streamed running sum, so it may be at
    most 4 x that max abs error.  Measured (MI355X), kernel / yardstick: N = 257, dh 64: 2.1e-06 / 2.2e-06; N = 100, dh 32: 1.2e-06 / 1.2e-06; N = 1025, dh 64: 4.4e-06 / 2.2e-06."""
    nb, heads = 2, 2
    gen = torch.Generator().manual_seed(N + dh)
    qkv = torch.randn(nb, N, 3 * heads * dh, generator=gen)
    qkv[..., : heads * dh] *= 2.0                                                # sharper rows than unit-variance scores give
    exact = attention_torch(qkv.double(), heads)
    e_torch = float((attention_torch(qkv, heads).double() - exact).abs().max())
    got = attention_f32(qkv.to(DEV), heads).cpu()
    e_kernel = float((got.double() - exact).abs().max())
    print(f"attention N={N} dh={dh}: max abs error against float64: kernel {e_kernel:.3e}, torch fp32 CPU {e_torch:.3e}, ratio {e_kernel / e_torch:.2f}")
    assert e_kernel <= 4.0 * e_torch


def test_batch_invariance_bit_for_bit():
    heads, dh, N = 4, 32, 77
    gen = torch.Generator().manual_seed(3)
    qkv = torch.randn(6, N, 3 * heads * dh, generator=gen).to(DEV)
    full = attention_f32(qkv, heads)
    assert torch.equal(full, attention_f32(qkv, heads))
    for b in (0, 3, 5):
        assert torch.equal(attention_f32(qkv[b:b + 1].contiguous(), heads)[0], full[b]), b
    assert torch.equal(attention_f32(qkv[2:5].contiguous(), heads), full[2:5])


def test_head_widths_other_than_32_and_64_are_refused():
    from maskbit_amd import _lib
    lib = _lib.load()
    qkv, out = torch.zeros(1, 4, 3 * 48, device=DEV), torch.zeros(1, 4, 48, device=DEV)
    assert lib.mb_attention_f32(qkv.data_ptr(), out.data_ptr(), 1, 4, 48, 1, torch.cuda.current_stream().cuda_stream) == -3
    assert b"32 or 64" in lib.mb_last_error()
