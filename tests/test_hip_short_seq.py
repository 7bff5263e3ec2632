"""128 x 128 models: 8 x 8 = 64 image tokens + the class token.  N = 65 is shorter than the 256 keys up to which the one-block attention kernel leaves
its staged copies of key N - 1 unmasked, so attention runs the streaming kernel (one 128-key block, every key >= N masked); everything else is the same
code at a smaller N.  The launches themselves are tested in tests/test_hip_attention_exact.py."""
import pytest
import torch

from oracle import maskbit_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("heads", [4, 2])
def test_generator_65_tokens_vs_oracle(heads):
    """head widths 32 and 64: the plain forward against the float64 oracle (the bound of the 1025-token test), batch invariance"""
    from maskbit_amd import LFQBert
    cfg = O.GenCfg(bits=12, splits=2, hidden=128, depth=1, heads=heads, mlp=256, seq=64, nclass=10)
    sd = O.make_generator_weights(cfg, seed=128 + heads, head_gain=12.0)
    m = LFQBert(img_size=128, hidden_dim=cfg.hidden, codebook_size=2 ** cfg.bits, codebook_splits=cfg.splits, depth=cfg.depth, heads=cfg.heads,
                mlp_dim=cfg.mlp, dropout=0.1, nclass=cfg.nclass, input_stride=16)
    assert m.seq_len == 64
    m.load_state_dict(sd, strict=True)
    m = m.eval().requires_grad_(False).to(DEV)
    b = 3
    g = torch.Generator().manual_seed(b)
    toks = torch.randint(0, 65, (b, 64, 2), generator=g); y = torch.randint(0, 10, (b,), generator=g)
    drop = torch.tensor([False, True, False])
    out = m(toks.to(DEV), y.to(DEV), drop.to(DEV))
    ref = O.lfq_bert_forward(sd, cfg, toks, y, drop)
    rel = float((out.cpu() - ref).norm() / ref.norm())
    print(f"65 tokens, heads {heads}: rel-Frobenius logit error {rel:.2e}")
    assert out.shape == (b, 64, 2, 64) and torch.isfinite(out).all() and rel < 2e-3
    assert torch.equal(m(toks[1:2].to(DEV), y[1:2].to(DEV), drop[1:2].to(DEV)), out[1:2])      # batch invariance
