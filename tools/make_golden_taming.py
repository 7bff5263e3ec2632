"""Golden fixtures of the Taming VQGAN tokenizer: the reference's OriginalVQModel (modeling/taming_vqgan.py) run on the CPU in fp32 on seeded
weights.  Needs the reference checkout (MASKBIT_REFERENCE, as oracle/make_golden.py); writes tensor-only .npz files to tests/golden/
(tok_taming_full, tok_taming_statedict).

Weights come from maskbit_amd.synth.make_taming_weights, the codebook from make_vq_codebook with per-channel mean / std measured on the latents
(after quant_conv) of the fixture's own images, as for tok_vq_full10.  The gain on the q / k weights is the smallest of GAINS at which, in this
fp32 run, every one of the seven AttnBlocks has a mean maximum attention probability inside [0.2, 0.9]: with the plain draw the softmax is
nearly uniform and the attention would not be tested end to end.  The fixture keeps the seeds and the gain (+ sha256 sentinels of a weight and
of the codebook): the tests regenerate the tensors.

    python tools/make_golden_taming.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as MG  # noqa: E402
from maskbit_amd.synth import make_taming_weights, make_vq_codebook  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SEED = 700
GAINS = (1.0, 1.25, 1.5, 1.75, 2.0, 2.25, 2.5, 3.0, 3.5, 4.0)
ATTN = ("encoder.down.4.attn.0", "encoder.down.4.attn.1", "encoder.mid.attn_1", "decoder.mid.attn_1",
        "decoder.up.4.attn.0", "decoder.up.4.attn.1", "decoder.up.4.attn.2")
HOOK_ROWS = (0, 37, 100, 255)                      # pixels of the 16 x 16 map whose AttnBlock outputs are kept
CROPS = ((0, 0), (120, 120), (240, 240), (37, 201))


def max_prob(block, x):
    """Mean over the queries of the largest attention probability of an AttnBlock on its input x (taming_autoencoder.py:149-163)."""
    h = block.norm(x)
    b, c = h.shape[:2]
    q = block.q(h).reshape(b, c, -1).permute(0, 2, 1)
    k = block.k(h).reshape(b, c, -1)
    w = torch.softmax(torch.bmm(q, k) * (int(c) ** (-0.5)), dim=2)
    return float(w.max(dim=2).values.mean())


def gaps(z, emb):
    """fp64 distances of every latent row to every entry: (gap between the best and the second best, ||z||^2 + max ||e||^2) per row."""
    zf = z.permute(0, 2, 3, 1).reshape(-1, z.shape[1]).double()
    e = emb.double()
    d = (zf[:, None, :] - e[None, :, :]).pow(2).sum(-1)
    top2 = d.topk(2, dim=1, largest=False).values
    return (top2[:, 1] - top2[:, 0]).float(), (zf.pow(2).sum(1) + e.pow(2).sum(1).max()).float()


def latent(model, x):
    return model.quant_conv(model.encoder(x * 2.0 - 1.0))


def run(OriginalVQModel, gain, x):
    sd = make_taming_weights(SEED, gain)
    model = OriginalVQModel(None)
    model.load_state_dict(sd, strict=True)
    model.eval().requires_grad_(False)
    z = latent(model, x)
    mean, std = z.mean((0, 2, 3)), z.std((0, 2, 3))
    cb = make_vq_codebook(1024, 256, SEED + 2, mean, std)
    model.quantize.embedding.weight.copy_(cb)
    probs, outs, hooks = {}, {}, []
    mods = dict(model.named_modules())

    def hook(name):
        def fn(m, inp, out):                        # (returns None: the output stays the module's)
            probs[name] = max_prob(m, inp[0])
            outs[name] = out
        return fn

    for name in ATTN:
        hooks.append(mods[name].register_forward_hook(hook(name)))
    zq, res = model.encode(x)
    idx = res["min_encoding_indices"]
    rec = model.decode_tokens(idx.reshape(x.shape[0], -1))
    for h in hooks:
        h.remove()
    return sd, model, cb, mean, std, z, zq, res, rec, [probs[n] for n in ATTN], outs


def main():
    MG._import_reference()
    from modeling.taming_vqgan import OriginalVQModel
    assert os.path.realpath(sys.modules["modeling.taming_vqgan"].__file__).startswith(os.path.realpath(MG.REF))
    torch.set_grad_enabled(False)
    x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(SEED + 1))
    for gain in GAINS:
        sd, model, cb, mean, std, z, zq, res, rec, probs, outs = run(OriginalVQModel, gain, x)
        print(f"gain {gain}: mean max attention probability per block " + " ".join(f"{p:.3f}" for p in probs))
        if all(0.2 <= p <= 0.9 for p in probs):
            break
    assert all(0.2 <= p <= 0.9 for p in probs), "no gain of GAINS puts every block's mean maximum probability inside [0.2, 0.9]"
    idx = res["min_encoding_indices"]
    gap, scale = gaps(z, cb)
    usage = torch.bincount(idx.flatten(), minlength=1024)
    print(f"codes used {int((usage > 0).sum())} / 1024, gap min {float(gap.min()):.3g} median {float(gap.median()):.3g}, "
          f"codebook loss {float(res['codebook_loss']):.4g}, recon range [{float(rec.min()):.3f}, {float(rec.max()):.3f}]")

    def rows(name):                                 # [2, 512, 16, 16] -> [2, len(HOOK_ROWS), 512]
        t = outs[name].permute(0, 2, 3, 1).reshape(2, 256, 512)
        return t[:, list(HOOK_ROWS)].numpy()

    crops = {f"crop_{y}_{xx}": rec[:, :, y:y + 16, xx:xx + 16].numpy() for (y, xx) in CROPS}
    np.savez_compressed(
        os.path.join(OUT, "tok_taming_full.npz"), seed=np.int64(SEED), qk_gain=np.float64(gain), w_sha_conv_in=MG.sha(sd["encoder.conv_in.weight"]),
        cb_sha=MG.sha(cb), cb_mean=mean.numpy(), cb_std=std.numpy(), z=z.numpy(), indices=idx.numpy(), gap=gap.numpy(), scale=scale.numpy(),
        codebook_loss=np.float32(res["codebook_loss"]), commitment_loss=np.float32(res["commitment_loss"]),
        quantizer_loss=np.float32(res["quantizer_loss"]), recon_half=rec[:, :, ::2, ::2].numpy().astype(np.float16),
        hook_rows=np.array(HOOK_ROWS, dtype=np.int64), attn_enc_first=rows(ATTN[0]), attn_dec_last=rows(ATTN[-1]),
        max_prob=np.array(probs, dtype=np.float64), **crops)
    items = list(OriginalVQModel(None).state_dict().items())
    np.savez_compressed(os.path.join(OUT, "tok_taming_statedict.npz"), names=np.array([k for k, _ in items]),
                        shapes=np.array([list(v.shape) + [-1] * (4 - v.dim()) for _, v in items], dtype=np.int64),
                        num_parameters=np.int64(sum(v.numel() for _, v in items)))
    for f in ("tok_taming_full", "tok_taming_statedict"):
        print(f, os.path.getsize(os.path.join(OUT, f + ".npz")))


if __name__ == "__main__":
    main()
