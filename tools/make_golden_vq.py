"""Golden fixtures of the lookup (VQ) tokenizer: the reference's ConvVQModel with quantizer_type="lookup" (SimpleVectorizer), run on the CPU
in fp32 on seeded weights.  Needs the reference checkout (MASKBIT_REFERENCE, as oracle/make_golden.py); writes tensor-only .npz files to
tests/golden/ (tok_vq_tiny, tok_vq_legacy256_tiny, tok_vq_full12, tok_vq_full10, tok_vq_statedicts).

Conv weights come from maskbit_amd.synth.make_tokenizer_weights, the codebook from make_vq_codebook with per-channel mean / std measured on
the encoder's latents of the fixture's own images (so that the argmin is not trivial; the reference's uniform(+-1/C) init would collapse it).
Full-size fixtures keep only the seeds (+ sha256 sentinels of a weight and of the codebook): the tests regenerate the tensors.

    python tools/make_golden_vq.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as MG  # noqa: E402
from oracle import maskbit_oracle as O  # noqa: E402
from maskbit_amd.synth import make_vq_codebook  # noqa: E402
from maskbit_amd.conv_vqgan import legacy_to_canonical  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")

# the three shipped lookup tokenizers (configs/tokenizer/vqgan_plus_{10,12}bit.yaml, configs/external/maskgit_tokenizer.yaml)
SHIPPED = {
    "vqgan_plus_10bit": (dict(codebook_size=1024, token_size=256, sample_with_conv=True), False),
    "vqgan_plus_12bit": (dict(codebook_size=4096, token_size=64, sample_with_conv=True), False),
    "maskgit": (dict(codebook_size=1024, token_size=256, sample_with_conv=False, entropy_loss_weight=0.02), True),
}


def vq_config(cfg: O.TokCfg, C: int, l2: bool = False, **over) -> MG.Cfg:
    c = dict(MG.tok_config(cfg))
    c.update(quantizer_type="lookup", codebook_size=C, entropy_loss_weight=0.0, use_l2_normalisation=l2)
    c.update(over)
    return MG.Cfg(c)


def shipped_config(over) -> MG.Cfg:
    c = vq_config(O.TokCfg(token_size=over["token_size"]), over["codebook_size"])
    c.update(over)
    return c


def ref_model(ConvVQModel, config, sd, legacy=False):
    m = ConvVQModel(config, legacy=legacy)
    m.load_state_dict(sd, strict=True)
    return m.eval().requires_grad_(False)


def to_legacy(sd, R):
    return legacy_to_canonical(sd, R)               # the level map is its own inverse


def latent_stats(model, x):
    with torch.no_grad():
        z = model.encoder(x)
    return z.mean((0, 2, 3)), z.std((0, 2, 3))


def gaps(z: torch.Tensor, emb: torch.Tensor, l2: bool):
    """fp64 distances of every latent row to every entry: (gap between the best and the second best, ||z||^2 + max ||e||^2) per row."""
    zf = z.permute(0, 2, 3, 1).reshape(-1, z.shape[1]).double()
    e = emb.double()
    if l2:
        zf = torch.nn.functional.normalize(zf, dim=-1)
        e = torch.nn.functional.normalize(e, dim=-1)
    d = (zf[:, None, :] - e[None, :, :]).pow(2).sum(-1)
    top2 = d.topk(2, dim=1, largest=False).values
    return (top2[:, 1] - top2[:, 0]).float(), (zf.pow(2).sum(1) + e.pow(2).sum(1).max()).float()


def run(model, x, l2):
    with torch.no_grad():
        z = model.encoder(x)
        zq, res = model.encode(x)
        rec = model.decode_tokens(res["min_encoding_indices"].reshape(x.shape[0], -1))
    gap, scale = gaps(z, model.quantize.embedding.weight, l2)
    idx = res["min_encoding_indices"]
    usage = torch.bincount(idx.flatten(), minlength=model.quantize.embedding.weight.shape[0])
    out = dict(z=z.numpy(), indices=idx.numpy(), gap=gap.numpy(), scale=scale.numpy(), codes_used=np.int64(int((usage > 0).sum())),
               codebook_loss=np.float32(res["codebook_loss"]), commitment_loss=np.float32(res["commitment_loss"]),
               quantizer_loss=np.float32(res["quantizer_loss"]))
    print(f"  codes used {int((usage > 0).sum())} / {usage.numel()}, gap min {float(gap.min()):.3g} median {float(gap.median()):.3g}, "
          f"codebook loss {float(res['codebook_loss']):.4g}")
    return out, rec


def main():
    _, ConvVQModel, *_ = MG._import_reference()
    torch.set_grad_enabled(False)

    # ---- tiny, K = 64, C = 512, with and without L2 normalisation
    cfg = O.TokCfg(token_size=64, hidden_channels=64, channel_mult=(1, 1, 2), num_resolutions=3, num_res_blocks=1)
    sd = O.make_tokenizer_weights(cfg, seed=31, with_encoder=True, lfq_buffers=False)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(32))
    probe = ref_model(ConvVQModel, vq_config(cfg, 512), {**sd, "quantize.embedding.weight": torch.zeros(512, 64)})
    mean, std = latent_stats(probe, x)
    cb = make_vq_codebook(512, 64, 33, mean, std)
    out = dict(seed=np.int64(31), image=x.numpy(), codebook=cb.numpy(), w_sha_conv_in=MG.sha(sd["decoder.conv_in.weight"]))
    for l2 in (False, True):
        print(f"tok_vq_tiny l2={l2}")
        m = ref_model(ConvVQModel, vq_config(cfg, 512, l2), {**sd, "quantize.embedding.weight": cb})
        r, rec = run(m, x, l2)
        tag = "l2_" if l2 else ""
        out.update({tag + k: v for k, v in r.items()})
        out[tag + "recon"] = rec.numpy()
    np.savez_compressed(os.path.join(OUT, "tok_vq_tiny.npz"), **out)

    # ---- tiny legacy layout, K = 256, C = 128, average-pool encoder (the MaskGIT tokenizer's shape)
    cfg = O.TokCfg(token_size=256, hidden_channels=64, channel_mult=(1, 1, 2), num_resolutions=3, num_res_blocks=1, sample_with_conv=False)
    sd = O.make_tokenizer_weights(cfg, seed=41, with_encoder=True, lfq_buffers=False)
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(42))
    conf = vq_config(cfg, 128)
    probe = ref_model(ConvVQModel, conf, {**sd, "quantize.embedding.weight": torch.zeros(128, 256)})
    mean, std = latent_stats(probe, x)
    cb = make_vq_codebook(128, 256, 43, mean, std)
    print("tok_vq_legacy256_tiny")
    m = ref_model(ConvVQModel, conf, to_legacy({**sd, "quantize.embedding.weight": cb}, cfg.num_resolutions), legacy=True)
    r, rec = run(m, x, False)
    np.savez_compressed(os.path.join(OUT, "tok_vq_legacy256_tiny.npz"), seed=np.int64(41), image=x.numpy(), codebook=cb.numpy(), recon=rec.numpy(),
                        w_sha_conv_in=MG.sha(sd["decoder.conv_in.weight"]), **r)

    # ---- full-size shapes of the shipped VQGAN+ tokenizers on one 256 x 256 image (weights / codebook regenerated from the seeds)
    for name, (over, _), seed in (("tok_vq_full12", SHIPPED["vqgan_plus_12bit"], 500), ("tok_vq_full10", SHIPPED["vqgan_plus_10bit"], 600)):
        C, K = over["codebook_size"], over["token_size"]
        cfg = O.TokCfg(token_size=K)
        sd = O.make_tokenizer_weights(cfg, seed=seed, with_encoder=True, lfq_buffers=False)
        x = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(seed + 1))
        conf = shipped_config(over)
        probe = ref_model(ConvVQModel, conf, {**sd, "quantize.embedding.weight": torch.zeros(C, K)})
        mean, std = latent_stats(probe, x)
        cb = make_vq_codebook(C, K, seed + 2, mean, std)
        print(name)
        m = ref_model(ConvVQModel, conf, {**sd, "quantize.embedding.weight": cb})
        r, rec = run(m, x, False)
        crops = {f"crop_{y}_{xx}": rec[:, :, y:y + 16, xx:xx + 16].numpy() for (y, xx) in ((0, 0), (120, 120), (240, 240), (37, 201))}
        np.savez_compressed(os.path.join(OUT, name + ".npz"), seed=np.int64(seed), cb_mean=mean.numpy(), cb_std=std.numpy(),
                            recon_half=rec[:, :, ::2, ::2].numpy().astype(np.float16), w_sha_conv_in=MG.sha(sd["encoder.conv_in.weight"]),
                            cb_sha=MG.sha(cb), **crops, **r)

    # ---- state-dict names and shapes of the three shipped configs
    sdl = {}
    for name, (over, legacy) in SHIPPED.items():
        m = ConvVQModel(shipped_config(over), legacy=legacy)
        items = list(m.state_dict().items())
        sdl[name + "_names"] = np.array([k for k, _ in items])
        sdl[name + "_shapes"] = np.array([list(v.shape) + [-1] * (4 - v.dim()) for _, v in items], dtype=np.int64)
    np.savez_compressed(os.path.join(OUT, "tok_vq_statedicts.npz"), **sdl)
    for f in ("tok_vq_tiny", "tok_vq_legacy256_tiny", "tok_vq_full12", "tok_vq_full10", "tok_vq_statedicts"):
        print(f, os.path.getsize(os.path.join(OUT, f + ".npz")))


if __name__ == "__main__":
    main()
