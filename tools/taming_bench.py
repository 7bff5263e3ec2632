"""Timing of the Taming VQGAN tokenizer (OriginalVQModel) next to the VQGAN+ 10-bit lookup tokenizer in the same process: encode and
decode_tokens of 64 images at 256 x 256, with device events around the calls (profiler off) and then with the library's own event timing
(mb_prof: the encode / decode entries, the seven AttnBlocks and the attention launches inside them), and the attention kernel alone
(mb_spatial_attention) at B = 64 for N = 256 and N = 1024.  Random seeded weights (maskbit_amd.synth).

    python tools/taming_bench.py [--reps 10] [--batch 64]

Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from maskbit_amd import OriginalVQModel, _lib  # noqa: E402
from maskbit_amd.synth import make_taming_weights, make_vq_codebook  # noqa: E402
from vq_bench import timed, tokenizer  # noqa: E402


def taming(dev):
    sd = make_taming_weights(7, 2.0)
    sd["quantize.embedding.weight"] = make_vq_codebook(1024, 256, 8, torch.zeros(256), torch.ones(256))
    m = OriginalVQModel(None)
    m.load_state_dict(sd, strict=True)
    return m.eval().requires_grad_(False).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B = args.batch
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, 3, 256, 256, generator=g).to(dev)
    codes = torch.randint(0, 1024, (B, 256), generator=g).to(dev)
    models = {"taming": taming(dev), "vqgan_plus_10bit": tokenizer("vqgan_plus_10bit", dev)}
    # ---- end to end, profiler off, the two tokenizers alternating
    for rnd in range(2):
        for name, m in models.items():
            enc = timed(lambda: m.encode(x), args.reps)
            dec = timed(lambda: m.decode_tokens(codes), args.reps)
            print(json.dumps(dict(what="events", round=rnd, tokenizer=name, batch=B, encode_ms=round(enc, 3), decode_ms=round(dec, 3))))
    # ---- the library's own timing
    for name, m in models.items():
        _lib.prof_enable(True)
        for _ in range(args.reps):
            m.encode(x)
            m.decode_tokens(codes)
        torch.cuda.synchronize()
        prof = _lib.prof_read()
        _lib.prof_enable(False)
        out = {k: dict(calls=c, ms_per_call=round(ms / c, 4)) for k, (c, ms) in prof.items()}
        print(json.dumps(dict(what="mb_prof", tokenizer=name, batch=B, reps=args.reps, kernels=out)))
        if name == "taming":
            total = (prof["taming_encode"][1] + prof["taming_decode"][1]) / args.reps
            blocks = prof["taming_attn_block"][1] / args.reps
            kern = prof["spatial_attention"][1] / args.reps
            print(json.dumps(dict(what="attention_share", batch=B, forward_ms=round(total, 3), attn_blocks_ms=round(blocks, 3),
                                  attn_kernel_ms=round(kern, 3), blocks_share=round(blocks / total, 4), kernel_share=round(kern / total, 4))))
    # ---- the attention kernel alone
    lib = _lib.load()
    for N in (256, 1024):
        qkv = (torch.randn(B * N, 1536, device=dev, generator=torch.Generator(device=dev).manual_seed(N)) * 1.5).half()
        out = torch.empty(B * N, 512, dtype=torch.float16, device=dev)
        s = torch.cuda.current_stream().cuda_stream

        def go():
            _lib.check(lib.mb_spatial_attention(qkv.data_ptr(), qkv.data_ptr() + 1024, qkv.data_ptr() + 2048, out.data_ptr(), None, B, N, 1536, 512, s))
        ms = timed(go, 10 * args.reps)
        flop = 4.0 * B * N * N * 512
        print(json.dumps(dict(what="mb_spatial_attention", batch=B, N=N, ms=round(ms, 4), tflops=round(flop / ms / 1e9, 1))))


if __name__ == "__main__":
    main()
