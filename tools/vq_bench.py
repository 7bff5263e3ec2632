"""Timing of the lookup (VQ) tokenizer against the LFQ one in the same process: ``forward`` (encode + decode) in images/s at B = 16 and 64 for
the VQGAN+ 10-bit (1024 x 256) and 12-bit (4096 x 64) shapes and the LFQ 12-bit tokenizer, ``decode_tokens`` at B = 64, and the nearest-codeword
search alone (``mb_vq_argmin`` on the encoder's row count) timed with HIP events.  Random seeded weights (maskbit_amd.synth).

    python tools/vq_bench.py [--reps 10]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/vq_bench.py --reps 3     # per-kernel times, vq_search_kernel among them

Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from hip_helpers import Cfg  # noqa: E402
from maskbit_amd import ConvVQModel, _lib  # noqa: E402
from maskbit_amd.synth import TokCfg, make_tokenizer_weights, make_vq_codebook  # noqa: E402


def tokenizer(kind: str, dev):
    if kind == "lfq12":
        tc = TokCfg(token_size=12)
        cfg = Cfg(quantizer_type="lookup-free", codebook_size=4096, token_size=12, commitment_cost=0.25, num_channels=3, hidden_channels=128,
                  channel_mult=[1, 1, 2, 2, 4], num_resolutions=5, num_res_blocks=2, sample_with_conv=True)
        sd = make_tokenizer_weights(tc, seed=7, with_encoder=True)
    else:
        C, K = {"vqgan_plus_10bit": (1024, 256), "vqgan_plus_12bit": (4096, 64)}[kind]
        tc = TokCfg(token_size=K)
        cfg = Cfg(quantizer_type="lookup", codebook_size=C, token_size=K, commitment_cost=0.25, num_channels=3, hidden_channels=128,
                  channel_mult=[1, 1, 2, 2, 4], num_resolutions=5, num_res_blocks=2, sample_with_conv=True)
        sd = make_tokenizer_weights(tc, seed=7, with_encoder=True, lfq_buffers=False)
        sd["quantize.embedding.weight"] = make_vq_codebook(C, K, 8, torch.zeros(K), torch.ones(K))
    m = ConvVQModel(cfg)
    m.load_state_dict(sd, strict=True)
    return m.eval().requires_grad_(False).to(dev)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    for kind in ("lfq12", "vqgan_plus_12bit", "vqgan_plus_10bit"):
        m = tokenizer(kind, dev)
        for B in (16, 64):
            x = torch.rand(B, 3, 256, 256, generator=g).to(dev)
            ms = timed(lambda: m(x), args.reps)
            print(json.dumps(dict(what="forward", tokenizer=kind, batch=B, ms=round(ms, 3), images_per_s=round(B / ms * 1e3, 1))))
        codes = torch.randint(0, m.codebook_size, (64, 256), generator=g).to(dev)
        ms = timed(lambda: m.decode_tokens(codes), args.reps)
        print(json.dumps(dict(what="decode_tokens", tokenizer=kind, batch=64, ms=round(ms, 3))))
        if kind != "lfq12":
            C, K = m.codebook_size, m.token_size
            for B in (16, 64):
                N = B * 256
                z = torch.randn(N, K, device=dev)
                cb = m.quantize.embedding.weight.detach().contiguous()
                idx = torch.empty(N, dtype=torch.int64, device=dev)
                dist = torch.empty(N, dtype=torch.float32, device=dev)
                lib = _lib.load()
                s = torch.cuda.current_stream().cuda_stream
                ms = timed(lambda: _lib.check(lib.mb_vq_argmin(z.data_ptr(), cb.data_ptr(), N, C, K, 0, 0, idx.data_ptr(), dist.data_ptr(), s)),
                           args.reps)
                print(json.dumps(dict(what="vq_argmin (incl. codebook prep + allocations)", tokenizer=kind, batch=B, rows=N, ms=round(ms, 4),
                                      gflop=round(2 * N * C * K / 1e9, 2))))
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
