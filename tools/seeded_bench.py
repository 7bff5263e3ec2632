"""Seeded sampling against the explicit-noise path (profiles/seeded_noise.md).  Three modes, on the GPU box from the repo root:

    python tools/seeded_bench.py e2e [rounds]       end-to-end images/s of run_seeded (sample_seeded's loop) against run_chunked (sample()'s loop) on
                                                    BASELINE configs[1] (10-bit, 16 steps, no guidance, B = 16) and configs[2] (12-bit, 64 steps, CFG 7.1,
                                                    B = 64), decode to uint8 included: warm-up of both, then the two versions alternated `rounds` times in
                                                    this one process; per version median, min and max.
    python tools/seeded_bench.py mem                peak device memory torch reports for one configs[4]-shard run (14-bit, 256 steps, CFG, B = 32) with
                                                    and without the noise tensors.
    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/seeded_bench.py steps
                                                    the step kernels alone: seeded and explicit instantiation alternated, B = 64 with C = 64 and 512,
                                                    B = 16 with C = 32 (n m = 512 slots), 20 launches each after a warm-up."""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from maskbit_amd import _lib, parity_replay as PR, synth                     # noqa: E402
from maskbit_amd.sampling import build_plan, check_seeds, run_chunked, run_seeded, seeded_plan   # noqa: E402

dev = torch.device("cuda")


def models(run):
    from maskbit_amd import ConvVQModel
    import bench
    g = PR.load_run(run)
    gen, _ = PR.build_models(dev, with_tokenizer=False, name=run)
    bits = int(g["bits"])
    cfg = bench.tok_config(); cfg["codebook_size"], cfg["token_size"] = 2 ** bits, bits
    tok = ConvVQModel(cfg)
    tok.load_state_dict(synth.make_tokenizer_weights(synth.TokCfg(token_size=bits), seed=7), strict=False)
    return gen, tok.eval().requires_grad_(False).to(dev), g["kw"]


def config(run, B, cfg_scale=None):
    gen, tok, kw = models(run)
    N = int(kw["num_steps"])
    scale = float(kw["guidance_scale"]) if cfg_scale is None else cfg_scale
    args = (scale, kw["guidance_annealing"], float(kw["scale_pow"]), 1.0, False, kw["mask_schedule_strategy"])
    labels = (torch.arange(B) * 37 % 1000).to(dev)
    seeds = check_seeds(list(range(B)), B)
    rt = float(kw["randomize_temperature"])
    explicit = lambda: run_chunked(gen, tok, labels, build_plan(N, 512, *args), rt, want_steps=False, want_image=False, want_u8=True)
    seeded = lambda: run_seeded(gen, tok, labels, seeded_plan(N, *args), seeds, rt, want_steps=False, want_image=False, want_u8=True)
    return explicit, seeded, N


def timed(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def e2e(rounds):
    for tag, run, B, reps in (("configs[1] 10-bit / 16 steps / no CFG", PR.RUN_CFG1, 16, 8), ("configs[2] 12-bit / 64 steps / CFG 7.1", "sample_full12_64", 64, 1)):
        explicit, seeded, N = config(run, B)
        torch.manual_seed(0)
        for fn in (explicit, seeded, explicit, seeded):
            fn()
        t = {"explicit": [], "seeded": []}
        for _ in range(rounds):
            t["explicit"].append(timed(explicit, reps))
            t["seeded"].append(timed(seeded, reps))
        for k, v in t.items():
            print(f"{tag}, B = {B}, {k:8s}: median {statistics.median(v) * 1e3:8.2f} ms  min {min(v) * 1e3:8.2f}  max {max(v) * 1e3:8.2f}  "
                  f"= {B / statistics.median(v):7.1f} images/s   ({rounds} rounds of {reps})", flush=True)


def mem():
    explicit, seeded, N = config(PR.RUN_CFG5, 32)
    for k, fn in (("seeded", seeded), ("explicit", explicit)):
        fn(); torch.cuda.synchronize()
        torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn(); torch.cuda.synchronize()
        print(f"configs[4] shard (14-bit, {N} steps, B = 32), {k:8s}: torch peak allocated {torch.cuda.max_memory_allocated() / 2 ** 20:9.1f} MiB "
              f"(before the run {base / 2 ** 20:.1f} MiB), reserved {torch.cuda.max_memory_reserved() / 2 ** 20:9.1f} MiB", flush=True)


def steps():
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    for B, C in ((64, 64), (64, 512), (16, 32)):
        n, m = 256, 2
        lc, lu = torch.randn(B, n, m, C, device=dev) * 3, torch.randn(B, n, m, C, device=dev) * 3
        q, cn = torch.empty(B * n * m, C, device=dev).exponential_(1), torch.randn(B, n, m, device=dev)
        tin = torch.full((B, n, m), C, dtype=torch.int64, device=dev)
        tout, pred = torch.empty_like(tin), torch.empty_like(tin)
        num_regen = torch.full((B,), n * m, dtype=torch.int32, device=dev)
        seeds = check_seeds(list(range(B)), B).to(dev)
        for i in range(22):                                                   # (two warm-up rounds, then 20)
            _lib.check(lib.mb_sample_step_edit(lc.data_ptr(), lu.data_ptr(), 1.5, 1.0, q.data_ptr(), cn.data_ptr(), 0.5, num_regen.data_ptr(), tin.data_ptr(),
                                               tout.data_ptr(), pred.data_ptr(), B, n, m, C, st))
            _lib.check(lib.mb_sample_step_seeded(lc.data_ptr(), lu.data_ptr(), 1.5, 1.0, seeds.data_ptr(), 3, 4.5, 0.5, 0.5, num_regen.data_ptr(), tin.data_ptr(),
                                                 tout.data_ptr(), pred.data_ptr(), B, n, m, C, st))
        torch.cuda.synchronize()
        print(f"B {B} C {C}: 22 launches of each instantiation", flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "e2e"
    if mode == "e2e":
        e2e(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    elif mode == "mem":
        mem()
    elif mode == "steps":
        steps()
    else:
        sys.exit(__doc__)
