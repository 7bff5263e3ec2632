"""Mixed requests in one batch against the best grouping the seeded path allows (profiles/requests.md).  On the GPU box from the repo root:

    python tools/requests_bench.py [rounds]

64 requests at BASELINE configs[2]'s settings (12-bit generator, CFG 7.1 cosine, arccos schedule, decode to uint8 included) whose num_steps cycle
through 16, 32 and 64 (22 / 21 / 21 requests):
    requests : one run_requests call (sample_requests' loop) -- 64 images, sum N = 2368 guided sequence-forwards, one decode of 64;
    grouped  : the same requests grouped by N, one run_seeded call (sample_seeded's loop) per group -- batches of 22, 21 and 21, three decodes.
Warm-up of both, then the two alternated `rounds` times in this one process; per version median, min and max of the wall time of all 64 images
(host clock around work that ends in a device synchronise), the shader clock and socket power sampled over the timed rounds, and the ratio."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from maskbit_amd import SampleRequest                                            # noqa: E402
from maskbit_amd.sampling import check_seeds, run_requests, run_seeded, seeded_plan   # noqa: E402
from maskbit_amd.telemetry import ClockSampler                                   # noqa: E402
from seeded_bench import models                                                  # noqa: E402

dev = torch.device("cuda")
STEPS = (16, 32, 64)
B = 64


def main(rounds):
    gen, tok, kw = models("sample_full12_64")
    sched = dict(guidance_scale=float(kw["guidance_scale"]), guidance_annealing=kw["guidance_annealing"], scale_pow=float(kw["scale_pow"]),
                 softmax_temperature=1.0, use_sampling_annealing=False, mask_schedule_strategy=kw["mask_schedule_strategy"])
    rt = float(kw["randomize_temperature"])
    reqs = [SampleRequest(seed=j, label=j * 37 % 1000, num_steps=STEPS[j % 3], randomize_temperature=rt, **sched) for j in range(B)]
    groups = []
    for N in STEPS:
        idx = [j for j in range(B) if reqs[j].num_steps == N]
        groups.append((seeded_plan(N, sched["guidance_scale"], sched["guidance_annealing"], sched["scale_pow"], 1.0, False, sched["mask_schedule_strategy"]),
                       torch.tensor([reqs[j].label for j in idx], device=dev), check_seeds([reqs[j].seed for j in idx], len(idx))))

    def requests():
        return run_requests(gen, tok, reqs, None, None, want_image=False, want_u8=True)[1]

    def grouped():
        return [run_seeded(gen, tok, y, plan, sd, rt, want_steps=False, want_image=False, want_u8=True)[1] for plan, y, sd in groups]

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for fn in (requests, grouped, requests, grouped):
        fn()
    t = {"requests": [], "grouped": []}
    with ClockSampler(0, period_s=0.05) as cs:
        for _ in range(rounds):
            t["requests"].append(timed(requests))
            t["grouped"].append(timed(grouped))
    forwards = sum(r.num_steps for r in reqs)
    print(f"{B} requests, num_steps {STEPS} cycled ({[sum(r.num_steps == N for r in reqs) for N in STEPS]} requests), {forwards} guided sequence-forwards, "
          f"precision {gen.resolved_precision()}")
    for k, v in t.items():
        print(f"{k:9s}: median {statistics.median(v) * 1e3:8.2f} ms  min {min(v) * 1e3:8.2f}  max {max(v) * 1e3:8.2f}  = {B / statistics.median(v):7.1f} images/s"
              f"   ({rounds} rounds)", flush=True)
    print(f"ratio grouped / requests (medians): {statistics.median(t['grouped']) / statistics.median(t['requests']):.3f}")
    print("telemetry:", json.dumps(cs.summary()))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5)
