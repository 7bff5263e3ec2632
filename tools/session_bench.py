"""A sampling session against closed sample_requests runs on one arrival trace (profiles/session.md).  On the GPU box from the repo root:

    python tools/session_bench.py [out.json]

Requests at BASELINE configs[2]'s settings (12-bit generator, CFG 7.1 cosine, arccos schedule, decode to uint8 included) with num_steps drawn from
{16, 32, 64}; the trace -- TRACE_REQUESTS arrivals with exponential inter-arrival times of mean TRACE_MEAN_MS, seed TRACE_SEED -- is replayed in real
time two ways in this one process:
    closed  : whenever the previous call has finished, one run_requests call (sample_requests' loop) on whatever has arrived since;
    session : a SamplingSession of 64 rows; every step admits what has arrived.
Latency = arrival -> the host has seen the request's image complete on the device (an event behind the call / the step).  The session is kept one
step ahead of the device, no more: the host waits for step t - 1 after it has enqueued step t.
Then the uniform case, 64 equal 64-step requests submitted before tick 0 (into one session that is kept, as a front end keeps one) against
run_requests of the same list, alternated five times, with the host time spent inside step(); and one more session run of it, and one of the
trace, under mb_prof_* for the session's own kernels next to the tick's forward."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from maskbit_amd import SampleRequest, SamplingSession, _lib                     # noqa: E402
from maskbit_amd.sampling import run_requests                                    # noqa: E402
from maskbit_amd.telemetry import ClockSampler                                   # noqa: E402
from seeded_bench import models                                                  # noqa: E402

dev = torch.device("cuda")
STEPS = (16, 32, 64)
TRACE_REQUESTS, TRACE_MEAN_MS, TRACE_SEED = 128, 33.0, 20240
ROWS = 64
SESSION_KERNELS = ("session_row_table", "session_plan", "session_codes", "session_move", "session_admit")


def make_trace(sched, rt):
    g = torch.Generator().manual_seed(TRACE_SEED)
    gaps = torch.empty(TRACE_REQUESTS, dtype=torch.float64).exponential_(1.0, generator=g) * (TRACE_MEAN_MS / 1e3)
    steps = torch.randint(0, 3, (TRACE_REQUESTS,), generator=g)
    at = torch.cumsum(gaps, 0) - gaps[0]                                         # the first request arrives at 0
    reqs = [SampleRequest(seed=1000 + j, label=j * 37 % 1000, num_steps=STEPS[int(steps[j])], randomize_temperature=rt, **sched) for j in range(TRACE_REQUESTS)]
    return at.tolist(), reqs


def replay_closed(gen, tok, at, reqs):
    done, nxt, calls = {}, 0, 0
    t0 = time.perf_counter()
    while nxt < len(reqs):
        now = time.perf_counter() - t0
        if at[nxt] > now:
            time.sleep(at[nxt] - now)
            now = time.perf_counter() - t0
        end = nxt
        while end < len(reqs) and at[end] <= now:
            end += 1
        run_requests(gen, tok, reqs[nxt:end], True, None, want_image=False, want_u8=True)
        torch.cuda.synchronize()
        stamp = time.perf_counter() - t0
        for j in range(nxt, end):
            done[j] = stamp
        nxt, calls = end, calls + 1
    return done, time.perf_counter() - t0, calls


def replay_session(gen, tok, at, reqs):
    s = SamplingSession(gen, tok, max_active=ROWS, max_steps=max(STEPS), guided=True, return_uint8=True)
    done, nxt, pending = {}, 0, []                                               # pending: (event, tickets) of the steps not yet seen complete
    t0 = time.perf_counter()

    def settle(keep):
        while len(pending) > keep:
            ev, tickets = pending.pop(0)
            ev.synchronize()
            stamp = time.perf_counter() - t0
            for t in tickets:
                done[t] = stamp
    while nxt < len(reqs) or s.active or s.queued:
        now = time.perf_counter() - t0
        if nxt < len(reqs) and not (s.active or s.queued) and at[nxt] > now:
            settle(0)
            now = time.perf_counter() - t0
            if at[nxt] > now:
                time.sleep(at[nxt] - now)
                now = time.perf_counter() - t0
        while nxt < len(reqs) and at[nxt] <= now:
            assert s.submit(reqs[nxt]) == nxt
            nxt += 1
        out = s.step()
        ev = torch.cuda.Event()
        ev.record()
        pending.append((ev, [f.ticket for f in out]))
        settle(1)
    settle(0)
    return done, time.perf_counter() - t0, s.ticks


def latency(done, at):
    v = sorted(done[j] - at[j] for j in range(len(at)))
    return {"mean_ms": 1e3 * statistics.mean(v), "p50_ms": 1e3 * v[len(v) // 2], "p95_ms": 1e3 * v[min(len(v) - 1, int(0.95 * len(v)))], "max_ms": 1e3 * v[-1]}


def main(out_path):
    gen, tok, kw = models("sample_full12_64")
    sched = dict(guidance_scale=float(kw["guidance_scale"]), guidance_annealing=kw["guidance_annealing"], scale_pow=float(kw["scale_pow"]),
                 softmax_temperature=1.0, use_sampling_annealing=False, mask_schedule_strategy=kw["mask_schedule_strategy"])
    rt = float(kw["randomize_temperature"])
    at, reqs = make_trace(sched, rt)
    result = {"trace": {"requests": TRACE_REQUESTS, "mean_interarrival_ms": TRACE_MEAN_MS, "seed": TRACE_SEED, "span_s": at[-1],
                        "num_steps": {N: sum(r.num_steps == N for r in reqs) for N in STEPS}}, "precision": gen.resolved_precision()}
    uniform = [SampleRequest(seed=j, label=j * 37 % 1000, num_steps=64, randomize_temperature=rt, **sched) for j in range(ROWS)]

    def closed_uniform():
        run_requests(gen, tok, uniform, True, None, want_image=False, want_u8=True)

    session = SamplingSession(gen, tok, max_active=ROWS, max_steps=64, guided=True, return_uint8=True)   # one session, as a front end keeps one
    host_s = []                                                                 # per run: host time inside step() -- the enqueue, nothing waits

    def session_uniform():
        for r in uniform:
            session.submit(r)
        done, host, ticks0 = 0, 0.0, session.ticks
        while session.active or session.queued:
            t0 = time.perf_counter()
            done += len(session.step())
            host += time.perf_counter() - t0
        host_s.append(host)
        assert done == ROWS and session.ticks - ticks0 == 64

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for fn in (closed_uniform, session_uniform):                                # warm-up: every kernel of both paths, the engines at full size
        fn()
    torch.cuda.synchronize()
    with ClockSampler(0, period_s=0.05) as cs:
        for name, fn in (("closed", replay_closed), ("session", replay_session)):
            done, wall, units = fn(gen, tok, at, reqs)
            assert sorted(done) == list(range(TRACE_REQUESTS))
            result[name] = dict(latency(done, at), wall_s=wall, images_per_s=TRACE_REQUESTS / wall, calls_or_ticks=units)
            print(name, json.dumps(result[name]), flush=True)
        t = {"closed": [], "session": []}
        for _ in range(5):
            t["closed"].append(timed(closed_uniform))
            t["session"].append(timed(session_uniform))
    result["uniform"] = {k: {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v)} for k, v in t.items()}
    result["uniform"]["session_host_enqueue_ms"] = {"median_ms": 1e3 * statistics.median(host_s[-5:]), "max_ms": 1e3 * max(host_s[-5:])}
    result["telemetry"] = cs.summary()
    print("uniform", json.dumps(result["uniform"]), flush=True)
    # the session's own kernels, in a run of their own (event timing of every launch slows the host)
    _lib.prof_enable(True, every=1)
    try:
        session_uniform()
        torch.cuda.synchronize()
        prof = _lib.prof_read()
    finally:
        _lib.prof_enable(False)
    own = {k: {"calls": prof[k][0], "total_ms": prof[k][1]} for k in SESSION_KERNELS if k in prof}
    rest = sum(ms for k, (_, ms) in prof.items() if k not in SESSION_KERNELS and k != "sample_step_requests" and not k.startswith("conv") and not k.startswith("dec"))
    result["prof_uniform"] = {"session_kernels": own, "session_kernels_total_ms": sum(v["total_ms"] for v in own.values()),
                              "sample_step_requests_ms": prof.get("sample_step_requests", (0, 0.0))[1], "other_ms": rest, "ticks": 64,
                              "all": {k: list(v) for k, v in prof.items()}}
    print("prof", json.dumps(result["prof_uniform"]["session_kernels"]), "total", result["prof_uniform"]["session_kernels_total_ms"], flush=True)
    # ... and on the trace, where ticks admit, retire and move (timing ignored: the profiling slows the host)
    _lib.prof_enable(True, every=1)
    try:
        _, _, ticks = replay_session(gen, tok, at, reqs)
        torch.cuda.synchronize()
        prof = _lib.prof_read()
    finally:
        _lib.prof_enable(False)
    result["prof_trace"] = {"ticks": ticks, "all": {k: list(v) for k, v in prof.items()}}
    print("prof_trace", ticks, json.dumps({k: list(prof[k]) for k in SESSION_KERNELS if k in prof}), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
