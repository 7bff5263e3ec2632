"""GPU tests of the sampling session (include/maskbit_hip.h "sampling session").

Every comparison is bit for bit.  The session's kernels run per launch through the diagnostic entries against the torch restatement of the hole-fill
rule in tests/test_session_cpu.py; the session itself runs on the tiny models against ``run_requests`` on each request ALONE."""
import ctypes
import dataclasses
import functools

import pytest
import torch

from test_hip_edit import MASK, tiny_models, tokens_with_masks
from test_hip_requests import five_alone, run_steps
from test_hip_seeded import DEV, KW, stream
from test_requests_cpu import five_requests
from test_session_cpu import DONE_PATTERNS, compact, done_pattern, hole_fill

pytestmark = pytest.mark.gpu

GUARD = 2                                                                                          # rows allocated beyond max_active, never to be touched
FIELDS = ("label", "seed", "num_regen", "slot", "local_step", "N")


def oracle_codes(pred, C, m):
    from oracle import maskbit_oracle as O
    bits = (C.bit_length() - 1) * m
    return O.combine_groups(pred.cpu(), bits, m).long()


class Rows:
    """The arrays of mb_session_rows for ``cap`` rows (+ GUARD rows behind them) with distinct values in every field of every row."""

    def __init__(self, cap, max_steps, P, seed):
        g = torch.Generator().manual_seed(seed)
        R = cap + GUARD
        self.cap, self.max_steps, self.P = cap, max_steps, P
        self.label = 1000 + 3 * torch.arange(R, dtype=torch.int64)
        self.seed = torch.randperm(R, generator=g).to(torch.int64) * (2 ** 40 + 12345) - 2 ** 62
        self.num_regen = (7 + 2 * torch.arange(R)).to(torch.int32)
        self.slot = torch.cat([torch.randperm(cap, generator=g), torch.full((GUARD,), -9)]).to(torch.int32)
        self.N = (1 + torch.arange(R) % max_steps).to(torch.int32)
        self.local_step = torch.zeros(R, dtype=torch.int32)
        self.pool = torch.randint(-2 ** 31, 2 ** 31 - 1, (R, max_steps, 6), generator=g, dtype=torch.int64).to(torch.int32)
        self.tokens = torch.arange(R * P, dtype=torch.int64).reshape(R, P) * 3 + 2 ** 33            # a pure copy: any int64 will do, all distinct

    def to_device(self):
        self.dev = {k: getattr(self, k).to(DEV) for k in FIELDS + ("pool", "tokens")}
        return self

    def struct(self):
        from maskbit_amd import _lib
        d = self.dev
        return _lib.SessionRows(*[d[k].data_ptr() for k in FIELDS + ("pool",)], self.cap, self.max_steps)

    def back(self):
        return {k: v.cpu() for k, v in self.dev.items()}


# ---- 1. the kernels, per launch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 2, 3, 65, 130])
@pytest.mark.parametrize("n,m", [(16, 2), (512, 2), (16, 1), (15, 1)])
def test_plan_and_move_kernels_equal_the_restatement(n, m, A):
    """P = 32 and P = 1024 (two 4 KiB chunks per move), m = 1, and an odd P = 15 (rows not 16-byte aligned: the 8-byte path); A up to past two waves
    of the plan kernel's ballot; the five hand-written done patterns and a seeded random one.  After one retire: rows [0, A') hold the restatement's
    rows in every field, the plan snapshot is the restatement's lists, the k codes are the oracle's combine of the finished rows' predictions in
    ascending row order, slot[] is still a permutation, and nothing outside is touched."""
    from maskbit_amd import _lib
    lib = _lib.load()
    C, P, cap, SENT = 64, n * m, A + 3, -77
    for pi, name in enumerate(DONE_PATTERNS):
        done = done_pattern(name, A, seed=P)
        rows = Rows(cap, 9, P, seed=100 * A + pi)
        rows.N[:A] = 5 + torch.arange(A, dtype=torch.int32)                                        # distinct
        rows.local_step[:A] = torch.where(done, rows.N[:A], (torch.arange(A) % 5).to(torch.int32))  # unfinished: below N
        rows.local_step[A:] = rows.N[A:]                                                           # (rows above A look finished: they must not be read)
        rows.to_device()
        before = rows.back()
        pred = torch.randint(0, C, (A, n, m), generator=torch.Generator().manual_seed(A + pi))
        pred_dev = pred.to(DEV)
        codes_all = torch.full((A, n), SENT, dtype=torch.int64, device=DEV)
        codes = torch.full((A + GUARD, n), SENT, dtype=torch.int64, device=DEV)
        plan = torch.full((2 + 3 * cap + GUARD,), SENT, dtype=torch.int32, device=DEV)
        st = rows.struct()
        _lib.check(lib.mb_session_retire(ctypes.byref(st), rows.dev["tokens"].data_ptr(), pred_dev.data_ptr(), codes_all.data_ptr(), codes.data_ptr(),
                                         plan.data_ptr(), A, n, m, C, stream()), "mb_session_retire")
        after = rows.back()
        fin, src, dst, Ap = hole_fill(done)
        k = len(fin)
        # the snapshot
        plan = plan.cpu()
        assert plan[0].item() == k and plan[1].item() == len(src), (name, plan[:2].tolist())
        assert plan[2:2 + k].tolist() == fin and plan[2 + cap:2 + cap + len(src)].tolist() == src and plan[2 + 2 * cap:2 + 2 * cap + len(dst)].tolist() == dst
        assert bool((plan[2 + 3 * cap:] == SENT).all())
        # the surviving rows
        want = compact(done, {f: before[f][:A] for f in FIELDS + ("tokens",)})
        for f in FIELDS + ("tokens",):
            assert torch.equal(after[f][:Ap], want[f]), (name, f)
            assert torch.equal(after[f][A:], before[f][A:]), (name, f, "rows outside the active prefix")
        for f in ("label", "seed", "num_regen", "local_step", "N", "tokens"):                      # sources are read, never written
            assert torch.equal(after[f][Ap:A], before[f][Ap:A]), (name, f)
        assert sorted(after["slot"][:cap].tolist()) == list(range(cap))                            # the finished rows' slots are free again, above A'
        assert torch.equal(after["pool"], before["pool"])
        # the codes
        codes = codes.cpu()
        if k:
            assert torch.equal(codes[:k], oracle_codes(pred[torch.tensor(fin)], C, m)), name
        assert bool((codes[k:] == SENT).all())


def test_row_table_kernel_gathers_raw_records_and_increments():
    """A = 130 of 131 rows, permuted slots, local steps at 0 and at N - 1: row[r] is pool[slot[r]][local_step[r]] as raw 24-byte records."""
    from maskbit_amd import _lib
    lib = _lib.load()
    A, cap, S, SENT = 130, 131, 7, -5
    rows = Rows(cap, S, 4, seed=9)
    rows.local_step[:] = torch.where(torch.arange(cap + GUARD) % 2 == 0, torch.zeros_like(rows.N), rows.N - 1)
    rows.to_device()
    before = rows.back()
    out = torch.full((cap + GUARD, 6), SENT, dtype=torch.int32, device=DEV)
    st = rows.struct()
    _lib.check(lib.mb_session_row_table(ctypes.byref(st), out.data_ptr(), A, stream()), "mb_session_row_table")
    after, out = rows.back(), out.cpu()
    r = torch.arange(A)
    assert torch.equal(out[:A], before["pool"][before["slot"][:A].long(), before["local_step"][:A].long()])
    assert bool((out[A:] == SENT).all())
    assert torch.equal(after["local_step"][:A], before["local_step"][:A] + 1) and torch.equal(after["local_step"][A:], before["local_step"][A:])
    for f in ("label", "seed", "num_regen", "slot", "N", "pool", "tokens"):
        assert torch.equal(after[f], before[f]), f
    assert len(set(before["slot"][:A].tolist())) == A and before["slot"][:A].tolist() != r.tolist()   # (permuted)


@pytest.mark.parametrize("A,K,cap", [(2, 3, 6), (0, 1, 1), (1, 70, 72)])
@pytest.mark.parametrize("from_tokens", [False, True])
def test_admit_kernel_appends_rows(A, K, cap, from_tokens):
    """K requests at rows [A, A + K), all-masked and from tokens (K = 70: two launches of 64 and 6 requests): start tokens clamped to [0, C] as
    edit_load_tokens does, num_regen = the masked count, label, seed, N, local step 0, the N records in the row's pool slot; nothing else touched."""
    from maskbit_amd import _lib
    lib = _lib.load()
    n, m, C, S = 16, 2, 64, 6
    P = n * m
    g = torch.Generator().manual_seed(17 * K + A)
    rows = Rows(cap, S, P, seed=K)
    rows.local_step[:] = 3
    rows.to_device()
    before = rows.back()
    labels = torch.randint(0, 1000, (K,), generator=g)
    seeds = torch.randint(-2 ** 62, 2 ** 62, (K,), generator=g)
    num_steps = [1 + (3 * k + 2) % S for k in range(K)]
    sched = torch.randint(-2 ** 31, 2 ** 31 - 1, (sum(num_steps), 6), generator=g, dtype=torch.int64).to(torch.int32)
    init = None
    if from_tokens:
        init = torch.randint(0, C + 1, (K, n, m), generator=g)
        init[0, 0, 0], init[0, 1, 1], init[K - 1, 5, 0] = -5, C + 9, 2 ** 40                       # outside [0, C]: clamped to 0, C, C
    want_tokens = torch.full((K, n, m), C) if init is None else init.clamp(0, C)
    dev = [t.to(DEV) for t in (labels, seeds, sched)] + [init.to(DEV) if from_tokens else None]
    st = rows.struct()
    _lib.check(lib.mb_session_admit_rows(ctypes.byref(st), rows.dev["tokens"].data_ptr(), A, K, dev[0].data_ptr(), dev[1].data_ptr(), (ctypes.c_int * K)(*num_steps),
                                         dev[2].data_ptr(), dev[3].data_ptr() if from_tokens else None, n, m, C, stream()), "mb_session_admit_rows")
    after = rows.back()
    new = slice(A, A + K)
    assert torch.equal(after["tokens"][new], want_tokens.reshape(K, P))
    assert after["num_regen"][new].tolist() == (want_tokens == C).sum(dim=(1, 2)).tolist()
    assert torch.equal(after["label"][new], labels) and torch.equal(after["seed"][new], seeds)
    assert after["N"][new].tolist() == num_steps and after["local_step"][new].tolist() == [0] * K
    want_pool, off = before["pool"].clone(), 0
    for k, N in enumerate(num_steps):
        want_pool[int(before["slot"][A + k]), :N] = sched[off:off + N]
        off += N
    assert torch.equal(after["pool"], want_pool)
    assert torch.equal(after["slot"], before["slot"])
    for f in FIELDS + ("tokens",):
        assert torch.equal(after[f][:A], before[f][:A]) and torch.equal(after[f][A + K:], before[f][A + K:]), f


# ---- 2. the session on the tiny models ----------------------------------------------------------------------------------------------------------
def alone(r, guided=True, init=None):
    """The yardstick: the request alone through run_requests -> (image [3, H, W], step tokens [N, n, m], codes [n])."""
    gm, tm = tiny_models()
    img, (st,) = run_steps(gm, tm, [r], guided=guided, init=init)
    return img[0].clone(), st.clone(), oracle_codes(st[-1:], MASK, 2)[0].to(DEV)


def check_finished(f, want, what=""):
    img, st, codes = want
    assert torch.equal(f.codes, codes), (what, f.ticket, int((f.codes != codes).sum()))
    if f.image.dtype == torch.uint8:
        from oracle import maskbit_oracle as O
        assert torch.equal(f.image.cpu(), O.to_uint8_nhwc(img[None].cpu())[0]), (what, f.ticket)
    else:
        assert torch.equal(f.image, img), (what, f.ticket)


def replay(session, arrivals, want, predictions=True):
    """arrivals: {tick: [requests submitted before it]} -> per ticket (first tick it ran, tick it finished); every Finished and (with ``predictions``)
    every tick's predictions are checked against ``want[ticket]`` on the way."""
    first, last, tick = {}, {}, 0
    pending = sum(len(v) for v in arrivals.values())
    while pending or session.active or session.queued:
        for r in arrivals.get(tick, ()):
            session.submit(r)
            pending -= 1
        out = session.step(return_predictions=predictions)
        done, preds = out if predictions else (out, {})
        assert session.active <= session.max_active
        for t, p in preds.items():
            first.setdefault(t, tick)
            assert torch.equal(p, want[t][1][tick - first[t]]), (t, tick)
        for f in done:
            last[f.ticket] = tick
            check_finished(f, want[f.ticket], tick)
        tick += 1
        assert tick < 200
    return first, last


@pytest.mark.parametrize("u8", [False, True])
def test_staggered_arrival_with_moves(u8):
    """five_requests (N = 8, 3, 5, 8, 1) through three rows: two before tick 0, one after tick 1, one after tick 2, one after tick 6.  Request 1 leaves
    row 1 at tick 2 and request 2 moves down from row 2; request 3 then waits for nothing and takes row 2; requests 0 and 4 leave together at tick 7."""
    from maskbit_amd import SamplingSession
    gm, tm = tiny_models()
    reqs, want = five_requests(), dict(enumerate(five_alone()))
    want = {t: (img, st, oracle_codes(st[-1:], MASK, 2)[0].to(DEV)) for t, (img, st) in want.items()}
    s = SamplingSession(gm, tm, max_active=3, max_steps=8, guided=True, return_uint8=u8)
    first, last = replay(s, {0: reqs[0:2], 2: reqs[2:3], 3: reqs[3:4], 7: reqs[4:5]}, want, predictions=not u8)
    N = [r.num_steps for r in reqs]
    if not u8:
        assert first == {0: 0, 1: 0, 2: 2, 3: 3, 4: 7}                                             # admitted in submission order, at the first tick with a free row
        assert last == {t: first[t] + N[t] - 1 for t in range(5)}
    assert last == {0: 7, 1: 2, 2: 6, 3: 10, 4: 7}
    assert (s.active, s.queued, s.ticks) == (0, 0, 11)


def test_a_full_session_queues_in_submission_order():
    """Two rows, all five requests submitted at once: the queue holds three, and each is admitted -- never ahead of an earlier one -- at the first tick
    with a free row; each finishes N - 1 ticks later."""
    from maskbit_amd import SamplingSession
    gm, tm = tiny_models()
    reqs = five_requests()
    want = {t: (img, st, oracle_codes(st[-1:], MASK, 2)[0].to(DEV)) for t, (img, st) in enumerate(five_alone())}
    s = SamplingSession(gm, tm, max_active=2, max_steps=8)
    for r in reqs:
        s.submit(r)
    assert s.queued == 5
    first, last = replay(s, {}, want)
    # rows free up after ticks 2 (request 1) and 7 (requests 0 and 2): request 2 enters at 3, requests 3 and 4 at 8
    assert first == {0: 0, 1: 0, 2: 3, 3: 8, 4: 8} and last == {0: 7, 1: 2, 2: 7, 3: 15, 4: 8}


@functools.lru_cache(maxsize=None)
def churn_requests():
    from maskbit_amd import SampleRequest
    return [SampleRequest(seed=100000 + j, label=j % 10, num_steps=(2, 4, 1, 6)[j % 4], guidance_scale=(3.0, 0.0, 5.5)[j % 3], softmax_temperature=0.9 + 0.01 * j,
                          randomize_temperature=1.0 + 0.25 * j) for j in range(40)]


def test_churn_of_forty_requests():
    """40 requests, three submitted per tick into eight rows: every tick admits, retires and moves; every result equals the request alone."""
    from maskbit_amd import SamplingSession
    gm, tm = tiny_models()
    reqs = churn_requests()
    want = {t: alone(r) for t, r in enumerate(reqs)}
    s = SamplingSession(gm, tm, max_active=8, max_steps=6)
    first, last = replay(s, {t: reqs[3 * t:3 * t + 3] for t in range(14)}, want)
    assert sorted(last) == list(range(40)) and all(last[t] == first[t] + reqs[t].num_steps - 1 for t in range(40))
    assert [first[t] for t in range(40)] == sorted(first[t] for t in range(40))                    # admission order is submission order
    assert max(first[t] - t // 3 for t in range(40)) > 0                                           # (the queue did fill: someone waited)


def test_everything_at_once_equals_sample_requests():
    """All five submitted before tick 0 with room for all: the session's left-aligned run and sample_requests' right-aligned run agree per request."""
    from maskbit_amd import SamplingSession, sample_requests
    gm, tm = tiny_models()
    reqs = five_requests()
    img, steps = sample_requests(gm, tm, reqs, guided=True)
    s = SamplingSession(gm, tm, max_active=8, max_steps=8)
    assert [s.submit(r) for r in reqs] == [0, 1, 2, 3, 4]
    done = s.drain()
    assert sorted(f.ticket for f in done) == [0, 1, 2, 3, 4] and [f.ticket for f in done] == [4, 1, 2, 0, 3]   # by finishing tick, then by row
    for f in done:
        assert f.request is reqs[f.ticket]
        assert torch.equal(f.image, img[f.ticket]) and torch.equal(f.codes, oracle_codes(steps[f.ticket][-1][None], MASK, 2)[0].to(DEV)), f.ticket
    assert s.ticks == 8


def test_another_call_between_ticks_changes_nothing():
    """sample_seeded on the same models between two ticks (it overwrites the engine's own token buffers and its guided-forward label cache): the
    session's later results are unchanged, and the call's result is what it is without a session."""
    from maskbit_amd import SamplingSession, sample_seeded
    gm, tm = tiny_models()
    reqs = five_requests()
    want = {t: (img, st, oracle_codes(st[-1:], MASK, 2)[0].to(DEV)) for t, (img, st) in enumerate(five_alone())}
    seeds, y = [5, 2 ** 64 - 1, 2 ** 63 + 17], torch.tensor([1, 4, 8], device=DEV)
    kw = dict(KW, num_steps=3)
    want_img, want_steps = sample_seeded(gm, tm, seeds, y, **kw)
    s = SamplingSession(gm, tm, max_active=4, max_steps=8)
    for r in reqs[:4]:
        s.submit(r)
    done = []
    for tick in range(8):
        done += s.step()
        if tick in (0, 1, 4):                                                                      # with 4, with 4 and (after request 1 left) with 2 active
            got_img, got_steps = sample_seeded(gm, tm, seeds, y, **kw)
            assert torch.equal(got_img, want_img) and all(torch.equal(a, b) for a, b in zip(got_steps, want_steps))
    assert sorted(f.ticket for f in done) == [0, 1, 2, 3] and s.active == 0
    for f in done:
        check_finished(f, want[f.ticket])


def test_requests_start_from_their_own_token_maps():
    """init_tokens per request (512 / 100 / 7 masked slots; one map on the host, one on the device, one request without a map) through two rows:
    each equals run_requests of the request alone from its map, and the known slots come back in every prediction."""
    from maskbit_amd import SampleRequest, SamplingSession
    gm, tm = tiny_models()
    init, regen = tokens_with_masks([512, 100, 7], seed=31)
    base = dict(KW, guidance_annealing="none")
    reqs = [SampleRequest(seed=21, label=1, **dict(base, num_steps=4)),
            SampleRequest(seed=2 ** 63 + 1, label=4, **dict(base, num_steps=2, guidance_scale=2.0, softmax_temperature=0.8)),
            SampleRequest(seed=2 ** 64 - 1, label=8, **dict(base, num_steps=4, randomize_temperature=3.0, mask_schedule_strategy="linear")),
            SampleRequest(seed=77, label=3, **dict(base, num_steps=3))]
    want = {b: alone(r, init=init[b:b + 1]) for b, r in enumerate(reqs[:3])}
    want[3] = alone(reqs[3])
    s = SamplingSession(gm, tm, max_active=2, max_steps=4)
    s.submit(reqs[0], init_tokens=init[0])
    s.submit(reqs[1], init_tokens=init[1].to(DEV))
    s.submit(reqs[2], init_tokens=init[2])
    s.submit(reqs[3])
    seen = {t: [] for t in range(4)}
    finished = []
    while s.active or s.queued:
        done, preds = s.step(return_predictions=True)
        finished += done
        for t, p in preds.items():
            seen[t].append(p)
    assert sorted(f.ticket for f in finished) == [0, 1, 2, 3]
    for f in finished:
        check_finished(f, want[f.ticket])
    for t in range(4):
        assert torch.equal(torch.stack(seen[t]), want[t][1]), t
    for b in range(3):
        keep = ~regen[b].to(DEV)
        assert torch.equal(torch.stack(seen[b])[:, keep], init[b].to(DEV)[keep].expand(reqs[b].num_steps, -1))


def test_unguided_session():
    """guided=False with zero-scale requests: every tick runs the plain forward; each request equals itself alone with guided=False."""
    from maskbit_amd import SamplingSession
    gm, tm = tiny_models()
    reqs = [dataclasses.replace(r, guidance_scale=0.0) for r in five_requests()[:3]]
    want = {t: alone(r, guided=False) for t, r in enumerate(reqs)}
    s = SamplingSession(gm, tm, max_active=2, max_steps=8, guided=False)
    first, last = replay(s, {0: reqs[:2], 1: reqs[2:]}, want)
    assert last == {0: 7, 1: 2, 2: 7}


def test_empty_and_drained_session():
    """step() on an empty session returns [] and launches nothing; after drain() the session is empty and its rows are used again."""
    from maskbit_amd import SamplingSession, _lib
    gm, tm = tiny_models()
    reqs, ref = five_requests(), five_alone()
    want = {t: (img, st, oracle_codes(st[-1:], MASK, 2)[0].to(DEV)) for t, (img, st) in enumerate(ref)}
    s = SamplingSession(gm, tm, max_active=2, max_steps=8)
    _lib.prof_enable(True)
    try:
        assert s.step() == [] and s.step(return_predictions=True) == ([], {}) and s.drain() == []
        assert _lib.prof_read() == {}
    finally:
        _lib.prof_enable(False)
    assert s.ticks == 0
    assert s.submit(reqs[1]) == 0 and s.submit(reqs[4]) == 1
    done = s.drain()
    assert [f.ticket for f in done] == [1, 0] and (s.active, s.queued, s.ticks) == (0, 0, 3)
    _lib.prof_enable(True)
    try:
        assert s.step() == []                                                                      # drained: a session object exists, and still nothing runs
        assert _lib.prof_read() == {}
    finally:
        _lib.prof_enable(False)
    assert s.submit(reqs[2]) == 2 and s.submit(reqs[1]) == 3                                       # tickets go on counting; the rows are used again
    again = s.drain()
    assert [f.ticket for f in again] == [3, 2] and (s.active, s.queued, s.ticks) == (0, 0, 8)
    for f, t in zip(done + again, (4, 1, 1, 2)):
        check_finished(f, want[t])
