"""GPU tests of per-sample sampling arguments (include/maskbit_hip.h "per-sample sampling arguments").

Every comparison is bit for bit, and the yardstick is always the seeded code the requests path was built on, called per sample at B = 1:
``mb_sample_step_seeded`` for the step kernels, ``sample_seeded`` / ``sample_from_tokens(seeds=)`` and the request run alone for the run."""
import ctypes
import dataclasses
import functools

import pytest
import torch

from test_hip_edit import MASK, tiny_models, tokens_with_masks
from test_hip_seeded import DEV, KW, conf_weight, dev_seeds, step_seeded, stream
from test_requests_cpu import five_requests

pytestmark = pytest.mark.gpu


def f32(v):
    return ctypes.c_float(v).value


# ---- 1. the step kernels -----------------------------------------------------------------------------------------------------------------------
def step_requests(lib, lc, lu, rows, seeds, num_regen, tin, C):
    """One mb_sample_step_requests call on device tensors -> (pred, tokens_out).  rows: [(scale, temperature, ratio, rt, w, step)] per sample."""
    from maskbit_amd import _lib
    B, n, m = tin.shape
    table = torch.zeros((B, 6), dtype=torch.int32)
    table.view(torch.float32)[:, :5] = torch.tensor([r[:5] for r in rows], dtype=torch.float64).to(torch.float32)
    table[:, 5] = torch.tensor([r[5] for r in rows], dtype=torch.int32)
    table = table.to(DEV)
    tout, pred = torch.empty_like(tin), torch.empty_like(tin)
    _lib.check(lib.mb_sample_step_requests(lc.data_ptr(), lu.data_ptr() if lu is not None else None, table.data_ptr(), seeds.data_ptr(), num_regen.data_ptr(),
                                           tin.data_ptr(), tout.data_ptr(), pred.data_ptr(), B, n, m, C, stream()), "mb_sample_step_requests")
    return pred, tout


def check_step_against_single_sample_seeded_steps(n, m, C, guided, masked, rows, seeds):
    from maskbit_amd import _lib
    from test_edit_cpu import random_slot_masks
    lib = _lib.load()
    B, P = len(masked), n * m
    g = torch.Generator().manual_seed(2000 + C + P)
    regen = random_slot_masks(masked, P, seed=C + 1).reshape(B, n, m)
    known = torch.randint(0, C, (B, n, m), generator=g)
    tin = torch.where(regen, torch.full_like(known, C), known).to(DEV)
    lc = (3.0 * torch.randn(B, n, m, C, generator=g)).to(DEV)
    lu = (3.0 * torch.randn(B, n, m, C, generator=g)).to(DEV) if guided else None
    num_regen = torch.tensor([k + 3 * b for b, k in enumerate(masked)], dtype=torch.int32, device=DEV)   # (the initial count of an edit run: >= the current one)
    sd = dev_seeds(seeds)
    pred, out = step_requests(lib, lc, lu, rows, sd, num_regen, tin, C)
    for b, (scale, temp, ratio, rt, w, step) in enumerate(rows):
        want_pred, want_out = step_seeded(lib, lc[b:b + 1].contiguous(), lu[b:b + 1].contiguous() if guided else None, scale, temp, sd[b:b + 1].contiguous(), step,
                                          rt, w, ratio, num_regen[b:b + 1].contiguous(), tin[b:b + 1].contiguous(), C)
        assert torch.equal(pred[b:b + 1], want_pred), (b, int((pred[b:b + 1] != want_pred).sum()))
        assert torch.equal(out[b:b + 1], want_out), b
    assert torch.equal(pred[~regen.to(DEV)], tin[~regen.to(DEV)])                                  # known slots kept
    return pred, out


ROWS3 = [(1.5, 0.8, 0.43, 4.5, conf_weight(3, 7), 3), (0.0, 1.25, 0.71, 8.2, conf_weight(0, 5), 0), (7.1, 0.55, 0.12, 2.0, conf_weight(10, 12), 10)]


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("C", [40, 64, 128, 256, 512, 1024, 2048, 4096])
def test_requests_step_equals_three_single_sample_seeded_steps(C, guided):
    """B = 3, n = 16, m = 2 (P = 32: 96 rows, six workgroups), one C per CPL instantiation and 40 for the ragged tail; 32 / 17 / 5 masked slots among
    known tokens and a different num_regen per sample; every sample has its own scale (one of them 0), temperature, step, randomize temperature,
    conf weight and ratio."""
    pred, out = check_step_against_single_sample_seeded_steps(16, 2, C, guided, [32, 17, 5], ROWS3, [2 ** 64 - 1, 0, 2 ** 63 + 5])
    assert int(pred.max()) < C and int(pred.min()) >= 0
    assert (out == C).sum(dim=(1, 2)).tolist() == [13, 14, 1]                                      # floor32(ratio_b * num_regen_b): 0.43 * 32, 0.71 * 20, 0.12 * 11


def test_requests_step_at_1024_slots():
    """n = 512, m = 2 (P = 1024: the 1024-thread threshold block), C = 64, B = 2."""
    check_step_against_single_sample_seeded_steps(512, 2, 64, True, [1024, 300], ROWS3[:2], [7, 2 ** 64 - 9])


# ---- 2. the run --------------------------------------------------------------------------------------------------------------------------------
def run_steps(gm, tm, reqs, guided=None, init=None):
    """-> (images in request order or None, [per request: its step tokens stacked [N_b, n, m]])."""
    from maskbit_amd.sampling import request_steps, run_requests
    img, _, st, pos = run_requests(gm, tm, list(reqs), guided, init, want_image=tm is not None)
    return img, [torch.stack(s) for s in request_steps(list(reqs), st, pos)]


@functools.lru_cache(maxsize=None)
def five_alone():
    """Each of the five requests run alone, guided: the reference of the independence tests, computed once."""
    gm, tm = tiny_models()
    out = []
    for r in five_requests():
        img, (st,) = run_steps(gm, tm, [r], guided=True)
        out.append((img[0].clone(), st.clone()))
    return out


@pytest.mark.parametrize("scale", [7.1, 0.0])
def test_uniform_requests_equal_sample_seeded(scale):
    """The two cases where both entries run the same forwards: annealing "none" at scale 7.1 (every step guided) and scale 0 (none)."""
    from maskbit_amd import SampleRequest, sample_requests, sample_seeded
    gm, tm = tiny_models()
    seeds, y = [5, 2 ** 64 - 1, 2 ** 63 + 17], [1, 4, 8]
    kw = dict(KW, guidance_scale=scale, guidance_annealing="none")
    want_img, want_steps = sample_seeded(gm, tm, seeds, torch.tensor(y, device=DEV), **kw)
    img, steps = sample_requests(gm, tm, [SampleRequest(seed=s, label=l, **kw) for s, l in zip(seeds, y)])
    assert img.dtype == torch.float32 and torch.equal(img, want_img)
    assert [len(s) for s in steps] == [8, 8, 8]
    for b in range(3):
        for i in range(8):
            assert torch.equal(steps[b][i], want_steps[i][b]), (b, i)
    u8, _ = sample_requests(gm, tm, [SampleRequest(seed=s, label=l, **kw) for s, l in zip(seeds, y)], return_uint8=True)
    from oracle import maskbit_oracle as O
    assert u8.dtype == torch.uint8 and torch.equal(u8.cpu(), O.to_uint8_nhwc(want_img.cpu()))


def test_a_request_does_not_depend_on_its_batch():
    """Five requests with N = (8, 3, 5, 8, 1) that differ in scale, temperature, annealing, schedule and randomize temperature -- one with scale 0.0,
    one with cosine annealing, whose first step has scale 0 --: together, permuted, and scattered in a batch of 35, each equals itself alone (guided)."""
    from maskbit_amd import SampleRequest
    from maskbit_amd.sampling import build_request_plan
    gm, tm = tiny_models()
    reqs, alone = five_requests(), five_alone()
    assert [r.num_steps for r in reqs] == [8, 3, 5, 8, 1] and reqs[1].guidance_scale == 0.0
    assert float(build_request_plan(reqs[:1])[2].view(torch.float32)[0, 0, 0]) == 0.0               # the cosine request's first scale

    def check(batch, where):
        img, steps = run_steps(gm, tm, batch, guided=True)
        for j, (want_img, want_st) in zip(where, alone):
            assert torch.equal(steps[j], want_st), (j, [int((a != b).sum()) for a, b in zip(steps[j], want_st)])
            assert torch.equal(img[j], want_img), j
    check(reqs, range(5))
    perm = [3, 0, 4, 2, 1]
    inv = [perm.index(b) for b in range(5)]
    check([reqs[b] for b in perm], inv)
    where = [0, 7, 16, 17, 34]
    big = [SampleRequest(seed=100000 + j, label=j % 10, num_steps=(2, 4, 1, 6)[j % 4], guidance_scale=(3.0, 0.0, 5.5)[j % 3], softmax_temperature=0.9 + 0.01 * j,
                         randomize_temperature=1.0 + 0.25 * j) for j in range(35)]
    for j, r in zip(where, reqs):
        big[j] = r
    check(big, where)
    assert not torch.equal(alone[0][1], alone[3][1])                                                # (the two 8-step requests are different runs)
    # ... and `guided` is part of what a request's result depends on: the scale-0 request run unguided takes the plain forward
    _, (plain,) = run_steps(gm, None, [reqs[1]], guided=None)
    assert plain.shape == alone[1][1].shape and int(plain[-1].max()) < MASK


def test_only_the_active_prefix_is_written_and_bad_batches_are_refused():
    """Through the C entry: step_tokens pre-filled with a sentinel keeps it at every inactive (t, position) and holds a token in [0, C) at every active
    one.  Then the refusals that need a handle: 2 B (guided) or B sequences beyond the engine's, in front of every launch."""
    from maskbit_amd import _lib
    from maskbit_amd.sampling import build_request_plan
    lib = _lib.load()
    gm, _ = tiny_models()
    reqs = five_requests()
    order, active, table = build_request_plan(reqs)
    B, S, SENTINEL = 5, 8, -7
    labels = torch.tensor([reqs[b].label for b in order], device=DEV)
    seeds = dev_seeds([reqs[b].seed for b in order])
    table_dev = table.to(DEV)
    steps = torch.full((S, B, 256, 2), SENTINEL, dtype=torch.int64, device=DEV)
    codes = torch.empty((B, 256), dtype=torch.int64, device=DEV)
    arr = (ctypes.c_int * S)(*active)
    plan = _lib.RequestPlan(S, 1, arr, table_dev.data_ptr())
    hgen = gm.engine(2 * B)
    with torch.cuda.device(DEV):
        _lib.check(lib.mb_sample_requests(hgen, None, ctypes.byref(plan), labels.data_ptr(), B, None, seeds.data_ptr(), steps.data_ptr(), codes.data_ptr(),
                                          None, None, stream()), "mb_sample_requests")
    is_active = torch.tensor([[p < active[t] for p in range(B)] for t in range(S)], device=DEV)
    assert bool((steps[~is_active] == SENTINEL).all())
    assert int(steps[is_active].min()) >= 0 and int(steps[is_active].max()) < MASK
    alone = five_alone()
    for p, b in enumerate(order):
        assert torch.equal(steps[S - reqs[b].num_steps:, p], alone[b][1]), b
    from oracle import maskbit_oracle as O
    assert torch.equal(codes.cpu(), O.combine_groups(steps[-1].cpu(), 12, 2).long())
    big = 1 << 20
    one = (ctypes.c_int * 1)(big)
    _lib.prof_enable(True)
    try:
        for guided, need in ((1, 2 * big), (0, big)):
            plan = _lib.RequestPlan(1, guided, one, table_dev.data_ptr())
            rc = lib.mb_sample_requests(hgen, None, ctypes.byref(plan), labels.data_ptr(), big, None, seeds.data_ptr(), None, None, None, None, stream())
            assert rc < 0 and f"B={big} needs {need} sequences, engine holds" in lib.mb_last_error().decode()
        plan = _lib.RequestPlan(S, 1, arr, table_dev.data_ptr())
        rc = lib.mb_sample_requests(hgen, None, ctypes.byref(plan), labels.data_ptr(), B, None, seeds.data_ptr(), None, None, codes.data_ptr(), None, stream())
        assert rc < 0 and "image requested without a decoder" in lib.mb_last_error().decode()
        assert _lib.prof_read() == {}                                                               # refused in front of every launch
    finally:
        _lib.prof_enable(False)


def test_requests_from_their_own_token_maps_equal_sample_from_tokens():
    """init_tokens with 512 / 100 / 7 masked slots and N = (4, 2, 4) -- the sorted order (0, 2, 1) differs from the request order --: each request
    equals sample_from_tokens(seeds=) of its own map alone, with guidance_annealing "none" (every step guided in both)."""
    from maskbit_amd import SampleRequest, sample_from_tokens, sample_requests
    gm, tm = tiny_models()
    init, regen = tokens_with_masks([512, 100, 7], seed=31)
    base = dict(KW, guidance_annealing="none")
    reqs = [SampleRequest(seed=21, label=1, **dict(base, num_steps=4)),
            SampleRequest(seed=2 ** 63 + 1, label=4, **dict(base, num_steps=2, guidance_scale=2.0, softmax_temperature=0.8)),
            SampleRequest(seed=2 ** 64 - 1, label=8, **dict(base, num_steps=4, randomize_temperature=3.0, mask_schedule_strategy="linear"))]
    for tokens in (init, init.to(DEV)):                                                             # host- and device-resident maps
        img, steps = sample_requests(gm, tm, reqs, init_tokens=tokens)
        for b, r in enumerate(reqs):
            kw = {k: v for k, v in dataclasses.asdict(r).items() if k not in ("seed", "label")}
            want_img, want_steps = sample_from_tokens(gm, tm, init[b:b + 1], torch.tensor([r.label]), seeds=[r.seed], **kw)
            assert len(steps[b]) == r.num_steps and torch.equal(torch.stack(steps[b]), torch.stack(want_steps)[:, 0]), b
            assert torch.equal(img[b], want_img[0]), b
            keep = ~regen[b].to(DEV)
            assert torch.equal(torch.stack(steps[b])[:, keep], init[b].to(DEV)[keep].expand(r.num_steps, -1))   # known slots come back in every step


def test_a_request_does_not_depend_on_its_batch_full_size_12_bit():
    """BASELINE's 12-bit generator at the product default precision, B = 3, N = (3, 2, 1), guided: forwards at 1, 2 and 3 pairs; each request equals
    itself alone."""
    from hip_helpers import hip_generator
    from maskbit_amd import SampleRequest
    from oracle import maskbit_oracle as O
    cfg = O.GenCfg(bits=12, splits=2)
    gm = hip_generator(cfg, O.make_generator_weights(cfg, seed=100, head_gain=12.0))
    gm.precision = -1
    assert gm.resolved_precision() == 2
    reqs = [SampleRequest(seed=2 ** 64 - 1, label=3, num_steps=3, guidance_scale=7.1, randomize_temperature=8.2, mask_schedule_strategy="arccos"),
            SampleRequest(seed=42, label=980, num_steps=2, guidance_scale=0.0, softmax_temperature=0.9),
            SampleRequest(seed=2 ** 63, label=417, num_steps=1, guidance_scale=3.0, guidance_annealing="linear")]
    from maskbit_amd.sampling import build_request_plan
    assert build_request_plan(reqs)[1] == [1, 2, 3]
    _, base = run_steps(gm, None, reqs, guided=True)
    for b, r in enumerate(reqs):
        _, (st,) = run_steps(gm, None, [r], guided=True)
        assert torch.equal(st, base[b]), b
    assert gm.saturation_count() == 0


def test_sample_requests_consumes_no_torch_generator():
    from maskbit_amd import sample_requests
    gm, tm = tiny_models()
    reqs = five_requests()[1:3]
    torch.manual_seed(123)
    cpu, dev = torch.get_rng_state(), torch.cuda.get_rng_state()
    a, _ = sample_requests(gm, tm, reqs)
    assert torch.equal(torch.get_rng_state(), cpu) and torch.equal(torch.cuda.get_rng_state(), dev)
    torch.manual_seed(456)                                                                         # ... and none enters the result
    b, _ = sample_requests(gm, tm, reqs)
    assert torch.equal(a, b)
