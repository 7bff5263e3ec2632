"""GPU tests of per-sample seeded sampling (include/maskbit_hip.h "per-sample seeded sampling").

The chain of evidence: (1) the noise the device generates, dumped by ``mb_seeded_noise`` from the step kernel's own device function, equals the
numpy restatement of the header's definition (tests/seeded_reference.py) -- uniforms exactly, the logarithms within the bound of the number format;
(2) the fused step equals the explicit-noise step fed those dumped tensors, bit for bit -- so everything the existing suites establish for the
explicit step holds for the seeded one; (3) the whole seeded run equals the explicit edit run fed every step's dumped noise; (4) a sample's tokens
do not depend on its batch; (5)-(8) the public entries built on it.  Bounds are derived where they are used; none comes from what the kernels give."""
import ctypes

import numpy as np
import pytest
import torch

import seeded_reference as S
from test_hip_edit import MASK, inpaint_case, step_edit, tiny_models, tokens_with_masks
from test_seeded_cpu import CHI2_999_63, chi_square, race_probabilities

pytestmark = pytest.mark.gpu

DEV = "cuda"
C_LIST = [32, 40, 64, 128, 512, 1024, 4096]
EDGE_SEEDS = [0, 2 ** 63, 2 ** 64 - 1]
KW = dict(softmax_temperature=1.0, randomize_temperature=8.2, mask_schedule_strategy="arccos", num_steps=8, guidance_scale=7.1,
          guidance_annealing="cosine", use_sampling_annealing=False, scale_pow=3.0)


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev_seeds(seeds):
    from maskbit_amd.sampling import check_seeds
    return check_seeds(list(seeds), len(seeds)).to(DEV)


def conf_weight(i, N):
    """float32(1 - (i + 1) / N), as the host hands it over."""
    return ctypes.c_float(1 - (i + 1) / N).value


def dump_noise(lib, seeds, step, rt, w, P, C):
    """mb_seeded_noise -> (exp_u [B*P, C], exp_noise [B*P, C], conf_u [B*P], conf_noise [B*P]) on the device."""
    from maskbit_amd import _lib
    B = seeds.shape[0]
    eu, e = torch.empty(B * P, C, device=DEV), torch.empty(B * P, C, device=DEV)
    cu, c = torch.empty(B * P, device=DEV), torch.empty(B * P, device=DEV)
    _lib.check(lib.mb_seeded_noise(seeds.data_ptr(), step, rt, w, eu.data_ptr(), e.data_ptr(), cu.data_ptr(), c.data_ptr(), B, P, C, stream()), "mb_seeded_noise")
    return eu, e, cu, c


def step_seeded(lib, lc, lu, scale, temp, seeds, step, rt, w, ratio, num_regen, tin, C):
    """One mb_sample_step_seeded call on device tensors -> (pred, tokens_out)."""
    from maskbit_amd import _lib
    B, n, m = tin.shape
    tout, pred = torch.empty_like(tin), torch.empty_like(tin)
    _lib.check(lib.mb_sample_step_seeded(lc.data_ptr(), lu.data_ptr() if lu is not None else None, scale, temp, seeds.data_ptr(), step, rt, w, ratio,
                                         num_regen.data_ptr(), tin.data_ptr(), tout.data_ptr(), pred.data_ptr(), B, n, m, C, stream()), "mb_sample_step_seeded")
    return pred, tout


def ulp32(x):
    """Spacing of float32 at |x| (x float64)."""
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


# ---- 1. the generated noise against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [0, 5])
@pytest.mark.parametrize("C", C_LIST)
def test_generated_noise_equals_the_restatement(C, step):
    """B = 3 (seeds 0, 2^63, 2^64 - 1), P = 16.  Uniforms: exactly equal.  exp_noise against float64 -log(u): 4 ulp (3 for logf, OpenCL's bound, + 1
    for the rounding of the comparison's own reference).  conf_noise at randomize_temperature = conf_weight = 1 (both products exact) against float64
    g = -log(-log(u)): the inner logarithm returns q(1 + d) with |d| <= 3 * 2^-23 (3 ulp of q, an ulp being at most 2^-23 relative); the outer one
    sees log(q) + log(1 + d), an ABSOLUTE shift of at most |d| (1 + |d|), and adds its own 3 ulp of g; + 1 ulp of g for the comparison:
    |got - g| <= 3 * 2^-23 (1 + 2^-20) + 4 ulp(g)."""
    from maskbit_amd import _lib
    lib = _lib.load()
    P = 16
    eu, e, cu, c = dump_noise(lib, dev_seeds(EDGE_SEEDS), step, 1.0, 1.0, P, C)
    want_eu, want_cu = S.exp_uniforms(EDGE_SEEDS, step, P, C), S.conf_uniforms(EDGE_SEEDS, step, P)
    assert np.array_equal(eu.cpu().numpy().reshape(3, P, C), want_eu)
    assert np.array_equal(cu.cpu().numpy().reshape(3, P), want_cu)
    q = S.exp_noise64(want_eu)
    err = np.abs(e.cpu().numpy().reshape(3, P, C).astype(np.float64) - q) / ulp32(q)
    g = S.gumbel64(want_cu)
    gerr = np.abs(c.cpu().numpy().reshape(3, P).astype(np.float64) - g)
    gbound = 3 * 2.0 ** -23 * (1 + 2.0 ** -20) + 4 * ulp32(g)
    print(f"C {C} step {step}: exp_noise max {err.max():.2f} ulp; conf_noise max error / bound {np.max(gerr / gbound):.3f}")
    assert err.max() <= 4.0
    assert np.all(gerr <= gbound)
    assert float(e.min()) > 0.0                                                                    # q is never 0: the race never divides by it


def test_noise_scaling_is_two_roundings_in_the_reference_order():
    """(g * randomize_temperature) * w with both products rounded to float32, from the g the device itself computed at 1, 1."""
    from maskbit_amd import _lib
    lib = _lib.load()
    seeds = dev_seeds([7, 8])
    rt, w = 8.2, conf_weight(2, 7)
    g = dump_noise(lib, seeds, 4, 1.0, 1.0, 512, 4)[3]
    got = dump_noise(lib, seeds, 4, rt, w, 512, 4)[3]
    want = (g.cpu().numpy() * np.float32(rt)).astype(np.float32) * np.float32(w)
    assert np.array_equal(got.cpu().numpy(), want.astype(np.float32))
    assert torch.equal(dump_noise(lib, seeds, 4, rt, 0.0, 512, 4)[3].abs(), torch.zeros(1024, device=DEV))    # the last step's weight is 0


# ---- 2. the fused step against the explicit step fed the dumped noise ------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("C", C_LIST)
def test_seeded_step_equals_the_explicit_step_on_the_dumped_noise(C, guided):
    """n = 20, m = 2 (P = 40: 160 rows, ten workgroups, the last rows of a sample and the first of the next in one workgroup), B = 4 with 40 / 17 /
    3 / 1 masked slots among known tokens, step 3 of 7: tokens_out and pred_out of mb_sample_step_seeded equal mb_sample_step_edit's on the tensors
    mb_seeded_noise wrote, bit for bit."""
    from maskbit_amd import _lib
    from test_edit_cpu import random_slot_masks
    lib = _lib.load()
    M, n, m, step, N = [40, 17, 3, 1], 20, 2, 3, 7
    B, P = len(M), n * m
    g = torch.Generator().manual_seed(1000 + C)
    regen = random_slot_masks(M, P, seed=C).reshape(B, n, m)
    known = torch.randint(0, C, (B, n, m), generator=g)
    tin = torch.where(regen, torch.full_like(known, C), known).to(DEV)
    lc = (3.0 * torch.randn(B, n, m, C, generator=g)).to(DEV)
    lu = (3.0 * torch.randn(B, n, m, C, generator=g)).to(DEV) if guided else None
    num_regen = torch.tensor(M, dtype=torch.int32, device=DEV)
    seeds = dev_seeds([2 ** 64 - 1, 0, 2 ** 63, 123456789012345])
    rt, w, ratio = 4.5, conf_weight(step, N), 0.43
    _, e, _, c = dump_noise(lib, seeds, step, rt, w, P, C)
    want_pred, want_out = step_edit(lib, lc, lu, 1.5, 0.8, e, c, ratio, num_regen, tin, C=C)
    pred, out = step_seeded(lib, lc, lu, 1.5, 0.8, seeds, step, rt, w, ratio, num_regen, tin, C)
    assert torch.equal(pred, want_pred), f"pred differs at {int((pred != want_pred).sum())} slots"
    assert torch.equal(out, want_out)
    assert torch.equal(pred[~regen.to(DEV)], tin[~regen.to(DEV)])                                  # known slots kept
    assert (out == C).sum(dim=(1, 2)).tolist() == [17, 7, 1, 0]                                    # floor32(0.43 M_b) re-masked; nothing at nm = 1
    other, _ = step_seeded(lib, lc, lu, 1.5, 0.8, seeds, step + 1, rt, w, ratio, num_regen, tin, C)
    assert not torch.equal(other, pred)                                                            # (the step index enters the noise)


# ---- 3. the whole run -------------------------------------------------------------------------------------------------------------------------
def all_step_noise(lib, seeds, N, rt, P, C):
    qs, cs = zip(*[dump_noise(lib, seeds, i, rt, conf_weight(i, N), P, C)[1::2] for i in range(N)])
    return torch.stack(qs), torch.stack(cs)


def test_seeded_run_equals_the_edit_run_on_the_dumped_noise_and_step_chunks():
    """Tiny generator, guidance 7.1 with cosine annealing (zero-scale first step), 8 arccos steps, B = 3: sample_seeded equals run_loop's edit path
    from an all-masked map fed every step's dumped noise -- every step's tokens and the image, bit for bit; the run in step chunks (both token-buffer
    parities) equals the whole run; a seeded chunk does not continue an edit run, nor the other way round."""
    from maskbit_amd import _lib, sample_seeded
    from maskbit_amd.sampling import build_edit_plan, check_seeds, run_loop, run_seeded, seeded_plan
    lib = _lib.load()
    gm, tm = tiny_models()
    seeds = [5, 2 ** 64 - 1, 2 ** 63 + 17]
    y = torch.tensor([1, 4, 8], device=DEV)
    B, N = 3, 8
    img, steps = sample_seeded(gm, tm, seeds, y, **KW)
    assert isinstance(steps, list) and len(steps) == N and img.shape == (B, 3, 64, 64) and img.dtype == torch.float32
    steps = torch.stack(steps)
    q, c = all_step_noise(lib, dev_seeds(seeds), N, KW["randomize_temperature"], 512, MASK)
    eplan = build_edit_plan(N, 7.1, "cosine", 3.0, 1.0, False, "arccos")
    assert eplan[0][0] == 0.0 and eplan[0][1] != 0.0
    full = torch.full((B, 256, 2), MASK, dtype=torch.int64, device=DEV)
    img_e, u8_e, steps_e, codes_e = run_loop(gm, tm, y, eplan, q, c.reshape(N, B, 256, 2), want_u8=True, init_tokens=full)
    assert torch.equal(steps, steps_e), [int((a != b).sum()) for a, b in zip(steps, steps_e)]
    assert torch.equal(img, img_e)
    assert int(steps[-1].max()) < MASK and int(steps.min()) >= 0
    splan, sd = seeded_plan(N, 7.1, "cosine", 3.0, 1.0, False, "arccos"), check_seeds(seeds, B)
    parts = []
    for (b0, b1) in ((0, 3), (3, 4), (4, 8)):
        img_c, u8_c, st, codes_c = run_seeded(gm, tm, y, splan, sd, KW["randomize_temperature"], want_u8=True, step_range=(b0, b1))
        parts.append(st)
    assert torch.equal(torch.cat(parts), steps) and torch.equal(img_c, img) and torch.equal(u8_c, u8_e) and torch.equal(codes_c, codes_e)
    run_seeded(gm, tm, y, splan, sd, 8.2, want_image=False, step_range=(0, 3))
    with pytest.raises(RuntimeError, match="does not continue"):
        run_loop(gm, tm, y, eplan, q[3:4], c[3:4].reshape(1, B, 256, 2), want_image=False, step_range=(3, 4), init_tokens=full)
    run_loop(gm, tm, y, eplan, q[0:3], c[0:3].reshape(3, B, 256, 2), want_image=False, step_range=(0, 3), init_tokens=full)
    with pytest.raises(RuntimeError, match="does not continue"):
        run_seeded(gm, tm, y, splan, sd, 8.2, want_image=False, step_range=(3, 4))


def test_a_chunk_continues_a_run_of_its_own_kind_only():
    """Tiny generator, B = 2, 4 guided steps, the three kinds of run -- plain (mb_sample), edit (mb_sample_edit, mixed masks), seeded (mb_sample_seeded)
    -- with the same batch, plan length and guidance flag, so that the kind alone tells them apart.  After steps [0, 3) of one kind, step [3, 4) of
    each other kind is refused (an argument refusal: nothing is launched); after the refusal a fresh [0, 3) + [3, 4) of the first kind equals its
    unchunked run, bit for bit."""
    from maskbit_amd import _lib
    from maskbit_amd.sampling import build_edit_plan, build_plan, check_seeds, run_loop, run_seeded, seeded_plan
    from test_hip_edit import dev_noise
    gm, tm = tiny_models()
    B, N, rt = 2, 4, 8.2
    y = torch.tensor([3, 7], device=DEV)
    sched = (7.1, "cosine", 3.0, 1.0, False, "arccos")
    plans = {"plain": build_plan(N, 512, *sched), "edit": build_edit_plan(N, *sched), "seeded": seeded_plan(N, *sched)}
    assert all(p[0] == plans["plain"][0] and p.use_cfg for p in plans.values())
    q, c = dev_noise(23, B, N, rt)
    init = tokens_with_masks([512, 100], seed=13)[0].to(DEV)
    sd = check_seeds([11, 2 ** 64 - 3], B)

    def run(kind, step_range):
        b0, b1 = step_range or (0, N)
        if kind == "seeded":
            return run_seeded(gm, tm, y, plans[kind], sd, rt, want_u8=True, step_range=step_range)
        return run_loop(gm, tm, y, plans[kind], q[b0:b1], c[b0:b1], want_u8=True, step_range=step_range, init_tokens=init if kind == "edit" else None)
    whole = {kind: run(kind, None) for kind in plans}
    assert not torch.equal(whole["plain"][2], whole["edit"][2]) and not torch.equal(whole["edit"][2], whole["seeded"][2])   # three different runs
    for first in plans:
        for other in plans:
            if other == first:
                continue
            run(first, (0, 3))
            _lib.prof_enable(True)
            try:
                with pytest.raises(RuntimeError, match=f"of a 4-step {other} run with B = 2 does not continue the run in progress .*{first} run"):
                    run(other, (3, 4))
                assert _lib.prof_read() == {}, (first, other)                                      # refused in front of every launch
            finally:
                _lib.prof_enable(False)
            _, _, st03, _ = run(first, (0, 3))                                                     # (a rejected chunk ends the run: start again)
            img, u8, st34, codes = run(first, (3, 4))
            ref = whole[first]
            assert torch.equal(torch.cat([st03, st34]), ref[2]), (first, other)
            assert torch.equal(img, ref[0]) and torch.equal(u8, ref[1]) and torch.equal(codes, ref[3]), (first, other)


# ---- 4. a sample does not depend on its batch -------------------------------------------------------------------------------------------------
def seeded_steps(gm, seeds, y, plan, rt=8.2):
    from maskbit_amd.sampling import check_seeds, run_seeded
    return run_seeded(gm, None, y.to(DEV), plan, check_seeds(list(seeds), len(seeds)), rt, want_image=False)[2]


def test_a_sample_does_not_depend_on_its_batch_tiny():
    """Per-sample step tokens of five seeds: alone, permuted, and embedded at scattered positions of a batch of 35."""
    from maskbit_amd.sampling import seeded_plan
    gm, _ = tiny_models()
    plan = seeded_plan(8, 7.1, "cosine", 3.0, 1.0, False, "arccos")
    seeds, y = [11, 2 ** 64 - 3, 2 ** 63, 0, 999], torch.tensor([1, 4, 8, 0, 9])
    base = seeded_steps(gm, seeds, y, plan)                                                        # [8, 5, 256, 2]
    for b in range(5):
        assert torch.equal(seeded_steps(gm, seeds[b:b + 1], y[b:b + 1], plan)[:, 0], base[:, b]), b
    perm = [3, 0, 4, 2, 1]
    assert torch.equal(seeded_steps(gm, [seeds[i] for i in perm], y[perm], plan), base[:, perm])
    where = [0, 7, 16, 17, 34]
    big_seeds, big_y = [100000 + j for j in range(35)], torch.arange(35) % 10
    for j, b in zip(where, range(5)):
        big_seeds[j], big_y[j] = seeds[b], y[b]
    assert torch.equal(seeded_steps(gm, big_seeds, big_y, plan)[:, where], base)
    assert not torch.equal(base[:, 0], base[:, 1])
    assert not torch.equal(seeded_steps(gm, [12], y[:1], plan)[:, 0], base[:, 0])                 # another seed under the same label: other tokens


def test_a_sample_does_not_depend_on_its_batch_full_size_12_bit():
    """BASELINE's 12-bit generator at the product default precision, guidance on, 3 steps: B = 3 against each sample at B = 1."""
    from hip_helpers import hip_generator
    from maskbit_amd.sampling import seeded_plan
    from oracle import maskbit_oracle as O
    cfg = O.GenCfg(bits=12, splits=2)
    gm = hip_generator(cfg, O.make_generator_weights(cfg, seed=100, head_gain=12.0))
    gm.precision = -1
    assert gm.resolved_precision() == 2
    plan = seeded_plan(3, 7.1, "none", 3.0, 1.0, False, "arccos")
    seeds, y = [2 ** 64 - 1, 42, 2 ** 63], torch.tensor([3, 980, 417])
    base = seeded_steps(gm, seeds, y, plan)
    for b in range(3):
        assert torch.equal(seeded_steps(gm, seeds[b:b + 1], y[b:b + 1], plan)[:, 0], base[:, b]), b
    assert gm.saturation_count() == 0


# ---- 5. the run-level entries ----------------------------------------------------------------------------------------------------------------
def test_generate_uint8_seeded_does_not_depend_on_the_batch_size():
    from maskbit_amd import generate_uint8, sample_seeded
    gm, tm = tiny_models()
    labels = torch.tensor([1, 4, 8, 0, 9, 3])
    seed = 2 ** 64 - 2                                                                             # (seed + j) mod 2^64 wraps inside the run
    by2 = np.concatenate(list(generate_uint8(gm, tm, labels, 2, seed=seed, **KW)))
    by3 = list(generate_uint8(gm, tm, labels, 3, seed=seed, return_codes=True, **KW))
    assert by2.shape == (6, 64, 64, 3) and by2.dtype == np.uint8
    assert np.array_equal(by2, np.concatenate([b[0] for b in by3]))
    # image 4 of the run, regenerated alone
    img, _ = sample_seeded(gm, tm, [(seed + 4) % 2 ** 64], labels[4:5], **KW)
    from oracle import maskbit_oracle as O
    assert np.array_equal(O.to_uint8_nhwc(img.cpu()).numpy()[0], by2[4])


def test_sample_sharded_seeded_is_identical_for_any_world_size(monkeypatch):
    """One process plays the ranks of a world of two (shards [0:3] and [3:5] of five samples) and rank 6 of a world of eight (an empty shard);
    the gather is replaced by the identity.  The shards concatenated equal the single-rank run of the five."""
    import torch.distributed as dist
    from maskbit_amd import parallel
    gm, tm = tiny_models()
    labels, seeds = torch.tensor([1, 4, 8, 0, 9]), [3, 2 ** 63, 77, 2 ** 64 - 1, 5]
    kw = dict(noise="seeded", seeds=seeds, num_steps=8, randomize_temperature=8.2)
    whole = parallel.sample_sharded(gm, tm, labels, **kw)
    assert whole.shape == (5, 64, 64, 3) and whole.dtype == torch.uint8
    rank = {"r": 0, "w": 2}
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: rank["r"])
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: rank["w"])
    monkeypatch.setattr(parallel, "gather_images", lambda local, group=None, equal=None: local)
    shards = []
    for r in (0, 1):
        rank["r"] = r
        shards.append(parallel.sample_sharded(gm, tm, labels, **kw))
    assert [s.shape[0] for s in shards] == [3, 2] and torch.equal(torch.cat(shards), whole)
    rank["r"], rank["w"] = 6, 8
    assert parallel.sample_sharded(gm, tm, labels, **kw).shape == (0, 64, 64, 3)


# ---- 6. no generator is consumed -------------------------------------------------------------------------------------------------------------
def test_sample_seeded_consumes_no_torch_generator():
    from maskbit_amd import sample_seeded
    gm, tm = tiny_models()
    torch.manual_seed(123)
    cpu, dev = torch.get_rng_state(), torch.cuda.get_rng_state()
    a, _ = sample_seeded(gm, tm, [1, 2], torch.tensor([3, 7], device=DEV), **KW)
    assert torch.equal(torch.get_rng_state(), cpu) and torch.equal(torch.cuda.get_rng_state(), dev)
    torch.manual_seed(456)                                                                         # ... and none enters the result
    b, _ = sample_seeded(gm, tm, torch.tensor([1, 2]), torch.tensor([3, 7]), **KW)
    assert torch.equal(a, b)


# ---- 7. the distribution on the device ---------------------------------------------------------------------------------------------------------
def test_device_race_picks_follow_the_softmax():
    """One mb_sample_step_seeded over B = 32, P = 512, C = 64, every slot masked, one logit row broadcast: 16 384 draws.  Chi-square of the pred counts
    against the float64 softmax below chi2.ppf(0.999, 63); the seeds (1000 .. 1031, step 2) are ones for which the CPU restatement is within it."""
    from maskbit_amd import _lib
    lib = _lib.load()
    B, n, m, C, step = 32, 256, 2, 64, 2
    seeds = list(range(1000, 1000 + B))
    row = torch.from_numpy(np.log(race_probabilities(C))).float()
    p = torch.softmax(row.double(), 0).numpy()
    R = B * n * m
    assert R * p.min() >= 2.0
    chi_ref = chi_square(S.race_picks(seeds, step, n * m, p), p, R)
    lc = row.to(DEV).expand(B, n, m, C).contiguous()
    tin = torch.full((B, n, m), C, dtype=torch.int64, device=DEV)
    num_regen = torch.full((B,), n * m, dtype=torch.int32, device=DEV)
    pred, out = step_seeded(lib, lc, None, 0.0, 1.0, dev_seeds(seeds), step, 4.5, 0.5, 0.5, num_regen, tin, C)
    chi_dev = chi_square(pred.cpu().numpy(), p, R)
    print(f"chi-square: device {chi_dev:.2f}, restatement {chi_ref:.2f} (bound {CHI2_999_63})")
    assert chi_ref < CHI2_999_63
    assert chi_dev < CHI2_999_63
    assert (out == C).sum(dim=(1, 2)).tolist() == [256] * B                                        # floor(0.5 * 512) re-masked per sample


# ---- 8. editing with seeds --------------------------------------------------------------------------------------------------------------------
def test_inpaint_and_sample_from_tokens_with_seeds():
    """Everything regenerated: inpaint(seeds=) and sample_from_tokens(seeds=) equal sample_seeded.  A partial mask: the kept cells carry the encoder's
    codes, the result does not depend on the batch the image is edited in, and torch's generators are not consumed."""
    from maskbit_amd import inpaint, sample_from_tokens, sample_seeded
    from oracle import maskbit_oracle as O
    from test_edit_cpu import token_mask_ref
    gm, tm = tiny_models()
    images, mask, y = inpaint_case()
    seeds = [21, 2 ** 63 + 1, 2 ** 64 - 1, 4]
    want, steps = sample_seeded(gm, tm, seeds[:2], y[:2], **KW)
    kw = {k: v for k, v in KW.items() if k not in ("softmax_temperature", "use_sampling_annealing")}
    got, codes, tmask = inpaint(gm, tm, images[:2].to(DEV), torch.ones(2, 64, 64, dtype=torch.bool), y[:2], keep_known_pixels=False, seeds=seeds[:2], **kw)
    assert torch.equal(got, want) and bool(tmask.all())
    assert torch.equal(codes.cpu(), O.combine_groups(steps[-1].cpu(), 12, 2).long())
    img2, steps2 = sample_from_tokens(gm, tm, torch.full((2, 256, 2), MASK, dtype=torch.int64), y[:2], seeds=seeds[:2], **KW)
    assert torch.equal(img2, want) and all(torch.equal(a, b) for a, b in zip(steps, steps2))
    # partial masks (a rectangle, one pixel, nothing, everything)
    torch.manual_seed(3)
    cpu, dev = torch.get_rng_state(), torch.cuda.get_rng_state()
    img, codes, tmask = inpaint(gm, tm, images.to(DEV), mask.to(DEV), y, seeds=seeds, **kw)
    assert torch.equal(torch.get_rng_state(), cpu) and torch.equal(torch.cuda.get_rng_state(), dev)
    want_tmask = token_mask_ref(mask, 4)
    assert torch.equal(tmask.cpu(), want_tmask)
    enc = tm.encode(images.to(DEV))[1]["min_encoding_indices"].reshape(4, 256)
    keep = ~want_tmask.reshape(4, 256)
    assert torch.equal(codes.cpu()[keep], enc.cpu()[keep])                                         # kept cells carry the encoder's codes
    assert int(codes.min()) >= 0 and int(codes.max()) < 4096
    outside = (~mask).unsqueeze(1).expand(-1, 3, -1, -1)
    assert torch.equal(img.cpu()[outside], images[outside])                                        # kept pixels: the input's bits
    assert torch.equal(img[2].cpu(), images[2]) and torch.equal(codes[2], enc[2])                  # the empty mask
    one, codes1, _ = inpaint(gm, tm, images[:1].to(DEV), mask[:1].to(DEV), y[:1], seeds=seeds[:1], **kw)
    assert torch.equal(one[0], img[0]) and torch.equal(codes1[0], codes[0])                        # sample 0 edited alone
    # known tokens come back in every step's prediction
    init, regen = tokens_with_masks([512, 200, 37, 0], seed=9)
    _, st = sample_from_tokens(gm, tm, init, y, seeds=seeds, **KW)
    st = torch.stack(st).cpu()
    assert torch.equal(st[:, ~regen], init[~regen].expand(8, -1)) and int(st[-1].max()) < MASK
