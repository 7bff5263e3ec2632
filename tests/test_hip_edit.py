"""GPU tests of masked-token image editing: the per-sample step kernel bit for bit against the oracle's step, the edit loop against the plain loop
(all-masked) and against forward + step composed on the host (mixed masks, step chunks), the invariants of a free run, teacher-forced token parity
of an edit run, and ``inpaint`` end to end.  Expected values come from tests/test_edit_cpu.py's restatements (the oracle's ``sample_step`` per
sample, ``max_pool2d``, ``torch.where``)."""
import functools

import pytest
import torch

from conftest import load_golden, golden_weights
from hip_helpers import hip_generator, hip_tokenizer
from oracle import maskbit_oracle as O
from test_edit_cpu import (TINY_GEN, TINY_TOK, composite_ref, edit_step_oracle, expected_masked_after, random_slot_masks, token_mask_ref)

pytestmark = pytest.mark.gpu

DEV = "cuda"
MASK = 64


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def tiny_weights():
    gsd = golden_weights(load_golden("gen_tiny.npz"))
    tsd = O.make_tokenizer_weights(TINY_TOK, seed=int(load_golden("tok_tiny.npz")["seed"]), with_encoder=True)
    return gsd, tsd


@functools.lru_cache(maxsize=None)
def tiny_models():
    gsd, tsd = tiny_weights()
    return hip_generator(TINY_GEN, gsd), hip_tokenizer(TINY_TOK, tsd)


def tokens_with_masks(sizes, seed, known=None):
    """int64 [B, 256, 2]: MASK at sizes[b] random slots of sample b, ``known`` (default: random tokens) everywhere else.  -> (tokens, regen bool)."""
    B = len(sizes)
    regen = random_slot_masks(sizes, 512, seed).reshape(B, 256, 2)
    if known is None:
        known = torch.randint(0, MASK, (B, 256, 2), generator=torch.Generator().manual_seed(seed + 1))
    return torch.where(regen, torch.full_like(known, MASK), known), regen


def step_edit(lib, lc, lu, scale, temp, q, cn, ratio, num_regen, tin, C=MASK):
    """One mb_sample_step_edit call on device tensors -> (pred, tokens_out)."""
    from maskbit_amd import _lib
    B, n, m = tin.shape
    tout, pred = torch.empty_like(tin), torch.empty_like(tin)
    _lib.check(lib.mb_sample_step_edit(lc.data_ptr(), lu.data_ptr() if lu is not None else None, scale, temp, q.data_ptr(), cn.data_ptr(), ratio,
                                       num_regen.data_ptr(), tin.data_ptr(), tout.data_ptr(), pred.data_ptr(), B, n, m, C, stream()), "mb_sample_step_edit")
    return pred, tout


def dev_noise(seed, B, steps, rt):
    """The reference's draws on a CPU model (per step exponential_ then Gumbel from one generator), on the device."""
    torch.manual_seed(seed)
    g = torch.distributions.Gumbel(0.0, 1.0)
    qs, cs = [], []
    for i in range(steps):
        qs.append(torch.empty(B * 512, 64).exponential_(1))
        cs.append(g.sample((B, 256, 2)) * rt * (1 - (i + 1) / steps))
    return torch.stack(qs).to(DEV), torch.stack(cs).to(DEV)


# ---- 1. the step kernel, bit for bit -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def recorded_run():
    """A guided eight-step CPU run of the tiny model, B = 6: the logits and the noise of every step."""
    gsd, _ = tiny_weights()
    y = torch.arange(6) % 10
    rec = []
    torch.manual_seed(21)
    O.sample_loop(lambda t, yy, dd: O.lfq_bert_forward(gsd, TINY_GEN, t, yy, dd), 6, y, num_steps=8, guidance_scale=7.1, guidance_annealing="cosine",
                  scale_pow=3.0, randomize_temperature=8.2, mask_schedule_strategy="arccos", mask_token=MASK, codebook_splits=2, record=rec)
    return rec


def test_edit_step_bit_exact_vs_oracle():
    """mb_sample_step_edit on the recorded logits and noise, from token states with 512 / 256 / 37 / 3 / 1 / 0 masked slots: pred and tokens_out equal
    the oracle's step run per sample as a batch of one with num_maskable = M_b (tokens_out = pred where nm_b <= 1).  The state follows the expected
    tokens_out, so M_b = 3 reaches nm = 1 in mid-run."""
    from maskbit_amd import _lib
    lib = _lib.load()
    M = [512, 256, 37, 3, 1, 0]
    tokens, regen = tokens_with_masks(M, seed=7)
    num_regen = torch.tensor(M, dtype=torch.int32, device=DEV)
    guard_seen = False
    for i, r in enumerate(recorded_run()):
        nm = (tokens == MASK).sum(dim=(1, 2)).tolist()
        guard_seen |= nm[3] == 1
        want_pred, want_out = edit_step_oracle(r.logits_c, r.logits_u, r.scale, 1.0, r.exp_noise, r.conf_noise, tokens, MASK, r.mask_ratio, M)
        pred, out = step_edit(lib, r.logits_c.to(DEV).contiguous(), r.logits_u.to(DEV).contiguous(), r.scale, 1.0, r.exp_noise.to(DEV).contiguous(),
                              r.conf_noise.to(DEV).contiguous(), r.mask_ratio, num_regen, tokens.to(DEV).contiguous())
        assert torch.equal(pred.cpu(), want_pred), f"step {i}: pred differs at {int((pred.cpu() != want_pred).sum())} positions"
        assert torch.equal(out.cpu(), want_out), f"step {i}: re-mask differs, masked counts {(out == MASK).sum(dim=(1, 2)).tolist()} from {nm}"
        assert torch.equal(want_out[~regen], tokens[~regen])                                   # (the expected values keep the known tokens)
        tokens = want_out
    assert guard_seen


def test_edit_step_single_group_1024_codes_bit_exact_vs_oracle():
    """m = 1, C = 1024, n = 16 (sixteen logits per lane; the 512-thread threshold block over 16 slots): masked counts 16 / 7 / 2 / 1 / 0."""
    from maskbit_amd import _lib
    lib = _lib.load()
    M, n, C, N = [16, 7, 2, 1, 0], 16, 1024, 4
    B = len(M)
    g = torch.Generator().manual_seed(31)
    regen = random_slot_masks(M, n, seed=32).reshape(B, n, 1)
    known = torch.randint(0, C, (B, n, 1), generator=g)
    tokens = torch.where(regen, torch.full_like(known, C), known)
    num_regen = torch.tensor(M, dtype=torch.int32, device=DEV)
    gum = torch.distributions.Gumbel(0.0, 1.0)
    torch.manual_seed(33)
    for i in range(N):
        ratio = float(O.masking_ratio((i + 1) / N, "cosine"))
        lc, lu = 3.0 * torch.randn(B, n, 1, C, generator=g), 3.0 * torch.randn(B, n, 1, C, generator=g)
        q = torch.empty(B * n, C).exponential_(1, generator=g)
        cn = gum.sample((B, n, 1)) * 4.5 * (1 - (i + 1) / N)
        want_pred, want_out = edit_step_oracle(lc, lu, 1.5, 0.8, q, cn, tokens, C, ratio, M)
        pred, out = step_edit(lib, lc.to(DEV), lu.to(DEV), 1.5, 0.8, q.to(DEV), cn.to(DEV), ratio, num_regen, tokens.to(DEV), C=C)
        assert torch.equal(pred.cpu(), want_pred) and torch.equal(out.cpu(), want_out), i
        tokens = want_out


# ---- 2. every slot masked: the plain run ---------------------------------------------------------------------------------------------------
def test_all_masked_edit_run_equals_the_plain_run():
    from maskbit_amd import sample, sample_from_tokens
    from maskbit_amd.sampling import build_edit_plan, build_plan, run_loop
    gm, tm = tiny_models()
    B, N = 3, 8
    y = torch.tensor([1, 4, 8], device=DEV)
    q, c = dev_noise(17, B, N, 8.2)
    plan = build_plan(N, 512, 7.1, "cosine", 3.0, 1.0, False, "arccos")
    eplan = build_edit_plan(N, 7.1, "cosine", 3.0, 1.0, False, "arccos")
    full = torch.full((B, 256, 2), MASK, dtype=torch.int64, device=DEV)
    img, u8, steps, codes = run_loop(gm, tm, y, plan, q, c, want_u8=True)
    img_e, u8_e, steps_e, codes_e = run_loop(gm, tm, y, eplan, q, c, want_u8=True, init_tokens=full)
    assert torch.equal(steps_e, steps) and torch.equal(codes_e, codes) and torch.equal(img_e, img) and torch.equal(u8_e, u8)
    with pytest.raises(ValueError):
        run_loop(gm, tm, y, eplan, q, c)                                                       # an edit plan without tokens
    with pytest.raises(ValueError):
        run_loop(gm, tm, y, plan, q, c, init_tokens=full)
    # the public entry under a seed draws what sample() draws
    kw = dict(softmax_temperature=1.0, randomize_temperature=8.2, mask_schedule_strategy="arccos", num_steps=9, guidance_scale=7.1,
              guidance_annealing="cosine", use_sampling_annealing=False, scale_pow=3.0)
    torch.manual_seed(5)
    img1, steps1 = sample(gm, tm, num_samples=B, labels=y, mask_token=MASK, patch_size=16, codebook_size=4096, codebook_splits=2, **kw)
    torch.manual_seed(5)
    img2, steps2 = sample_from_tokens(gm, tm, full.cpu(), y, **kw)
    assert isinstance(steps2, list) and len(steps2) == 9
    assert torch.equal(img2, img1) and all(torch.equal(a, b) for a, b in zip(steps1, steps2))


# ---- 3. the loop is forward + step --------------------------------------------------------------------------------------------------------
def test_edit_loop_equals_stepwise_composition_and_step_chunks():
    """mb_sample_edit == mb_gen_forward_cfg (the conditional forward alone where the scale is exactly 0, as in mb_sample) + mb_sample_step_edit composed
    on the host, bit for bit, from mixed masks; the same run fed in step chunks; a chunk of one kind does not continue a run of the other."""
    from maskbit_amd import _lib
    from maskbit_amd.sampling import build_edit_plan, build_plan, run_loop
    lib = _lib.load()
    gm, tm = tiny_models()
    M = [512, 200, 37, 3, 0]
    B, N = len(M), 7
    y = torch.tensor([1, 4, 8, 0, 9], device=DEV)
    q, c = dev_noise(11, B, N, 4.5)
    eplan = build_edit_plan(N, 3.0, "linear", 1.0, 1.0, False, "arccos")
    plan = build_plan(N, 512, 3.0, "linear", 1.0, 1.0, False, "arccos")
    assert eplan[0][0] == 0.0 and all(s != 0.0 for s in eplan[0][1:])
    init, regen = tokens_with_masks(M, seed=9)
    init = init.to(DEV)
    img, u8, steps, codes = run_loop(gm, tm, y, eplan, q, c, want_u8=True, init_tokens=init)
    num_regen = torch.tensor(M, dtype=torch.int32, device=DEV)
    tok = init
    for i in range(N):
        if eplan[0][i] == 0.0:
            lc, lu = gm(tok, y, torch.zeros(B, dtype=torch.bool, device=DEV)), None
        else:
            lg = gm.forward_cfg(tok, y)
            lc, lu = lg[:B].contiguous(), lg[B:].contiguous()
        pred, tok = step_edit(lib, lc, lu, eplan[0][i], eplan[1][i], q[i], c[i], eplan[2][i], num_regen, tok)
        assert torch.equal(pred, steps[i]), i
    assert torch.equal(codes.cpu(), O.combine_groups(steps[-1].cpu(), 12, 2).long())
    assert torch.equal(steps.cpu()[:, ~regen], init.cpu()[~regen].expand(N, -1))                # known slots in every step's prediction
    parts = []
    for (b0, b1) in ((0, 3), (3, 4), (4, 7)):                                                  # odd / even chunk starts: both token-buffer parities
        img_c, u8_c, st, codes_c = run_loop(gm, tm, y, eplan, q[b0:b1], c[b0:b1], want_u8=True, step_range=(b0, b1), init_tokens=init)
        parts.append(st)
    assert torch.equal(torch.cat(parts), steps) and torch.equal(codes_c, codes) and torch.equal(img_c, img) and torch.equal(u8_c, u8)
    # an edit run is continued by edit chunks only, a plain run by plain chunks only
    run_loop(gm, tm, y, eplan, q[0:3], c[0:3], want_image=False, step_range=(0, 3), init_tokens=init)
    with pytest.raises(RuntimeError, match="does not continue"):
        run_loop(gm, tm, y, plan, q[3:4], c[3:4], want_image=False, step_range=(3, 4))
    _, _, st34, _ = run_loop(gm, tm, y, eplan, q[3:4], c[3:4], want_image=False, step_range=(3, 4), init_tokens=init)   # the right continuation still works
    assert torch.equal(st34, steps[3:4])
    run_loop(gm, tm, y, plan, q[0:3], c[0:3], want_image=False, step_range=(0, 3))
    with pytest.raises(RuntimeError, match="does not continue"):
        run_loop(gm, tm, y, eplan, q[3:4], c[3:4], want_image=False, step_range=(3, 4), init_tokens=init)


# ---- 4. invariants of a free run -----------------------------------------------------------------------------------------------------------
def test_free_edit_run_invariants():
    """A free run from 512 / 300 / 37 / 3 / 1 / 0 masked slots: every step's prediction keeps the known tokens, the masked count each step leaves is
    k_i(b) of the contract (float32 on the host), no mask token is left in the last prediction.  The device loop gives the predictions; the masked
    counts come from forward + step composed on the host, which the previous test shows to be the same run."""
    from maskbit_amd import _lib
    from maskbit_amd.sampling import build_edit_plan, run_loop
    lib = _lib.load()
    gm, _ = tiny_models()
    M = [512, 300, 37, 3, 1, 0]
    B, N = len(M), 8
    y = (torch.arange(B) % 10).to(DEV)
    q, c = dev_noise(23, B, N, 8.2)
    eplan = build_edit_plan(N, 3.0, "none", 1.0, 1.0, False, "arccos")
    init, regen = tokens_with_masks(M, seed=13)
    _, _, steps, codes = run_loop(gm, None, y, eplan, q, c, want_image=False, init_tokens=init.to(DEV))
    steps = steps.cpu()
    for i in range(N):
        assert torch.equal(steps[i][~regen], init[~regen]), i
    assert int((steps[-1] == MASK).sum()) == 0 and int(steps.min()) >= 0
    assert bool((steps[:-1][:, regen] < MASK).all())                                            # a prediction never holds the mask token
    num_regen = torch.tensor(M, dtype=torch.int32, device=DEV)
    tok = init.to(DEV)
    nm = list(M)
    for i in range(N):
        lg = gm.forward_cfg(tok, y)
        pred, tok = step_edit(lib, lg[:B].contiguous(), lg[B:].contiguous(), eplan[0][i], eplan[1][i], q[i], c[i], eplan[2][i], num_regen, tok)
        assert torch.equal(pred.cpu(), steps[i])
        want = [expected_masked_after(eplan[2][i], M[b], nm[b]) for b in range(B)]
        got = (tok == MASK).sum(dim=(1, 2)).tolist()
        assert got == want, (i, got, want)
        assert bool(((tok == MASK).cpu() <= regen).all())                                      # never a known slot
        nm = got
    assert nm == [1, 1, 1, 0, 0, 0]                                                            # (the last step leaves k = 1 where it still re-masks; only pred leaves the loop)


# ---- 5. teacher-forced parity of an edit run -----------------------------------------------------------------------------------------------
def test_teacher_forced_token_parity_of_an_edit_run_tiny():
    """The CPU oracle drives an eight-step guided edit run of the tiny model (the loop restated from the oracle's step, as in the first test) from the
    reference's own final tokens (tests/golden/sample_tiny_none_cfg.npz) with 512 / 384 / 256 / 128 slots masked again: 1 280 sampled slots at step
    0.  The HIP path redoes every step from the CPU's inputs and noise; mismatch over the slots sampled at that step < 1e-2, the bound
    tests/test_hip_sampling.py::test_demo_call_site_replays_reference_run_tiny holds this model to over a whole run.
    Measured on an MI355X: see profiles/edit.md."""
    from maskbit_amd import _lib
    lib = _lib.load()
    gsd, _ = tiny_weights()
    gm, _ = tiny_models()
    z = load_golden("sample_tiny_none_cfg.npz")
    final = torch.from_numpy(z["steps"][-1])                                                    # [3, 256, 2]
    known = final[[0, 1, 2, 0]]
    y = torch.from_numpy(z["labels"])[[0, 1, 2, 0]].long()
    M = [512, 384, 256, 128]
    B, N = len(M), 8
    tokens, _ = tokens_with_masks(M, seed=41, known=known)
    num_regen = torch.tensor(M, dtype=torch.int32, device=DEV)
    drop = torch.cat([torch.zeros(B, dtype=torch.bool), torch.ones(B, dtype=torch.bool)])
    gum = torch.distributions.Gumbel(0.0, 1.0)
    torch.manual_seed(43)
    bad = tot = 0
    for i in range(N):
        ratio = float(O.masking_ratio((i + 1) / N, "arccos"))
        lg = O.lfq_bert_forward(gsd, TINY_GEN, torch.cat([tokens, tokens]), torch.cat([y, y]), drop)
        lc, lu = torch.chunk(lg, 2, dim=0)
        qn = torch.empty(B * 512, 64).exponential_(1)
        cn = gum.sample((B, 256, 2)) * 4.5 * (1 - (i + 1) / N)
        want_pred, want_out = edit_step_oracle(lc, lu, 3.0, 1.0, qn, cn, tokens, MASK, ratio, M)
        tin = tokens.to(DEV).contiguous()
        dl = gm.forward_cfg(tin, y.to(DEV))
        pred, _ = step_edit(lib, dl[:B].contiguous(), dl[B:].contiguous(), 3.0, 1.0, qn.to(DEV), cn.to(DEV), ratio, num_regen, tin)
        msk = tokens == MASK
        if i == 0:
            assert int(msk.sum()) == 1280
        bad += int((pred.cpu() != want_pred)[msk].sum())
        tot += int(msk.sum())
        assert torch.equal(pred.cpu()[~msk], tokens[~msk])
        tokens = want_out
    print(f"edit run, tiny: teacher-forced {bad}/{tot} = {bad / tot:.2e}")
    assert bad / tot < 1e-2


# ---- 6. inpaint end to end -----------------------------------------------------------------------------------------------------------------
def inpaint_case():
    g = torch.Generator().manual_seed(51)
    images = torch.rand(4, 3, 16, 16, generator=g).repeat_interleave(4, 2).repeat_interleave(4, 3) * 0.8 + 0.2 * torch.rand(4, 3, 64, 64, generator=g)
    mask = torch.zeros(4, 64, 64, dtype=torch.bool)
    mask[0, 5:23, 9:42] = True                                                                 # a rectangle off the stride-4 grid
    mask[1, 13, 30] = True                                                                     # one pixel
    mask[3] = True                                                                             # (sample 2: nothing)
    return images, mask, torch.tensor([1, 4, 8, 2])


def test_inpaint_end_to_end():
    from maskbit_amd import inpaint
    gm, tm = tiny_models()
    images, mask, y = inpaint_case()
    kw = dict(randomize_temperature=8.2, mask_schedule_strategy="arccos", num_steps=8, guidance_scale=7.1, guidance_annealing="cosine", scale_pow=3.0)
    torch.manual_seed(3)
    img, codes, tmask = inpaint(gm, tm, images.to(DEV), mask.to(DEV), y, **kw)
    torch.manual_seed(3)
    u8, codes_u8, tmask_u8 = inpaint(gm, tm, images, mask.unsqueeze(1).to(torch.uint8), y.to(DEV), return_uint8=True, **kw)   # host inputs, [B,1,H,W] uint8 mask
    assert img.shape == (4, 3, 64, 64) and img.dtype == torch.float32 and img.device.type == "cuda"
    assert u8.shape == (4, 64, 64, 3) and u8.dtype == torch.uint8
    assert codes.shape == (4, 256) and codes.dtype == torch.int64 and torch.equal(codes, codes_u8) and torch.equal(tmask, tmask_u8)
    want_tmask = token_mask_ref(mask, 4)
    assert tmask.dtype == torch.bool and torch.equal(tmask.cpu(), want_tmask)
    assert want_tmask.sum(dim=(1, 2)).tolist() == [5 * 9, 1, 0, 256]
    enc = tm.encode(images.to(DEV))[1]["min_encoding_indices"].reshape(4, 256)
    keep = ~want_tmask.reshape(4, 256)
    assert torch.equal(codes.cpu()[keep], enc.cpu()[keep])                                     # kept cells carry the encoder's codes
    assert int(codes.min()) >= 0 and int(codes.max()) < 4096
    dec, dec_u8 = tm.decode_tokens_uint8(codes)
    want, want_u8 = composite_ref(dec.cpu(), images, mask)
    assert torch.equal(img.cpu(), want)                                                        # outside: the input's bits; inside: decode_tokens(codes)
    outside = (~mask).unsqueeze(1).expand(-1, 3, -1, -1)
    assert torch.equal(img.cpu()[outside], images[outside]) and torch.equal(img.cpu()[~outside], dec.cpu()[~outside])
    assert torch.equal(u8.cpu(), want_u8)
    assert torch.equal(u8.cpu()[mask], dec_u8.cpu()[mask]) and torch.equal(u8.cpu()[~mask], O.to_uint8_nhwc(images)[~mask])
    # the empty mask: the input image and the encoder's codes
    assert torch.equal(img[2].cpu(), images[2]) and torch.equal(codes[2], enc[2])
    # without the composite the image is the decoder's, everywhere
    torch.manual_seed(3)
    raw, codes_raw, _ = inpaint(gm, tm, images.to(DEV), mask.to(DEV), y, keep_known_pixels=False, **kw)
    assert torch.equal(codes_raw, codes) and torch.equal(raw, dec)


def test_inpaint_full_mask_equals_sample():
    from maskbit_amd import inpaint, sample
    gm, tm = tiny_models()
    images = inpaint_case()[0][:2]
    y = torch.tensor([3, 7], device=DEV)
    kw = dict(softmax_temperature=1.0, randomize_temperature=8.2, mask_schedule_strategy="arccos", num_steps=8, guidance_scale=7.1,
              guidance_annealing="cosine", use_sampling_annealing=False, scale_pow=3.0)
    torch.manual_seed(9)
    want, steps = sample(gm, tm, num_samples=2, labels=y, mask_token=MASK, patch_size=16, codebook_size=4096, codebook_splits=2, **kw)
    torch.manual_seed(9)
    got, codes, tmask = inpaint(gm, tm, images.to(DEV), torch.ones(2, 64, 64, dtype=torch.bool), y, keep_known_pixels=False, **kw)
    assert torch.equal(got, want) and bool(tmask.all())
    assert torch.equal(codes.cpu(), O.combine_groups(steps[-1].cpu(), 12, 2).long())
    torch.manual_seed(9)
    got_u8, _, _ = inpaint(gm, tm, images.to(DEV), torch.ones(2, 64, 64, dtype=torch.bool), y, keep_known_pixels=False, return_uint8=True, **kw)
    assert torch.equal(got_u8.cpu(), O.to_uint8_nhwc(want.cpu()))


# ---- the helper kernels on their own -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,H,W", [(1, 6, 10), (2, 6, 10), (4, 12, 20), (8, 24, 40), (16, 48, 80), (32, 64, 96)])
def test_token_mask_kernel_every_stride(stride, H, W):
    """Every load width of edit_token_mask_kernel (1 / 2 / 4 / 8 / 16 bytes, and rows of two 16-byte pieces), non-square, B = 3: isolated pixels in the
    corners of blocks, a rectangle off the grid, an empty and a full image."""
    from maskbit_amd import _lib
    lib = _lib.load()
    pm = torch.zeros(3, H, W, dtype=torch.uint8)
    pm[0, stride - 1, stride - 1] = 1
    pm[0, H - 1, 0] = 255
    pm[0, 0, W - 1] = 2
    pm[0, H // 2, W // 2] = 1
    pm[1, 1:H - 1, 1:W // 2 + 1] = 1
    pm[2] = 1
    d = pm.to(DEV)
    out = torch.full((3, H // stride, W // stride), 9, dtype=torch.uint8, device=DEV)
    _lib.check(lib.mb_edit_token_mask(d.data_ptr(), out.data_ptr(), 3, H, W, stride, stream()), "mb_edit_token_mask")
    assert torch.equal(out.cpu().bool(), token_mask_ref(pm, stride)) and int(out.max()) == 1


@pytest.mark.parametrize("C,H,W,outs", [(3, 8, 12, "both"), (1, 4, 4, "both"), (4, 6, 8, "f32"), (2, 5, 20, "u8")])
def test_composite_and_init_kernels(C, H, W, outs):
    from maskbit_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(61 + C)
    B = 3
    gen = torch.randn(B, C, H, W, generator=g) * 0.7 + 0.5                                      # values on both sides of [0, 1]
    orig = torch.rand(B, C, H, W, generator=g)
    orig[0, 0, 0, 0], gen[0, 0, 0, 1] = 1.0, 1.0                                                # 255 exactly
    pm = (torch.rand(B, H, W, generator=g) < 0.4).to(torch.uint8) * 3
    want, want_u8 = composite_ref(gen, orig, pm)
    out = torch.zeros(B, C, H, W, device=DEV) if outs != "u8" else None
    u8 = torch.zeros(B, H, W, C, dtype=torch.uint8, device=DEV) if outs != "f32" else None
    d_gen, d_orig, d_pm = gen.to(DEV), orig.to(DEV), pm.to(DEV)
    _lib.check(lib.mb_edit_composite(d_gen.data_ptr(), d_orig.data_ptr(), d_pm.data_ptr(), out.data_ptr() if out is not None else None,
                                     u8.data_ptr() if u8 is not None else None, B, C, H, W, stream()), "mb_edit_composite")
    torch.cuda.synchronize()
    assert out is None or torch.equal(out.cpu(), want)
    assert u8 is None or torch.equal(u8.cpu(), want_u8)
    # mb_edit_init: codes + slot mask -> grouped tokens and counts (m = C groups of 3 bits here, n = H * W cells)
    n, m, gb = H * W, C, 3
    codes = torch.randint(0, 1 << (gb * m), (B, n), generator=g)
    slot = torch.rand(B, n, m, generator=g) < 0.3
    slot[1] = False
    slot[2] = True
    tok = torch.empty(B, n, m, dtype=torch.int64, device=DEV)
    cnt = torch.empty(B, dtype=torch.int32, device=DEV)
    d_codes, d_slot = codes.to(DEV), slot.to(DEV).view(torch.uint8)
    _lib.check(lib.mb_edit_init(d_codes.data_ptr(), d_slot.data_ptr(), tok.data_ptr(), cnt.data_ptr(), B, n, m, 1 << gb,
                                stream()), "mb_edit_init")
    split = (codes.unsqueeze(-1) >> (gb * torch.arange(m))) & ((1 << gb) - 1)
    assert torch.equal(tok.cpu(), torch.where(slot, torch.full_like(split, 1 << gb), split))
    assert cnt.cpu().tolist() == slot.sum(dim=(1, 2)).tolist()
    assert torch.equal(O.combine_groups(split, gb * m, m).long(), codes)                       # (the split is the inverse of the loop's combine)
