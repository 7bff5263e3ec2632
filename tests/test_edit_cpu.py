"""CPU checks of masked-token image editing (maskbit_amd/editing.py, the mb_edit_* / mb_sample_edit additions of the C ABI): the edit plan, the
struct layout, every refusal that must come before any device work, and the restatements tests/test_hip_edit.py compares the kernels with --
the per-sample step contract restated from the oracle's ``sample_step``, the token mask as a max-pool, the composite as a ``torch.where``."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from hip_helpers import Cfg, tok_config
from oracle import maskbit_oracle as O

TINY_GEN = O.GenCfg(bits=12, splits=2, hidden=128, depth=2, heads=4, mlp=256, seq=256, nclass=10)
TINY_TOK = O.TokCfg(token_size=12, hidden_channels=64, channel_mult=(1, 1, 2), num_resolutions=3, num_res_blocks=1)


# ---- the restatements (shared with tests/test_hip_edit.py) ------------------------------------------------------------------------------
def edit_step_oracle(logits_c, logits_u, scale, temperature, exp_noise, conf_noise, tokens, mask_token, mask_ratio, num_regen):
    """The edit step's contract from the oracle's own step: every sample on its own as a batch of one with num_maskable = its initial masked count;
    a sample with fewer than two masked slots is not re-masked (tokens_out = pred).  -> (pred, tokens_out) [B, n, m]."""
    B, n, m = tokens.shape
    C = logits_c.shape[-1]
    preds, outs = [], []
    for b in range(B):
        pred, out = O.sample_step(logits_c[b:b + 1], None if logits_u is None else logits_u[b:b + 1], scale, temperature,
                                  exp_noise.reshape(B, n * m, C)[b], conf_noise[b:b + 1], tokens[b:b + 1], mask_token,
                                  torch.tensor(mask_ratio, dtype=torch.float32), int(num_regen[b]))
        if int((tokens[b] == mask_token).sum()) <= 1:
            out = pred
        preds.append(pred)
        outs.append(out)
    return torch.cat(preds), torch.cat(outs)


def expected_masked_after(ratio, num_regen: int, nm: int) -> int:
    """Masked count a step leaves when the confidences are distinct: k of the contract, in float32 as on the device."""
    if nm <= 1:
        return 0
    mask_len = int(torch.floor(torch.tensor(ratio, dtype=torch.float32) * torch.tensor(float(num_regen), dtype=torch.float32)))
    return min(max(mask_len, 1), nm - 1)


def token_mask_ref(pixel_mask: torch.Tensor, stride: int) -> torch.Tensor:
    """bool / uint8 [B, H, W] -> bool [B, H / stride, W / stride]: any pixel of the block set."""
    return F.max_pool2d((pixel_mask != 0).float().unsqueeze(1), stride).squeeze(1) > 0


def composite_ref(gen: torch.Tensor, orig: torch.Tensor, pixel_mask: torch.Tensor):
    """-> (fp32 NCHW with the original pixels where the mask is 0, its uint8 NHWC = trunc(clamp * 255))."""
    x = torch.where((pixel_mask != 0).unsqueeze(1), gen, orig)
    return x, O.to_uint8_nhwc(x)


def random_slot_masks(sizes, P: int, seed: int) -> torch.Tensor:
    """bool [len(sizes), P] with exactly sizes[b] slots set in row b."""
    g = torch.Generator().manual_seed(seed)
    out = torch.zeros(len(sizes), P, dtype=torch.bool)
    for b, k in enumerate(sizes):
        out[b, torch.randperm(P, generator=g)[:k]] = True
    return out


# ---- plan and ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,ann,sp,strat,anneal_t", [(8, "cosine", 3.0, "arccos", False), (16, "none", 4.0, "linear", True), (5, "linear", 1.0, "cosine", False),
                                                    (64, "cosine", 3.0, "root", False), (7, "none", 1.0, "square", True)])
def test_edit_plan_matches_the_float32_formulas_and_build_plan(N, ann, sp, strat, anneal_t):
    from maskbit_amd.sampling import build_edit_plan, build_plan, plan_arrays
    plan = build_edit_plan(N, 7.1, ann, sp, 0.9, anneal_t, strat)
    scale, temp, ratio = plan
    ref = build_plan(N, 512, 7.1, ann, sp, 0.9, anneal_t, strat)
    assert scale == ref[0] and temp == ref[1]
    for i in range(N):
        r = O.masking_ratio((i + 1) / N, strat)
        assert r.dtype == torch.float32 and ratio[i] == float(r)
        assert float(ctypes.c_float(ratio[i]).value) == ratio[i]                               # a float32 value: survives the c_float array exactly
        assert int(torch.floor(r * 512)) == ref[2][i]                                          # all-masked: the device's floor(ratio * M) is build_plan's mask_len
    arrays = plan_arrays(plan)
    assert arrays[2]._type_ is ctypes.c_float and list(arrays[2]) == ratio and arrays[3]
    assert plan_arrays(ref)[2]._type_ is ctypes.c_int                                         # the plain plan keeps its integer lengths
    with pytest.raises(ValueError):
        build_edit_plan(4, 3.0, "none", 1.0, 1.0, False, "bogus")
    with pytest.raises(ValueError):
        build_edit_plan(4, 3.0, "bogus", 1.0, 1.0, False, "linear")


DEGENERATE = dict(num_steps=1, guidance_annealing="linear", guidance_scale=3.0)               # the only annealed scale is 3.0 * 0 / 1 = 0.0


def test_one_plan_type_and_one_forced_guidance_rule():
    from maskbit_amd.sampling import build_edit_plan, build_plan, forced_guidance, plan_arrays, seeded_plan
    plain = build_plan(1, 512, 3.0, "linear", 1.0, 1.0, False, "arccos")
    edit = build_edit_plan(1, 3.0, "linear", 1.0, 1.0, False, "arccos")
    assert type(plain) is type(edit) and plain[0] == edit[0] == [0.0]
    for plan in (plain, edit):
        assert plan_arrays(plan)[3] is False and not plan.force_guidance                       # the builders do not apply the rule ...
        forced = forced_guidance(plan, 3.0)                                                    # ... the helper does
        assert type(forced) is type(plan) and forced.edit == plan.edit and forced.force_guidance and tuple(forced) == tuple(plan)
        assert plan_arrays(forced)[3] is True and plan_arrays(plan)[3] is False                # (a new plan: the argument is unchanged)
        assert plan_arrays(forced_guidance(plan, 0.0))[3] is False                             # no guidance asked for: nothing to force
        assert plan_arrays(plan) is plan_arrays(plan)                                          # the arrays are built once per plan
    assert plan_arrays(seeded_plan(1, 3.0, "linear", 1.0, 1.0, False, "arccos"))[3] is True
    assert plan_arrays(seeded_plan(1, 0.0, "linear", 1.0, 1.0, False, "arccos"))[3] is False
    cos = build_plan(8, 512, 3.0, "cosine", 4.0, 1.0, False, "arccos")                         # step 1's scale is 4.47e-7: tiny, not zero
    assert cos[0][0] == 0.0 and 4.4e-7 < cos[0][1] < 4.5e-7
    assert plan_arrays(cos)[3] is True and forced_guidance(cos, 3.0) is cos and not cos.force_guidance
    for plan, third in ((cos, ctypes.c_int), (build_edit_plan(8, 3.0, "cosine", 4.0, 1.0, False, "arccos"), ctypes.c_float)):
        scale, temp, col = plan                                                                # still three sequences of num_steps
        assert len(scale) == len(temp) == len(col) == 8 and plan[0] is scale and plan[2] is col
        arrays = plan_arrays(plan)
        assert [a._type_ for a in arrays[:3]] == [ctypes.c_float, ctypes.c_float, third] and [len(a) for a in arrays[:3]] == [8, 8, 8]
        assert list(arrays[2]) == col


def test_edit_plan_struct_matches_the_header():
    from maskbit_amd import _lib
    header = open(os.path.join(ROOT, "include", "maskbit_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} mb_edit_plan;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    names, size = [], 0
    for f in fields:
        if "*" in f:
            assert f.startswith("const float*")
            names.append(f.split("*")[1].strip())
            size += ctypes.sizeof(ctypes.c_void_p)
        else:
            assert f.startswith("int ")
            for nm in f[4:].split(","):
                names.append(nm.strip())
                size += ctypes.sizeof(ctypes.c_int)
    assert names == [n for n, _ in _lib.EditPlan._fields_] == ["num_steps", "use_guidance", "scale", "temperature", "mask_ratio", "step_begin", "step_end"]
    assert ctypes.sizeof(_lib.EditPlan) == size == ctypes.sizeof(_lib.SamplePlan) == 8 + 3 * 8 + 8
    assert _lib.EditPlan.mask_ratio.offset == _lib.SamplePlan.mask_len.offset
    assert "#define MB_ABI_VERSION 8" in header                                                # additions only
    lib = _lib.load()
    for name in ("mb_sample_step_edit", "mb_sample_edit", "mb_edit_init", "mb_edit_token_mask", "mb_edit_composite"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, header)


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    """The checks in front of every launch: null pointers, aliasing, sizes, alignment (no device is touched before they pass)."""
    from maskbit_amd import _lib
    lib = _lib.load()
    p = 4096                                                                                   # any non-null, aligned address: never dereferenced
    assert lib.mb_sample_step_edit(p, None, 1.0, 1.0, p, p, 0.5, None, p, p + 64, None, 1, 16, 1, 64, None) == -1 and b"null" in lib.mb_last_error()
    assert lib.mb_sample_step_edit(p, None, 1.0, 1.0, p, p, 0.5, p, p, p, None, 1, 16, 1, 64, None) == -1 and b"alias" in lib.mb_last_error()
    assert lib.mb_sample_step_edit(p, None, 1.0, 1.0, p, p, 0.5, p, p, p + 64, None, 0, 16, 1, 64, None) == -1 and b"sizes" in lib.mb_last_error()
    assert lib.mb_sample_step_edit(p, None, 1.0, 1.0, p, p, 0.5, p, p, p + 64, None, 1, 8192, 2, 64, None) == -1 and b"too large" in lib.mb_last_error()
    assert lib.mb_sample_edit(None, None, None, p, 1, p, p, p, None, None, None, None, None) == -1
    assert lib.mb_edit_init(p, p, None, p, 1, 16, 1, 64, None) == -1 and b"null" in lib.mb_last_error()
    assert lib.mb_edit_init(p, p, p, p, 1, 16, 1, 48, None) == -1 and b"power of two" in lib.mb_last_error()
    assert lib.mb_edit_init(p, p, p, p, 1, 8192, 2, 64, None) == -1 and b"8192" in lib.mb_last_error()
    assert lib.mb_edit_token_mask(p, None, 1, 64, 64, 4, None) == -1
    assert lib.mb_edit_token_mask(p, p, 1, 64, 64, 3, None) == -1 and b"power of two" in lib.mb_last_error()
    assert lib.mb_edit_token_mask(p, p, 1, 64, 60, 8, None) == -1
    assert lib.mb_edit_token_mask(p + 2, p, 1, 64, 64, 4, None) == -1 and b"aligned" in lib.mb_last_error()
    assert lib.mb_edit_composite(p, p, p, None, None, 1, 3, 64, 64, None) == -1 and b"no output" in lib.mb_last_error()
    assert lib.mb_edit_composite(p, None, p, p, None, 1, 3, 64, 64, None) == -1
    assert lib.mb_edit_composite(p + 4, p, p, p, None, 1, 3, 64, 64, None) == -1 and b"aligned" in lib.mb_last_error()
    assert lib.mb_edit_composite(p, p, p, p, None, 1, 5, 64, 64, None) == -1 and b"channels" in lib.mb_last_error()
    assert lib.mb_edit_composite(p, p, p, p, None, 1, 3, 64, 62, None) == -1


# ---- refusals of the Python surface ------------------------------------------------------------------------------------------------------
def cpu_models(nclass=10):
    from maskbit_amd import ConvVQModel, LFQBert
    gm = LFQBert(hidden_dim=128, codebook_size=4096, codebook_splits=2, depth=1, heads=4, mlp_dim=256, nclass=nclass)
    tm = ConvVQModel(tok_config(TINY_TOK))
    return gm, tm


def test_exports():
    import maskbit_amd
    import modeling.modules
    from maskbit_amd import editing
    assert maskbit_amd.inpaint is editing.inpaint and maskbit_amd.sample_from_tokens is editing.sample_from_tokens
    assert "inpaint" in maskbit_amd.__all__ and "sample_from_tokens" in maskbit_amd.__all__
    assert not hasattr(modeling.modules, "inpaint") and not hasattr(modeling.modules, "sample_from_tokens")   # the reference has no such names


def test_sample_from_tokens_refuses_before_any_device_work():
    from maskbit_amd import sample_from_tokens
    gm, tm = cpu_models()
    tok = torch.full((2, 256, 2), 64, dtype=torch.int64)
    y = torch.tensor([1, 2])
    with pytest.raises(TypeError):
        sample_from_tokens(torch.nn.Linear(2, 2), tm, tok, y)
    with pytest.raises(TypeError):
        sample_from_tokens(gm, object(), tok, y)
    with pytest.raises(TypeError):
        sample_from_tokens(gm, tm, tok.int(), y)
    with pytest.raises(ValueError):
        sample_from_tokens(gm, tm, tok[:, :255], y)
    with pytest.raises(ValueError):
        sample_from_tokens(gm, tm, tok.reshape(2, 512, 1), y)
    for bad in (65, -1):
        t = tok.clone()
        t[1, 7, 1] = bad
        with pytest.raises(ValueError, match="token outside"):
            sample_from_tokens(gm, tm, t, y)
    with pytest.raises(ValueError):
        sample_from_tokens(gm, tm, tok, torch.tensor([1, 2, 3]))
    with pytest.raises(IndexError):
        sample_from_tokens(gm, tm, tok, torch.tensor([1, 11]))                                 # _check_labels: as sample()
    with pytest.raises(ValueError):
        sample_from_tokens(gm, tm, tok, y, mask_schedule_strategy="bogus")
    with pytest.raises(ValueError):
        sample_from_tokens(gm, tm, tok, y, guidance_annealing="bogus")
    with pytest.raises(RuntimeError, match="no CPU path"):                                     # everything valid: only the device is missing
        sample_from_tokens(gm, tm, tok, y)


def test_inpaint_refuses_before_any_device_work():
    from maskbit_amd import ConvVQModel, inpaint
    gm, tm = cpu_models()
    img = torch.rand(2, 3, 64, 64)
    mask = torch.zeros(2, 64, 64, dtype=torch.bool)
    y = torch.tensor([1, 2])
    with pytest.raises(TypeError):
        inpaint(object(), tm, img, mask, y)
    with pytest.raises(TypeError):
        inpaint(gm, gm, img, mask, y)
    with pytest.raises(TypeError):
        inpaint(gm, tm, img, mask.float(), y)                                                  # mask dtype
    with pytest.raises(TypeError):
        inpaint(gm, tm, img, mask.long(), y)
    with pytest.raises(TypeError):
        inpaint(gm, tm, (img * 255).to(torch.uint8), mask, y)
    for bad in (mask[:1], mask[:, :32], mask.unsqueeze(-1), torch.zeros(2, 3, 64, 64, dtype=torch.bool)):
        with pytest.raises(ValueError):
            inpaint(gm, tm, img, bad, y)
    for bad in (img[:, :, :32, :32], torch.rand(2, 3, 128, 128), torch.rand(2, 1, 64, 64), img[0], torch.rand(2, 3, 64, 32)):
        with pytest.raises(ValueError, match="images must be"):                                # 256 tokens at stride 4 are 64 x 64 pixels
            inpaint(gm, tm, bad, mask, y)
    with pytest.raises(ValueError):
        inpaint(gm, tm, img, mask, torch.tensor([1]))
    with pytest.raises(IndexError):
        inpaint(gm, tm, img, mask, torch.tensor([1, 11]))
    with pytest.raises(ValueError):
        inpaint(gm, tm, img, mask, y, mask_schedule_strategy="bogus")
    # a lookup tokenizer must hold exactly the codes the generator reads
    vq = dict(tok_config(TINY_TOK), quantizer_type="lookup", use_l2_normalisation=False)
    for size in (8192, 2048):
        with pytest.raises(ValueError, match="codebook"):
            inpaint(gm, ConvVQModel(Cfg(vq, codebook_size=size)), img, mask, y)
    with pytest.raises(RuntimeError, match="no CPU path"):
        inpaint(gm, ConvVQModel(Cfg(vq, codebook_size=4096)), img, mask, y)
    for ok_mask in (mask, mask.unsqueeze(1), mask.to(torch.uint8)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            inpaint(gm, tm, img, ok_mask, y)


def test_every_public_entry_builds_its_plan_through_the_one_helper(monkeypatch):
    """CPU-resident models, the degenerate schedule: each entry passes its argument checks, builds its plan through ``sampling.forced_guidance`` (a
    spy in its place) with ``force_guidance`` set, and stops at the missing device.  No caller keeps a copy of the rule."""
    from maskbit_amd import editing, generate_uint8, harness, inpaint, sample, sample_from_tokens, sample_seeded, sampling
    from maskbit_amd.parallel import sample_sharded
    gm, tm = cpu_models()
    seen = []
    real = sampling.forced_guidance

    def spy(plan, guidance_scale):
        out = real(plan, guidance_scale)
        seen.append((plan.edit, guidance_scale, out.force_guidance, out))
        return out
    for mod in (sampling, editing, harness):                                                   # (parallel imports it from sampling at call time)
        if hasattr(mod, "forced_guidance"):
            monkeypatch.setattr(mod, "forced_guidance", spy)
    ran = []
    real_run = sampling._run
    monkeypatch.setattr(sampling, "_run", lambda model, vq, labels, plan, *a, **kw: (ran.append(plan), real_run(model, vq, labels, plan, *a, **kw))[1])
    y = torch.tensor([1, 2])
    tok = torch.full((2, 256, 2), 64, dtype=torch.int64)
    img, mask = torch.rand(2, 3, 64, 64), torch.ones(2, 64, 64, dtype=torch.bool)
    entries = [
        ("sample", False, lambda: sample(gm, tm, num_samples=2, labels=y, mask_token=64, codebook_size=4096, codebook_splits=2, **DEGENERATE)),
        ("sample_seeded", True, lambda: sample_seeded(gm, tm, [5, 6], y, **DEGENERATE)),
        ("sample_from_tokens", True, lambda: sample_from_tokens(gm, tm, tok, y, **DEGENERATE)),
        ("sample_from_tokens seeded", True, lambda: sample_from_tokens(gm, tm, tok, y, seeds=[5, 6], **DEGENERATE)),
        ("inpaint", True, lambda: inpaint(gm, tm, img, mask, y, **DEGENERATE)),
        ("generate_uint8", False, lambda: next(generate_uint8(gm, tm, y, 2, **DEGENERATE))),
        ("generate_uint8 seeded", True, lambda: next(generate_uint8(gm, tm, y, 2, seed=5, **DEGENERATE))),
        ("sample_sharded", False, lambda: sample_sharded(gm, tm, y, noise="rank", scale_pow=1.0, **DEGENERATE)),
        ("sample_sharded seeded", True, lambda: sample_sharded(gm, tm, y, noise="seeded", seeds=[5, 6], scale_pow=1.0, **DEGENERATE)),
    ]
    for name, edit, call in entries:
        del seen[:], ran[:]
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
        assert len(seen) == 1 and seen[0][:3] == (edit, 3.0, True), (name, seen)
        assert all(p is seen[0][3] for p in ran), name                                         # what reached the runner is the helper's plan


# ---- the restatements themselves ---------------------------------------------------------------------------------------------------------
def test_token_mask_and_composite_restatements():
    pm = torch.zeros(2, 8, 8, dtype=torch.uint8)
    pm[0, 3, 5] = 1                                                                            # one pixel -> one cell
    pm[1, 1:5, 2:7] = 7                                                                        # a rectangle off the grid -> every cell it touches
    tm = token_mask_ref(pm, 4)
    assert tm.dtype == torch.bool and tm.tolist() == [[[False, True], [False, False]], [[True, True], [True, True]]]
    assert token_mask_ref(pm, 2)[1].tolist() == [[False, True, True, True], [False, True, True, True], [False, True, True, True], [False] * 4]
    gen, orig = torch.full((2, 3, 8, 8), 1.7), torch.rand(2, 3, 8, 8)
    gen[0, 1, 3, 5] = -0.3
    x, u8 = composite_ref(gen, orig, pm)
    keep = (pm == 0).unsqueeze(1).expand_as(x)
    assert torch.equal(x[keep], orig[keep]) and torch.equal(x[~keep], gen[~keep])
    assert u8.shape == (2, 8, 8, 3) and u8[0, 3, 5].tolist() == [255, 0, 255]
    assert torch.equal(u8[1, 0, 0], (orig[1, :, 0, 0] * 255).to(torch.uint8))


def test_step_contract_on_the_oracle():
    """The per-sample rule on the CPU with random logits in the place of a model, eight arccos steps, initial masked counts 512 / 256 / 37 / 3 / 1 / 0:
    known slots never change, the masked counts follow k of the contract, the all-masked sample equals the reference's own loop step, and -- the reason
    for the nm <= 1 rule -- the reference's clamp would wipe the known tokens of a sample with one masked slot."""
    M = [512, 256, 37, 3, 1, 0]
    B, P, C, N = len(M), 512, 64, 8
    g = torch.Generator().manual_seed(3)
    regen = random_slot_masks(M, P, seed=4).reshape(B, 256, 2)
    known = torch.randint(0, C, (B, 256, 2), generator=g)
    tokens = torch.where(regen, torch.full_like(known, C), known)
    gum = torch.distributions.Gumbel(0.0, 1.0)
    torch.manual_seed(5)
    full = tokens[:1].clone()
    for i in range(N):
        ratio = float(O.masking_ratio((i + 1) / N, "arccos"))
        lc, lu = torch.randn(B, 256, 2, C, generator=g), torch.randn(B, 256, 2, C, generator=g)
        q = torch.empty(B * P, C).exponential_(1, generator=g)
        cn = gum.sample((B, 256, 2)) * 4.5 * (1 - (i + 1) / N)
        nm = (tokens == C).sum(dim=(1, 2)).tolist()
        pred, out = edit_step_oracle(lc, lu, 2.0, 1.0, q, cn, tokens, C, ratio, M)
        assert torch.equal(pred[~regen], known[~regen]) and torch.equal(out[~regen], known[~regen])
        assert (out == C).sum(dim=(1, 2)).tolist() == [expected_masked_after(ratio, M[b], nm[b]) for b in range(B)]
        assert bool(((out == C) <= (tokens == C)).all())                                       # only masked slots are masked again
        # sample 0 (every slot masked) is the reference's step with num_maskable = n * m
        p0, o0 = O.sample_step(lc[:1], lu[:1], 2.0, 1.0, q[:P], cn[:1], full, C, torch.tensor(ratio), P)
        assert torch.equal(p0, pred[:1]) and torch.equal(o0, out[:1])
        full = o0
        if nm[4] == 1:                                                                         # what the rule prevents
            _, wiped = O.sample_step(lc[4:5], lu[4:5], 2.0, 1.0, q[4 * P:5 * P], cn[4:5], tokens[4:5], C, torch.tensor(ratio), 1)
            assert int((wiped == C).sum()) == P
        tokens = out
    assert int((pred == C).sum()) == 0                                                         # the last prediction is complete
