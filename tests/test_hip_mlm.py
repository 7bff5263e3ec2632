"""GPU checks of masked-token validation (csrc/mlm.hip behind maskbit_amd.get_mask_tokens / MLMLoss / MaskedTokenEvaluator /
eval_masked_prediction) against the reference's recorded results (tests/golden/mlm.npz) and, for inputs without a golden, against the float64
restatement of tests/mlm_reference.py.

Bounds (none of them comes from the code under test):
  masks, masked tokens, counts   exact.
  the two losses                 relative, against ref64 (or the restatement): 4 x the largest E_rel of the golden, E_rel = |ref32 - ref64| /
                                 |ref64| = the reference's own fp32 evaluation error (1.01e-7 -> bound 4.03e-7); the margin the SSIM bound of
                                 test_hip_evaluator.py gives over its E_ref.  fp32 per row with fp64 sums should not err more than the reference's
                                 all-fp32 chain.
  the two accuracies             4 fp32 ulps of ref32: the reference forms the mean and the power in fp32, here they are a float64 quotient
                                 and power of exact counts rounded once.
The unit per golden case, and the measured ratios once a GPU run has recorded them: profiles/mlm_eval.md.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden, golden_weights
from hip_helpers import hip_generator, hip_tokenizer
from oracle import maskbit_oracle as O
from maskbit_amd.synth import make_mlm_case
from mlm_reference import CONFIGS, KEYS, loss_bound, loss_case, mask_case, mask_tokens_ref, mlm_golden, mlm_loss64, row_losses64, unpack_mask
from test_edit_cpu import TINY_GEN, TINY_TOK

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOSS_CASES = [str(n) for n in mlm_golden()["loss_cases"]]
MASK_CASES = [str(n) for n in mlm_golden()["mask_cases"]]
ACC_ULPS = 4


def evaluator(ls=0.1, ss=False):
    from maskbit_amd import MaskedTokenEvaluator
    return MaskedTokenEvaluator(label_smoothing=ls, sum_splits=ss)


def one_update(logits, targets, masks, ls=0.1, ss=False):
    ev = evaluator(ls, ss)
    ev.update(logits.to(DEV), targets.to(DEV), masks.to(DEV))
    return ev, ev.result()


def within_ulps(a: float, b: float, n: int) -> bool:
    return abs(a - b) <= n * float(np.spacing(np.float32(abs(b))))


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit for bit, NaN entries (a decile without rows) included."""
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def check_losses(r, ref, what):
    """r: a result dict; ref: a dict with the two float64 losses.  -> the larger error in units of E_rel."""
    bound = loss_bound()
    ratios = []
    for key in ("mlm_loss", "masked_token_loss"):
        v = float(r[key])
        rel = abs(v - ref[key]) / abs(ref[key])
        ratios.append(rel / (bound / 4.0))
        print(f"{what} {key}: {v!r} vs {ref[key]!r} rel {rel:.3e} = {ratios[-1]:.3f} x E_rel")
        assert np.isfinite(v) and rel <= bound, (what, key, v, ref[key], rel, bound)
    return max(ratios)


# ---- masking ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MASK_CASES)
def test_mask_and_masked_tokens_bit_exact_with_the_reference(name):
    from maskbit_amd import get_mask_tokens
    z = mlm_golden()
    tokens, mask_token, mode, lo, seed = mask_case(name)
    gold = unpack_mask(z[name + ".mask"], tokens.shape)
    dev_tokens = tokens.to(DEV)
    torch.manual_seed(seed)                                                      # the global CPU generator, as a reference script seeds it
    masked, mask = get_mask_tokens(dev_tokens, mask_token, mode=mode, min_masking_ratio=lo)
    assert mask.dtype == torch.bool and mask.device.type == "cuda" and masked.dtype == torch.int64 and masked.shape == tokens.shape
    assert torch.equal(mask.cpu(), gold)
    assert torch.equal(masked.cpu(), torch.where(gold, torch.full_like(tokens, mask_token), tokens))
    assert torch.equal(dev_tokens.cpu(), tokens) and masked.data_ptr() != dev_tokens.data_ptr()          # the input is untouched
    masked2, mask2 = get_mask_tokens(dev_tokens, mask_token, mode=mode, min_masking_ratio=lo, generator=torch.Generator().manual_seed(seed))
    assert torch.equal(mask2, mask) and torch.equal(masked2, masked)


def test_mask_scalar_path_and_other_ranks():
    """n * m not a multiple of 4 and a misaligned token view take the one-slot path; [B, n] tokens work as [B, n, 1]."""
    from maskbit_amd import get_mask_tokens
    for shape, seed, mask_seed in (((3, 7, 3), 1, 10), ((2, 5), 2, 11), ((4, 16, 2), 3, 10)):       # seeds under which every sample is partly masked
        tokens = torch.randint(0, 64, shape, generator=torch.Generator().manual_seed(seed))
        dev_tokens = tokens.to(DEV)
        if shape == (4, 16, 2):                                                  # base 8 bytes off 16-byte alignment
            dev_tokens = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), dev_tokens.flatten()])[1:].view(shape)
            assert dev_tokens.data_ptr() % 16 == 8
        masked, mask = get_mask_tokens(dev_tokens, 64, mode="cosine", generator=torch.Generator().manual_seed(mask_seed))
        ref_masked, ref_mask, _ = mask_tokens_ref(tokens, 64, "cosine", generator=torch.Generator().manual_seed(mask_seed))
        per_sample = ref_mask.flatten(1).sum(1)
        assert bool((per_sample > 0).all()) and bool((per_sample < ref_mask[0].numel()).all())      # a condition on the inputs, checked on the reference side
        assert torch.equal(mask.cpu(), ref_mask) and torch.equal(masked.cpu(), ref_masked)


# ---- loss against the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LOSS_CASES)
def test_loss_vs_reference(name):
    from maskbit_amd import MLMLoss
    z = mlm_golden()
    logits, targets, mask = (t.to(DEV) for t in loss_case(name))
    counts = [int(v) for v in z[name + ".counts"]]
    for i, (ls, ss) in enumerate(CONFIGS):
        loss, d = MLMLoss(label_smoothing=ls, sum_splits=ss)(logits, targets, mask)
        assert tuple(d) == KEYS and loss is d["mlm_loss"]
        assert all(v.dim() == 0 and v.dtype == torch.float32 and v.device.type == "cuda" and not v.requires_grad for v in d.values())
        ev, r = one_update(logits, targets, mask, ls, ss)
        assert all(torch.equal(r[k], d[k]) for k in KEYS)                        # bit for bit
        assert [r["num_tokens"], r["num_masked"]] == counts[:2]
        assert [int(ev._state[4]), int(ev._state[5])] == counts[2:]
        assert r["sample_counts"].sum(0).tolist() == [counts[2], counts[3], counts[1]]
        ref64, ref32 = z[name + ".ref64"][i], z[name + ".ref32"][i]
        check_losses(r, {"mlm_loss": ref64[0], "masked_token_loss": ref64[2]}, f"{name} eps={ls} sum_splits={ss}")
        for k in (1, 3):
            assert within_ulps(float(r[KEYS[k]]), float(ref32[k]), ACC_ULPS), (KEYS[k], float(r[KEYS[k]]), ref32[k])


# ---- ties -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,pairs", [(64, [(0, 63), (5, 6)]), (512, [(3, 259), (3, 300), (255, 256)]), (4100, [(1023, 4099), (4095, 4096)]),
                                     (10, [(1, 9)])])
def test_ties_take_the_first_index(C, pairs):
    """One row per sample ([B, 1, 1, C]), so the per-sample correct count is 'prediction == target'.  Rows: two equal maxima at (i, j) per pair,
    and one all-equal row."""
    g = torch.Generator().manual_seed(C)
    x = torch.randn(len(pairs) + 1, 1, 1, C, generator=g)
    for r, (i, j) in enumerate(pairs):
        x[r, 0, 0, i] = x[r, 0, 0, j] = 9.0
    x[-1] = 0.25
    first = torch.tensor([i for i, _ in pairs] + [0]).view(-1, 1, 1)
    later = torch.tensor([j for _, j in pairs] + [C - 1]).view(-1, 1, 1)
    assert torch.equal(torch.argmax(x, dim=-1), first)                            # torch.argmax of the same tensor on the CPU
    mask = torch.ones_like(first, dtype=torch.bool)
    ev, _ = one_update(x, first, mask)
    assert ev.last_sample_counts[:, 0].tolist() == [1] * len(first)
    ev, r = one_update(x, later, mask)
    assert ev.last_sample_counts[:, 0].tolist() == [0] * len(first) and float(r["correct_tokens"]) == 0.0


# ---- range and edge cases ---------------------------------------------------------------------------------------------------------------
def test_large_logits_stay_finite_and_within_the_bound():
    logits, targets = make_mlm_case(2, 16, 2, 64, 41)
    logits = logits * 2500.0                                                      # 1e4 * randn
    assert float(logits.abs().max()) > 3e4
    mask = torch.rand(2, 16, 2, generator=torch.Generator().manual_seed(42)) < 0.5
    for ls in (0.1, 0.0):
        _, r = one_update(logits, targets, mask, ls)
        check_losses(r, mlm_loss64(logits, targets, mask, ls), f"1e4 logits eps={ls}")


def test_minus_inf_in_other_classes_is_finite_without_smoothing():
    logits, targets = make_mlm_case(2, 16, 2, 64, 43)
    hole = torch.rand(logits.shape, generator=torch.Generator().manual_seed(44)) < 0.3
    hole.scatter_(-1, targets.unsqueeze(-1), False)                               # never the target's class
    logits = logits.masked_fill(hole, float("-inf"))
    logits[0, 0, 0] = float("-inf")
    logits[0, 0, 0, targets[0, 0, 0]] = 1.5                                       # a row with the target alone: loss 0
    mask = torch.rand(2, 16, 2, generator=torch.Generator().manual_seed(45)) < 0.5
    _, r = one_update(logits, targets, mask, 0.0)
    check_losses(r, mlm_loss64(logits, targets, mask, 0.0), "-inf eps=0")
    _, r = one_update(logits, targets, mask, 0.1)                                 # with smoothing the mean of the log-probabilities is -inf, as in torch
    assert float(r["mlm_loss"]) == float("inf") == mlm_loss64(logits, targets, mask, 0.1)["mlm_loss"]


def test_mask_all_false_and_all_true():
    logits, targets = make_mlm_case(3, 16, 2, 64, 46)
    _, r = one_update(logits, targets, torch.zeros(3, 16, 2, dtype=torch.bool))
    assert torch.isnan(r["masked_token_loss"]) and torch.isnan(r["masked_correct_tokens"]) and r["num_masked"] == 0
    assert torch.isfinite(r["mlm_loss"]) and torch.isfinite(r["correct_tokens"])
    check_losses({"mlm_loss": r["mlm_loss"], "masked_token_loss": r["mlm_loss"]},
                 {k: mlm_loss64(logits, targets, torch.ones(3, 16, 2), 0.1)["mlm_loss"] for k in ("mlm_loss", "masked_token_loss")}, "mask all false")
    ev, r = one_update(logits, targets, torch.ones(3, 16, 2, dtype=torch.bool))
    assert torch.equal(r["masked_token_loss"], r["mlm_loss"]) and torch.equal(r["masked_correct_tokens"], r["correct_tokens"])
    assert torch.equal(ev._state[0], ev._state[1]) and r["num_masked"] == r["num_tokens"] == 96         # the float64 sums themselves, bit for bit
    assert int(r["by_mask_fraction"][9, 2]) == 96 and torch.isnan(r["by_mask_fraction"][:9, 0]).all()


def test_target_out_of_range_raises_at_result_and_nothing_faults():
    logits, targets = make_mlm_case(2, 16, 2, 64, 47)
    mask = torch.rand(2, 16, 2, generator=torch.Generator().manual_seed(48)) < 0.5
    for bad in (64, -1, 2 ** 40):
        t = targets.clone()
        t[1, 3, 1] = bad
        ev = evaluator()
        ev.update(logits.to(DEV), t.to(DEV), mask.to(DEV))                        # update itself does not look at the values
        with pytest.raises(IndexError, match="outside"):
            ev.result()
        st = ev._state.cpu()
        assert int(st[36]) == 1 and int(st[2]) == 63                              # the other rows were counted, the bad one entered nothing
        keep = torch.ones(64, dtype=torch.bool)
        keep[32 + 3 * 2 + 1] = False
        loss, _ = row_losses64(logits, targets, 0.1)
        assert abs(float(st[:1].view(torch.float64)) - float(loss[keep].sum())) <= loss_bound() * float(loss[keep].sum())


@pytest.mark.parametrize("C", [64, 512])
def test_misaligned_logits_give_the_same_values(C):
    logits, targets = make_mlm_case(2, 16, 2, C, 49)
    mask = torch.rand(2, 16, 2, generator=torch.Generator().manual_seed(50)) < 0.5
    aligned = logits.to(DEV)
    view = torch.cat([torch.zeros(1, device=DEV), aligned.flatten()])[1:].view(logits.shape)
    assert aligned.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    a, b = evaluator(), evaluator()
    a.update(aligned, targets.to(DEV), mask.to(DEV))
    b.update(view, targets.to(DEV), mask.to(DEV))
    assert torch.equal(a._state, b._state) and torch.equal(a.last_sample_sums, b.last_sample_sums)
    assert torch.equal(a.last_sample_counts, b.last_sample_counts) and float(a.last_sample_sums.min()) > 0


# ---- exact invariances --------------------------------------------------------------------------------------------------------------------
def test_per_sample_figures_do_not_depend_on_the_batch():
    logits, targets = make_mlm_case(64, 16, 2, 64, 51)
    mask = torch.rand(64, 16, 2, generator=torch.Generator().manual_seed(52)) < 0.5
    logits, targets, mask = logits.to(DEV), targets.to(DEV), mask.to(DEV)
    ev = evaluator()
    ev.update(logits, targets, mask)
    sums, counts = ev.last_sample_sums.clone(), ev.last_sample_counts.clone()
    assert sums.shape == (64, 2) and counts.shape == (64, 3) and bool((sums > 0).all())
    for b in (0, 1, 37, 63):
        ev.update(logits[b:b + 1], targets[b:b + 1], mask[b:b + 1])
        assert torch.equal(ev.last_sample_sums[0], sums[b]) and torch.equal(ev.last_sample_counts[0], counts[b]), b


def test_split_batch_same_update_twice_and_reset():
    logits, targets = make_mlm_case(8, 16, 2, 64, 53)
    thresholds = torch.linspace(0.05, 0.95, 8).view(8, 1, 1)                      # samples in several mask-fraction deciles
    mask = torch.rand(8, 16, 2, generator=torch.Generator().manual_seed(54)) < thresholds
    logits, targets, mask = logits.to(DEV), targets.to(DEV), mask.to(DEV)
    whole, parts, again = evaluator(), evaluator(), evaluator()
    whole.update(logits, targets, mask)
    again.update(logits, targets, mask)
    parts.update(logits[:3], targets[:3], mask[:3])
    parts.update(logits[3:], targets[3:], mask[3:])
    assert torch.equal(whole._state, again._state) and torch.equal(whole.last_sample_sums, again.last_sample_sums)
    assert torch.equal(whole._state, parts._state) and torch.equal(whole.last_sample_sums[3:], parts.last_sample_sums)
    rw, rp = whole.result(), parts.result()
    assert parts._num_updates == 2 and parts._num_examples == 8
    assert all(torch.equal(rw[k], rp[k]) for k in KEYS) and same_bits(rw["by_mask_fraction"], rp["by_mask_fraction"])
    table = rw["by_mask_fraction"]
    assert table.shape == (10, 3) and int(table[:, 2].sum()) == rw["num_masked"] == int(mask.sum())
    assert int((table[:, 2] > 0).sum()) >= 4
    per = mask.flatten(1).sum(1).cpu()
    for k in range(10):                                                           # the deciles, with integer arithmetic
        members = torch.minimum(10 * per // 32, torch.tensor(9)) == k
        assert int(table[k, 2]) == int(per[members].sum())
    whole.reset_metrics()
    assert whole._num_examples == 0 and whole.last_sample_sums is None and not bool(whole._state.any())
    with pytest.raises(ValueError, match="No examples"):
        whole.result()
    whole.update(logits, targets, mask)
    assert torch.equal(whole._state, again._state)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tiny_tokenizer():
    return hip_tokenizer(TINY_TOK, O.make_tokenizer_weights(TINY_TOK, seed=int(load_golden("tok_tiny.npz")["seed"]), with_encoder=True))


def tiny_generators():
    yield "lfq", hip_generator(TINY_GEN, golden_weights(load_golden("gen_tiny.npz")))
    from maskbit_amd import Bert
    cfg = O.GenCfg(bits=12, splits=2, hidden=128, depth=1, heads=2, mlp=256, nclass=10, kind="bert")
    m = Bert(img_size=256, hidden_dim=cfg.hidden, codebook_size=2 ** cfg.bits, codebook_splits=cfg.splits, depth=cfg.depth, heads=cfg.heads,
             mlp_dim=cfg.mlp, dropout=0.1, nclass=cfg.nclass, input_stride=16)
    m.load_state_dict(O.make_generator_weights(cfg, seed=5, head_gain=8.0), strict=True)
    yield "bert", m.eval().requires_grad_(False).to(DEV)


def test_eval_masked_prediction_end_to_end():
    from maskbit_amd import eval_masked_prediction, get_mask_tokens, mask_token_for, split_factorized_tokens
    g = torch.Generator().manual_seed(77)
    loader = [{"image": torch.rand(b, 3, 64, 64, generator=g), "class_id": torch.randint(0, 10, (b,), generator=g), "__key__": ["x"] * b}
              for b in (3, 2)]
    tok = tiny_tokenizer()
    for name, model in tiny_generators():
        dropout = 0.5 if name == "lfq" else 0.0
        ev = evaluator()
        ev.update(torch.zeros(1, 4, 2, 64, device=DEV), torch.zeros(1, 4, 2, dtype=torch.int64, device=DEV), torch.ones(1, 4, 2, dtype=torch.bool, device=DEV))
        r = eval_masked_prediction(model, tok, loader, ev, mask_schedule_strategy="cosine", class_label_dropout=dropout,
                                   generator=torch.Generator().manual_seed(5))          # resets what was there before
        assert ev._num_examples == 5 and ev._num_updates == 2 and r["num_tokens"] == 5 * 512
        # by hand: encode, split, get_mask_tokens from the same stream, the model, and the float64 restatement on the model's own logits
        hand = torch.Generator().manual_seed(5)
        all_logits, all_tokens, all_masks = [], [], []
        for batch in loader:
            _, d = tok.encode(batch["image"].to(DEV))
            tokens = split_factorized_tokens(d["min_encoding_indices"].reshape(batch["image"].shape[0], -1), codebook_size=4096, splits=2)
            masked, mask = get_mask_tokens(tokens, mask_token_for(4096, 2), mode="cosine", generator=hand)
            drop = (torch.rand(tokens.shape[0], generator=hand) < dropout) if dropout > 0 else None
            all_logits.append(model(masked, batch["class_id"].to(DEV), drop).cpu())
            all_tokens.append(tokens.cpu())
            all_masks.append(mask.cpu())
        assert mask_token_for(4096, 2) == 64 and all(int(t.max()) < 64 for t in all_tokens)
        ref = mlm_loss64(torch.cat(all_logits), torch.cat(all_tokens), torch.cat(all_masks), 0.1)
        assert r["num_masked"] == ref["masked"] and 0 < ref["masked"] < ref["rows"]
        assert r["sample_counts"][:, 2].tolist() == all_masks[-1].flatten(1).sum(1).tolist()           # identical masks, sample by sample
        assert [int(ev._state[4]), int(ev._state[5])] == [ref["correct"], ref["masked_correct"]]
        check_losses(r, ref, "eval_masked_prediction " + name)
        for key in ("correct_tokens", "masked_correct_tokens"):
            assert within_ulps(float(r[key]), ref[key], 1), key                   # a float64 figure of exact counts, rounded once
        assert int(r["by_mask_fraction"][:, 2].sum()) == r["num_masked"]
        if name == "lfq":                                                         # a fresh evaluator with the defaults when none is given
            r2 = eval_masked_prediction(model, tok, loader, mask_schedule_strategy="cosine", class_label_dropout=dropout,
                                        generator=torch.Generator().manual_seed(5))
            assert all(torch.equal(r2[k], r[k]) for k in KEYS)
    with pytest.raises(TypeError):
        eval_masked_prediction(torch.nn.Identity(), tok, loader)
