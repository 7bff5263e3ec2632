"""The yardstick of tests/test_hip_sampling_step.py, validated on the CPU before it judges a kernel: tests/sampling_reference.py's float64
restatement, rounding model and checkers against the float32 oracle and against deliberately wrong float32 chains, on the random cases the GPU
file runs.  Measured figures: profiles/sampling_step.md."""
import math

import pytest
import torch

import sampling_reference as R
from oracle import maskbit_oracle as O

CASES = pytest.mark.parametrize("case", R.RANDOM_CASES, ids=lambda c: c.name)


def oracle_step(inp):
    """O.sample_step on a case's inputs; an edit case per sample as a batch of one with num_maskable = num_regen[b], a sample with fewer than two
    masked slots left as pred (the edit contract of include/maskbit_hip.h, as tests/test_edit_cpu.py states it)."""
    C = inp["logits_c"].shape[-1]
    tokens, lu = inp["tokens"], inp["logits_u"]
    B, n, m = tokens.shape
    if not inp["edit"]:
        # mask_ratio * num_maskable = k_mask_len exactly: the mask length is the caller's in the plain step
        return O.sample_step(inp["logits_c"], lu, inp["scale"], inp["temperature"], inp["exp_noise"], inp["conf_noise"], tokens, C,
                             torch.tensor(float(inp["k_mask_len"])), 1)
    preds, outs = [], []
    for b in range(B):
        pred, out = O.sample_step(inp["logits_c"][b:b + 1], None if lu is None else lu[b:b + 1], inp["scale"], inp["temperature"],
                                  inp["exp_noise"].reshape(B, n * m, C)[b], inp["conf_noise"][b:b + 1], tokens[b:b + 1], C,
                                  torch.tensor(inp["mask_ratio"], dtype=torch.float32), int(inp["num_regen"][b]))
        preds.append(pred)
        outs.append(pred if int((tokens[b] == C).sum()) <= 1 else out)
    return torch.cat(preds), torch.cat(outs)


def error_ratios(inp, ref, model, r32, top, st):
    """Largest observed float32 error / bound of the float32 chain ``r32``: of a score difference against the top class over every live class of
    every masked row, and of a confidence over every masked slot."""
    C = inp["logits_c"].shape[-1]
    masked = (inp["tokens"].reshape(-1) == C).unsqueeze(1)
    top = top.unsqueeze(1)
    ls = torch.log(r32["ratio"].double())
    err = ((ls.gather(1, top) - ls) - (ref["score"].gather(1, top) - ref["score"])).abs()
    look = (ref["logp"] > R.LOGP_FLOOR) & masked & (torch.arange(C).unsqueeze(0) != top)
    draw = float((err / (model.dcls.gather(1, top) + model.dcls))[look].max())
    fin = torch.isfinite(st["conf"])
    conf = float(((r32["conf"].double() - st["conf"]).abs() / st["dconf"])[fin].max())
    return draw, conf


@CASES
def test_oracle_passes_and_the_input_conditions_hold(case):
    """The float32 oracle passes both checkers (its summation order is torch's own: the order-free depth C - 1 in the place of the kernel's), and so
    does the float32 chain in the kernel's order under the kernel's depth; observed error / bound <= 1; at most 1 % of the masked rows have more
    than one candidate; no sample's k-th / (k+1)-th gap lies inside the band."""
    inp = R.make_case(case)
    refmodel = R.reference_of(inp)
    pred, out = oracle_step(inp)
    bad, _, _ = R.check_step(inp, pred, out, sum_depth=case.C - 1)
    assert not bad, bad
    r32 = R.step32(inp)
    bad, sd, st = R.check_step(inp, r32["pred"], r32["tokens_out"], refmodel=refmodel)
    assert not bad, bad
    draw, conf = error_ratios(inp, *refmodel, r32, sd["top"], st)
    print(f"{case.name}: error / bound draw {draw:.3f} conf {conf:.3f}; rows with more than one candidate {sd['multi_share']:.2%} of "
          f"{sd['masked_rows']}; smallest k-th gap / band {st['min_gap_over_band']:.3g}; largest band {max(st['bands']):.2e}")
    assert 0.0 < draw <= 1.0 and 0.0 < conf <= 1.0
    assert sd["multi_share"] <= 0.01
    assert st["min_gap_over_band"] > 1.0


@CASES
def test_wrong_rules_fail_the_checkers(case):
    """``conf < thr`` re-masks k - 1 slots: rejected on every case.  A sample's own masked count in the place of sample 0's: rejected on the plain
    cases whose mask length lies above the masked counts (where the count decides k) and whose samples differ in it."""
    inp = R.make_case(case)
    refmodel = R.reference_of(inp)
    r = R.step32(inp, "lt")
    bad, _, _ = R.check_step(inp, r["pred"], r["tokens_out"], refmodel=refmodel)
    assert any("re-masked, k =" in b for b in bad), bad
    if not case.edit and case.B > 1 and case.mask_ratio > 0.5:
        assert len(set(R.masked_counts(inp["tokens"], case.C).tolist())) > 1
        r = R.step32(inp, "own_count")
        bad, _, _ = R.check_step(inp, r["pred"], r["tokens_out"], refmodel=refmodel)
        assert bad


def test_plain_cases_with_a_deciding_count_exist():
    assert sum(1 for c in R.RANDOM_CASES if not c.edit and c.B > 1 and c.mask_ratio > 0.5) >= 2


@pytest.mark.parametrize("mutant", ("fma", "no_renorm", "conf_pn"))
def test_rounding_level_variants_lie_inside_the_model(mutant):
    """What the float64 band checkers cannot see: the contracted combine (one rounding in the place of two), the draw without Categorical's
    renormalisation and the confidence from pn are the float64 restatement's own value with FEWER or OTHER roundings of the same size, so every
    bound derived from the operations admits them on random inputs (shown on the guided cases at scale 7.1 and sigma 6).  Each of them therefore has
    exact rows of its own, on which it gives another integer than the reference: ``fma_flip_pairs``, ``renorm_flip_rows``, ``conf_pn_rows`` and
    the three ``*_fails_the_exact_*`` tests below; tests/test_hip_sampling_step.py runs the same rows on the kernel."""
    for case in R.RANDOM_CASES:
        if not (case.guided and case.scale == 7.1 and case.sigma == 6.0):
            continue
        inp = R.make_case(case)
        refmodel = R.reference_of(inp)
        r = R.step32(inp, mutant)
        bad, sd, st = R.check_step(inp, r["pred"], r["tokens_out"], refmodel=refmodel)
        draw, conf = error_ratios(inp, *refmodel, r, sd["top"], st)
        print(f"{mutant} on {case.name}: violations {len(bad)}, error / bound draw {draw:.3f} conf {conf:.3f}")
        assert not bad and draw <= 1.0 and conf <= 1.0


def test_contraction_fails_the_exact_tie_rows():
    """The rows tests/test_hip_sampling_step.py::test_cfg_combine_exact adds against a contraction: an exact tie under the reference's three
    roundings (pred = the lower class), broken towards the higher class by x + fma(s, d)."""
    count, C = 8, 8
    x, y, w = R.fma_flip_pairs(count)
    assert bool((w.abs() > 1.0).all())
    lc, lu = torch.full((count, 1, 1, C), -math.inf), torch.zeros(count, 1, 1, C)
    lc[:, 0, 0, 2], lu[:, 0, 0, 2] = x, y
    lc[:, 0, 0, 5], lu[:, 0, 0, 5] = w, w
    inp = {"logits_c": lc, "logits_u": lu, "scale": R.f32(7.1), "temperature": 1.0, "exp_noise": torch.ones(count, C),
           "conf_noise": torch.zeros(count, 1, 1), "tokens": torch.full((count, 1, 1), C, dtype=torch.int64), "edit": False, "k_mask_len": 1}
    assert R.step32(inp)["pred"].reshape(-1).tolist() == [2] * count
    assert R.step32(inp, "fma")["pred"].reshape(-1).tolist() == [5] * count
    pred, _ = O.sample_step(lc, lu, inp["scale"], 1.0, inp["exp_noise"], inp["conf_noise"], inp["tokens"], C, torch.tensor(1.0), 1)
    assert pred.reshape(-1).tolist() == [2] * count


def test_reference_pieces():
    """The count rules and the float32 floor of the restatement on values worked out by hand."""
    C = 4
    tokens = torch.tensor([[[4], [4], [4], [1], [2]], [[4], [0], [1], [2], [3]]])                # masked counts 3 and 1
    assert R.masked_counts(tokens, C).tolist() == [3, 1]
    assert [R.k_reference(tokens, C, ml) for ml in (0, 1, 2, 9)] == [1, 1, 2, 2]
    assert R.k_reference(tokens[1:], C, 3) == 0 and R.k_reference(tokens[1:] * 0, C, 3) == -1     # the wrapped indices sorted[-1], sorted[-2]
    assert R.k_edit(tokens, C, 0.5, [5, 5]) == [2, None]
    assert R.mask_len32(R.f32(0.7), 10) == 7 and math.floor(R.f32(0.7) * 10) == 6
    assert [R.sum_depth_kernel(c) for c in (2, 64, 65, 200, 4096)] == [6, 6, 7, 9, 69]
    e = torch.rand(5, 200) + 0.1
    assert torch.allclose(R._row_sum_kernel_order(e).double(), e.double().sum(dim=1), rtol=9 * R.U, atol=0.0)


def test_lost_renormalisation_fails_the_exact_rows():
    """The rows tests/test_hip_sampling_step.py::test_renormalisation_exact_rows runs: a tie under the reference's arithmetic (pred = the lower
    class), broken towards the higher class when the draw is taken from p / q."""
    lc, q, want, wrong = R.renorm_flip_rows(8)
    n = lc.shape[0]
    inp = {"logits_c": lc.reshape(n, 1, 1, 64), "logits_u": None, "scale": 0.0, "temperature": 1.0, "exp_noise": q,
           "conf_noise": torch.zeros(n, 1, 1), "tokens": torch.full((n, 1, 1), 64, dtype=torch.int64), "edit": False, "k_mask_len": 1}
    assert R.step32(inp)["pred"].reshape(-1).tolist() == want
    assert R.step32(inp, "no_renorm")["pred"].reshape(-1).tolist() == wrong
    pred, _ = O.sample_step(inp["logits_c"], None, 0.0, 1.0, q, inp["conf_noise"], inp["tokens"], 64, torch.tensor(1.0), 1)
    assert pred.reshape(-1).tolist() == want


def test_confidence_from_pn_fails_the_exact_rows():
    """The samples tests/test_hip_sampling_step.py::test_confidence_from_p_exact_rows runs: which of two slots is re-masked depends on whether the
    confidence is log p or log pn."""
    lc, cn, want, wrong = R.conf_pn_rows(6)
    n = lc.shape[0]
    assert not torch.equal(want, wrong)
    tokens = torch.full((n, 2, 1), 8, dtype=torch.int64)
    inp = {"logits_c": lc, "logits_u": None, "scale": 0.0, "temperature": 1.0, "exp_noise": torch.ones(2 * n, 8), "conf_noise": cn, "tokens": tokens,
           "edit": False, "k_mask_len": 1}
    assert torch.equal(R.step32(inp)["tokens_out"], want)
    assert torch.equal(R.step32(inp, "conf_pn")["tokens_out"], wrong)
    _, out = O.sample_step(lc, None, 0.0, 1.0, inp["exp_noise"], cn, tokens, 8, torch.tensor(1.0), 1)
    assert torch.equal(out, want)
