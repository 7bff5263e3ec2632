"""GPU tests of the sampling step per launch: every case is one ``mb_sample_step`` or ``mb_sample_step_edit`` call on caller buffers, no forward.

Exact cases: inputs on which float32 is exact (one-hot logits: p = 1, log p = 0, the confidence IS conf_noise), expected values integers from the
rule as oracle/maskbit_oracle.py:201-228 writes it (``torch.sort(...)[k - 1]``, ``conf <= thr``), compared with ``torch.equal``.
Random cases: tests/sampling_reference.py's float64 restatement and rounding model, through its two checkers.

Which case reaches which instantiation:
  sample_rows_kernel<1>   C = 2, 3, 8, 32, 64 of the class / noise sweeps; every threshold case (C = 2);  random c8_*, c64_*
  sample_rows_kernel<2>   C = 65, 100, 128;                                                               random c100_*, c128_*
  sample_rows_kernel<4>   C = 256;                                                                        random c200_*
  sample_rows_kernel<8>   C = 512;                                                                        random c512_*
  sample_rows_kernel<16>  C = 1000, 1024;                                                                 random c1000_*
  sample_rows_kernel<32>  C = 2048;                                                                       random c2048_*
  sample_rows_kernel<64>  C = 4095, 4096;                                                                 random c4096_*
  sample_thresh_kernel<false> / <true>: every threshold case runs the plain and the edit step;            random *_plain / *_edit
  threshold block of 512 threads: P < 1024 (1, 2, 63, 511, 512, 1000; random P = 63, 512); of 1024: P = 1024, 1025, 2048, 8192; random P = 1025
"""
import math

import pytest
import torch

import sampling_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
NEG = -math.inf


def run_step(lc, lu, scale, temperature, q, cn, tokens, C, k_mask_len=None, ratio=None, num_regen=None, want_pred=True):
    """One launch pair on copies of the CPU tensors -> (pred or None, tokens_out) on the CPU.  tokens [B, n, m]; the outputs are pre-filled with
    values no step writes, so a slot left unwritten shows."""
    from maskbit_amd import _lib
    lib = _lib.load()
    B, n, m = tokens.shape
    d = [None if t is None else t.to(DEV).contiguous() for t in (lc, lu, q, cn, tokens)]
    out = torch.full_like(d[4], -7)
    pred = torch.full_like(d[4], -9) if want_pred else None
    ptr = lambda t: None if t is None else t.data_ptr()                                      # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    if num_regen is None:
        rc = lib.mb_sample_step(ptr(d[0]), ptr(d[1]), scale, temperature, ptr(d[2]), ptr(d[3]), int(k_mask_len), ptr(d[4]), ptr(out), ptr(pred),
                                B, n, m, C, s)
    else:
        nr = num_regen.to(torch.int32).to(DEV)
        rc = lib.mb_sample_step_edit(ptr(d[0]), ptr(d[1]), scale, temperature, ptr(d[2]), ptr(d[3]), float(ratio), nr.data_ptr(), ptr(d[4]), ptr(out),
                                     ptr(pred), B, n, m, C, s)
    _lib.check(rc, "sample step")
    torch.cuda.synchronize()
    return (pred.cpu() if want_pred else None), out.cpu()


def expected_out(conf, pred, ks, mask_token):
    """The re-mask rule on float32 confidences [B, P], exactly as the oracle writes it; ks[b] None: sample b keeps pred."""
    out = pred.clone()
    for b, k in enumerate(ks):
        if k is None:
            continue
        thr = torch.sort(conf[b]).values[k - 1]
        out[b] = torch.where(conf[b] <= thr, torch.full_like(pred[b], mask_token), pred[b])
    return out


# ---- exact: class and noise addressing -----------------------------------------------------------------------------------------------------------
SWEEP_C = (2, 8, 32, 64, 128, 256, 512, 1024, 2048, 4096, 3, 65, 100, 1000, 4095)
CHUNK = 2048          # rows per launch: 2048 x 4096 floats = 32 MiB, the largest buffer of this file


def sweep_chunks(C):
    return [(a, min(a + CHUNK, C)) for a in range(0, C, CHUNK)]


@pytest.mark.parametrize("C", SWEEP_C)
def test_class_addressing_one_hot(C):
    """Row t: logit 0 at class t, -inf elsewhere, q = 1, every class t of [0, C) (so 0, 63, 64, 65, C - 1 and every lane / slot seam): pred == t, and
    log p = 0 exactly, so the confidences are conf_noise and tokens_out is the rule on conf_noise (k = 3, distinct noise)."""
    for a, e in sweep_chunks(C):
        rows = e - a
        t = torch.arange(a, e)
        lc = torch.full((rows, C), NEG)
        lc[torch.arange(rows), t] = 0.0
        cn = (torch.randperm(rows, generator=torch.Generator().manual_seed(C)).float() - rows // 2) * 0.25
        tokens = torch.full((1, rows, 1), C, dtype=torch.int64)
        pred, out = run_step(lc, None, 0.0, 1.0, torch.ones(rows, C), cn, tokens, C, k_mask_len=3)
        assert torch.equal(pred.reshape(-1), t)
        k = R.k_reference(tokens, C, 3)
        assert torch.equal(out, expected_out(cn.reshape(1, rows), pred.reshape(1, rows), [k], C).reshape(1, rows, 1))
        assert int((out == C).sum()) == min(max(k, 0), rows)


@pytest.mark.parametrize("C", SWEEP_C)
def test_noise_addressing(C):
    """Equal logits, q = 1 except q_t = 0.5: the ratio of class t is twice every other (division by a power of two is exact), pred == t."""
    for a, e in sweep_chunks(C):
        rows = e - a
        t = torch.arange(a, e)
        q = torch.ones(rows, C)
        q[torch.arange(rows), t] = 0.5
        tokens = torch.full((1, rows, 1), C, dtype=torch.int64)
        pred, _ = run_step(torch.zeros(rows, C), None, 0.0, 1.0, q, torch.zeros(rows), tokens, C, k_mask_len=1)
        assert torch.equal(pred.reshape(-1), t)


PAIRS = ((0, 1), (2, 65), (65, 66), (63, 64), (70, 129), (1, 64), (127, 128), (63, 4032), (4031, 4095), (190, 1000), (62, 2047))


@pytest.mark.parametrize("C", SWEEP_C)
def test_tie_rule_lowest_index(C):
    """Row 0: all logits equal, q = 1: pred == 0.  Row i: classes a < b share the top (0 against -4 elsewhere): pred == a, with the lower index in a
    higher lane than the other ((2, 65), (63, 64), (70, 129), (63, 4032) ...), in the same register slot or an earlier one."""
    pairs = [(a, b) for a, b in PAIRS + ((0, C - 1), (C - 2, C - 1)) if 0 <= a < b < C]
    rows = 1 + len(pairs)
    lc = torch.full((rows, C), -4.0)
    lc[0] = 1.5
    want = [0]
    for i, (a, b) in enumerate(pairs, start=1):
        lc[i, a] = lc[i, b] = 0.0
        want.append(a)
    tokens = torch.full((1, rows, 1), C, dtype=torch.int64)
    pred, _ = run_step(lc, None, 0.0, 1.0, torch.ones(rows, C), torch.zeros(rows), tokens, C, k_mask_len=1)
    assert pred.reshape(-1).tolist() == want


@pytest.mark.parametrize("C", (8, 100, 1024, 4096))
def test_cfg_combine_exact(C):
    """logits_c = 1 everywhere; logits_u = -2 at class t and +inf elsewhere; scale 2: the combine 1 + 2 (1 - u) is 7 at t and -inf elsewhere, exact in
    float32, so the one-hot is placed by the combine alone: pred == t and the confidence is conf_noise.  The last rows are exact ties under the three
    roundings of the reference's combine at scale 7.1 that a contraction to x + fma(s, d) breaks in favour of the HIGHER class."""
    ts = sorted({0, 1, 5, 63 % C, 64 % C, 65 % C, C // 2, C - 1})
    rows = len(ts)
    lc, lu = torch.ones(rows, C), torch.full((rows, C), math.inf)
    lu[torch.arange(rows), torch.tensor(ts)] = -2.0
    cn = torch.arange(rows).float() * 0.5 - 1.0
    tokens = torch.full((1, rows, 1), C, dtype=torch.int64)
    pred, out = run_step(lc, lu, 2.0, 1.0, torch.ones(rows, C), cn, tokens, C, k_mask_len=2)
    assert pred.reshape(-1).tolist() == ts
    assert torch.equal(out.reshape(1, rows), expected_out(cn.reshape(1, rows), pred.reshape(1, rows), [2], C))
    # no contraction in the combine
    lc, lu, want = fma_rows(C)
    rows = lc.shape[0]
    tokens = torch.full((1, rows, 1), C, dtype=torch.int64)
    pred, _ = run_step(lc, lu, R.f32(7.1), 1.0, torch.ones(rows, C), torch.zeros(rows), tokens, C, k_mask_len=1)
    assert pred.reshape(-1).tolist() == want


def test_renormalisation_exact_rows():
    """``renorm_flip_rows``: classes 1 and 33 tie exactly when the draw is argmax(fl(fl(p / sum p) / q)) (pred = 1) and do not when Categorical's
    renormalisation is lost (pred = 33).  IEEE operations only, for any expf of 1 ulp."""
    lc, q, want, _ = R.renorm_flip_rows(8)
    rows = lc.shape[0]
    tokens = torch.full((1, rows, 1), 64, dtype=torch.int64)
    pred, _ = run_step(lc, None, 0.0, 1.0, q, torch.zeros(rows), tokens, 64, k_mask_len=1)
    assert pred.reshape(-1).tolist() == want


def test_confidence_from_p_exact_rows():
    """``conf_pn_rows``: samples of two masked slots in which log p and log pn of slot 0 lie on different sides of slot 1's exact confidence; k = 1
    re-masks the slot the reference's confidence (from p, sampling.py:113) makes the smaller."""
    lc, cn, want, _ = R.conf_pn_rows(6)
    n = lc.shape[0]
    tokens = torch.full((n, 2, 1), 8, dtype=torch.int64)
    pred, out = run_step(lc, None, 0.0, 1.0, torch.ones(2 * n, 8), cn, tokens, 8, k_mask_len=1)
    assert pred.reshape(n, 2).tolist() == [[1, 3]] * n
    assert torch.equal(out, want)


def fma_rows(C, count=8):
    x, y, w = R.fma_flip_pairs(count)
    lc, lu = torch.full((count, C), NEG), torch.zeros(count, C)
    want = []
    for i in range(count):
        a = (i * 37) % (C - 1)
        b = C - 1 if i % 2 == 0 else a + 1
        lc[i, a], lu[i, a] = x[i], y[i]
        lc[i, b], lu[i, b] = w[i], w[i]
        want.append(a)
    return lc, lu, want


# ---- exact: the threshold stage ------------------------------------------------------------------------------------------------------------------
COUNTS = ("zero", "one", "two", "all", "half")
THRESH_SHAPES = ((1, 1), (1, 3), (2, 1), (2, 3), (2, 17), (63, 1), (63, 3), (63, 17), (511, 3), (512, 3), (1000, 3), (1024, 3), (1025, 1), (1025, 3),
                 (1025, 17), (2048, 3), (8192, 1), (8192, 3))


def thresh_inputs(P, B, variant):
    """One-hot logits over C = 2 (so conf == conf_noise exactly), masked counts 0 / 1 / 2 / P / P // 2 over the samples, rotated by ``variant`` so that
    each of them is sample 0's in turn; conf_noise on a grid of P // 4 + 2 values (ties, at the threshold too)."""
    g = torch.Generator().manual_seed(1000 * P + 10 * B + variant)
    C = 2
    t = torch.randint(0, C, (B, P), generator=g)
    lc = torch.full((B * P, C), NEG)
    lc[torch.arange(B * P), t.reshape(-1)] = 0.0
    cn = (torch.randint(0, P // 4 + 2, (B, P), generator=g).float() - P // 8) * 0.25
    tokens = torch.randint(0, C, (B, P), generator=g)
    for b in range(B):
        nm = {"zero": 0, "one": min(1, P), "two": min(2, P), "all": P, "half": P // 2}[COUNTS[(b + variant) % len(COUNTS)]]
        tokens[b, torch.randperm(P, generator=g)[:nm]] = C
    return lc, cn, tokens, t


@pytest.mark.parametrize("P,B", THRESH_SHAPES)
def test_threshold_stage_exact(P, B):
    """Plain and edit step over masked counts 0, 1, 2, P (the wrapped indices sorted[-2] and sorted[-1] included), k_mask_len 0, 1, the masked count - 1
    and above it, ties and +inf at the threshold; the plain step takes SAMPLE 0's count for every sample, the edit step each sample's own and
    leaves a sample with fewer than two masked slots as pred.  P = 1 with no masked slot is left out: the reference indexes sorted[-2] of one value
    there and raises.  One launch of each size runs with pred_out = NULL."""
    C = 2
    for variant in range(len(COUNTS)):
        lc, cn, tokens, t = thresh_inputs(P, B, variant)
        masked = tokens == C
        nm = masked.sum(dim=1).tolist()
        want_pred = torch.where(masked, t, tokens)
        conf = torch.where(masked, torch.zeros(B, P), torch.full((B, P), math.inf)) + cn          # log 1 + noise; +inf at known slots
        q = torch.ones(B * P, C)
        for j, kml in enumerate((0, 1, nm[0] - 1, nm[0] + 5)):
            k = R.k_reference(tokens, C, kml)
            if k - 1 < -P:
                continue
            pred, out = run_step(lc, None, 0.0, 1.0, q, cn, tokens.reshape(B, P, 1), C, k_mask_len=kml, want_pred=(j != 3))
            assert pred is None or torch.equal(pred.reshape(B, P), want_pred), (variant, kml)
            assert torch.equal(out.reshape(B, P), expected_out(conf, want_pred, [k] * B, C)), (variant, kml, nm)
        num_regen = torch.tensor([max(n_, 1) + (b % 2) * 3 for b, n_ in enumerate(nm)], dtype=torch.int32)
        for j, ratio in enumerate((0.0, 0.3, R.f32(0.7), 1.5)):
            ks = R.k_edit(tokens, C, ratio, num_regen)
            pred, out = run_step(lc, None, 0.0, 1.0, q, cn, tokens.reshape(B, P, 1), C, ratio=ratio, num_regen=num_regen, want_pred=(j != 0))
            assert pred is None or torch.equal(pred.reshape(B, P), want_pred), (variant, ratio)
            want = expected_out(conf, want_pred, ks, C)
            assert torch.equal(out.reshape(B, P), want), (variant, ratio, nm)
            assert torch.equal(want[~masked], tokens[~masked])                                    # (the edit rule never re-masks a known slot)


def test_sample_zero_rule_and_float32_floor():
    """Samples with 10 / 9 / 40 / 3 masked slots of 63, distinct noise.  Plain step, k_mask_len 7: k = min(7, 10 - 1) = 7 from sample 0 for all; sample
    3 has 3 masked slots, its 7-th smallest confidence is a known slot's +inf, and it is re-masked whole.  k_mask_len 30: k = 9 for all.  Edit step,
    ratio 0.7f with num_regen 10: floor(0.7f * 10) is 7 in float32 (the product rounds to 7.0) and 6 in float64; 7 slots are re-masked."""
    C, P, B = 2, 63, 4
    g = torch.Generator().manual_seed(5)
    nm = [10, 9, 40, 3]
    t = torch.randint(0, C, (B, P), generator=g)
    lc = torch.full((B * P, C), NEG)
    lc[torch.arange(B * P), t.reshape(-1)] = 0.0
    cn = torch.stack([torch.randperm(P, generator=g).float() * 0.125 - 3.0 for _ in range(B)])
    tokens = torch.randint(0, C, (B, P), generator=g)
    for b in range(B):
        tokens[b, torch.randperm(P, generator=g)[:nm[b]]] = C
    masked = tokens == C
    want_pred = torch.where(masked, t, tokens)
    conf = torch.where(masked, torch.zeros(B, P), torch.full((B, P), math.inf)) + cn
    q = torch.ones(B * P, C)
    for kml, k, counts in ((7, 7, [7, 7, 7, P]), (30, 9, [9, 9, 9, P])):
        assert R.k_reference(tokens, C, kml) == k
        pred, out = run_step(lc, None, 0.0, 1.0, q, cn, tokens.reshape(B, P, 1), C, k_mask_len=kml)
        assert torch.equal(pred.reshape(B, P), want_pred)
        assert torch.equal(out.reshape(B, P), expected_out(conf, want_pred, [k] * B, C))
        assert (out.reshape(B, P) == C).sum(dim=1).tolist() == counts
    ratio = R.f32(0.7)
    assert R.mask_len32(ratio, 10) == 7 and math.floor(ratio * 10) == 6
    num_regen = torch.tensor([10, 10, 63, 10], dtype=torch.int32)
    ks = R.k_edit(tokens, C, ratio, num_regen)
    assert ks == [7, 7, 39, 2]
    pred, out = run_step(lc, None, 0.0, 1.0, q, cn, tokens.reshape(B, P, 1), C, ratio=ratio, num_regen=num_regen)
    assert torch.equal(out.reshape(B, P), expected_out(conf, want_pred, ks, C))
    assert (out.reshape(B, P) == C).sum(dim=1).tolist() == ks


# ---- random cases against the float64 checkers -------------------------------------------------------------------------------------------------
def run_case(inp, B0=None, B1=None):
    C = inp["logits_c"].shape[-1]
    sl = slice(B0, B1)
    P = inp["tokens"].shape[1] * inp["tokens"].shape[2]
    nb = inp["tokens"][sl].shape[0]
    first = 0 if B0 is None else B0
    q = inp["exp_noise"].reshape(-1, P, C)[first:first + nb].reshape(-1, C)
    lu = None if inp["logits_u"] is None else inp["logits_u"][sl]
    if inp["edit"]:
        return run_step(inp["logits_c"][sl], lu, inp["scale"], inp["temperature"], q, inp["conf_noise"][sl], inp["tokens"][sl], C,
                        ratio=inp["mask_ratio"], num_regen=inp["num_regen"][sl])
    return run_step(inp["logits_c"][sl], lu, inp["scale"], inp["temperature"], q, inp["conf_noise"][sl], inp["tokens"][sl], C,
                    k_mask_len=inp["k_mask_len"])


@pytest.mark.parametrize("case", R.RANDOM_CASES, ids=lambda c: c.name)
def test_random_case_against_float64_checkers(case):
    """Every masked row's pred within delta_draw of the float64 top score, every known row's pred its token; with the kernel's own pred every slot
    outside the 2 delta_conf band on the right side of the float64 threshold and the re-masked count exactly k."""
    inp = R.make_case(case)
    pred, out = run_case(inp)
    bad, sd, st = R.check_step(inp, pred, out)
    print(f"{case.name}: masked rows {sd['masked_rows']}, rows with more than one candidate {sd['multi_share']:.2%}, "
          f"smallest k-th gap / band {st['min_gap_over_band']:.3g}")
    assert not bad, bad
    assert sd["multi_share"] <= 0.01 and st["min_gap_over_band"] > 1.0


# ---- invariance ------------------------------------------------------------------------------------------------------------------------------------
def test_same_launch_twice_and_sample_alone():
    """The same launch twice: equal outputs.  A sample's rows give the same pred (and, under the per-sample edit rule, the same tokens_out) whether
    the sample runs alone or as sample 5 of 17."""
    case = R.Case("c100_p63_b17_edit", 100, 21, 3, 17, 6.0, True, 3.0, 0.6, True, 211)
    inp = R.make_case(case)
    pred, out = run_case(inp)
    pred2, out2 = run_case(inp)
    assert torch.equal(pred, pred2) and torch.equal(out, out2)
    bad, _, _ = R.check_step(inp, pred, out)
    assert not bad, bad
    p5, o5 = run_case(inp, 5, 6)
    assert torch.equal(p5[0], pred[5]) and torch.equal(o5[0], out[5])


# ---- the accepted sizes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,P", [(4097, 1), (2, 8193)])
def test_sizes_past_the_bound_are_refused_without_a_launch(C, P):
    """C = 4096 and P = 8192 are served (the class sweep at C = 4096, the threshold cases at P = 8192, B = 1 and 3, with C = 2); one more is refused
    with 'too large' and nothing is written."""
    from maskbit_amd import _lib
    lib = _lib.load()
    lc = torch.zeros(P, C, device=DEV)
    q = torch.ones(P, C, device=DEV)
    cn = torch.zeros(P, device=DEV)
    tokens = torch.full((1, P, 1), C, dtype=torch.int64, device=DEV)
    nr = torch.full((1,), P, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    for edit in (False, True):
        out, pred = torch.full_like(tokens, -7), torch.full_like(tokens, -9)
        if edit:
            rc = lib.mb_sample_step_edit(lc.data_ptr(), None, 0.0, 1.0, q.data_ptr(), cn.data_ptr(), 0.5, nr.data_ptr(), tokens.data_ptr(),
                                         out.data_ptr(), pred.data_ptr(), 1, P, 1, C, s)
        else:
            rc = lib.mb_sample_step(lc.data_ptr(), None, 0.0, 1.0, q.data_ptr(), cn.data_ptr(), 1, tokens.data_ptr(), out.data_ptr(), pred.data_ptr(),
                                    1, P, 1, C, s)
        assert rc != 0 and b"too large" in lib.mb_last_error()
        torch.cuda.synchronize()
        assert bool((out == -7).all()) and bool((pred == -9).all())
