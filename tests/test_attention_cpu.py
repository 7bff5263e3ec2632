"""The net of tests/test_hip_attention_exact.py has no blind spot (no GPU needed): the builders of tests/attention_reference.py keep their own
promises at every shape the GPU file launches, the float64 reference is torch's scaled_dot_product_attention, every wrong kernel of
attention_reference.FAULTS changes the expected output of an exact case (and, unless it is a single rounding, leaves the band of a band case), and the
right kernel's arithmetic -- fp16 probabilities, fp32 sums -- stays inside the band."""
import pytest
import torch

import attention_reference as R

ALL_N = R.ONE_BLOCK_N + R.STREAM_N


@pytest.mark.parametrize("N", ALL_N)
def test_builders_hold_at_every_launched_shape(N):
    for d, heads in R.widths(N):
        for nseq, pairs in ((R.NSEQ, 0), (2 * R.PAIRS, R.PAIRS)):
            c = R.grouped_case(nseq, N, d, heads)                               # (check_grouped runs inside)
            sizes = R.group_sizes(N, d // heads)
            assert set(sizes) >= {1 << k for k in range(8) if (1 << (k + 1)) - 1 <= N}, "every size 1 .. 128 that fits occurs"
            last = torch.gather(c.group, 2, torch.full((nseq, heads, 1), N - 1)).flatten()
            assert all(sizes[g] <= 2 for g in last.tolist()), "key N - 1 sits in a group of one or two"
            if N >= 3 and nseq * heads >= 2:
                assert {sizes[g] for g in last.tolist()} == {1, 2}
            assert bool((c.target < 0).any()) and bool((c.target >= 0).any()) or N == 1
            want = R.expected_grouped(c, pairs)
            ref = (R.pair(c.qkv, pairs, N, d, heads) if pairs else R.plain(c.qkv, nseq, N, d, heads)).half()
            assert torch.equal(want, ref), "the float64 softmax and the group arithmetic disagree"
            v = R.split(c.qkv, nseq, N, d, heads)[2]
            if N > 1:
                assert float(v[:, :, N - 1].abs().min()) >= 8 and len({tuple(r.tolist()) for r in v[:, :, N - 1].reshape(-1, d // heads)}) == nseq * heads
            if N >= 2:
                s = R.scale_case(nseq, N, d, heads)
                assert torch.equal(R.expected_scale(s, pairs), (R.pair(s.qkv, pairs, N, d, heads) if pairs else R.plain(s.qkv, nseq, N, d, heads)).half())
            if N <= d // heads:
                p = R.permutation_case(nseq, N, d, heads)
                if not pairs:
                    assert torch.equal(R.expected_permutation(p), R.plain(p.qkv, nseq, N, d, heads).half())
            if N > 288 and not pairs:                                           # streaming: where the row maximum is first met, groups across blocks
                first, nblk = R.first_blocks(c)
                blocks = {b for b, _ in first}
                assert 0 in blocks and nblk - 1 in blocks and (nblk < 3 or blocks & set(range(1, nblk - 1))), (N, blocks)
                assert any(many for _, many in first), "no group has members in several blocks"


@pytest.mark.parametrize("N", R.PROBS_N)
def test_probability_builders_hold(N):
    """the grouped cases without all-zero queries that the probabilities test launches: exact head means, rows summing to 1"""
    for d, heads in R.widths(N):
        c = R.grouped_case(R.NSEQ, N, d, heads, zero_every=0)                   # (check_grouped runs inside)
        assert not bool((c.target < 0).any())
        want = R.expected_probs_grouped(c)
        assert float((want.sum(-1) - 1).abs().max()) == 0.0
        assert bool(((want * heads * 128) == (want * heads * 128).round()).all()), "every weight is a multiple of 1 / (heads 2^k), k <= 7"
        assert float((R.probs(c.qkv, R.NSEQ, N, d, heads) - want).abs().max()) < 1e-15


@pytest.mark.parametrize("N", R.F4_N)
def test_e2m1_builders_hold(N):
    d, heads = (64, 1) if N == 1025 else (128, 2)
    for nseq in (R.NSEQ, 2 * R.PAIRS):
        c = R.f4_value_case(nseq, N, d, heads)
        o = R.exact_grouped(c)
        assert torch.equal(o.half(), R.plain(c.qkv, nseq, N, d, heads).half()) and torch.equal(o.half().double(), o) and len({tuple(r.tolist()) for r in o[: N - 1, :8]}) > 16      # one V row each, many different rows
        lo = R.f4_lo_case(nseq, N, d, heads)
        o = R.exact_grouped(lo)
        rem = (o - o.half().double()).reshape(nseq * N, heads, 64)
        assert set(rem.abs().unique().tolist()) == {0.0, 2.0 ** -7} and bool((rem.abs().amax(-1) > 0).all())


def test_float64_reference_is_scaled_dot_product_attention():
    torch.manual_seed(0)
    for nseq, N, d, heads in ((3, 65, 128, 2), (2, 300, 128, 4), (4, 17, 64, 1)):
        qkv = torch.randn(nseq * N, 3 * d).half()
        q, k, v = R.split(qkv, nseq, N, d, heads)
        want = torch.nn.functional.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(nseq * N, d)
        assert float((R.plain(qkv, nseq, N, d, heads) - want).abs().max()) < 1e-13
        pr = R.probs(qkv, nseq, N, d, heads)
        assert float((pr - torch.softmax(q @ k.transpose(-1, -2) / (d // heads) ** 0.5, -1).mean(1)).abs().max()) < 1e-15
        if nseq % 2 == 0:
            o = want.reshape(nseq, N, d)
            assert float((R.pair(qkv, nseq // 2, N, d, heads).reshape(nseq, N, d) - torch.cat([o[: nseq // 2], o[nseq // 2:] - o[: nseq // 2]])).abs().max()) < 1e-13


SHAPES_CPU = ((65, 128, 2), (65, 128, 4), (300, 128, 2), (385, 128, 4))
PAIR_FAULTS = ("twin_from_rounded", "twin_offset_1")


def _exact_outputs(fault, N, d, heads):
    """(wrong, right) expected fp16 outputs of every exact case at one shape, in the kernel form the fault lives in"""
    nseq, P = 2 * R.PAIRS, R.PAIRS
    out = []
    if fault == "avg_before_norm":
        c = R.grouped_case(nseq, N, d, heads, zero_every=0)
        return [(R.probs(c.qkv, nseq, N, d, heads, fault), R.expected_probs_grouped(c))]
    for c, expected in ((R.grouped_case(nseq, N, d, heads), R.expected_grouped), (R.scale_case(nseq, N, d, heads), R.expected_scale)):
        if fault in PAIR_FAULTS:
            out.append((R.pair(c.qkv, P, N, d, heads, fault).half(), expected(c, P)))
        else:
            out.append((R.plain(c.qkv, nseq, N, d, heads, fault).half(), expected(c)))
    return out


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_wrong_kernel_changes_an_exact_case(fault):
    changed = []
    for N, d, heads in SHAPES_CPU:
        for wrong, right in _exact_outputs(fault, N, d, heads):
            same = (wrong == right) | (torch.isnan(wrong) & torch.isnan(right)) if wrong.dtype == torch.float16 else (wrong - right).abs() <= 1e-30
            changed.append(int((~same).sum()))
    print(f"{fault}: elements changed per (shape, exact case) {changed}")
    assert max(changed) > 0, f"no exact case tells {fault} from the right kernel"
    if fault == "pad_copies_288":                                                # the defect found by reading: N < 256, all-zero queries and key N - 1
        c = R.grouped_case(R.NSEQ, 65, 128, 2)
        wrong, right = R.plain(c.qkv, R.NSEQ, 65, 128, 2, fault).half(), R.expected_grouped(c)
        rows = (wrong != right).any(1).reshape(R.NSEQ, 65)
        zero_q = (c.target < 0).any(1)
        assert bool(rows[zero_q].all()), "every all-zero query must see the extra copies of key N - 1"
        sizes = R.group_sizes(65, 64)
        hit = 0
        for s in range(R.NSEQ):
            for h in range(2):
                g_last = int(c.group[s, h, 64])
                if sizes[g_last] == 2:                                           # key N - 1 shares a group: weights (1 + 192) : 1 instead of 1 : 1
                    aimed = c.target[s, h] == g_last
                    cols = (wrong != right).reshape(R.NSEQ, 65, 2, 64)[s, :, h].any(-1)
                    assert bool(aimed.any()) and bool(cols[aimed].all()), "every query aimed at the size-2 group of key N - 1 must change"
                    hit += 1
        assert hit > 0


@pytest.mark.parametrize("fault", [f for f in R.FAULTS if f not in R.SINGLE_ROUNDING_FAULTS])
def test_every_wrong_kernel_leaves_the_band(fault):
    nseq, P = 2 * R.PAIRS, R.PAIRS
    worst = 0.0
    for N, d, heads in SHAPES_CPU:
        for kind, seed in R.BAND_CASES[:5]:
            c = R.band_case(kind, seed, nseq, N, d, heads)
            if fault == "avg_before_norm":
                (ref, bound), wrong = R.band_probs(c), R.probs(c.qkv, nseq, N, d, heads, fault)
            elif fault in PAIR_FAULTS:
                (ref, bound), wrong = R.band_pair(c, P), R.pair(c.qkv, P, N, d, heads, fault)
            else:
                (ref, bound), wrong = R.band_plain(c), R.plain(c.qkv, nseq, N, d, heads, fault)
            worst = max(worst, float(((wrong - ref).abs() / bound).nan_to_num(nan=float("inf")).max()))
        if worst > 1:
            break
    print(f"{fault}: largest error / bound {worst:.1f}")
    assert worst > 1.0, f"{fault} stays inside the band on every band case"


@pytest.mark.parametrize("N,d,heads", SHAPES_CPU + ((257, 128, 2), (17, 128, 4)))
def test_the_right_arithmetic_stays_inside_the_band(N, d, heads):
    nseq, P = 2 * R.PAIRS, R.PAIRS
    worst = 0.0
    for kind, seed in R.BAND_CASES:
        c = R.band_case(kind, seed, nseq, N, d, heads)
        for (ref, bound), got in ((R.band_plain(c), R.emulate_fp16_p(c)), (R.band_pair(c, P), R.emulate_fp16_p(c, P))):
            worst = max(worst, float(((got.double() - ref).abs() / bound).max()))
    print(f"N {N} d {d} heads {heads}: fp16-probability arithmetic, largest error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("N", ALL_N)
def test_the_right_arithmetic_reproduces_every_exact_case(N):
    """fp32 scores, exp2 and sums with fp16 probabilities (torch on the CPU; its roundings of max * c and 1 / sum differ from the device's) give the
    expected rows bit for bit in both forms: no exact case hangs on a tie that such a rounding decides"""
    for d, heads in R.widths(N):
        for nseq, pairs in ((R.NSEQ, 0), (2 * R.PAIRS, R.PAIRS)):
            cases = [(R.grouped_case(nseq, N, d, heads), R.expected_grouped)]
            if N >= 2:
                cases.append((R.scale_case(nseq, N, d, heads), R.expected_scale))
            if N <= d // heads:
                cases.append((R.permutation_case(nseq, N, d, heads), R.expected_permutation))
            for c, expected in cases:
                assert torch.equal(R.emulate_fp16_p(c, pairs), expected(c, pairs)), f"{c.label} pairs {pairs}"
