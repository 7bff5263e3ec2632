"""Exact GPU tests of the attention launches (attention.hip): attention_kernel<DH, 0 / 4 / 5>, attention_long_kernel<DH, pair or not> and
attention_probs_kernel<DH>, one launch at a time through mb_attention, mb_attention_pair(_f4) and mb_attention_probs, at every length where the code
takes another path: 1 .. 288 around the 16-key tiles and the 256-key mask boundary of the one-block kernel, 289 .. 1025 around the 128-key blocks of
the streaming kernels.

The inputs are the cases of tests/attention_reference.py.  EXACT cases (grouped keys, permutations, the scale probe) must come out EQUAL to the
expected fp16 rows, bit for bit; BAND cases (rising / falling / spiked / Gaussian scores) must stay inside the per-element bound derived from the
operations.  Inputs and outputs live in the middle of NaN-filled buffers (bytes: 0xA5) with 320 guard rows on either side: a key row staged from
beyond the last sequence is a NaN in the output, a store outside the output is a changed guard.  Every exact launch runs twice (equal bits) and
sequence 1 alone must equal sequence 1 inside the batch.  tests/test_attention_cpu.py proves that this net tells the wrong kernels of
attention_reference.FAULTS from the right one; profiles/attention_exact.md records the derivation of the band and what was measured."""
import functools

import pytest
import torch

import attention_reference as R
from hip_helpers import attention, attention_pair, attention_probs, f4_block_exponent, f4_decode, f4_scale_index

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 320                                  # guard rows: more than the 288 key rows the one-block kernel stages


def _lib():
    from maskbit_amd import _lib as L
    return L.load()


def _guarded(rows, cols, dtype):
    buf = torch.full((rows + 2 * GUARD, cols), 0xA5 if dtype == torch.uint8 else float("nan"), device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + rows]


def _guards_untouched(buf):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]])
    return bool((g == 0xA5).all()) if buf.dtype == torch.uint8 else bool(torch.isnan(g).all())


def _input(qkv):
    """The packed rows in the middle of a NaN-filled buffer: rows read beyond either end of the batch are NaN."""
    _, view = _guarded(qkv.shape[0], qkv.shape[1], torch.float16)
    view.copy_(qkv)
    return view


def _launch(lib, c, pairs, qkv=None, nseq=None):
    """One launch of mb_attention (pairs = 0) or mb_attention_pair on case c -> the fp16 output rows (guards and NaN checked)."""
    x = _input(c.qkv if qkv is None else qkv)
    nseq = nseq or c.nseq
    buf, out = _guarded(nseq * c.N, c.d, torch.float16)
    if pairs:
        attention_pair(lib, x, out, nseq // 2, c.N, c.d, c.heads)
    else:
        attention(lib, x, out, nseq, c.N, c.d, c.heads)
    torch.cuda.synchronize()
    assert _guards_untouched(buf), f"{c.label}: guard rows written"
    return out.cpu()


def _where(c, idx):
    r, col = idx
    s, q, h = r // c.N, r % c.N, col // c.dh
    tgt = f", aims at group {int(c.target[s, h, q])}" if c.target is not None else ""
    return f"sequence {s} query {q} head {h} column {col % c.dh}{tgt}"


def _equal(c, got, want, what):
    assert not bool(torch.isnan(got).any()), f"{c.label} {what}: {int(torch.isnan(got).sum())} output elements are NaN (unwritten, or a NaN key row was staged)"
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        first = bad[0].tolist()
        raise AssertionError(f"{c.label} {what}: {len(bad)} of {got.numel()} elements differ from the exact result, first at {_where(c, first)}: "
                             f"{float(got[tuple(first)])} != {float(want[tuple(first)])}; sequences {sorted(set((bad[:, 0] // c.N).tolist()))}")


def _in_band(c, got, ref, bound, what):
    assert not bool(torch.isnan(got).any()), f"{c.label} {what}: NaN in the output"
    ratio = (got.double() - ref).abs() / bound
    worst = float(ratio.max())
    print(f"{c.label} {what}: largest error / bound {worst:.3f}")
    assert worst <= 1.0, f"{c.label} {what}: error {worst:.2f} x the bound at {_where(c, divmod(int(ratio.argmax()), c.d))}"
    return worst


ALL_N = R.ONE_BLOCK_N + R.STREAM_N
SHAPES = [(N, d, heads) for N in ALL_N for d, heads in R.widths(N)]


@functools.lru_cache(maxsize=None)
def _exact_cases(nseq, N, d, heads):
    cases = [(R.grouped_case(nseq, N, d, heads), R.expected_grouped)]
    if N <= d // heads:
        cases.append((R.permutation_case(nseq, N, d, heads), R.expected_permutation))
    if N >= 2:
        cases.append((R.scale_case(nseq, N, d, heads), R.expected_scale))
    return cases


def _exact(N, d, heads, pairs):
    lib = _lib()
    nseq = 2 * pairs if pairs else R.NSEQ
    for c, expected in _exact_cases(nseq, N, d, heads):
        want = expected(c, pairs) if pairs else expected(c)
        got = _launch(lib, c, pairs)
        _equal(c, got, want, "pair" if pairs else "plain")
        again = _launch(lib, c, pairs)
        assert torch.equal(got.view(torch.int16), again.view(torch.int16)), f"{c.label}: two runs differ"
        # sequence 1 (pair form: pair 1) alone = the same rows inside the batch
        rows = c.qkv.reshape(nseq, N, 3 * d)
        if pairs:
            alone = _launch(lib, c, pairs, qkv=rows[[1, pairs + 1]].reshape(2 * N, 3 * d), nseq=2)
            inside = got.reshape(nseq, N, d)[[1, pairs + 1]].reshape(2 * N, d)
        else:
            alone = _launch(lib, c, 0, qkv=rows[1], nseq=1)
            inside = got.reshape(nseq, N, d)[1]
        assert torch.equal(alone.view(torch.int16), inside.view(torch.int16)), f"{c.label}: sequence 1 alone differs from sequence 1 in the batch"


@pytest.mark.parametrize("N,d,heads", SHAPES)
def test_plain_attention_exact_cases(N, d, heads):
    """mb_attention: all-zero queries (uniform over exactly N keys), key N - 1 in a group of one or two, groups across tiles and blocks"""
    _exact(N, d, heads, 0)


@pytest.mark.parametrize("N,d,heads", SHAPES)
def test_pair_attention_exact_cases(N, d, heads):
    """mb_attention_pair: conditional rows as above; twin rows = fp16(o_u - o_c) with o_c needing 12 - 13 bits: the subtraction is in fp32"""
    _exact(N, d, heads, R.PAIRS)


@pytest.mark.parametrize("N,d,heads", SHAPES)
def test_plain_attention_band_cases(N, d, heads):
    lib = _lib()
    worst = 0.0
    for kind, seed in R.BAND_CASES:
        c = R.band_case(kind, seed, R.NSEQ, N, d, heads)
        ref, bound = R.band_plain(c)
        worst = max(worst, _in_band(c, _launch(lib, c, 0), ref, bound, "plain"))
    print(f"plain N {N} d {d} heads {heads}: largest error / bound over the ten band cases {worst:.3f}")


@pytest.mark.parametrize("N,d,heads", SHAPES)
def test_pair_attention_band_cases(N, d, heads):
    lib = _lib()
    worst = 0.0
    for kind, seed in R.BAND_CASES:
        c = R.band_case(kind, seed, 2 * R.PAIRS, N, d, heads)
        ref, bound = R.band_pair(c, R.PAIRS)
        worst = max(worst, _in_band(c, _launch(lib, c, R.PAIRS), ref, bound, "pair"))
    print(f"pair N {N} d {d} heads {heads}: largest error / bound over the ten band cases {worst:.3f}")


# ---- e2m1 copies -------------------------------------------------------------------------------------------------------------------------------------------
def _f4_buffers(c, nseq_f4, n):
    """n x (guarded out4 [rows, 2d] bytes, guarded scale bytes)"""
    return [(_guarded(c.nseq * c.N, 2 * c.d, torch.uint8), _guarded(c.heads * nseq_f4 * (c.N - 1), 1, torch.uint8)) for _ in range(n)]


def _f4_check(c, out4, scales, nseq_f4, tile, what, check_scale=True):
    """decode(out4) * 2^(scale - 127) == tile [nseq_f4 N, d] float64 on the token rows of the first nseq_f4 sequences, the scale byte ==
    f4_block_exponent(amax) - 2 clamped at 0; every other byte of both buffers untouched."""
    N, d, heads = c.N, c.d, c.heads
    out4, scales = out4.cpu(), scales.cpu().flatten()
    r = torch.arange(c.nseq * N)
    seq, tok = r // N, r % N
    keep = (seq < nseq_f4) & (tok < N - 1)
    assert bool((out4[~keep] == 0xA5).all()), f"{c.label} {what}: e2m1 bytes written in class-token or twin rows"
    assert bool((out4[:, d // 2:] == 0xA5).all()), f"{c.label} {what}: e2m1 bytes written past the d / 2 of a row"
    idx = torch.stack([f4_scale_index(h, nseq_f4, seq[keep], tok[keep], (N - 1) // 64) for h in range(heads)], 1)        # [rows, heads]
    written = torch.zeros_like(scales, dtype=torch.bool)
    written[idx.flatten()] = True
    assert int(written.sum()) == idx.numel() and bool((scales[~written] == 0xA5).all()), f"{c.label} {what}: scale bytes written outside the token rows"
    sb = scales[idx].double()                                                                                        # [rows, heads]
    dec = f4_decode(out4[keep], d).reshape(-1, heads, 64) * (2.0 ** (sb - 127)).unsqueeze(-1)
    want = tile[keep[: nseq_f4 * N]].reshape(-1, heads, 64)
    if not torch.equal(dec, want):
        bad = (dec != want).nonzero()[0].tolist()
        raise AssertionError(f"{c.label} {what}: {int((dec != want).sum())} decoded e2m1 values differ from the fp32 tile, first at token row {bad[0]} head {bad[1]} "
                             f"column {bad[2]}: {float(dec[tuple(bad)])} != {float(want[tuple(bad)])}")
    if check_scale:
        amax = want.abs().amax(-1)
        assert bool((amax > 0).all())
        assert torch.equal(sb, (f4_block_exponent(amax) - 2).clamp(min=0).double()), f"{c.label} {what}: scale bytes differ from f4_block_exponent(amax) - 2"


@pytest.mark.parametrize("N", R.F4_N)
def test_plain_attention_e2m1_copy_is_the_fp32_tile(N):
    """mb_attention with out4 (attention_kernel<64, 5>, attention_long_kernel<64>): V from the e2m1 grid, every query on one key"""
    lib = _lib()
    d, heads = (64, 1) if N == 1025 else (128, 2)
    c = R.f4_value_case(R.NSEQ, N, d, heads)
    want = R.expected_grouped(c)
    x = _input(c.qkv)
    buf, out = _guarded(c.nseq * N, d, torch.float16)
    ((b4, o4), (bs, os_)), = _f4_buffers(c, c.nseq, 1)
    attention(lib, x, out, c.nseq, N, d, heads, o4, os_)
    torch.cuda.synchronize()
    assert _guards_untouched(buf) and _guards_untouched(b4) and _guards_untouched(bs)
    _equal(c, out.cpu(), want, "plain with e2m1 copy")
    assert torch.equal(out.cpu().view(torch.int16), _launch(lib, c, 0).view(torch.int16)), "fp16 rows differ from the launch without the copy"
    _f4_check(c, o4, os_, c.nseq, want.double(), "plain")


@pytest.mark.parametrize("lo", [False, True])
@pytest.mark.parametrize("N", R.F4_N)
def test_pair_attention_e2m1_copies_are_the_fp32_tiles(N, lo):
    """mb_attention_pair_f4 (attention_kernel<64, 4>, attention_long_kernel<64, true>): the value copy of the conditional rows; with `lo` also the copy of
    o - fp16(o), once all zero (value case) and once +- one power of two from size-2 groups whose average needs 12 bits"""
    lib = _lib()
    d, heads = (64, 1) if N == 1025 else (128, 2)
    P = R.PAIRS
    for c in [R.f4_value_case(2 * P, N, d, heads)] + ([R.f4_lo_case(2 * P, N, d, heads)] if lo else []):
        value_case = c.label.startswith("e2m1 values")
        want = R.expected_grouped(c, P)
        x = _input(c.qkv)
        buf, out = _guarded(c.nseq * N, d, torch.float16)
        f4 = _f4_buffers(c, P, 2 if lo else 1)
        flat = [v for (_, v4), (_, vs) in f4 for v in (v4, vs)] + [None] * (4 - 2 * len(f4))
        attention_pair(lib, x, out, P, N, d, heads, *flat)
        torch.cuda.synchronize()
        assert _guards_untouched(buf) and all(_guards_untouched(b4) and _guards_untouched(bs) for (b4, _), (bs, _) in f4)
        _equal(c, out.cpu(), want, "pair with e2m1 copy")
        assert torch.equal(out.cpu().view(torch.int16), _launch(lib, c, P).view(torch.int16)), "fp16 rows differ from the launch without the copy"
        o_c = R.exact_grouped(c)[: P * N]                                        # one V row, or the mean of two
        if value_case:
            _f4_check(c, f4[0][0][1], f4[0][1][1], P, o_c, "pair values")
        if lo:
            lo_tile = o_c - o_c.half().double()
            assert value_case == (not bool(lo_tile.any()))
            _f4_check(c, f4[1][0][1], f4[1][1][1], P, lo_tile, "pair lo halves", check_scale=not value_case)


def test_shapes_without_an_e2m1_copy():
    """head width 32 or N = 300: the pair entry refuses, the plain entry computes the rows and writes no copy"""
    lib = _lib()
    for N, d, heads in ((257, 128, 4), (300, 128, 2), (65, 128, 2)):
        c = R.grouped_case(2 * R.PAIRS, N, d, heads)
        x = _input(c.qkv)
        buf, out = _guarded(c.nseq * N, d, torch.float16)
        ((b4, o4), (bs, os_)), = _f4_buffers(c, c.nseq, 1)
        with pytest.raises(RuntimeError, match="no e2m1 copy"):
            attention_pair(lib, x, out, R.PAIRS, N, d, heads, o4, os_)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf).all()), "a refused launch wrote rows"
        attention(lib, x, out, c.nseq, N, d, heads, o4, os_)
        torch.cuda.synchronize()
        _equal(c, out.cpu(), R.expected_grouped(c), "plain, copy asked for")
        assert bool((b4 == 0xA5).all()) and bool((bs == 0xA5).all()), f"N {N} heads {heads}: an e2m1 copy was written"


def test_entries_refuse_head_widths_other_than_32_and_64():
    lib = _lib()
    x = torch.zeros(2 * 17, 3 * 96, device=DEV, dtype=torch.float16)
    out = torch.full((2 * 17, 96), float("nan"), device=DEV, dtype=torch.float16)
    p = torch.full((2, 17, 17), float("nan"), device=DEV)
    for heads in (1, 2, 6):                                                  # 96, 48, 16
        with pytest.raises(RuntimeError, match="head width"):
            attention(lib, x, out, 2, 17, 96, heads)
        with pytest.raises(RuntimeError, match="head width"):
            attention_pair(lib, x, out, 1, 17, 96, heads)
        with pytest.raises(RuntimeError, match="head width"):
            attention_probs(lib, x, p, 2, 17, 96, heads)
    with pytest.raises(RuntimeError, match="bad arguments"):
        attention(lib, x, out, 2, 17, 96, 3, out)                            # out4 without its scales
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(p).all())


# ---- head-averaged probabilities -------------------------------------------------------------------------------------------------------------------------
def _probs(lib, c):
    x = _input(c.qkv)
    buf, out = _guarded(c.nseq * c.N, c.N, torch.float32)
    attention_probs(lib, x, out, c.nseq, c.N, c.d, c.heads)
    torch.cuda.synchronize()
    assert _guards_untouched(buf)
    got = out.cpu().reshape(c.nseq, c.N, c.N)
    assert not bool(torch.isnan(got).any()), f"{c.label}: unwritten probabilities"
    return got


@pytest.mark.parametrize("N,d,heads", [(N, d, heads) for N in R.PROBS_N for d, heads in R.widths(N)])
def test_attention_probs_exact_and_band_cases(N, d, heads):
    lib = _lib()
    c = R.grouped_case(R.NSEQ, N, d, heads, zero_every=0)
    got, want = _probs(lib, c), R.expected_probs_grouped(c)
    err = (got.double() - want).abs()
    assert float(err.max()) <= 1e-30, f"{c.label}: probabilities differ from sum_h [j in S_h(i)] / (heads |S_h(i)|) by {float(err.max()):.3e} at {divmod(int(err.argmax()), N)}"
    assert float((got.double().sum(-1) - 1).abs().max()) <= 1e-6
    assert torch.equal(got, _probs(lib, c)), "two runs differ"
    worst = 0.0
    for kind, seed in R.BAND_CASES:
        b = R.band_case(kind, seed, R.NSEQ, N, d, heads)
        ref, bound = R.band_probs(b)
        g = _probs(lib, b).double()
        ratio = (g - ref).abs() / bound
        worst = max(worst, float(ratio.max()))
        assert float(ratio.max()) <= 1.0, f"{b.label}: probability error {float(ratio.max()):.2f} x the bound"
    print(f"probs N {N} d {d} heads {heads}: largest error / bound over the ten band cases {worst:.3f}")
