"""Exact GPU tests of the trunk GEMM family (gemm.hip, gemm_ht.hip): every instantiation, the edges of the tile list and the persistent walk.

Operands are the small integers of tests/gemm_reference.py, so the output of epilogues 0, 2 and 4 must EQUAL the float64 reference bit for bit (GELU
epilogues 1 and 3: float64 GELU of the exact pre-activation within the bounds of test_hip_gemm.py, 2e-3 max for fp16 and 2e-4 max for fp32 outputs).
Every output lives inside a larger buffer pre-filled with NaN (bytes: 0xA5) with a guard band of more than one full tile of rows on either side: after
the launch no NaN is left in the output and the guard bands are untouched.  Every persistent instantiation runs under mb_set_cu_count(n) for n in
0, 1, 3, 13 -- walk lengths of 1, all tiles, and ragged tails that are no multiple of the 8 XCDs -- and all runs must give the same bits (as must the
one-tile-per-workgroup forms, variant + 1000, where the entry takes a variant).  tests/test_gemm_exact_cpu.py proves that this net has no blind
spot; profiles/gemm_exact.md records what was measured (GELU error, exactness of the scaled MFMA on the mini-tile operands)."""
import itertools

import pytest
import torch

import gemm_reference as R
from hip_helpers import gemm, gemm_act_split, gemm_ex, gemm_mini, gemm_mini_split

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 288                                  # guard rows before and after an output: more than a 256-row tile and its class row


def _lib():
    from maskbit_amd import _lib as L
    return L.load()


def _guarded(rows, cols, dtype):
    """-> (whole buffer, the output view in its middle)."""
    buf = torch.full((rows + 2 * GUARD, cols), 0xA5 if dtype == torch.uint8 else float("nan"), device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + rows]


def _guards_untouched(buf):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]])
    return bool((g == 0xA5).all()) if buf.dtype == torch.uint8 else bool(torch.isnan(g).all())


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32 if t.dtype == torch.float32 else t.dtype)


def _out(c):
    """Guarded output buffers of a case -> (buf, view, out32 argument, out16 argument)."""
    rows = len(R.kept_rows(c)) if c.epi == 4 else c.M
    buf, view = _guarded(rows, c.N, torch.float16 if c.epi in (0, 1) else torch.float32)
    return buf, view, (None if c.epi in (0, 1) else view), (view if c.epi in (0, 1) else None)


def _check(c, got, want, label):
    """got against the float64 reference: equal for the exact epilogues, within the GELU bound otherwise.  -> the GELU error relative to max |ref|."""
    assert not bool(torch.isnan(got).any()), f"{label}: {int(torch.isnan(got).sum())} output elements were not written"
    if c.epi in R.EXACT_EPIS:
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            raise AssertionError(f"{label}: {len(bad)} elements differ from float64, first at (row, column) {bad[0].tolist()}: "
                                 f"{float(got[tuple(bad[0])])} != {float(want[tuple(bad[0])])}; rows {sorted(set(bad[:, 0].tolist()))[:8]}")
        return 0.0
    top = float(want.abs().max())
    err = float((got.double() - want).abs().max())
    print(f"{label}: GELU error {err:.3e} = {err / top:.2e} max |ref| (bound {2e-3 if c.epi == 1 else 2e-4:.0e})")
    assert err < (2e-3 if c.epi == 1 else 2e-4) * top, label
    return err / top


def _same_bits(first, other, label):
    if not torch.equal(_bits(first), _bits(other)):
        bad = (_bits(first) != _bits(other)).nonzero()
        raise AssertionError(f"{label}: {len(bad)} elements differ between runs, first at {bad[0].tolist()}; rows {sorted(set(bad[:, 0].tolist()))[:8]}")


def _walk(lib, counts, run):
    """run(n) under mb_set_cu_count(n) for every n; the count is restored whatever happens."""
    try:
        for n in counts:
            assert lib.mb_set_cu_count(n) == 0
            run(n)
            torch.cuda.synchronize()
    finally:
        lib.mb_set_cu_count(0)


def _run_plain(lib, c, variant):
    buf, view, o32, o16 = _out(c)
    if c.A2 is not None:
        gemm_act_split(lib, c.epi, c.A, c.A2, c.W, c.bias, c.res if c.epi == 2 else None, o32, o16, c.M, c.N, c.K, variant)
    else:
        gemm(lib, c.epi, c.A, c.W, c.bias, c.res if c.epi == 2 else None, o32, o16, c.M, c.N, c.K, c.period, variant)
    torch.cuda.synchronize()
    assert _guards_untouched(buf), f"guard band written (variant {variant})"
    return view


# ---- the 128 x 128 kernel (variant -1): every M < 512 launch, ragged N --------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("epi", [0, 1, 2, 3])
def test_small_kernel_ragged_shapes(epi, split):
    lib = _lib()
    for i, (M, N) in enumerate(itertools.product(R.SMALL_M, R.SMALL_N)):
        K = 64 if split else R.KS[i % 4]                                       # split activations: kw = 64
        c = R.make_case(epi, M, N, K, split=split, seed=100 + i, dev=DEV)
        _check(c, _run_plain(lib, c, -1), R.expected(c), f"128x128 epi {epi} M {M} N {N} K {K}{' split' if split else ''}")


@pytest.mark.parametrize("M,period", R.LOGITS_SHAPES)
def test_small_kernel_logits_epilogue_drops_every_period_th_row(M, period):
    lib = _lib()
    for i, N in enumerate(R.SMALL_N):
        c = R.make_case(4, M, N, R.KS[i], period=period, seed=200 + i, dev=DEV)
        got = _run_plain(lib, c, -1)
        assert got.shape[0] == M - M // period
        _check(c, got, R.expected(c), f"128x128 epi 4 M {M} N {N} period {period}")


# ---- the half-tile kernel: MT 6 / 8, sequence tiles, auto; persistent walks and one tile per workgroup ---------------------------------------------------
def _ht_all_runs(lib, c, label):
    """Every variant x CU count (+ the one-tile-per-workgroup forms): the first run against float64, all others against its bits."""
    first = []
    want = R.expected(c)

    def one(variant, n):
        got = _run_plain(lib, c, variant)
        if not first:
            first.append(got.clone())
            _check(c, got, want, f"{label} variant {variant}")
        else:
            _same_bits(first[0], got, f"{label} variant {variant} CUs {n}")

    for variant in R.HT_VARIANTS:
        _walk(lib, R.CU_COUNTS, lambda n: one(variant, n))
    for variant in (1006, 1008, 1257):
        one(variant, 0)


@pytest.mark.parametrize("M,N,K", R.HT_SHAPES)
def test_half_tile_kernel_all_variants_and_walks(M, N, K):
    lib = _lib()
    base = R.make_case(0, M, N, K, seed=M, dev=DEV)
    for bm in (192, 256):
        tiles = ((M + bm - 1) // bm) * (N // 256)
        print(f"half-tile M {M} N {N} K {K} MT {bm // 32}: tiles_m {(M + bm - 1) // bm} tiles_n {N // 256}, walk lengths {[R.walk_length(tiles, n) for n in R.CU_COUNTS]}")
    for epi in (0, 1, 2, 3):
        _ht_all_runs(lib, base.with_epi(epi), f"half-tile epi {epi} M {M} N {N} K {K}")


@pytest.mark.parametrize("M,N,kw", [(513, 512, 64), (771, 768, 64), (1288, 512, 512)])
def test_half_tile_kernel_split_activations(M, N, kw):
    lib = _lib()
    base = R.make_case(0, M, N, kw, split=True, seed=M + 1, dev=DEV)
    for epi in (0, 1, 2, 3):
        _ht_all_runs(lib, base.with_epi(epi), f"half-tile split epi {epi} M {M} N {N} kw {kw}")


@pytest.mark.parametrize("M,N,K", [(513, 512, 192), (2313, 768, 128)])
def test_half_tile_kernel_layernorm_residual_walks(M, N, K):
    """mb_gemm_ex re-derives LayerNorm(residual rows) from {mean, rstd} in its epilogue, in place: bit-equal to the plain-residual GEMM fed with the fp32
    rows mb_layernorm stores -- in every variant and walk."""
    from maskbit_amd import _lib as L
    lib = _lib()
    c = R.make_case(2, M, N, K, seed=M + 2, dev=DEV)
    torch.manual_seed(M)
    y = torch.randn(M, N, device=DEV) * 1.7 + 0.3
    g, b = torch.rand(N, device=DEV) + 0.5, torch.randn(N, device=DEV) * 0.2
    x32, stats = torch.empty_like(y), torch.empty(M, 2, device=DEV)
    L.check(lib.mb_layernorm(y.data_ptr(), g.data_ptr(), b.data_ptr(), 1e-12, x32.data_ptr(), None, None, stats.data_ptr(), M, N, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    c.res = x32
    plain = _run_plain(lib, c, 0).clone()

    def one(variant, n):
        buf, view = _guarded(M, N, torch.float32)
        view.copy_(y)
        gemm_ex(lib, 2, c.A, c.W, c.bias, view, view, None, M, N, K, stats, g, b, 0, variant)
        torch.cuda.synchronize()
        assert _guards_untouched(buf)
        _same_bits(plain, view, f"LayerNorm residual M {M} variant {variant} CUs {n}")

    for variant in R.HT_VARIANTS:
        _walk(lib, R.CU_COUNTS, lambda n: one(variant, n))
    for variant in (-1, 1006, 1008, 1257):
        one(variant, 0)


# ---- sequence tiles (seq_rows 257 / 1025): plain and pair, 0 / 1 / 2 mini-tile sets, the e2m1 output copies, column-split tiles ---------------------------
def _f4_out(c, rows_c, lo_copy):
    """Guarded e2m1 output copies of a GELU launch: (out4 [M, 2 N] bytes, scales) (+ the lo-half copy)."""
    nscale = (c.N // 64) * c.nseq * (c.seq_rows - 1)
    bufs = []
    for _ in range(2 if lo_copy else 1):
        bufs += [_guarded(c.M, 2 * c.N, torch.uint8), _guarded(nscale, 1, torch.uint8)]
    return bufs


def _f4_untouched(c, out4):
    """Bytes the e2m1 copy must leave alone: class-token rows, rows beyond the conditional ones, bytes past the N / 2 of a row."""
    r = torch.arange(c.M, device=DEV)
    skip = (r >= c.rows_c) | (r % c.seq_rows == c.seq_rows - 1)
    return bool((out4[skip] == 0xA5).all()) and bool((out4[:, c.N // 2:] == 0xA5).all())


def _ns(c, n):
    """The column split launch_ht picks for a plain residual GEMM with mini-tiles (gemm_ht.hip)."""
    if c.pair_rows or c.epi != 2 or not c.lo:
        return 1
    tiles = c.nseq * ((c.seq_rows - 1) // 256) * (c.N // 256)
    cus = n if n else torch.cuda.get_device_properties(0).multi_processor_count
    return 4 if tiles * 4 <= cus else 2 if tiles * 2 <= cus else 1


def _seq_runs(lib, c, label, launch, f4=False, lo_copy=False):
    want = R.expected(c)
    first = []
    splits = set()

    def one(n):
        buf, view, o32, o16 = _out(c)
        f4b = _f4_out(c, c.rows_c, lo_copy) if f4 else []
        launch(c, o32, o16, [v for _, v in f4b])
        torch.cuda.synchronize()
        assert _guards_untouched(buf) and all(_guards_untouched(b) for b, _ in f4b), f"{label} CUs {n}: guard band written"
        splits.add(_ns(c, n))
        if f4:
            assert all(_f4_untouched(c, v) for _, v in f4b[0::2]), f"{label} CUs {n}: e2m1 copy written outside the conditional token rows"
        if not first:
            first.extend([view.clone()] + [v.clone() for _, v in f4b])
            _check(c, view, want, label)
        else:
            _same_bits(first[0], view, f"{label} CUs {n}")
            for a, (_, v) in zip(first[1:], f4b):
                assert torch.equal(a, v), f"{label} CUs {n}: e2m1 output copy differs between walks"

    _walk(lib, R.CU_COUNTS, one)
    return splits


@pytest.mark.parametrize("pair,nseq,sq,N,K,nlo", R.SEQ_SHAPES)
def test_sequence_tiles_plain_and_pair_with_mini_tile_sets(pair, nseq, sq, N, K, nlo):
    lib = _lib()
    base = R.make_case(0, nseq * sq, N, K, seq_rows=sq, pair=bool(pair), nlo=nlo, seed=sq + nseq + nlo, dev=DEV)
    if nlo:
        print(f"mini-tile operands: sum |a||w| at most {R.mini_precondition(base.with_epi(2)):.0f} quanta of 2^-6 (< 2^22)")
    tiles = nseq * (sq - 1) // (128 if pair else 256) * (N // 256)
    label = f"{'pair' if pair else 'plain'} {nseq} x {sq} N {N} K {K} nlo {nlo}"
    print(f"{label}: tiles {tiles}, walk lengths {[R.walk_length(tiles, n) for n in R.CU_COUNTS]}")

    def launch(c, o32, o16, f4v):
        f4v = f4v + [None] * (4 - len(f4v))
        gemm_mini(lib, c.epi, c.A, c.W, c.bias, c.res if c.epi == 2 else None, o32, o16, c.rows_c, bool(pair), N, K, [s.tensors() for s in c.lo],
                  f4v[0], f4v[1], 0 if sq == 257 else sq, f4v[2], f4v[3])

    for epi in (0, 1, 2):
        f4 = epi == 1 and nlo > 0
        splits = _seq_runs(lib, base.with_epi(epi), f"{label} epi {epi}", launch, f4=f4, lo_copy=f4 and bool(pair) and nlo == 2)
        if epi == 2 and nlo and not pair:
            print(f"{label}: column splits NS over CU counts {R.CU_COUNTS}: {sorted(splits)}")
            if nseq == 1:                                          # one sequence, N = 256: quarter-, half- and whole-column tiles, equal bits
                assert splits == {4, 2, 1}


@pytest.mark.parametrize("epi", [0, 1])
@pytest.mark.parametrize("nseq,N,kw", R.MINI_SPLIT_SHAPES)
def test_sequence_tiles_split_activations_with_mini_tiles(nseq, N, kw, epi):
    lib = _lib()
    c = R.make_case(epi, nseq * 257, N, kw, seq_rows=257, split=True, nlo=1, seed=nseq + 40, dev=DEV)
    R.mini_precondition(c)

    def launch(c, o32, o16, f4v):
        f4v = f4v + [None] * (2 - len(f4v))
        gemm_mini_split(lib, c.epi, c.A, c.A2, c.W, c.bias, o16, f4v[0], f4v[1], c.M, N, kw, c.lo[0].tensors())

    _seq_runs(lib, c, f"mini-split {nseq} x 257 N {N} kw {kw} epi {epi}", launch, f4=epi == 1)
