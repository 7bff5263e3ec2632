"""Exact GPU tests of the half-tile GEMM's K-loop addressing (gemm_ht.hip): scalar bases carried from K-tile to K-tile and from mini-tile to mini-tile,
32-bit byte offsets per lane.

Same method as tests/test_hip_gemm_exact.py: the integer operands of tests/gemm_reference.py, so epilogues 0 and 2 must EQUAL the float64 reference
bit for bit (GELU: within that file's bound), outputs inside NaN-filled buffers with guard bands.  The shapes are the smallest at which the carried
state can go wrong, and only (instantiation, K) combinations that file does not already run:
  K = 128  two K-tiles: the loop never reaches a K-tile whose refills are all live (no mini-tiles; with them that file runs it)
  K = 192  odd K-tile count (no mini-tiles: they need K % 128 == 0) -- plain and pair tiles without mini-tiles run it there, so it is not repeated
  K = 256  two mini-tiles per set / row half
  K = 384  an ODD number of mini-tiles per set / row half: the switch to the second set (pair) / second row half (plain) falls on an odd K-tile
  K = 640  ten K-tiles, five mini-tiles
for pair tiles (0, 1 and 2 operand sets), plain sequence tiles (0 and 1) and the half-column tiles (NS = 2, which exist with mini-tiles only); split
activations, whose lo halves take over the A stream in the middle of the K loop, with and without mini-tiles; and walks of several tiles per workgroup
(2 sequence pairs, N = 256 and 512, grids of 1 and 3 workgroups): the bases are re-made at every tile boundary and the class-row tile comes mid-walk."""
import pytest
import torch

import gemm_reference as R
from hip_helpers import gemm_act_split, gemm_mini, gemm_mini_split
from test_hip_gemm_exact import _check, _guards_untouched, _lib, _out, _same_bits, _walk

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _launch_seq(lib, c, N, K):
    buf, view, o32, o16 = _out(c)
    gemm_mini(lib, c.epi, c.A, c.W, c.bias, c.res if c.epi == 2 else None, o32, o16, c.rows_c, bool(c.pair_rows), N, K, [s.tensors() for s in c.lo])
    torch.cuda.synchronize()
    assert _guards_untouched(buf), "guard band written"
    return view


# (pair, sequences (pairs), N, K, nlo): see the module docstring for what each K is there for
K_CASES = [(1, 1, 256, 128, 0), (1, 1, 256, 256, 0), (1, 1, 256, 384, 0), (1, 1, 256, 640, 0),
           (1, 1, 256, 256, 1), (1, 1, 256, 384, 1), (1, 1, 256, 640, 1), (1, 1, 256, 256, 2), (1, 1, 256, 384, 2),
           (0, 2, 256, 128, 0), (0, 2, 256, 256, 0), (0, 2, 256, 384, 0), (0, 2, 256, 640, 0),
           (0, 2, 256, 256, 1), (0, 2, 256, 384, 1), (0, 2, 256, 640, 1)]


@pytest.mark.parametrize("pair,nseq,N,K,nlo", K_CASES)
def test_k_loop_lengths_pair_and_plain_tiles(pair, nseq, N, K, nlo):
    lib = _lib()
    base = R.make_case(0, nseq * 257, N, K, seq_rows=257, pair=bool(pair), nlo=nlo, seed=K + 3 * nlo + pair, dev=DEV)
    if nlo:
        R.mini_precondition(base.with_epi(2))
    for epi in (0, 1, 2):
        c = base.with_epi(epi)
        label = f"{'pair' if pair else 'plain'} {nseq} x 257 N {N} K {K} nlo {nlo} epi {epi}"
        try:
            # (plain residual GEMMs with mini-tiles pick column-split tiles by CU count: hold the grid to whole tiles here, NS = 2 has its own test)
            assert lib.mb_set_cu_count(1 if (nlo and not pair and epi == 2) else 0) == 0
            _check(c, _launch_seq(lib, c, N, K), R.expected(c), label)
        finally:
            lib.mb_set_cu_count(0)


@pytest.mark.parametrize("K", [256, 384, 640])
def test_k_loop_lengths_half_column_tiles(K):
    """NS = 2: one sequence, N = 256 is one whole tile; a grid sized for 2 CUs makes launch_ht pick the half-column form.  Equal bits to whole tiles."""
    lib = _lib()
    c = R.make_case(2, 257, 256, K, seq_rows=257, nlo=1, seed=K + 50, dev=DEV)
    R.mini_precondition(c)
    got = {}
    _walk(lib, (1, 2), lambda n: got.__setitem__(n, _launch_seq(lib, c, 256, K).clone()))
    _check(c, got[2], R.expected(c), f"NS 2 K {K}")
    _same_bits(got[1], got[2], f"NS 2 against whole tiles, K {K}")


@pytest.mark.parametrize("kw", [192, 256])
def test_split_activations_take_over_mid_loop(kw):
    """Plain sequence tiles over hi + lo activation halves (K = 2 kw): the A stream's base switches to the lo halves at K-tile kw / 64 while W starts over.
    kw = 192: the switch is the first move of the carried base (K-tile 3); no mini-tiles (they need kw % 128 == 0).  kw = 256: with mini-tiles, one per two
    K-tiles."""
    lib = _lib()
    M, N = 3 * 257, 256
    for epi in (0, 2) if kw % 128 else (0,):
        c = R.make_case(epi, M, N, kw, seq_rows=257, split=True, nlo=0 if kw % 128 else 1, seed=kw + 5, dev=DEV)
        buf, view, o32, o16 = _out(c)
        if c.lo:
            R.mini_precondition(c)
            gemm_mini_split(lib, epi, c.A, c.A2, c.W, c.bias, o16, None, None, M, N, kw, c.lo[0].tensors())
        else:
            gemm_act_split(lib, epi, c.A, c.A2, c.W, c.bias, c.res if epi == 2 else None, o32, o16, M, N, kw, 257)
        torch.cuda.synchronize()
        assert _guards_untouched(buf)
        _check(c, view, R.expected(c), f"split kw {kw} epi {epi} {'with' if c.lo else 'without'} mini-tiles")


@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("nlo", [0, 1])
def test_walks_of_several_tiles_carry_the_bases_across_tile_boundaries(N, nlo):
    """2 sequence pairs = 4 (N = 256) or 8 (N = 512) pair tiles on grids of 1 and 3 workgroups: every workgroup walks several tiles, the class-row tile
    (the second of a pair of sequences) comes in the middle of a walk.  All runs give the bits of the float64 reference."""
    lib = _lib()
    K = 256
    base = R.make_case(0, 2 * 257, N, K, seq_rows=257, pair=True, nlo=nlo, seed=N + nlo, dev=DEV)
    if nlo:
        R.mini_precondition(base.with_epi(2))
    for epi in (0, 2):
        c = base.with_epi(epi)
        want = R.expected(c)
        _walk(lib, (1, 3), lambda n: _check(c, _launch_seq(lib, c, N, K), want, f"pair 2 x 257 N {N} K {K} nlo {nlo} epi {epi} CUs {n}"))
