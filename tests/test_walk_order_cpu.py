"""The walk-order functions of mb_kernels.h (walk_tile, walk_seq, walk_row), evaluated on the host through the diagnostic entries mb_walk_*: both
directions are bijections, direction 1 is the exact mirror in time of direction 0, direction 0 of the GEMM walk is the map tests/gemm_reference.py
encodes, and the grid kernels' order follows the order in which a direction-0 GEMM walk completes the sequences."""
import itertools

import pytest

import gemm_reference as R


@pytest.fixture(scope="module")
def lib():
    from maskbit_amd import _lib
    return _lib.load()


GEMM_GEOS = [(pairs, sq, N) for pairs in (1, 2, 3, 64) for sq in (257, 1025) for N in (256, 1024, 3072)]


@pytest.mark.parametrize("pairs,sq,N", GEMM_GEOS)
def test_gemm_walk_both_directions(lib, pairs, sq, N):
    tiles_m, tiles_n = pairs * ((sq - 1) // 128), N // 256
    nt = tiles_m * tiles_n
    fwd = [lib.mb_walk_tile(vb, nt, 0) for vb in range(nt)]
    rev = [lib.mb_walk_tile(vb, nt, 1) for vb in range(nt)]
    assert fwd == [R.xcd_remap(vb, nt) for vb in range(nt)]                  # direction 0: the map the kernel always had
    assert sorted(fwd) == sorted(rev) == list(range(nt))
    assert rev == fwd[::-1]                                                  # direction 1: the mirror of the virtual block index
    assert lib.mb_walk_tile(nt, nt, 0) == -1 and lib.mb_walk_tile(-1, nt, 1) == -1

    def decode(L):                                                           # logical tile -> (tm, tn): make_plan's super-rows, as gemm_reference.tile_of
        sr = L // (8 * tiles_n)
        rows_sr = min(8, tiles_m - sr * 8)
        rem = L - sr * 8 * tiles_n
        return sr * 8 + rem % rows_sr, rem // rows_sr

    assert [decode(L) for L in fwd] == [R.tile_of(vb, tiles_m, tiles_n) for vb in range(nt)]
    want = set(itertools.product(range(tiles_m), range(tiles_n)))
    for grid in (1, 7, 256):
        g = min(grid, nt)
        # workgroup b takes virtual blocks b, b + g, ...: every tile once in either direction, and step k of direction 1 is the mirrored block of direction 0
        for d, order in ((0, fwd), (1, rev)):
            seen = [decode(order[vb]) for b in range(g) for vb in range(b, nt, g)]
            assert len(seen) == nt and set(seen) == want, (grid, d)
        for b in range(g):
            assert [rev[vb] for vb in range(b, nt, g)] == [fwd[nt - 1 - vb] for vb in range(b, nt, g)]


@pytest.mark.parametrize("n", [1, 2, 5, 8, 9, 64, 67])
@pytest.mark.parametrize("grp", [1, 4, 8])
def test_sequence_order_is_a_mirrored_bijection(lib, n, grp):
    fwd = [lib.mb_walk_seq(s, n, grp, 0) for s in range(n)]
    rev = [lib.mb_walk_seq(s, n, grp, 1) for s in range(n)]
    assert sorted(fwd) == list(range(n)) and rev == fwd[::-1]
    assert lib.mb_walk_seq(n, n, grp, 0) == -1 and lib.mb_walk_seq(0, n, 0, 0) == -1


@pytest.mark.parametrize("pairs", [1, 2, 5])
@pytest.mark.parametrize("heads", [1, 16])
def test_attention_workgroups(lib, pairs, heads):
    """attention: slot = blockIdx (direction 1: mirrored as a whole) -> (walk_seq(slot / heads), slot % heads), as attention_kernel derives it."""
    grp = lib.mb_walk_group(257, 1)
    assert grp == 4 and lib.mb_walk_group(1025, 1) == 1 and lib.mb_walk_group(257, 0) == 8 and lib.mb_walk_group(1025, 0) == 2
    nblk = pairs * heads

    def work(b, reverse):
        slot = nblk - 1 - b if reverse else b
        return lib.mb_walk_seq(slot // heads, pairs, grp, 0), slot % heads

    fwd, rev = [work(b, 0) for b in range(nblk)], [work(b, 1) for b in range(nblk)]
    assert sorted(fwd) == sorted(itertools.product(range(pairs), range(heads))) and rev == fwd[::-1]
    # the kernel's two steps equal the order function's own direction argument
    assert [p for p, _ in rev[::heads]] == [lib.mb_walk_seq(s, pairs, grp, 1) for s in range(pairs)]


@pytest.mark.parametrize("rows,sq,pair", [(3 * 257, 257, 1), (5 * 257, 257, 0), (2 * 1025, 1025, 1), (1001, 257, 1), (1001, 0, 0)])
def test_row_kernels(lib, rows, sq, pair):
    """Row counts that are no multiple of the 4 rows of a workgroup; rows that are not whole sequences (and an unknown sequence length) walk as one run."""
    assert rows % 4
    fwd = [lib.mb_walk_row(s, rows, sq, pair, 0) for s in range(rows)]
    rev = [lib.mb_walk_row(s, rows, sq, pair, 1) for s in range(rows)]
    assert sorted(fwd) == list(range(rows)) and rev == fwd[::-1]
    assert lib.mb_walk_row(rows, rows, sq, pair, 0) == -1
    if sq and rows % sq == 0:                                                # whole sequences: their order is walk_seq's, a sequence's rows stay in order
        grp = lib.mb_walk_group(sq, pair)
        assert fwd == [lib.mb_walk_seq(s // sq, rows // sq, grp, 0) * sq + s % sq for s in range(rows)]
    else:
        assert fwd == list(range(rows))


@pytest.mark.parametrize("pairs,N,grid", [(64, 3072, 256), (64, 1024, 256), (128, 1024, 256), (16, 4096, 256), (5, 1024, 7)])
def test_sequences_come_in_the_order_a_gemm_walk_completes_them(lib, pairs, N, grid):
    """The point of the shared function: a GEMM walk is eight sawteeth (one XCD-contiguous chunk each), so the sequences it finishes last are NOT the ones
    with the highest index.  The step of the persistent walk at which a direction-0 pair GEMM writes the last tile of a pair never decreases along
    direction 0 of walk_seq -- so direction 1 starts with the pairs written last -- wherever the chunks hold whole super-rows."""
    tiles_m, tiles_n = pairs * 2, N // 256
    nt = tiles_m * tiles_n
    g = min(grid, nt)
    done = [0] * pairs
    for vb in range(nt):
        tm, _ = R.tile_of(vb, tiles_m, tiles_n)
        done[tm // 2] = max(done[tm // 2], vb // g)
    order = [lib.mb_walk_seq(s, pairs, lib.mb_walk_group(257, 1), 0) for s in range(pairs)]
    steps = [done[p] for p in order]
    if pairs % 64 == 0:
        assert steps == sorted(steps) and steps[0] < steps[-1], steps
        assert order != list(range(pairs))                                   # one ramp over the pair index would get this wrong
    else:                                                                    # ragged chunks: the order is a heuristic there, still a bijection
        assert sorted(order) == list(range(pairs))
