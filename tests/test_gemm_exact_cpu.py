"""CPU checks of the exact-operand GEMM method (tests/gemm_reference.py): the generators leave no blind spot -- every wrong kernel listed in `mutations`
changes the expected output in every tile it touches --, the float64 reference equals a separately written einsum, the persistent walk's index
arithmetic is a bijection for every geometry tests/test_hip_gemm_exact.py launches, and the mini-tile operands meet the exactness precondition."""
import pytest
import torch

import gemm_reference as R

# one case per shape family of the GPU file, the epilogues spread over them: (id, make_case arguments)
_FAMILIES = [("small-%d-%d" % (M, N), dict(epi=i % 4, M=M, N=N, K=R.KS[i % 4])) for i, (M, N) in enumerate(zip(R.SMALL_M, (4, 132, 256, 132, 256)))]
_FAMILIES += [("logits-%d-%d" % mp, dict(epi=4, M=mp[0], N=R.SMALL_N[i % 3], K=128, period=mp[1])) for i, mp in enumerate(R.LOGITS_SHAPES)]
_FAMILIES += [("small-split", dict(epi=2, M=129, N=132, K=64, split=True)), ("ht-split", dict(epi=0, M=771, N=768, K=192, split=True))]
_FAMILIES += [("ht-%d" % M, dict(epi=i % 4, M=M, N=N, K=K)) for i, (M, N, K) in enumerate(R.HT_SHAPES)]
_FAMILIES += [("%s-%dx%d-nlo%d" % ("pair" if p else "seq", n, sq, nlo), dict(epi=i % 3, M=n * sq, N=N, K=K, seq_rows=sq, pair=bool(p), nlo=nlo))
              for i, (p, n, sq, N, K, nlo) in enumerate(R.SEQ_SHAPES)]
_FAMILIES += [("mini-split-%d" % n, dict(epi=i % 2, M=n * 257, N=N, K=kw, seq_rows=257, split=True, nlo=1)) for i, (n, N, kw) in enumerate(R.MINI_SPLIT_SHAPES)]

_cache = {}


def _case(name):
    if name not in _cache:
        _cache[name] = R.make_case(seed=len(_cache) + 1, **dict(_FAMILIES)[name])
    return _cache[name]


ALL_MUTATIONS = ("drop the first K-tile", "drop the middle K-tile", "drop the last K-tile", "swap two K-tiles between the hi and lo sweeps",
                 "read A instead of A2 in the second sweep", "class row of sequence s + 1", "omit the A_delta term on the u rows",
                 "swap rows m and m + 16 inside a tile", "swap two 4-column groups", "mini-tile set 0: scales of the 64-token group g + 1",
                 "mini-tile set 1: scales of the 64-token group g + 1", "skip the mini-tile set on the second 128-row half",
                 "bias of the previous tile (column block n0 - 256)")
_names = {}                                  # family -> the mutations it listed


def test_generators_make_every_row_column_and_ktile_distinguishable():
    for rows, cols, lim in ((600, 320, 3), (768, 1024, 2), (1, 128, 3), (4369, 192, 3)):
        v = R.int_operand(rows, cols, lim, 5)
        assert int(v.abs().max()) == lim and torch.equal(v.half().long(), v)                    # small integers, exact in fp16
        pad = (-rows) % 16
        groups = torch.cat([v, torch.zeros(pad, cols, dtype=v.dtype)]).reshape(-1, 16, cols // 64, 64)
        assert bool((groups.abs().sum((1, 3)) > 0).all())                                        # no all-zero (16-row, 64-column) tile
        assert bool((v.reshape(rows, -1, 64).abs().sum(-1) > 0).all())                           # ... not even of a single row
        assert torch.unique(v, dim=0).shape[0] == rows                                           # every row distinguishable
        if rows >= 64:
            assert torch.unique(v.t(), dim=0).shape[0] == cols                                   # every column
            assert torch.unique(v.reshape(rows, -1, 64).transpose(0, 1).reshape(cols // 64, -1), dim=0).shape[0] == cols // 64     # every K-tile
            zero_share = (groups == 0).double().mean((1, 3))
            assert float(zero_share.max() - zero_share.min()) > 0.2                              # the distribution differs between tiles


def test_fp16_store_model_clamps_then_rounds_to_nearest_even():
    x = torch.tensor([2049.0, 2051.0, 4098.0, 1e6, -1e6, 65519.0, -3.0], dtype=torch.float64)
    assert R.to_f16(x).tolist() == [2048.0, 2052.0, 4096.0, 65504.0, -65504.0, 65504.0, -3.0]


@pytest.mark.parametrize("name", [n for n, _ in _FAMILIES])
def test_reference_matches_a_separately_written_einsum(name):
    c = _case(name)
    assert torch.equal(R.pre_activation(c), R.einsum_reference(c))
    out = R.expected(c)
    assert out.shape == (c.M - (c.M // c.period if c.epi == 4 else 0), c.N) and bool(torch.isfinite(out.double()).all())
    if c.epi in R.EXACT_EPIS:                                                                    # integers (mini-tiles: multiples of 2^-6) below 2^15
        assert float(R.pre_activation(c).abs().max()) < 2.0 ** 15


@pytest.mark.parametrize("name", [n for n, _ in _FAMILIES])
def test_every_mutation_changes_every_tile_it_touches(name):
    c = _case(name)
    truth = R.finish(c, R.pre_activation(c))
    muts = R.mutations(c)
    _names[name] = [m[0] for m in muts]
    assert len(muts) >= 3
    for mname, wrong, touched in muts:
        assert mname in ALL_MUTATIONS and touched, mname
        diff = wrong != truth
        rows_hit = {s.start: diff[:, s].any(1) for s in {s.start: s for _, s in touched}.values()}       # per column tile: the rows that changed
        blind = [(int(r[0]), s.start) for r, s in touched if not bool(rows_hit[s.start][r].any())]
        assert not blind, f"{name}: '{mname}' leaves tiles (first row, first column) {blind[:5]} unchanged"


def test_all_mutations_of_the_list_were_exercised():
    """(the names were recorded by the parametrised test above; a family it has not visited in this run is listed here)"""
    for name, _ in _FAMILIES:
        if name not in _names:
            _names[name] = [m[0] for m in R.mutations(_case(name))]
    assert {m for names in _names.values() for m in names} == set(ALL_MUTATIONS)


def test_walk_index_arithmetic_is_a_bijection_for_every_gpu_geometry():
    geos = R.gpu_geometries()
    assert {2, 3, 6, 9, 10, 17, 18, 23} <= {tm for tm, _ in geos} and any(tm % 8 in (1, 7) and tn > 1 for tm, tn in geos)
    caught = 0
    for tm, tn in geos:
        want = {(m, n) for m in range(tm) for n in range(tn)}
        assert {R.tile_of(vb, tm, tn) for vb in range(tm * tn)} == want, (tm, tn)
        caught += {R.tile_of(vb, tm, tn, rows_sr_is_8=True) for vb in range(tm * tn)} != want
    # rows_sr = 8 breaks every geometry with a short last super-row of more than one column tile (with one, the split is the identity)
    assert caught == len([1 for tm, tn in geos if tm % 8 and tn > 1]) > 0
    for tiles in (1, 7, 8, 9, 69):                                   # xcd_remap alone
        assert sorted(R.xcd_remap(b, tiles) for b in range(tiles)) == list(range(tiles))


def test_walk_lengths_reached():
    assert [R.walk_length(69, n) for n in R.CU_COUNTS] == [1, 69, 23, 6] and R.walk_length(300, 0) == 2


@pytest.mark.parametrize("name", [n for n, a in _FAMILIES if a.get("nlo")])
def test_mini_tile_operands_meet_the_exactness_precondition(name):
    c = _case(name)
    worst = R.mini_precondition(c)
    assert 0 < worst < 2.0 ** 22
    for s in c.lo:
        tok = (torch.arange(c.rows_c) % c.seq_rows) < c.seq_rows - 1
        assert bool((s.a_dec[tok].reshape(int(tok.sum()), -1, 64).abs().amax(-1) > 0).all())     # no all-zero block
        q = s.a_dec * 8.0                                                                        # multiples of the quantum 2^-3 ...
        assert torch.equal(q, q.round()) and torch.equal(s.w_dec * 8.0, (s.w_dec * 8.0).round())
        pre = R.pre_activation(c) * 64.0                                                         # ... so the result is a multiple of 2^-6
        assert torch.equal(pre, pre.round())
