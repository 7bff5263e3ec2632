"""CPU checks of tests/head_reference.py, the references of the head GEMMs and the weight-preparation kernels (tests/test_hip_head.py): the exact cases
meet the precondition that makes equality legitimate; every wrong kernel the net is meant to catch changes what is expected -- the head mutations in
every 128 x 128 tile they touch, the weight-preparation mutations on every input built for them, the e2m1 value copy through the very checker the
GPU file uses --; the vectorised split / cast / w4lo statements agree with slow scalar restatements written with struct and numpy.float16; and the
scale choice of every w4 input is decided by float64 on all but MAX_UNDECIDED of the blocks."""
import math
import struct

import numpy as np
import pytest
import torch

import head_reference as H

_CASES = H.head_cases()
_seen = set()


# ---- head GEMM ---------------------------------------------------------------------------------------------------------------------------------------
def test_case_list_covers_every_listed_shape():
    e3 = {(c.M, c.N, c.kw, c.W2 is not None) for c in _CASES if c.epi == 3}
    assert e3 == {(M, N, kw, t) for M in H.HEAD_M for N in H.HEAD_N for kw in H.HEAD_KW for t in (True, False)}
    e4 = {(c.M, c.period, c.per_pos, c.W2 is not None) for c in _CASES if c.epi == 4}
    assert e4 == {(M, p, b, t) for M, p in H.LOGITS_SHAPES if M % p == 0 for b in (True, False) for t in (True, False)}
    assert [mp for mp in H.LOGITS_SHAPES if mp[0] % mp[1]] == [(600, 257)]                       # the one shape the entry must refuse
    assert {c.scale for c in _CASES if c.W2 is not None} == set(H.SCALES)
    assert {c.scale for c in _CASES if c.epi == 4 and c.W2 is not None and c.per_pos} == set(H.SCALES)


@pytest.mark.parametrize("i", range(len(_CASES)))
def test_exact_case_precondition_and_mutations(i):
    c = _CASES[i]
    assert 0 < H.head_precondition(c) < 2.0 ** 24, c.label
    truth = H.head_image(c, H.head_pre_activation(c))
    want = H.head_expected(c)
    assert want.shape == (H.head_out_rows(c), c.N) and bool(torch.isfinite(want.double()).all()), c.label
    if c.epi == 4:                                                                                # the compaction, written once more, row by row
        rows = [m for m in range(c.M) if m % c.period != c.period - 1]
        pre = H.head_pre_activation(c)
        assert torch.equal(want, pre[rows].float()) and bool(torch.isnan(truth[len(rows):]).all())
        assert all((m // c.period) * (c.period - 1) + m % c.period == j for j, m in enumerate(rows))
    # ... and the sum itself as one einsum over the concatenated sweeps: no A2 . W2 term
    A, A2, W = c.A.double(), c.A2.double(), c.W.double()
    acc = torch.einsum("mk,nk->mn", torch.cat([A, A2] + ([A] if c.W2 is not None else []), 1), torch.cat([W, W] + ([c.W2.double()] if c.W2 is not None else []), 1))
    assert torch.equal(acc, H.head_accumulator(c))
    muts = H.head_mutations(c)
    assert len(muts) >= 2
    for name, wrong, touched in muts:
        assert name in H.HEAD_MUTATIONS
        _seen.add(name)
        diff = H.images_differ(wrong, truth)
        blind = [(int(r[0]), s.start) for r, s in touched if not bool(diff[r][:, s].any())]
        assert not blind, f"{c.label}: '{name}' leaves tiles (first image row, first column) {blind[:5]} unchanged"


def test_every_head_mutation_was_exercised():
    for c in _CASES:
        if len(_seen) == len(H.HEAD_MUTATIONS):
            break
        _seen.update(m[0] for m in H.head_mutations(c))
    assert _seen == set(H.HEAD_MUTATIONS), set(H.HEAD_MUTATIONS) - _seen
    # each form lists what applies to it: the three-sweep per-position case of several sequences lists all twelve
    full = [c for c in _CASES if c.epi == 4 and c.W2 is not None and c.per_pos and c.M > c.period > 2 and c.scale != 1.0]
    assert full and all(len(H.head_mutations(c)) == 12 for c in full[:2])


# ---- scalar restatements -----------------------------------------------------------------------------------------------------------------------------------
def _f16(x: float) -> float:
    """fp32 value -> fp16 value, round to nearest even, by numpy's converter (overflow: inf)."""
    with np.errstate(over="ignore"):
        return float(np.float16(np.float32(x)))


def _f32(x: float) -> float:
    return struct.unpack("f", struct.pack("f", x))[0]


def _bits16(x: float) -> int:
    return int(np.float16(x).view(np.uint16))


@pytest.mark.parametrize("name,w", [(n, w) for N, K in ((3, 5), (16, 24)) for n, w, _ in H.split_inputs(N, K)])
def test_split_statement_agrees_with_a_scalar_restatement(name, w):
    hi, lo, scale = H.split_planes(w)
    flat = [float(v) for v in w.reshape(-1)]
    mx = max(abs(v) for v in flat)
    S = 0
    if mx > 0:
        e = 0                                                                                     # mx = f 2^e, f in [0.5, 1), by halving / doubling
        f = mx
        while f >= 1.0:
            f, e = f / 2, e + 1
        while f < 0.5:
            f, e = f * 2, e - 1
        S = 15 - e
        assert 2.0 ** 14 <= mx * 2.0 ** S < 2.0 ** 15
    assert float(scale) == 2.0 ** -S
    for i, v in enumerate(flat):
        ws = _f32(v * 2.0 ** S)
        assert ws == v * 2.0 ** S
        h = _f16(ws)
        d = _f32(ws - h)
        assert d == ws - h                                                                        # the subtraction is exact in fp32
        assert _bits16(h) == _bits16(float(hi.reshape(-1)[i])) and _bits16(_f16(d)) == _bits16(float(lo.reshape(-1)[i])), (name, i, v)
        assert abs(h + _f16(d) - ws) <= abs(ws) * 2.0 ** -21 + 2.0 ** -25                         # hi + lo restores w 2^S to ~22 bits (subnormal lo: 2^-25)


def test_split_inputs_hold_the_edges_they_are_named_for():
    got = {n: w for n, w, _ in H.split_inputs(768, 768)}
    hi, lo, scale = H.split_planes(got["far below the maximum"])
    sub = (hi.float().abs() < 2.0 ** -14) & (hi != 0)
    assert float(sub.float().mean()) > 0.9                                                        # fp16-subnormal hi values
    hi, _, scale = H.split_planes(got["one ulp below a power of two"])
    assert float(hi.float().max()) == 2.0 ** 15 and float(scale) == 2.0 ** -15
    hi, _, scale = H.split_planes(got["power-of-two maximum"])
    assert float(hi.float().max()) == 2.0 ** 14 and float(scale) == 2.0 ** -14
    hi, lo, scale = H.split_planes(got["all zero"])
    assert float(scale) == 1.0 and not bool(hi.any()) and not bool(lo.any())
    assert int(got["single in the second pass"].reshape(-1).nonzero()) >= H.GRID_PASS
    assert float(got["negative maximum"].min()) == -float(got["negative maximum"].abs().max())
    assert 768 * 768 > H.GRID_PASS and 64 * 128 < H.GRID_PASS


@pytest.mark.parametrize("N,K", H.SPLIT_SHAPES)
def test_split_mutations_change_the_inputs_built_for_them(N, K):
    seen = set()
    for name, w, catches in H.split_inputs(N, K):
        truth = H.split_planes(w)
        for m in catches:
            wrong = H.split_planes(w, **H.SPLIT_MUTATIONS[m])
            same = all(torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else a, b.view(torch.int16) if b.dtype == torch.float16 else b)
                       for a, b in zip(truth, wrong))
            assert not same, f"split {N} x {K}, input '{name}': mutation '{m}' changes nothing"
            seen.add(m)
    want = set(H.SPLIT_MUTATIONS) - ({"maximum over the first grid pass only"} if N * K <= H.GRID_PASS else set()) - \
        ({"lo truncated", "lo computed from w"} if N * K < 16 else set()) - ({"lo truncated"} if N * K < 1024 else set())
    assert seen >= want, want - seen


def test_cast_statement_agrees_with_a_scalar_restatement():
    for n in (7, 1025):
        x = H.cast_values(n)
        want = H.cast_reference(x)
        for i in range(n):
            v = float(x[i])
            if math.isnan(v):
                assert math.isnan(float(want[i]))
            else:
                assert _bits16(_f16(v)) == int(want[i].view(torch.int16)) & 0xffff, (i, v)
    x = H.cast_values(1025)
    h = H.cast_reference(x).float()
    assert bool(torch.isinf(h[x.abs() >= 65520]).all()) and float(h[0]) == 65504.0 and bool(torch.isinf(h[2])) and bool(torch.isnan(h[9]))
    assert bool(((h.abs() < 2.0 ** -14) & (h != 0)).any())                                        # fp16 subnormals
    t = 2.0 ** -24
    ties = H.cast_reference(torch.tensor([0.5 * t, 1.5 * t, 2.5 * t, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2049.0, 2051.0])).double()
    assert ties.tolist() == [0.0, 2 * t, 2 * t, 1.0, 1 + 2.0 ** -9, 2048.0, 2052.0]              # exact ties go to even
    assert int(H.cast_reference(torch.tensor([-0.0])).view(torch.int16)) & 0xffff == 0x8000
    assert all(len(H.cast_values(n)) == n for n in H.CAST_N) and max(H.CAST_N) // 4 // 256 + 1 > 2048   # the capped grid walks twice


_F4 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _e2m1(a: float) -> int:
    """Nearest e2m1 magnitude code of a >= 0, ties to the even code, saturating at 6 -- by comparison against the grid, no logarithm."""
    best = 7
    for c in range(7):
        mid = (_F4[c] + _F4[c + 1]) / 2
        if a < mid or (a == mid and c % 2 == 0):
            best = c
            break
    return best


def test_e2m1_rounding_of_the_helpers_agrees_with_a_grid_search():
    from hip_helpers import f4_codes
    v = torch.cat([torch.linspace(-7, 7, 2241, dtype=torch.float64), torch.tensor(H._MID + (6.0, 5.0000001, 4.9999999, 100.0), dtype=torch.float64)])
    got = f4_codes(v)
    for x, g in zip(v.tolist(), got.tolist()):
        assert g == (_e2m1(abs(x)) | (8 if x < 0 else 0)), x


@pytest.mark.parametrize("name,w", [(n, w) for n, w, use in H.w4_inputs(64, 128) if use != "w4"])
def test_w4lo_statement_agrees_with_a_scalar_restatement(name, w):
    N, K = w.shape
    w4, ws = H.w4lo_reference(w)
    want4, wants = bytearray(N * K // 2), bytearray(N * K // 128)
    for n in range(N):
        row = [float(v) for v in w[n]]
        err = [_f32(v - _f16(v)) for v in row]
        assert all(e == v - _f16(v) for e, v in zip(err, row))                                   # exact in fp32
        for j in range(K // 128):
            blk = err[128 * j:128 * j + 128]
            mx = max(abs(e) for e in blk)
            E = 0
            if mx > 0:                                                                            # the biased exponent E with mx 2^(129 - E) in (3, 6]
                E = 129
                while mx * 2.0 ** (129 - E) > 6.0:
                    E += 1
                while mx * 2.0 ** (129 - E) <= 3.0:
                    E -= 1
            wants[(((n >> 6) * (K >> 7) + j) * 16 + (n & 15)) * 4 + ((n >> 4) & 3)] = E - 2 if E >= 2 else 0
            for i, e in enumerate(blk):
                code = 0 if E < 2 else _e2m1(abs(e) * 2.0 ** (129 - E)) | (8 if e < 0 else 0)
                k = 128 * j + i
                r, c = n & 15, (k & 127) >> 5
                off = ((n >> 4) * (K >> 7) + (k >> 7)) * 1024 + r * 64 + ((c ^ ((r >> 1) & 3)) << 4) + ((k & 31) >> 1)
                want4[off] |= code << (4 * (k & 1))
    assert bytes(want4) == bytes(w4.tolist()) and bytes(wants) == bytes(ws.tolist()), name
    if name == "rows exactly fp16":
        codes, sb = H.w4_unpack(w4, ws, N, K)
        assert not bool(sb[0::3].any()) and not bool(codes[0::3].any()) and bool((sb[1::3] > 0).all())
    if name == "tie block":                                                                       # every value ON a midpoint of the block's scale
        codes, sb = H.w4_unpack(w4, ws, N, K)
        assert bool((sb == 127 - 14 + 0).all()) and set((codes & 7).reshape(-1).tolist()) == {0, 2, 4, 6, 7}    # only even codes, and the 6


# ---- e2m1 copies: mutations, the undecided share ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", H.W4_SHAPES)
def test_w4lo_mutations_are_caught(N, K):
    for name, w, use in H.w4_inputs(N, K):
        if use == "w4":
            continue
        H.w4lo_check(w, *H.w4lo_reference(w), label=name)
        if name in ("gaussian", "tie block"):
            for m, hooks in H.W4_LAYOUT_MUTATIONS.items():
                with pytest.raises(AssertionError):
                    H.w4lo_check(w, *H.w4lo_reference(w, **hooks), label=m)
    # the e2m1 copy of the error of fp16(w), not of w itself (what w4_from_f32 writes), is caught as well
    w = H.w4_inputs(N, K)[0][1]
    with pytest.raises(AssertionError):
        H.w4lo_check(w, *H.w4_emulate(w), label="value copy")


@pytest.mark.parametrize("N,K", H.W4_SHAPES)
def test_w4_checker_passes_the_contract_and_rejects_every_mutation(N, K):
    shares = {}
    for name, w, use in H.w4_inputs(N, K):
        if use == "w4lo":
            continue
        share, moved = H.w4_check(w, *H.w4_emulate(w), label=name)
        assert moved == 0 and share <= H.MAX_UNDECIDED, (name, share)
        shares[name] = share
        for m, hooks in H.W4_MUTATIONS.items():
            if hooks.get("block") == 256 and K % 256:
                continue
            if m == "quantise w instead of fp16(w)" and not (name == "a quarter ulp above the midpoints" or (name in ("gaussian", "student-t(3)") and N * K >= 2 ** 17)):
                continue                                                                          # (applies where some w 2^r and fp16(w) 2^r straddle a rounding boundary)
            with pytest.raises(AssertionError):
                H.w4_check(w, *H.w4_emulate(w, **hooks), label=m)
                pytest.fail(f"w4 {N} x {K}, input '{name}': mutation '{m}' passes the checker", pytrace=False)
    print(f"w4 {N} x {K}: undecided shares {shares}")
    # the checker reads r from the kernel: a kernel whose r is the argmin's neighbour on EVERY block is refused on the decided ones
    w = H.w4_inputs(N, K)[0][1]
    r = H.w4_choice(w.half().double().reshape(N, K // 128, 128))[2] + 1
    from hip_helpers import f4_codes
    codes = f4_codes(w.half().double().reshape(N, K // 128, 128) * (2.0 ** r.double())[..., None]).reshape(N, K)
    with pytest.raises(AssertionError, match="decided blocks carry another r"):
        H.w4_check(w, *H.w4_pack(codes, 127 - r), label="r + 1")


def test_w4_inputs_hold_the_edges_they_are_named_for():
    for N, K in ((64, 128), (192, 1152)):
        inputs = {n: w for n, w, _ in H.w4_inputs(N, K)}
        o = inputs["outlier 50 x rms"].half().double().reshape(N, K // 128, 128)
        r = H.w4_choice(o)[2]
        assert bool(((o.abs() * (2.0 ** r.double())[..., None]) > 6.5).any())                     # w4 saturates the outlier ...
        codes, sb = H.w4_unpack(*H.w4lo_reference(inputs["outlier 50 x rms"]), N, K)
        e = (inputs["outlier 50 x rms"].double() - inputs["outlier 50 x rms"].half().double()).reshape(N, K // 128, 128)
        assert float((e.abs() * (2.0 ** (127.0 - sb.double()))[..., None]).max()) <= 6.0           # ... w4lo clips nothing
        z = inputs["an all-zero block"]
        assert not bool(z[0, :128].any())
        c4, s4 = H.w4_unpack(*H.w4_emulate(z), N, K)
        assert int(s4[0, 0]) == 127 and not bool(c4[0, :128].any())
        assert float(inputs["gaussian"].abs().max()) < 65504 and float(inputs["student-t(3)"].abs().max()) < 65504
