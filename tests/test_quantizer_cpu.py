"""The restatements of tests/quantizer_reference.py are anchored before any kernel is compared with them (no GPU needed): against the reference's
own recorded outputs (tests/golden), against the oracle's bit helpers, and against their own premises -- the integer search cases are exact in fp32,
the special codebooks have the answer their construction promises, the l2 cases added to tests/test_hip_vq.py meet that test's clear-row share."""
import pytest
import torch

import quantizer_reference as R
from conftest import load_golden
from oracle import maskbit_oracle as O


@pytest.mark.parametrize("name", ["tok_tiny.npz", "tok_avgpool_tiny.npz"])
def test_lfq_pack_reproduces_the_recorded_indices(name):
    z = load_golden(name)
    zq = torch.from_numpy(z["enc_zq"]).float()                                   # [B, K, h, w], +-1
    B, K, h, w = zq.shape
    rows = zq.permute(0, 2, 3, 1).reshape(-1, K).half()
    idx, zq2, zraw = R.lfq_pack(rows, B, h * w, K)
    assert torch.equal(idx, torch.from_numpy(z["enc_indices"]).flatten())
    assert torch.equal(zq2.reshape(B, K, h, w), zq) and torch.equal(zraw, zq2)
    assert torch.equal(idx, O.bits_to_index(rows.float()))


@pytest.mark.parametrize("K", sorted(set(R.LFQ_K) | {64}))
def test_tokens_latent_pack_round_trip(K):
    t = R.lfq_tokens(K, 600)
    assert t.numel() == (1024 if K == 10 else 600)
    if K == 10:
        assert torch.equal(t, torch.arange(2 ** K))
    elif K < 63:
        assert int(t.min()) == 0 and int(t.max()) == 2 ** K - 1
    elif K == 64:
        assert int(t[-1]) == -1 and bool((t < 0).any()) and bool((t > 0).any())
    lat = R.lfq_latent(t, K)
    assert lat.shape == (t.numel(), 64) and bool((lat[:, :K].abs() == 1).all())
    assert torch.equal(lat[:, K:].view(torch.int16), torch.zeros_like(lat[:, K:]).view(torch.int16))
    idx, zq, zraw = R.lfq_pack(lat, 1, t.numel(), K)
    assert torch.equal(idx, t)
    assert torch.equal(zq, lat[:, :K].float().T[None]) and torch.equal(zraw, zq)
    if K <= 62:                                                                   # the oracle's helpers multiply by 1 << j in int64
        assert torch.equal(O.index_to_bits(t, K), lat[:, :K].float()) and torch.equal(O.bits_to_index(lat[:, :K].float()), t)


def test_lfq_pack_decides_the_edge_values_as_the_reference_does():
    bits = torch.tensor(R.H16_PROBES_BITS, dtype=torch.int32).to(torch.int16).view(torch.float16)
    want = [0, 0, 1, 0, 1, 0, 1, 0, 0, 1, 0, 1, 0]          # +0 -0 +sub -sub +max -max +inf -inf NaN +sub -sub +min normal -min normal
    assert (bits.float() > 0.0).long().tolist() == want
    idx, zq, _ = R.lfq_pack(bits[None, :], 1, 1, len(want))
    assert int(idx) == sum(b << j for j, b in enumerate(want))
    assert zq.flatten().tolist() == [1.0 if b else -1.0 for b in want]
    for K, Kp, B, HW in R.lfq_pack_cases():
        z = R.lfq_pack_case(K, Kp, B, HW)
        assert bool(z[:, K:].isnan().all()) and z.shape == (B * HW, Kp)
        if B * HW * K >= 64:
            live = z[:, :K].reshape(-1).view(torch.int16).tolist()
            assert set(bits.view(torch.int16).tolist()) <= set(live), "every probe is planted"
    assert R.bits_to_code(torch.ones(1, 64, dtype=torch.bool)).item() == -1
    assert R.bits_to_code(torch.tensor([[False] * 63 + [True]])).item() == -2 ** 63
    assert R.bits_to_code(torch.tensor([[False] * 31 + [True]])).item() == 2 ** 31


def test_lookup_restatement_reproduces_the_recorded_indices():
    z = load_golden("tok_vq_tiny.npz")
    lat = torch.from_numpy(z["z"])
    B, K, h, w = lat.shape
    rows = lat.permute(0, 2, 3, 1).reshape(-1, K)
    cb = torch.from_numpy(z["codebook"])
    idx, dist, zq, zraw = R.lookup_search(rows, cb, B, h * w)
    clear = torch.from_numpy(z["gap"]) > 0
    assert bool(clear.float().mean() > 0.99)
    assert torch.equal(idx[clear], torch.from_numpy(z["indices"]).flatten()[clear])
    assert torch.equal(zraw.reshape(B, K, h, w), lat)
    assert torch.equal(zq, cb[idx].reshape(B, h * w, K).permute(0, 2, 1))
    assert abs(float(dist.mean()) / K - float(z["codebook_loss"])) <= 1e-5 * float(z["codebook_loss"])
    # the same argmin as torch's over the reference's own expression, in float64
    d = rows.double().pow(2).sum(1, keepdim=True) + cb.double().pow(2).sum(1) - 2 * rows.double() @ cb.double().T
    assert torch.equal(idx, d.argmin(1))


@pytest.mark.parametrize("case", R.SEARCH_CASES, ids=lambda c: c.name)
def test_search_cases_keep_their_premises(case):
    z, cb, want = R.search_case(case)
    assert z.shape == (case.B * case.HW, case.K) and cb.shape == (case.C, case.K)
    assert R.search_premise(z, cb) < 2 ** 24
    assert float(z.abs().max()) <= 8 and float(cb.abs().max()) <= 8 and torch.equal(z.half().float(), z)
    idx, dist, zq, zraw = R.lookup_search(z, cb, case.B, case.HW)
    assert torch.equal(dist, dist.round()) and float(dist.max()) < 2 ** 24
    # lowest index among equal scores, by brute force in int64
    zi, ci = z.long(), cb.long()
    for r in range(0, z.shape[0], max(1, z.shape[0] // 7)):
        score = (ci * ci).sum(1) - 2 * (ci * zi[r]).sum(1)
        assert int(idx[r]) == int((score == score.min()).nonzero()[0])
    if want is not None:
        assert torch.equal(idx, want)
    if case.kind == "grid":
        assert len({tuple(r) for r in cb.tolist()}) == case.C and bool((dist == 0).all()) and {0, case.C - 1} <= set(idx.tolist())
    if case.kind == "padding":
        assert bool((cb.abs().sum(1) > 0).all()) and int(idx[0]) != 0 and float((cb[0] ** 2).sum()) > float((cb[37] ** 2).sum())
    if case.kind == "ties":
        flat = [p for places in R.TIE_PLACES for p in places]
        assert len(flat) == len(set(flat)) and max(flat) < case.C
        assert any(min(p) != p[0] for p in R.TIE_PLACES) and any(min(p) // 64 != max(p) // 64 for p in R.TIE_PLACES)
        assert all(int((cb == cb[places[0]]).all(1).sum()) == len(places) for places in R.TIE_PLACES)


def test_search_case_list_covers_what_it_must():
    cases = [c for c in R.SEARCH_CASES if c.kind == "random"]
    lo, hi = (1, 2, (1, 1)), (256, 1000, (2, 256))
    for ext in (lo, hi):
        assert {c.K for c in cases if (c.C, (c.B, c.HW)) == ext[1:]} == set(R.K_VALUES)
        assert {c.C for c in cases if (c.K, (c.B, c.HW)) == (ext[0], ext[2])} == set(R.C_VALUES)
        assert {(c.B, c.HW) for c in cases if (c.K, c.C) == ext[:2]} == set(R.BHW_VALUES)
    assert {(c.K, c.C) for c in R.SEARCH_CASES if c.kind == "grid"} == {(4, 65536)}
    many_ties = R.search_case(next(c for c in cases if (c.K, c.C, c.B * c.HW) == (1, 1000, 512)))
    assert len({float(v) for v in many_ties[1].flatten()}) == 7


def test_nonfinite_rows_in_the_restatement():
    z, cb, (r_nan, r_inf) = R.nonfinite_case()
    idx, dist, zq, zraw = R.lookup_search(z, cb, 1, z.shape[0])
    assert int(idx[r_nan]) == 0 and int(idx[r_inf]) == 0
    assert bool(dist[r_nan].isnan()) and float(dist[r_inf]) == float("inf")      # sum_k (z_k - e_0k)^2 as it stands
    keep = torch.ones(z.shape[0], dtype=torch.bool)
    keep[[r_nan, r_inf]] = False
    idx2, dist2, _, _ = R.lookup_search(z[keep], cb, 1, int(keep.sum()))
    assert torch.equal(idx[keep], idx2) and torch.equal(dist[keep], dist2)
    # torch.argmin over the reference's expression gives 0 for both rows as well (every score is NaN)
    d = z.pow(2).sum(1, keepdim=True) + cb.pow(2).sum(1) - 2 * z @ cb.T
    assert bool(d[[r_nan, r_inf]].isnan().all()) and d[[r_nan, r_inf]].argmin(1).tolist() == [0, 0]


def test_fp16_store_restatement():
    v = torch.tensor(R.ROUNDING_PROBES, dtype=torch.float32)
    h = R.to_h16_saturating(v)
    assert h[:7].tolist() == [65504.0, -65504.0, 65504.0, -65504.0, 65504.0, -65504.0, 65504.0]
    assert h[7].item() == 1.0 and h[8].item() == 1.0 + 2.0 ** -9                  # ties to even
    assert h[9].item() == 0.0 and h[10].item() == -2.0 ** -24 and h[11].item() == 2.0 ** -24 and h[12].item() == 0.0
    assert R.saturated(v) == 7                                                    # 65504 itself is not counted
    for K, C, npix in R.GATHER_CASES:
        codes, cb = R.gather_case(K, C, npix)
        out, sat = R.gather_latent(codes, cb, R.cin_pad_of(K))
        assert out.shape == (npix, R.cin_pad_of(K)) and sat >= 3 and len(set(codes.clamp(0, C - 1).tolist())) >= C - 10
        assert int(codes.min()) < -2 ** 40 and int(codes.max()) > 2 ** 40 and bool((codes == C).any()) and bool((codes == -1).any())
        assert torch.equal(out[:, K:].view(torch.int16), torch.zeros(npix, R.cin_pad_of(K) - K, dtype=torch.int16))
    assert R.GATHER_CASES[-1][2] * 64 > 4096 * 256 and 5 * 3277 * 64 > 4096 * 256
    for B, K, HW in R.PACK_LATENT_CASES:
        z = R.pack_latent_case(B, K, HW)
        out, sat = R.pack_latent(z, R.cin_pad_of(K))
        assert sat > 0 and torch.equal(out[:, :K].reshape(B, HW, K), R.to_h16_saturating(z).permute(0, 2, 1))
    for B, C, H, W in R.pack_image_cases():
        img = R.pack_image_case(B, C, H, W)
        out = R.pack_image(img)
        assert out.shape == (B * H * W, 64) and float(img.abs().max()) > R.H16_MAX and float(out.float().abs().max()) == R.H16_MAX
        assert torch.equal(out[:, :C].reshape(B, H, W, C).permute(0, 3, 1, 2), R.to_h16_saturating(img))


@pytest.mark.parametrize("CK", R.ARGMIN_L2_ADDED)
@pytest.mark.parametrize("l2", [False, True])
def test_added_argmin_cases_meet_the_clear_row_share(CK, l2):
    """tests/test_hip_vq.py::test_argmin_exact_vs_fp64 asserts that more than 90 % of the rows are clear; for the (C, K) added there the share is
    computed here from the same CPU-seeded inputs."""
    Cn, K = CK
    assert 64 < K <= 128                                                          # the Kp = 128 instantiation
    cb, zs = R.argmin_inputs(Cn, K, l2)
    for N, z in zs.items():
        clear, _ = R.clear_rows(z, cb, l2)
        share = float(clear.float().mean())
        print(f"C={Cn} K={K} l2={l2} N={N}: clear rows {share:.4f}")
        assert share > 0.9
