"""The engine's fp32 reference mode (LFQBert.precision = 5, MB_PREC_F32) end to end: its logits against the reference's own fp32 goldens with the float64
oracle as the arbiter, batch invariance and determinism, mb_sample against the host-driven recorded loop, teacher-forced replay of the reference's
recorded runs, and switching the mode on a live model."""
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, golden_weights
from hip_helpers import hip_generator
from oracle import maskbit_oracle as O
from oracle.make_golden_variants import VARIANTS

pytestmark = pytest.mark.gpu
DEV = "cuda"
TINY_GEN = O.GenCfg(bits=12, splits=2, hidden=128, depth=2, heads=4, mlp=256, seq=256, nclass=10)


def rel_fro(got, ref):
    return float((got.double().cpu() - ref.double()).norm() / ref.double().norm())


def oracle_f64(sd, cfg, tokens, labels, drop):
    """The oracle's forward (oracle/maskbit_oracle.py lfq_bert_forward / bert_forward) in float64 with the weights cast to double: its trunk as it is,
    the embedding and the head restated here only because the oracle builds its bit vectors in fp32."""
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    lab = torch.where(drop.bool(), torch.full_like(labels.long(), cfg.nclass), labels.long())
    if cfg.kind == "bert":
        x_tok = sum(sd[f"tok_emb_list.{g}.weight"][tokens[..., g]] for g in range(cfg.splits))
    else:
        x_tok = F.linear(O.token_bit_vectors(tokens, cfg).double(), sd["input_proj.weight"], sd["input_proj.bias"])
    x = torch.cat([x_tok, sd["class_emb.weight"][lab].unsqueeze(1)], dim=1) + sd["pos_emb"]
    x = O._trunk(sd, cfg, x)
    if cfg.kind == "bert":
        C_ = cfg.group_codes
        return torch.stack([torch.matmul(x, sd[f"tok_emb_list.{g}.weight"].t()[:, :C_])[:, :cfg.seq] + sd[f"bias.{g}"] for g in range(cfg.splits)], dim=2)
    logits = F.linear(x, sd["prediction_layer.weight"], sd["prediction_layer.bias"])
    return logits.reshape(tokens.shape[0], cfg.seq + 1, cfg.splits, cfg.group_codes)[:, :cfg.seq]


def _build(cfg, sd):
    from maskbit_amd import LFQBert
    from maskbit_amd.bert import Bert
    cls = Bert if cfg.kind == "bert" else LFQBert
    m = cls(img_size=256, hidden_dim=cfg.hidden, codebook_size=2 ** cfg.bits, codebook_splits=cfg.splits, depth=cfg.depth, heads=cfg.heads,
            mlp_dim=cfg.mlp, dropout=0.1, nclass=cfg.nclass, input_stride=16, use_prenorm=cfg.prenorm)
    m.load_state_dict(sd, strict=True)
    return m.eval().requires_grad_(False).to(DEV)


def _golden_cases():
    yield "gen_tiny", None
    yield "gen_full12", None
    for name in VARIANTS:
        yield "gen_variants_tiny", name


@pytest.mark.parametrize("fixture,variant", list(_golden_cases()), ids=lambda v: str(v))
def test_logits_against_the_reference_goldens_with_float64_as_arbiter(fixture, variant):
    """e_ref = rel-Frobenius error of the reference's fp32 GOLDEN against the float64 oracle: the reference's own fp32 noise.  The precision-5 logits'
    error against the same float64 result must be <= 4 e_ref (a sequential K = 4096 chain is 2-3 x noisier than a blocked sum) and < 1 / 20 of the
    best existing precision's on the same model, measured here.  Figures: profiles/f32_reference.md."""
    z = load_golden(fixture + ".npz")
    if variant:
        cfg, seed = VARIANTS[variant]
        sd = O.make_generator_weights(cfg, seed=seed, head_gain=20.0)
        key = variant + "."
    elif fixture == "gen_tiny":
        cfg, sd, key = TINY_GEN, golden_weights(z), ""
    else:
        cfg = O.GenCfg(bits=12, splits=2)
        sd, key = O.make_generator_weights(cfg, seed=int(z["seed"]), head_gain=float(z["head_gain"])), ""
    toks, labels, drop = (torch.from_numpy(z[key + k]) for k in ("tokens", "labels", "drop"))
    golden = torch.from_numpy(z[key + "logits"])
    exact = oracle_f64(sd, cfg, toks, labels, drop)
    e_ref = rel_fro(golden, exact)
    m = _build(cfg, sd)
    args = (toks.to(DEV), labels.to(DEV), drop.to(DEV))
    errs = {}
    for prec in (0, 1, 2, 3, 4, 5):
        m.precision = prec
        if prec < 5 and m.resolved_precision() in errs:
            continue
        out = m(*args)
        assert out.shape == golden.shape and out.dtype == torch.float32
        errs[m.resolved_precision()] = rel_fro(out, exact)
    best = min(v for p, v in errs.items() if p != 5)
    print(f"{fixture} {variant or ''}: rel-Frobenius error against float64: reference golden {e_ref:.3e}, precision 5 {errs[5]:.3e} "
          f"(ratio {errs[5] / e_ref:.2f}), existing modes {({p: f'{v:.2e}' for p, v in errs.items() if p != 5})}, best / precision 5 = {best / errs[5]:.0f}")
    assert errs[5] <= 4.0 * e_ref
    assert errs[5] < best / 20.0
    assert m.saturation_count() == 0


def test_batch_invariance_and_determinism_at_precision_5():
    z = load_golden("gen_tiny.npz")
    m = hip_generator(TINY_GEN, golden_weights(z))
    m.precision = 5
    t, y, d = torch.from_numpy(z["tokens"]).to(DEV), torch.from_numpy(z["labels"]).to(DEV), torch.from_numpy(z["drop"]).to(DEV)
    full = m(t, y, d)
    assert torch.equal(full, m(t, y, d))
    assert torch.equal(m(t[2:3], y[2:3], d[2:3])[0], full[2])
    big = m(t.repeat(7, 1, 1), y.repeat(7), d.repeat(7))              # 35 sequences: rows cross the GEMM's 128-row tiles at other places
    assert torch.equal(big[:5], full) and torch.equal(big[30:], full)
    # the guided forward is the plain forward over [cond | dropped]
    lg = m.forward_cfg(t, y)
    assert torch.equal(lg[:5], m(t, y, torch.zeros_like(d))) and torch.equal(lg[5:], m(t, y, torch.ones_like(d)))
    with pytest.raises(RuntimeError, match="attention maps are not available"):
        m(t, y, d, return_attn=True)


def test_mb_sample_equals_the_host_driven_recorded_loop_bit_for_bit():
    from maskbit_amd import parity_replay
    from maskbit_amd.checkpoint_check import record_run
    from maskbit_amd.sampling import run_loop
    z = load_golden("sample_tiny_cfg.npz")
    kw = {str(k): str(v) for k, v in zip(z["kw_keys"], z["kw_vals"])}
    kw = {k: (v if k in ("guidance_annealing", "mask_schedule_strategy") else (int(v) if k == "num_steps" else float(v))) for k, v in kw.items()}
    m = hip_generator(TINY_GEN, golden_weights(load_golden("gen_tiny.npz")))
    m.precision = 5
    labels = torch.from_numpy(z["labels"])
    record, (q, c) = record_run(m, labels, int(z["seed"]), **kw)
    plan = parity_replay.plan_of(record)
    assert any(s != 0.0 for s in plan[0]) and any(s == 0.0 for s in plan[0])             # guided and zero-scale steps both occur
    _, _, steps, _ = run_loop(m, None, labels.to(DEV), plan, q, c, want_image=False)
    assert torch.equal(steps.cpu(), record["steps"])
    for i in range(steps.shape[0]):                                                     # the record is consistent with its own masks
        assert torch.equal(parity_replay.tokens_in(record, i) == record["C"], record["masks"][i])
    ref = torch.from_numpy(z["steps"]).long()                                           # and it is the reference's run but for near-ties
    print(f"tiny run at precision 5 against the reference's fixture: {int((steps.cpu() != ref).sum())} of {ref.numel()} tokens differ (free-running)")


@pytest.fixture(scope="module")
def full_models():
    from maskbit_amd import parity_replay
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()                                                               # one full-size generator at a time
            cache[name] = parity_replay.build_models(DEV, with_tokenizer=False, name=name)[0]
        return cache[name]
    return get


@pytest.mark.parametrize("run,modes", [("sample_full10_16_nocfg", (2, 4)), ("sample_full12_64", (2, 3, 4))])
def test_teacher_forced_replay_of_the_reference_runs_at_precision_5(full_models, run, modes):
    """The reference's recorded runs replayed step by step: the fp32 mode's logit error is >= 100 x below the fp16 modes' and the near-tie density is
    linear in it, so its mismatches must be <= 1 + (the best existing mode's count on the same run, measured here) / 20.  Counts: profiles/f32_reference.md.
    (Without guidance precision 3 is precision 2: the activation-lo sets ride in the guided forward only.)"""
    from maskbit_amd import parity_replay
    gen = full_models(run)
    g = parity_replay.load_run(run)
    noise = parity_replay.reference_noise(g, DEV)
    counts = {}
    for prec in modes + (5,):
        gen.precision = prec
        counts[prec], total, per_step, _ = parity_replay.teacher_forced(gen, g=g, noise=noise)
    gen.precision = -1
    best = min(counts[p] for p in modes)
    print(f"{run}: mismatches over {total} sampled positions by precision: {counts}; bound for precision 5: {1 + best / 20:.2f}")
    assert counts[5] <= 1 + best / 20


def test_mode_switching_2_5_2_reproduces_the_logits():
    cfg = O.GenCfg(bits=12, splits=2, depth=2)
    m = _build(cfg, O.make_generator_weights(cfg, seed=5, head_gain=12.0))
    g = torch.Generator().manual_seed(2)
    t, y = torch.randint(0, 65, (3, 256, 2), generator=g).to(DEV), torch.tensor([3, 500, 999]).to(DEV)
    m.precision = 2
    assert m.resolved_precision() == 2
    a, ac = m(t, y), m.forward_cfg(t, y)
    m.precision = 5
    b = m(t, y)
    assert not torch.equal(a, b) and float((a - b).abs().max()) < 0.05 * float(b.abs().max())
    m.precision = 2
    assert torch.equal(m(t, y), a) and torch.equal(m.forward_cfg(t, y), ac)
