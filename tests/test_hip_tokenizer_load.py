"""GPU checks of the tokenizer handles' checkpoint loaders (mb_dec_load, mb_taming_load) called directly: what they refuse, with which code and
message, and that a refused entry leaves the handle as it was.  Three handles: a tiny lookup ConvVQModel, the same model with the LFQ quantizer
and OriginalVQModel.  Codes (include/maskbit_hip.h): -2 an entry the handle has no slot for, -4 an entry of the wrong size."""
import ctypes as C

import pytest
import torch

from hip_helpers import tok_config
from maskbit_amd import _lib
from maskbit_amd.synth import TokCfg, make_taming_weights, make_tokenizer_weights, make_vq_codebook

pytestmark = pytest.mark.gpu
DEV = "cuda"
TINY = TokCfg(token_size=12, hidden_channels=64, channel_mult=(1, 1, 2), num_resolutions=3, num_res_blocks=1)


def tiny(lookup: bool):
    from maskbit_amd import ConvVQModel
    sd = make_tokenizer_weights(TINY, seed=31, with_encoder=True, lfq_buffers=not lookup)
    cfg = tok_config(TINY)
    if lookup:
        sd["quantize.embedding.weight"] = make_vq_codebook(512, 12, 33, torch.zeros(12), torch.ones(12) * 0.5)
        cfg.update(quantizer_type="lookup", codebook_size=512, use_l2_normalisation=False)
    m = ConvVQModel(cfg)
    m.load_state_dict(sd, strict=True)
    return m, "mb_dec_load", torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(32))


def taming():
    from maskbit_amd import OriginalVQModel
    sd = make_taming_weights(41)
    sd["quantize.embedding.weight"] = make_vq_codebook(1024, 256, 43, torch.zeros(256), torch.ones(256) * 0.5)
    m = OriginalVQModel(None)
    m.load_state_dict(sd, strict=True)
    return m, "mb_taming_load", torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(42))


# (entry, the message's words): each is handed over one element short of its size in the state dict
SHORT_TINY = [("decoder.norm_out.weight", "wrong norm size"), ("encoder.norm_out.bias", "wrong norm size"),
              ("decoder.conv_in.bias", "wrong bias size"), ("encoder.down.0.down_conv.bias", "wrong bias size"),
              ("decoder.conv_in.weight", "wrong weight size"), ("encoder.down.0.down_conv.weight", "wrong weight size"),
              ("decoder.up.1.res_blocks.0.nin_shortcut.weight", "wrong weight size")]
SHORT_TAMING = [("decoder.norm_out.weight", "wrong norm size"), ("encoder.mid.attn_1.norm.bias", "wrong norm size"),
                ("decoder.conv_in.bias", "wrong bias size"), ("decoder.conv_out.bias", "wrong bias size"),
                ("decoder.conv_in.weight", "wrong weight size"), ("decoder.conv_out.weight", "wrong weight size"),
                ("encoder.down.0.downsample.conv.weight", "wrong weight size"),
                # one of q / k / v inside the stacked 1x1 convolution: the row-slice path
                ("encoder.mid.attn_1.k.weight", "wrong weight size"), ("encoder.mid.attn_1.k.bias", "wrong bias size")]
# ... and the row-slice entries with the size of the whole stacked convolution
STACKED_TAMING = [("encoder.mid.attn_1.k.weight", (3 * 512, 512, 1, 1), "wrong weight size"), ("encoder.mid.attn_1.k.bias", (3 * 512,), "wrong bias size")]
CASES = {"lookup": (lambda: tiny(True), SHORT_TINY, [], (512, 12), "expected [codebook_size, token_size]"),
         "lfq": (lambda: tiny(False), SHORT_TINY, [], None, None),
         "taming": (taming, SHORT_TAMING, STACKED_TAMING, (1024, 256), "expected [1024, 256]")}


def outputs(m, x):
    rec, res = m(x)
    torch.cuda.synchronize()
    return rec.clone(), res["min_encoding_indices"].clone(), m.saturation_count()


@pytest.mark.parametrize("which", list(CASES))
def test_loader_refusals_leave_the_handle_intact(which):
    make, short, more, cb_shape, cb_msg = CASES[which]
    m, entry, x = make()
    m = m.eval().requires_grad_(False).to(DEV)
    x = x.to(DEV)
    before = outputs(m, x)
    h = m._engine
    sd = m.state_dict()
    lib = _lib.load()
    load = getattr(lib, entry)
    stream = torch.cuda.current_stream().cuda_stream
    data = torch.zeros(1 << 21, device=DEV)              # more floats than any shape below names: a loader that took one would stay inside it

    def refused(name, shape):
        n = 1
        for v in shape:
            n *= v
        assert n <= data.numel()
        rc = load(h, name.encode(), data.data_ptr(), (C.c_int64 * len(shape))(*shape), len(shape), stream)
        return rc, lib.mb_last_error().decode()

    rc, msg = refused("decoder.no_such_layer.weight", (4,))
    assert rc == -2 and entry in msg and "unknown checkpoint entry" in msg and "decoder.no_such_layer.weight" in msg, (rc, msg)
    for name, shape, words in [(name, (sd[name].numel() - 1,), words) for name, words in short] + more:
        rc, msg = refused(name, shape)
        assert rc == -4 and entry in msg and words in msg and name in msg, (name, rc, msg)
    if cb_shape is not None:
        Cn, K = cb_shape
        assert tuple(sd["quantize.embedding.weight"].shape) == cb_shape
        for shape in ((Cn, K + 1), (Cn - 1, K), (Cn * K,), (Cn, K, 1)):
            rc, msg = refused("quantize.embedding.weight", shape)
            assert rc == -4 and entry in msg and cb_msg in msg, (shape, rc, msg)
    after = outputs(m, x)
    assert m._engine is h                                  # the same handle, not a reloaded one
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1]) and after[2] == before[2]
    assert bool(torch.isfinite(after[0]).all())
