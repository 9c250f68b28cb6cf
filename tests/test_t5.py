"""T5 prompt encoder, the parts that need no GPU: the host-side relative-position bucket table against
transformers, the Hugging Face directory loader, the C-ABI argument checks of eggroll_relbias_attention,
prompt-file parsing and the backend's errors."""
import json

import pytest
import torch

from hyperscalees_t2i_amd import _lib
from hyperscalees_t2i_amd import checkpoints as ck
from hyperscalees_t2i_amd.backend import InfinityBackend, InfinityConfig
from hyperscalees_t2i_amd.infinity_pipeline import T5PromptEncoder, aug_with_positive_prompt, load_prompts_from_txt
from hyperscalees_t2i_amd.t5 import T5Arch, T5Encoder, rel_bias_table, relative_position_bucket

from tests.t5_tiny import TINY, export_dir, hf_state, tiny_hf_encoder


# ---- bucket table ----------------------------------------------------------------------------
@pytest.mark.parametrize("nb,md", [(32, 128), (16, 64)])
def test_buckets_equal_transformers(nb, md):
    from transformers.models.t5.modeling_t5 import T5Attention
    d = torch.arange(-600, 601)
    ref = T5Attention._relative_position_bucket(d, bidirectional=True, num_buckets=nb, max_distance=md)
    got = relative_position_bucket(d, nb, md)
    assert got.dtype == torch.int64 and torch.equal(got, ref)
    assert int(got.min()) == 0 and int(got.max()) == nb - 1


def test_table_equals_compute_bias():
    from transformers import T5Config
    from transformers.models.t5.modeling_t5 import T5Attention
    torch.manual_seed(1)
    att = T5Attention(T5Config(**TINY), has_relative_attention_bias=True)
    N, R = 37, 40
    ref = att.compute_bias(N, N)[0]                                   # [H, N(query), N(key)]
    tab = rel_bias_table(att.relative_attention_bias.weight, R, 32, 128)
    assert tab.shape == (3, 2 * R - 1) and tab.dtype == torch.float32
    i, j = torch.arange(N)[:, None], torch.arange(N)[None, :]
    assert torch.equal(tab[:, j - i + R - 1], ref)
    with pytest.raises(ValueError):
        rel_bias_table(att.relative_attention_bias.weight, R, 16, 64)


# ---- loader ----------------------------------------------------------------------------------
def test_loader_round_trip_and_strictness(tmp_path):
    hf = tiny_hf_encoder(0)
    st, cfg = hf_state(hf), hf.config.to_dict()
    full = dict(st)
    full["decoder.block.0.layer.0.SelfAttention.q.weight"] = torch.zeros(192, 128)
    full["decoder.final_layer_norm.weight"] = torch.ones(128)
    full["lm_head.weight"] = torch.zeros(512, 128)
    enc = ck.load_t5_encoder(export_dir(tmp_path / "full", full, cfg))
    a = enc.arch
    assert (a.d_model, a.d_kv, a.num_heads, a.d_ff, a.num_layers, a.vocab_size) == (128, 64, 3, 256, 2, 512)
    assert a.inner == 192 and (a.num_buckets, a.max_distance, a.eps) == (32, 128, 1e-6)
    bf = lambda k: st[k].to(torch.bfloat16)  # noqa: E731
    assert torch.equal(enc.embed, bf("shared.weight"))
    assert torch.equal(enc.rel_bias, bf("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"))
    assert torch.equal(enc.final_ln, bf("encoder.final_layer_norm.weight"))
    for i, b in enumerate(enc.blocks):
        p = f"encoder.block.{i}.layer"
        assert torch.equal(b.wqkv, torch.cat([bf(f"{p}.0.SelfAttention.{n}.weight") for n in "qkv"]))
        assert torch.equal(b.wo, bf(f"{p}.0.SelfAttention.o.weight"))
        assert torch.equal(b.ln1, bf(f"{p}.0.layer_norm.weight")) and torch.equal(b.ln2, bf(f"{p}.1.layer_norm.weight"))
        assert torch.equal(b.wi0, bf(f"{p}.1.DenseReluDense.wi_0.weight"))
        assert torch.equal(b.wi1, bf(f"{p}.1.DenseReluDense.wi_1.weight"))
        assert torch.equal(b.wo_ff, bf(f"{p}.1.DenseReluDense.wo.weight"))
    # our own export reads back to the same bits; the sharded form with its index loads too
    ck.save_t5_encoder(enc, tmp_path / "ours")
    again = ck.load_t5_encoder(tmp_path / "ours")
    assert all(torch.equal(p, q) for p, q in zip(enc.parameters(), again.parameters()))
    from safetensors.torch import save_file
    sh = tmp_path / "sharded"
    sh.mkdir()
    keys = sorted(st)
    wmap = {}
    for s in range(2):
        fn = f"model-{s + 1:05d}-of-00002.safetensors"
        save_file({k: st[k] for k in keys[s::2]}, str(sh / fn))
        wmap.update({k: fn for k in keys[s::2]})
    (sh / "model.safetensors.index.json").write_text(json.dumps({"metadata": {}, "weight_map": wmap}))
    (sh / "config.json").write_text(json.dumps(cfg))
    third = ck.load_t5_encoder(sh)
    assert all(torch.equal(p, q) for p, q in zip(enc.parameters(), third.parameters()))
    # strict: a missing encoder key and an unused encoder key are refused
    lack = {k: v for k, v in st.items() if k != "encoder.block.1.layer.1.DenseReluDense.wi_1.weight"}
    with pytest.raises(ValueError, match="lacks"):
        ck.load_t5_encoder(export_dir(tmp_path / "lack", lack, cfg))
    extra = dict(st)
    extra["encoder.block.0.layer.0.SelfAttention.extra.weight"] = torch.zeros(4)
    with pytest.raises(ValueError, match="not used"):
        ck.load_t5_encoder(export_dir(tmp_path / "extra", extra, cfg))


def test_loader_refuses_what_is_not_built(tmp_path):
    hf = tiny_hf_encoder(0)
    st, cfg = hf_state(hf), hf.config.to_dict()
    with pytest.raises(NotImplementedError, match="d_kv"):
        ck.load_t5_encoder(export_dir(tmp_path / "dkv", st, {**cfg, "d_kv": 32}))
    with pytest.raises(NotImplementedError, match="feed_forward_proj"):
        ck.load_t5_encoder(export_dir(tmp_path / "relu", st, {**cfg, "feed_forward_proj": "relu"}))
    with pytest.raises(NotImplementedError):
        T5Encoder(T5Arch(d_kv=32, num_layers=1, vocab_size=8, d_model=64, d_ff=64, num_heads=1))
    binonly = tmp_path / "bin"
    binonly.mkdir()
    (binonly / "config.json").write_text(json.dumps(cfg))
    (binonly / "pytorch_model.bin").write_bytes(b"")
    with pytest.raises(FileNotFoundError, match="pytorch_model"):
        ck.load_t5_encoder(binonly)
    with pytest.raises(FileNotFoundError):
        ck.load_t5_encoder(tmp_path / "absent")


def test_default_arch_is_flan_t5_xl():
    a = T5Arch()
    assert (a.d_model, a.d_kv, a.num_heads, a.d_ff, a.num_layers) == (2048, 64, 32, 5120, 24)
    assert (a.num_buckets, a.max_distance, a.eps, a.vocab_size) == (32, 128, 1e-6, 32128)


# ---- C-ABI -----------------------------------------------------------------------------------
def _call(lib, q=4096, B=2, heads=2, N=16, hd=64, R=None):
    p = 4096   # never dereferenced: every call below is refused (or a no-op) before a launch
    return lib.eggroll_relbias_attention(q, 384, p, 384, p, 384, p, N if R is None else R, p, B, heads, N, hd, 1.0, p,
                                         128, None)


def test_capi_argument_checks():
    lib = _lib.load()
    for kw in (dict(hd=128), dict(N=513), dict(N=0), dict(q=None), dict(heads=0), dict(N=16, R=15)):
        assert _call(lib, **kw) == -1, kw
        assert b"relbias_attention" in lib.eggroll_last_error(), kw
    assert _call(lib, B=0) == 0
    assert _call(lib, B=0, q=None) == 0


# ---- prompt file, augmentation, backend errors -----------------------------------------------
def test_prompt_file_and_augmentation(tmp_path):
    txt = tmp_path / "p.txt"
    txt.write_text("  a red cat  \n\n# a comment\n   # indented comment\nan old man reading\n\t\nthe moon\n", encoding="utf-8")
    assert load_prompts_from_txt(txt) == ["a red cat", "an old man reading", "the moon"]
    tail = ". very smooth faces, good looking faces, face to the camera, perfect facial features"
    assert aug_with_positive_prompt("an old man reading") == "an old man reading" + tail
    assert aug_with_positive_prompt("a red cat") == "a red cat"
    assert aug_with_positive_prompt("a humane act") == "a humane act" + tail          # substring match, as the reference
    assert aug_with_positive_prompt("woman and child") == "woman and child" + tail    # appended once


def test_backend_and_encoder_errors(tmp_path):
    enc = tmp_path / "enc.pt"
    cfg = dict(encoded_prompt_path=str(enc), auto_encode_if_missing=True, synthetic_weights=True)
    with pytest.raises(FileNotFoundError, match="prompts_txt_path"):
        InfinityBackend("cpu", InfinityConfig(prompts_txt_path=str(tmp_path / "none.txt"), **cfg))._load_or_encode_prompts()
    txt = tmp_path / "p.txt"
    txt.write_text("a red cat\n")
    with pytest.raises(FileNotFoundError, match="text_encoder_ckpt"):
        InfinityBackend("cpu", InfinityConfig(prompts_txt_path=str(txt), text_encoder_ckpt=str(tmp_path / "no_t5"),
                                              **cfg))._load_or_encode_prompts()
    with pytest.raises(FileNotFoundError, match="google/flan-t5-xl"):       # the default: a hub id, not a directory
        InfinityBackend("cpu", InfinityConfig(prompts_txt_path=str(txt), **cfg))._load_or_encode_prompts()
    assert not enc.exists()
    assert InfinityConfig().auto_encode_if_missing is False
    with pytest.raises(FileNotFoundError, match="auto_encode disabled"):
        InfinityBackend("cpu", InfinityConfig(encoded_prompt_path=str(enc)))._load_or_encode_prompts()
    hf = tiny_hf_encoder(0)
    d = export_dir(tmp_path / "t5", hf_state(hf), hf.config.to_dict())
    with pytest.raises(ValueError, match="text_channels"):
        T5PromptEncoder(d, "cpu", 2048)
