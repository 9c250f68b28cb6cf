"""Gemma-2 prompt encoder, the parts that need no GPU: config -> arch and the refused configs, the Hugging
Face directory loader, the host-side RoPE tables against transformers, the C-ABI argument checks of
eggroll_softcap_attention / eggroll_rope_half, Sana's tokenise-and-select step and the backend's errors."""
import pytest
import torch

from hyperscalees_t2i_amd import _lib
from hyperscalees_t2i_amd import checkpoints as ck
from hyperscalees_t2i_amd.backend import SanaBackend, SanaConfig
from hyperscalees_t2i_amd.gemma2 import Gemma2Arch, Gemma2Encoder, rope_tables
from hyperscalees_t2i_amd.pipeline import GemmaPromptEncoder, SanaOneStep, load_prompts_from_txt, tokenize_for_sana

from tests.gemma2_tiny import export_dir, export_sharded, hf_config, hf_state, make_tokenizer, tiny_hf_model


def _is_norm(k: str) -> bool:
    return k.endswith("norm.weight")


def _as_built(st: dict) -> dict:
    """The checkpoint in the dtypes the build holds it in: norm weights fp32, everything else bf16."""
    return {k: (v.float() if _is_norm(k) else v.to(torch.bfloat16)) for k, v in st.items()}


# ---- config ----------------------------------------------------------------------------------
def test_default_arch_is_gemma_2_2b():
    a = Gemma2Arch()
    assert (a.hidden_size, a.num_layers, a.num_heads, a.num_kv_heads, a.head_dim) == (2304, 26, 8, 4, 256)
    assert (a.intermediate_size, a.softcap, a.query_pre_attn_scalar, a.rope_theta) == (9216, 50.0, 256.0, 10000.0)
    assert (a.eps, a.vocab_size, a.q_width, a.kv_width) == (1e-6, 256000, 2048, 1024)


def test_config_to_arch_and_refusals():
    cfg = hf_config(tiny_hf_model(0))
    a = ck.gemma2_arch_from_config(cfg)
    assert (a.hidden_size, a.num_layers, a.num_heads, a.num_kv_heads, a.head_dim) == (128, 2, 2, 1, 256)
    assert (a.intermediate_size, a.softcap, a.query_pre_attn_scalar, a.rope_theta) == (256, 5.0, 64.0, 10000.0)
    assert (a.eps, a.vocab_size, a.sliding_window) == (1e-6, 512, 4096)
    # gemma-2-2b's published config.json carries rope_theta at the top level and no rope_parameters
    flat = {k: v for k, v in cfg.items() if k != "rope_parameters"}
    assert ck.gemma2_arch_from_config({**flat, "rope_theta": 5000.0}).rope_theta == 5000.0
    assert ck.gemma2_arch_from_config({**cfg, "attn_logit_softcapping": None}).softcap == 0.0
    assert ck.gemma2_arch_from_config(ck.gemma2_config_from_arch(a)) == a
    with pytest.raises(NotImplementedError, match="head_dim"):
        ck.gemma2_arch_from_config({**cfg, "head_dim": 128})
    with pytest.raises(NotImplementedError, match="hidden_activation"):
        ck.gemma2_arch_from_config({**cfg, "hidden_activation": "gelu"})
    with pytest.raises(NotImplementedError, match="attention_bias"):
        ck.gemma2_arch_from_config({**cfg, "attention_bias": True})
    with pytest.raises(NotImplementedError):
        Gemma2Encoder(Gemma2Arch(head_dim=128, num_layers=1, vocab_size=8, hidden_size=64, intermediate_size=64))


# ---- loader ----------------------------------------------------------------------------------
def test_loader_round_trip_and_strictness(tmp_path):
    hf = tiny_hf_model(0)
    st, cfg = hf_state(hf), hf_config(hf)
    enc = ck.load_gemma2_encoder(export_dir(tmp_path / "plain", st, cfg))
    built = _as_built(st)
    assert torch.equal(enc.embed, built["embed_tokens.weight"])
    assert enc.final_ln.dtype == torch.float32 and torch.equal(enc.final_ln[0], built["norm.weight"])
    for i, b in enumerate(enc.blocks):
        p = f"layers.{i}"
        assert torch.equal(b.wqkv, torch.cat([built[f"{p}.self_attn.{n}_proj.weight"] for n in "qkv"]))
        assert b.wqkv.shape == (2 * 256 + 2 * 256, 128) and b.wqkv.dtype == torch.bfloat16
        assert torch.equal(b.wo, built[f"{p}.self_attn.o_proj.weight"])
        assert torch.equal(b.w_gate, built[f"{p}.mlp.gate_proj.weight"])
        assert torch.equal(b.w_up, built[f"{p}.mlp.up_proj.weight"])
        assert torch.equal(b.w_down, built[f"{p}.mlp.down_proj.weight"])
        for ours, theirs in (("ln_in", "input_layernorm"), ("ln_post_attn", "post_attention_layernorm"),
                             ("ln_pre_ff", "pre_feedforward_layernorm"), ("ln_post_ff", "post_feedforward_layernorm")):
            assert torch.equal(getattr(b, ours)[0], built[f"{p}.{theirs}.weight"]), (i, ours)
    # load -> save -> state: the original, in the dtypes the build holds
    from safetensors.torch import load_file
    ck.save_gemma2_encoder(enc, tmp_path / "ours")
    saved = load_file(str(tmp_path / "ours" / "model.safetensors"))
    assert set(saved) == set(built) and all(torch.equal(saved[k], built[k]) for k in built)
    again = ck.load_gemma2_encoder(tmp_path / "ours")
    assert again.arch == enc.arch and all(torch.equal(p, q) for p, q in zip(enc.parameters(), again.parameters()))
    # the `model.` prefix of a Gemma2ForCausalLM checkpoint, with its lm_head ignored
    pre = hf_state(hf, "model.")
    pre["lm_head.weight"] = torch.zeros(512, 128)
    lm = ck.load_gemma2_encoder(export_dir(tmp_path / "lm", pre, cfg))
    assert all(torch.equal(p, q) for p, q in zip(enc.parameters(), lm.parameters()))
    # the sharded form with its index
    sh = ck.load_gemma2_encoder(export_sharded(tmp_path / "sharded", pre, cfg))
    assert all(torch.equal(p, q) for p, q in zip(enc.parameters(), sh.parameters()))
    # strict: a missing tensor and an unused tensor are refused
    lack = {k: v for k, v in st.items() if k != "layers.1.pre_feedforward_layernorm.weight"}
    with pytest.raises(ValueError, match="lacks"):
        ck.load_gemma2_encoder(export_dir(tmp_path / "lack", lack, cfg))
    extra = dict(st)
    extra["layers.0.self_attn.q_norm.weight"] = torch.zeros(4)
    with pytest.raises(ValueError, match="not used"):
        ck.load_gemma2_encoder(export_dir(tmp_path / "extra", extra, cfg))
    with pytest.raises(FileNotFoundError):
        ck.load_gemma2_encoder(tmp_path / "absent")


# ---- RoPE tables -----------------------------------------------------------------------------
def test_rope_tables_equal_transformers():
    from transformers.models.gemma2.modeling_gemma2 import Gemma2RotaryEmbedding
    hf = tiny_hf_model(0)
    rot = Gemma2RotaryEmbedding(hf.config)
    cos_ref, sin_ref = rot(torch.zeros(1, 300, 128), torch.arange(300)[None])
    cos, sin = rope_tables(300, 256, 10000.0)
    assert cos.shape == sin.shape == (300, 128) and cos.dtype == sin.dtype == torch.float32
    assert torch.equal(torch.cat([cos, cos], -1), cos_ref[0]) and torch.equal(torch.cat([sin, sin], -1), sin_ref[0])


# ---- C-ABI -----------------------------------------------------------------------------------
def _attn(lib, q=4096, B=2, hq=4, hkv=2, N=16, hd=256, cap=5.0, ldq=2048):
    p = 4096   # never dereferenced: every call below is refused (or a no-op) before a launch
    return lib.eggroll_softcap_attention(q, ldq, p, 2048, p, 2048, p, B, hq, hkv, N, hd, 0.125, cap, p, 1024, None)


def test_capi_argument_checks():
    lib = _lib.load()
    for kw in (dict(hd=128), dict(N=0), dict(q=None), dict(hkv=0), dict(hq=3, hkv=2), dict(cap=-1.0), dict(q=4100),
               dict(ldq=1020), dict(B=-1)):
        assert _attn(lib, **kw) == -1, kw
        assert b"softcap_attention" in lib.eggroll_last_error(), kw
    assert _attn(lib, B=0) == 0
    assert _attn(lib, B=0, q=None) == 0
    p = 4096
    assert lib.eggroll_rope_half(p, 1024, 2, 16, 3, 128, p, p, None) == -1
    assert b"rope_half" in lib.eggroll_last_error()
    assert lib.eggroll_rope_half(p, 512, 2, 16, 3, 256, p, p, None) == -1       # row stride < 3 heads
    assert lib.eggroll_rope_half(None, 1024, 2, 16, 3, 256, p, p, None) == -1
    assert lib.eggroll_rope_half(None, 1024, 0, 16, 3, 256, p, p, None) == 0


# ---- tokenise and select ---------------------------------------------------------------------
def test_tokenise_and_select(tmp_path):
    from transformers import AutoTokenizer
    make_tokenizer(tmp_path / "tok")
    tok = AutoTokenizer.from_pretrained(str(tmp_path / "tok"))
    assert tok.padding_side == "left"                       # as Gemma's ships; the Sana path forces the right
    prompts = GemmaPromptEncoder.preprocess(["  A Photo of RED cat ", "an old man " * 200])
    assert prompts[0] == "a photo of red cat" and prompts[1] == ("an old man " * 200).strip()
    ids, mask = tokenize_for_sana(tok, prompts)
    assert ids.shape == mask.shape == (2, 300)
    vocab = tok.get_vocab()
    assert ids[0, :6].tolist() == [1] + [vocab[w] for w in "a photo of red cat".split()]      # BOS first
    assert not ids[0, 6:].any() and mask[0].tolist() == [1] * 6 + [0] * 294                   # padded on the right
    assert int(mask[1].sum()) == 300 and int(ids[1, 0]) == 1                                  # truncated at 300
    sel = GemmaPromptEncoder.select_index(300)
    assert len(sel) == 300 and sel[0] == 0 and sel[1:] == list(range(-299, 0))
    # a complex-human-instruction list: joined with newlines, prefixed; max length len(encode(chi)) + 300 - 2
    chi = ["given a user prompt generate an enhanced prompt", "user prompt "]     # the prompt is appended as is
    n_chi = len(tok.encode("\n".join(chi)))
    assert n_chi == 11                                                                         # BOS + 10 words
    ids2, mask2 = tokenize_for_sana(tok, prompts, chi)
    assert ids2.shape == (2, n_chi + 298)
    assert ids2[0, :n_chi].tolist() == tok.encode("\n".join(chi)) and ids2[0, n_chi:n_chi + 5].tolist() == ids[0, 1:6].tolist()
    picked = ids2[:, [i % ids2.shape[1] for i in sel]]
    assert picked.shape == (2, 300) and torch.equal(picked[:, 0], ids2[:, 0]) and torch.equal(picked[:, 1:], ids2[:, -299:])
    assert torch.equal(ids2[:, sel], picked)


def test_prompt_file(tmp_path):
    txt = tmp_path / "p.txt"
    txt.write_text("  a red cat  \n\n# a comment\n   # indented comment\nan old man reading\n\t\nthe moon\n", encoding="utf-8")
    assert load_prompts_from_txt(txt) == ["a red cat", "an old man reading", "the moon"]


# ---- backend errors --------------------------------------------------------------------------
def test_backend_and_encoder_errors(tmp_path):
    assert SanaConfig().auto_encode_if_missing is False and SanaConfig().text_encoder_path == ""
    enc = tmp_path / "enc.pt"
    with pytest.raises(FileNotFoundError, match="auto_encode disabled"):
        SanaBackend("cpu", SanaConfig(encoded_prompt_path=str(enc)))._load_or_encode_prompts()
    cfg = dict(encoded_prompt_path=str(enc), auto_encode_if_missing=True, synthetic_weights=True)
    with pytest.raises(FileNotFoundError, match="prompts_txt_path"):
        SanaBackend("cpu", SanaConfig(prompts_txt_path=str(tmp_path / "none.txt"), **cfg))._load_or_encode_prompts()
    txt = tmp_path / "p.txt"
    txt.write_text("a red cat\n")
    with pytest.raises(FileNotFoundError, match="Efficient-Large-Model/Sana_Sprint_1.6B_1024px_diffusers"):
        SanaBackend("cpu", SanaConfig(prompts_txt_path=str(txt), **cfg))._load_or_encode_prompts()   # a hub id
    with pytest.raises(FileNotFoundError, match="no_gemma"):
        SanaBackend("cpu", SanaConfig(prompts_txt_path=str(txt), text_encoder_path=str(tmp_path / "no_gemma"),
                                      **cfg))._load_or_encode_prompts()
    assert not enc.exists()
    # an instance built only to encode holds neither the transformer nor the DC-AE
    es = SanaOneStep("nowhere/model", device="cpu", encode_only=True)
    assert es.transformer is None and es.vae is None and es.text_encoder is None
    with pytest.raises(FileNotFoundError, match="nowhere/model"):
        es.encode_prompts(txt, enc)
    # an empty encoded_prompt_path still gives the synthetic prompts
    be = SanaBackend("cpu", SanaConfig(synthetic_prompts=3))
    be._load_or_encode_prompts()
    assert be.base_prompt_embeds.shape == (3, 300, 2304)
    # a width that does not match the transformer's caption_channels is refused before any weight loads
    hf = tiny_hf_model(0)
    d = export_dir(tmp_path / "g", hf_state(hf), hf_config(hf))
    make_tokenizer(d)
    with pytest.raises(ValueError, match="caption_channels"):
        GemmaPromptEncoder("unused", "cpu", text_encoder_path=str(d), caption_channels=2304)
