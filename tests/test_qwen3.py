"""Qwen3 prompt encoder, the parts that need no GPU: config -> arch and the refused configs, the Hugging Face
directory loader, the host-side RoPE tables against transformers, the C-ABI argument checks of
eggroll_causal_attention / eggroll_qk_norm_rope_half, Z-Image's template-and-tokenise step, its prompt-file
rule and the backend's errors."""
import pytest
import torch

from hyperscalees_t2i_amd import _lib
from hyperscalees_t2i_amd import checkpoints as ck
from hyperscalees_t2i_amd.backend import ZImageBackend, ZImageConfig
from hyperscalees_t2i_amd.qwen3 import Qwen3Arch, Qwen3Encoder, rope_tables
from hyperscalees_t2i_amd.zimage_pipeline import QwenPromptEncoder, ZImageTurboES, load_prompts_from_txt

from tests.qwen3_tiny import export_dir, export_sharded, hf_config, hf_state, make_tokenizer, tiny_hf_model


def _is_norm(k: str) -> bool:
    return k.endswith("norm.weight")


def _as_built(st: dict) -> dict:
    """The checkpoint in the dtypes the build holds it in: norm weights fp32, everything else bf16."""
    return {k: (v.float() if _is_norm(k) else v.to(torch.bfloat16)) for k, v in st.items()}


# ---- config ----------------------------------------------------------------------------------
def test_default_arch_is_qwen3_4b():
    a = Qwen3Arch()
    assert (a.hidden_size, a.num_layers, a.num_heads, a.num_kv_heads, a.head_dim) == (2560, 36, 32, 8, 128)
    assert (a.intermediate_size, a.vocab_size, a.eps, a.rope_theta) == (9728, 151936, 1e-6, 1e6)
    assert (a.q_width, a.kv_width, a.run_layers) == (4096, 1024, 35)
    from hyperscalees_t2i_amd.zimage import ZIMAGE_TURBO
    assert a.hidden_size == ZIMAGE_TURBO.cap_feat_dim


def test_config_to_arch_and_refusals():
    cfg = hf_config(tiny_hf_model(0))
    a = ck.qwen3_arch_from_config(cfg)
    assert (a.hidden_size, a.num_layers, a.num_heads, a.num_kv_heads, a.head_dim) == (128, 3, 4, 2, 128)
    assert (a.intermediate_size, a.rope_theta, a.eps, a.vocab_size) == (256, 1e6, 1e-6, 512)
    # Qwen3-4B's published config.json carries rope_theta at the top level and rope_scaling null
    flat = {k: v for k, v in cfg.items() if k != "rope_parameters"}
    assert ck.qwen3_arch_from_config({**flat, "rope_theta": 5000.0, "rope_scaling": None}).rope_theta == 5000.0
    assert ck.qwen3_arch_from_config({**cfg, "layer_types": ["full_attention"] * 3}) == a
    assert ck.qwen3_arch_from_config(ck.qwen3_config_from_arch(a)) == a
    for field, bad in (("head_dim", {"head_dim": 64}), ("attention_bias", {"attention_bias": True}),
                       ("hidden_act", {"hidden_act": "gelu"}),
                       ("rope", {"rope_parameters": {"rope_type": "yarn", "factor": 4.0, "rope_theta": 1e6}}),
                       ("rope", {"rope_parameters": None, "rope_scaling": {"type": "linear", "factor": 2.0}}),
                       ("use_sliding_window", {"use_sliding_window": True}),
                       ("layer_types", {"layer_types": ["full_attention", "sliding_attention", "full_attention"]}),
                       ("hidden_size", {"hidden_size": 132}), ("hidden_size", {"hidden_size": 8192})):
        with pytest.raises(NotImplementedError, match=field):
            ck.qwen3_arch_from_config({**cfg, **bad})
    with pytest.raises(NotImplementedError, match="head_dim"):
        Qwen3Encoder(Qwen3Arch(head_dim=256, num_layers=2, vocab_size=8, hidden_size=64, intermediate_size=64))
    with pytest.raises(ValueError):
        Qwen3Encoder(Qwen3Arch(num_heads=3, num_kv_heads=2, num_layers=2, vocab_size=8, hidden_size=64,
                               intermediate_size=64))


# ---- loader ----------------------------------------------------------------------------------
def test_loader_round_trip_and_strictness(tmp_path):
    hf = tiny_hf_model(0)
    st, cfg = hf_state(hf), hf_config(hf)
    enc = ck.load_qwen3_encoder(export_dir(tmp_path / "plain", st, cfg))
    built = _as_built(st)
    assert len(enc.blocks) == 2                      # 3 layers: hidden_states[-2] needs the first two
    names = [n for n, _ in enc.named_parameters()]
    assert not any("final" in n or n.startswith("norm") or "blocks.2" in n for n in names), names
    assert torch.equal(enc.embed, built["embed_tokens.weight"])
    for i, b in enumerate(enc.blocks):
        p = f"layers.{i}"
        assert torch.equal(b.wqkv, torch.cat([built[f"{p}.self_attn.{n}_proj.weight"] for n in "qkv"]))
        assert b.wqkv.shape == (4 * 128 + 2 * 2 * 128, 128) and b.wqkv.dtype == torch.bfloat16
        assert torch.equal(b.wo, built[f"{p}.self_attn.o_proj.weight"])
        assert torch.equal(b.w_gate, built[f"{p}.mlp.gate_proj.weight"])
        assert torch.equal(b.w_up, built[f"{p}.mlp.up_proj.weight"])
        assert torch.equal(b.w_down, built[f"{p}.mlp.down_proj.weight"])
        assert b.q_norm.dtype == torch.float32 and torch.equal(b.q_norm, built[f"{p}.self_attn.q_norm.weight"])
        assert torch.equal(b.k_norm, built[f"{p}.self_attn.k_norm.weight"]) and not torch.equal(b.q_norm, b.k_norm)
        for ours, theirs in (("ln_in", "input_layernorm"), ("ln_post_attn", "post_attention_layernorm")):
            w = getattr(b, ours)                     # held as w - 1, fp32 (rownorm's 1 + mscale operand)
            assert w.dtype == torch.float32 and torch.equal(w[0], built[f"{p}.{theirs}.weight"] - 1.0), (i, ours)
    # the `model.` prefix of a Qwen3ForCausalLM checkpoint, with its lm_head accepted and not loaded
    pre = hf_state(hf, "model.")
    pre["lm_head.weight"] = torch.zeros(512, 128)
    lm = ck.load_qwen3_encoder(export_dir(tmp_path / "lm", pre, cfg))
    assert all(torch.equal(p, q) for p, q in zip(enc.parameters(), lm.parameters()))
    assert [n for n, _ in lm.named_parameters()] == names
    # the sharded form with its index
    sh = ck.load_qwen3_encoder(export_sharded(tmp_path / "sharded", pre, cfg))
    assert all(torch.equal(p, q) for p, q in zip(enc.parameters(), sh.parameters()))
    # the last layer and the final norm may be absent: they are never read
    cut = {k: v for k, v in st.items() if not k.startswith("layers.2.") and k != "norm.weight"}
    short = ck.load_qwen3_encoder(export_dir(tmp_path / "cut", cut, cfg))
    assert all(torch.equal(p, q) for p, q in zip(enc.parameters(), short.parameters()))
    # save -> load: the same parameters
    ck.save_qwen3_encoder(enc, tmp_path / "ours")
    again = ck.load_qwen3_encoder(tmp_path / "ours")
    assert again.arch == enc.arch
    for (n, p), q in zip(enc.named_parameters(), again.parameters()):
        assert torch.allclose(p.float(), q.float(), rtol=0, atol=2e-7 if "ln_" in n else 0), n   # (w - 1) + 1 - 1
    # strict: a missing tensor, an unused tensor and a wrong shape are refused
    lack = {k: v for k, v in st.items() if k != "layers.1.self_attn.k_norm.weight"}
    with pytest.raises(ValueError, match="lacks"):
        ck.load_qwen3_encoder(export_dir(tmp_path / "lack", lack, cfg))
    for extra_key in ("layers.0.self_attn.q_proj.bias", "layers.2.self_attn.rotary.inv_freq", "layers.3.mlp.up_proj.weight"):
        extra = dict(st)
        extra[extra_key] = torch.zeros(4)
        with pytest.raises(ValueError, match="not used"):
            ck.load_qwen3_encoder(export_dir(tmp_path / f"extra{len(extra_key)}", extra, cfg))
    wrong = dict(st)
    wrong["layers.0.self_attn.q_norm.weight"] = torch.ones(64)
    with pytest.raises(ValueError, match="q_norm"):
        ck.load_qwen3_encoder(export_dir(tmp_path / "wrong", wrong, cfg))
    with pytest.raises(FileNotFoundError):
        ck.load_qwen3_encoder(tmp_path / "absent")


# ---- RoPE tables -----------------------------------------------------------------------------
def test_rope_tables_equal_transformers():
    """Exact: the same fp32 expressions in the same order (the matmul of Qwen3RotaryEmbedding has an inner
    dimension of 1, so it is the plain product)."""
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RotaryEmbedding
    hf = tiny_hf_model(0)
    rot = Qwen3RotaryEmbedding(hf.config)
    cos_ref, sin_ref = rot(torch.zeros(1, 512, 128), torch.arange(512)[None])
    cos, sin = rope_tables(512, 128, 1e6)
    assert cos.shape == sin.shape == (512, 64) and cos.dtype == sin.dtype == torch.float32
    assert torch.equal(torch.cat([cos, cos], -1), cos_ref[0]) and torch.equal(torch.cat([sin, sin], -1), sin_ref[0])


# ---- C-ABI -----------------------------------------------------------------------------------
def _attn(lib, q=4096, B=2, hq=4, hkv=2, N=16, hd=128, scale=0.088, ldq=1024, ldo=512, lens=4096):
    p = 4096   # never dereferenced: every call below is refused (or a no-op) before a launch
    return lib.eggroll_causal_attention(q, ldq, p, 1024, p, 1024, lens, B, hq, hkv, N, hd, scale, p, ldo, None)


def _nr(lib, x=4096, ldx=1024, B=2, N=16, hq=3, hkv=2, hd=128, eps=1e-6, wq=4096, cos=4096):
    p = 4096
    return lib.eggroll_qk_norm_rope_half(x, ldx, B, N, hq, hkv, hd, eps, wq, p, cos, p, None)


def test_capi_argument_checks():
    lib = _lib.load()
    for kw in (dict(hd=256), dict(hd=64), dict(N=0), dict(q=None), dict(lens=None), dict(hkv=0), dict(hq=3, hkv=2),
               dict(hq=2, hkv=4), dict(scale=0.0), dict(scale=float("inf")), dict(q=4100), dict(ldq=1020), dict(ldq=256),
               dict(ldo=384), dict(B=-1), dict(N=2 ** 31)):
        assert _attn(lib, **kw) == -1, kw
        assert b"causal_attention" in lib.eggroll_last_error(), kw
    assert _attn(lib, B=0) == 0
    assert _attn(lib, B=0, q=None) == 0
    for kw in (dict(hd=256), dict(ldx=512), dict(ldx=1028), dict(x=None), dict(wq=None), dict(cos=None), dict(x=4104),
               dict(cos=4100), dict(hq=0), dict(hkv=0), dict(N=0), dict(B=-1), dict(eps=-1.0)):
        assert _nr(lib, **kw) == -1, kw
        assert b"qk_norm_rope_half" in lib.eggroll_last_error(), kw
    assert _nr(lib, B=0) == 0
    assert _nr(lib, B=0, x=None) == 0


# ---- template and tokenise -------------------------------------------------------------------
def _encoder_without_weights(tok_dir):
    """A QwenPromptEncoder with its tokenizer only (template / tokenize need no encoder)."""
    from transformers import AutoTokenizer
    pe = QwenPromptEncoder.__new__(QwenPromptEncoder)
    pe.tokenizer, pe.encoder, pe.device = AutoTokenizer.from_pretrained(str(tok_dir)), None, "cpu"
    return pe


def test_template_and_tokenise(tmp_path):
    make_tokenizer(tmp_path / "tok")
    pe = _encoder_without_weights(tmp_path / "tok")
    assert pe.tokenizer.padding_side == "left"              # as Qwen's ships; the Z-Image path forces the right
    prompts = ["a photo of red cat", "an old man " * 40]
    s = pe.template(prompts)
    assert s[0] == "<|im_start|> user a photo of red cat <|im_end|> <|im_start|> assistant"   # the generation prompt
    assert "<think>" not in s[0] and "</think>" not in s[1]                                    # enable_thinking=True
    off = pe.tokenizer.apply_chat_template([{"role": "user", "content": "a"}], tokenize=False,
                                           add_generation_prompt=True, enable_thinking=False)
    assert off.endswith("assistant <think> </think>")       # the template does tell the two apart
    ids, mask = pe.tokenize(prompts, 32)
    assert pe.tokenizer.padding_side == "right" and ids.shape == mask.shape == (2, 32)
    v = pe.tokenizer.get_vocab()
    want = [v["<|im_start|>"], v["user"]] + [v[w] for w in prompts[0].split()] + [v["<|im_end|>"], v["<|im_start|>"],
                                                                                  v["assistant"]]
    assert ids[0, :10].tolist() == want and not ids[0, 10:].any()          # padded on the right with <pad> = 0
    assert mask[0].tolist() == [1] * 10 + [0] * 22
    assert int(mask[1].sum()) == 32 and ids[1, :2].tolist() == want[:2]     # 125 tokens truncated to the limit
    ids512, mask512 = pe.tokenize(prompts, 512)
    assert ids512.shape == (2, 512) and mask512.sum(-1).tolist() == [10, 125]
    with pytest.raises(RuntimeError, match="dropped"):
        pe.encode(prompts)
    # a tokenizer without a chat template is refused before any weight loads
    hf = tiny_hf_model(0)
    d = export_dir(tmp_path / "q", hf_state(hf), hf_config(hf))
    make_tokenizer(d, chat_template=False)
    with pytest.raises(ValueError, match="chat_template"):
        QwenPromptEncoder("unused", "cpu", text_encoder_path=str(d))
    # so is a width that does not match the transformer's cap_feat_dim
    make_tokenizer(d)
    with pytest.raises(ValueError, match="cap_feat_dim"):
        QwenPromptEncoder("unused", "cpu", text_encoder_path=str(d), cap_feat_dim=2560)


def test_prompt_file(tmp_path):
    txt = tmp_path / "p.txt"
    txt.write_text("  a red cat  \n\n# a comment\n   # indented\nan old man reading\n\t\nthe moon\n", encoding="utf-8")
    assert load_prompts_from_txt(txt) == ["a red cat", "# a comment", "# indented", "an old man reading", "the moon"]


# ---- backend errors --------------------------------------------------------------------------
def test_backend_and_encoder_errors(tmp_path):
    assert ZImageConfig().auto_encode_if_missing is False and ZImageConfig().text_encoder_path == ""
    enc = tmp_path / "enc.pt"
    with pytest.raises(FileNotFoundError, match="auto_encode disabled"):
        ZImageBackend("cpu", ZImageConfig(encoded_prompt_path=str(enc)))._load_or_encode_prompts()
    cfg = dict(encoded_prompt_path=str(enc), auto_encode_if_missing=True, synthetic_weights=True)
    with pytest.raises(FileNotFoundError, match="prompts_txt_path"):
        ZImageBackend("cpu", ZImageConfig(prompts_txt_path=str(tmp_path / "none.txt"), **cfg))._load_or_encode_prompts()
    txt = tmp_path / "p.txt"
    txt.write_text("a red cat\n")
    with pytest.raises(FileNotFoundError, match="Tongyi-MAI/Z-Image-Turbo"):
        ZImageBackend("cpu", ZImageConfig(prompts_txt_path=str(txt), **cfg))._load_or_encode_prompts()   # a hub id
    with pytest.raises(FileNotFoundError, match="no_qwen"):
        ZImageBackend("cpu", ZImageConfig(prompts_txt_path=str(txt), text_encoder_path=str(tmp_path / "no_qwen"),
                                          **cfg))._load_or_encode_prompts()
    assert not enc.exists()
    # an instance built only to encode holds neither the transformer nor the VAE, and says so when asked to generate
    es = ZImageTurboES("nowhere/model", device="cpu", encode_only=True)
    assert es.transformer is None and es.vae is None and es.text_encoder is None
    with pytest.raises(FileNotFoundError, match="nowhere/model"):
        es.encode_prompts(txt, enc)
    with pytest.raises(RuntimeError, match="encode_only"):
        es.generate_one_batch([torch.zeros(4, 2560)])
    with pytest.raises(RuntimeError, match="encode_only"):
        es.generate_population([torch.zeros(4, 2560)], torch.zeros(1, dtype=torch.long), torch.zeros(1, 8), 0, 0.0, 64, 64)
    # an empty encoded_prompt_path still gives the synthetic prompts
    be = ZImageBackend("cpu", ZImageConfig(synthetic_prompts=3))
    be._load_or_encode_prompts()
    assert len(be.base_prompt_embeds) == 3 and all(e.shape[1] == 2560 for e in be.base_prompt_embeds)
