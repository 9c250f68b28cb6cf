"""Shared pieces of tests/test_qwen3.py and tests/test_gpu_qwen3.py: a tiny random transformers Qwen3Model (the
oracle), its export as a local Hugging Face directory, and a word-level tokenizer with a chat template made
locally.

The oracle is built with attn_implementation="eager" in fp32.  The recipe makes every likely mistake visible
(fp32 on the CPU, lengths 5 / 40 / 130): initializer_range 0.08 puts the first layer's logits at std 1.05, |max|
4.4, so attention is far from uniform; every norm weight is redrawn from N(1, 0.3), so the norm weights are not
1; hidden_states[-2] differs from last_hidden_state by 0.71 relative and from hidden_states[-3] by 0.76; q / k
norm weights set to 1 move the output by 0.16 / 0.36 / 0.45, the q / k norm removed by 0.16 / 0.38 / 0.47,
adjacent-pair rotation instead of rotate-half by 0.15 / 0.54 / 0.71, against 0.009 / 0.013 / 0.016 for the same
model in bf16."""
import json
from pathlib import Path

import torch

TINY = dict(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=4,
            num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-6, rope_theta=1e6, initializer_range=0.08,
            pad_token_id=0)
SEQ = 192
LENS = [5, 40, 130]


def tiny_hf_model(seed: int = 0, **over):
    """fp32 eager Qwen3Model, random-initialised from `seed`, every *norm.weight ~ N(1, 0.3)."""
    from transformers import Qwen3Config, Qwen3Model
    torch.manual_seed(seed)
    m = Qwen3Model(Qwen3Config(**{**TINY, **over}, attn_implementation="eager")).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("norm.weight"):
                p.normal_(1.0, 0.3)
    return m


def hf_state(model, prefix: str = "") -> dict:
    return {prefix + k: v.detach().clone().contiguous() for k, v in model.state_dict().items()}


def hf_config(model) -> dict:
    return json.loads(model.config.to_json_string())


def export_dir(d: Path, state: dict, config: dict) -> Path:
    from safetensors.torch import save_file
    d = Path(d)
    d.mkdir(parents=True, exist_ok=True)
    save_file(state, str(d / "model.safetensors"))
    (d / "config.json").write_text(json.dumps(config))
    return d


def export_sharded(d: Path, state: dict, config: dict, shards: int = 2) -> Path:
    """The sharded form: model-0000k-of-0000n.safetensors + model.safetensors.index.json."""
    from safetensors.torch import save_file
    d = Path(d)
    d.mkdir(parents=True, exist_ok=True)
    keys, wmap = sorted(state), {}
    for s in range(shards):
        fn = f"model-{s + 1:05d}-of-{shards:05d}.safetensors"
        part = {k: state[k] for k in keys[s::shards]}
        save_file(part, str(d / fn))
        wmap.update({k: fn for k in part})
    (d / "model.safetensors.index.json").write_text(json.dumps({"metadata": {}, "weight_map": wmap}))
    (d / "config.json").write_text(json.dumps(config))
    return d


WORDS = ("a photo of red cat blue dog on the moon woman with hat an old man reading in park two birds over sea "
         "painting city at night small robot and its garden # comment").split()
SPECIALS = ["<|im_start|>", "<|im_end|>", "<think>", "</think>"]
# <|im_start|> role content <|im_end|> per message; <|im_start|> assistant for the generation prompt; the empty
# think block only when enable_thinking is false (Qwen3's template: thinking on leaves the turn open)
CHAT_TEMPLATE = ("{% for m in messages %}<|im_start|> {{ m['role'] }} {{ m['content'] }} <|im_end|> {% endfor %}"
                 "{% if add_generation_prompt %}<|im_start|> assistant"
                 "{% if enable_thinking is defined and enable_thinking is false %} <think> </think>{% endif %}"
                 "{% endif %}")


def make_tokenizer(d: Path, chat_template: bool = True) -> None:
    """WordLevel tokenizer files in d: <pad>=0, <unk>=1, the chat specials, `user`, `assistant`, WORDS; no BOS
    (Qwen's tokenizer adds none); padding_side left, as Qwen's ships."""
    from tokenizers import AddedToken, Tokenizer, models, pre_tokenizers
    vocab = {"<pad>": 0, "<unk>": 1}
    for w in SPECIALS + ["user", "assistant"] + WORDS:
        vocab.setdefault(w, len(vocab))
    tok = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    tok.add_special_tokens([AddedToken(s, special=True) for s in ["<pad>", "<unk>"] + SPECIALS])
    d = Path(d)
    d.mkdir(parents=True, exist_ok=True)
    tok.save(str(d / "tokenizer.json"))
    cfg = {"tokenizer_class": "PreTrainedTokenizerFast", "pad_token": "<pad>", "unk_token": "<unk>",
           "eos_token": "<|im_end|>", "padding_side": "left", "model_max_length": 8192}
    if chat_template:
        cfg["chat_template"] = CHAT_TEMPLATE
    (d / "tokenizer_config.json").write_text(json.dumps(cfg))


def padded_ids(lens, vocab: int, seed: int, seq: int = SEQ):
    """Right-padded random ids and their mask, [len(lens), seq]."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(len(lens), seq, dtype=torch.long)
    mask = torch.zeros(len(lens), seq, dtype=torch.long)
    for b, L in enumerate(lens):
        ids[b, :L] = torch.randint(8, vocab, (L,), generator=g)
        mask[b, :L] = 1
    return ids, mask


def rel_err(a: torch.Tensor, ref: torch.Tensor) -> float:
    return float((a.double() - ref.double()).norm() / ref.double().norm())
