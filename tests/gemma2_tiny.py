"""Shared pieces of tests/test_gemma2.py and tests/test_gpu_gemma2.py: a tiny random transformers Gemma2Model
(the oracle), its export as a local Hugging Face directory, and a word-level tokenizer made locally.

The oracle is built with attn_implementation="eager": the sdpa path of transformers drops the soft-cap
without a word.  The recipe makes every likely mistake visible: initializer_range 0.08 and
query_pre_attn_scalar 64 (!= head_dim 256) put the first layer's pre-cap logits at std 1.6, |max| 7.1 against
the cap of 5, and the norm weights are drawn from N(0, 0.3) so `1 + w` is not 1."""
import json
from pathlib import Path

import torch

TINY = dict(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
            num_key_value_heads=1, head_dim=256, attn_logit_softcapping=5.0, query_pre_attn_scalar=64,
            initializer_range=0.08, pad_token_id=0, bos_token_id=1, eos_token_id=2)
SEQ = 300          # SanaSprintPipeline.encode_prompt's max_sequence_length
LENS = [5, 40, 300]


def tiny_hf_model(seed: int = 0, **over):
    """fp32 eager Gemma2Model, random-initialised from `seed`, norm weights ~ N(0, 0.3)."""
    from transformers import Gemma2Config, Gemma2Model
    torch.manual_seed(seed)
    m = Gemma2Model(Gemma2Config(**{**TINY, **over}, attn_implementation="eager")).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("norm.weight") or n.endswith("layernorm.weight"):
                p.normal_(0.0, 0.3)
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
         "painting city at night small robot and its garden given user prompt generate enhanced for image").split()


def make_tokenizer(d: Path) -> None:
    """WordLevel tokenizer files in d: <pad>=0, <bos>=1, <eos>=2, <unk>=3, a TemplateProcessing that prepends
    <bos> (Gemma's tokenizer adds BOS and no EOS)."""
    from tokenizers import Tokenizer, models, pre_tokenizers, processors
    vocab = {"<pad>": 0, "<bos>": 1, "<eos>": 2, "<unk>": 3}
    for w in WORDS:
        vocab.setdefault(w, len(vocab))
    tok = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = pre_tokenizers.Whitespace()
    tok.post_processor = processors.TemplateProcessing(single="<bos> $A", special_tokens=[("<bos>", 1)])
    d = Path(d)
    d.mkdir(parents=True, exist_ok=True)
    tok.save(str(d / "tokenizer.json"))
    (d / "tokenizer_config.json").write_text(json.dumps(
        {"tokenizer_class": "PreTrainedTokenizerFast", "pad_token": "<pad>", "bos_token": "<bos>", "eos_token": "<eos>",
         "unk_token": "<unk>", "padding_side": "left", "model_max_length": 8192}))


def padded_ids(lens, vocab: int, seed: int, seq: int = SEQ):
    """Right-padded random ids (BOS first) and their mask, [len(lens), seq]."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(len(lens), seq, dtype=torch.long)
    mask = torch.zeros(len(lens), seq, dtype=torch.long)
    for b, L in enumerate(lens):
        ids[b, :L] = torch.randint(4, vocab, (L,), generator=g)
        ids[b, 0] = 1
        mask[b, :L] = 1
    return ids, mask


def rel_err(a: torch.Tensor, ref: torch.Tensor) -> float:
    return float((a.double() - ref.double()).norm() / ref.double().norm())
