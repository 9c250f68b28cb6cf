"""Shared pieces of tests/test_t5.py and tests/test_gpu_t5.py: a tiny random transformers T5EncoderModel
(the oracle), its export as a local Hugging Face directory, and a word-level tokenizer made locally."""
import json
from pathlib import Path

import torch

TINY = dict(vocab_size=512, d_model=128, d_kv=64, num_heads=3, d_ff=256, num_layers=2,
            feed_forward_proj="gated-gelu", relative_attention_num_buckets=32, relative_attention_max_distance=128)


def tiny_hf_encoder(seed: int = 0, **over):
    """fp32 T5EncoderModel, random-initialised from `seed`: 3 heads x 64 (inner 192 != d_model 128)."""
    from transformers import T5Config, T5EncoderModel
    torch.manual_seed(seed)
    return T5EncoderModel(T5Config(**{**TINY, **over})).eval()


def hf_state(model) -> dict:
    return {k: v.detach().clone().contiguous() for k, v in model.state_dict().items()}


def export_dir(d: Path, state: dict, config: dict) -> Path:
    from safetensors.torch import save_file
    d = Path(d)
    d.mkdir(parents=True, exist_ok=True)
    save_file(state, str(d / "model.safetensors"))
    (d / "config.json").write_text(json.dumps(config))
    return d


WORDS = ("a photo of red cat blue dog on the moon woman with hat an old man reading in park two birds over sea "
         "painting city at night small robot and its garden").split()


def make_tokenizer(d: Path) -> None:
    """WordLevel tokenizer files in d: <pad>=0, </s>=1, <unk>=2, a TemplateProcessing that appends </s>."""
    from tokenizers import Tokenizer, models, pre_tokenizers, processors
    vocab = {"<pad>": 0, "</s>": 1, "<unk>": 2}
    for w in WORDS:
        vocab.setdefault(w, len(vocab))
    tok = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = pre_tokenizers.Whitespace()
    tok.post_processor = processors.TemplateProcessing(single="$A </s>", special_tokens=[("</s>", 1)])
    d = Path(d)
    d.mkdir(parents=True, exist_ok=True)
    tok.save(str(d / "tokenizer.json"))
    (d / "tokenizer_config.json").write_text(json.dumps(
        {"tokenizer_class": "PreTrainedTokenizerFast", "pad_token": "<pad>", "eos_token": "</s>", "unk_token": "<unk>",
         "model_max_length": 512}))


def rel_err(a: torch.Tensor, ref: torch.Tensor) -> float:
    return float((a.double() - ref.double()).norm() / ref.double().norm())
