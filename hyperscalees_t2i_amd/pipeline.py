"""Sana-Sprint one-step generator (models/SanaSprint.py:10-164 `SanaOneStep`), ES-compatible
(models/baseEGG.py:14-77 `ESBaseModel` contract: `self.transformer` is the LoRA target,
`generate(...) -> (images, latents_out)`), plus the population entry point that evaluates every
local member in one batched forward.

One-step SCM / trigflow math exactly as the reference (models/SanaSprint.py:78-164):
  latents = randn(b, 32, h, w, Generator(device).manual_seed(seed), dtype=DTYPE) * sigma_data
  scm = sin(1.571) / (cos(1.571) + sin(1.571));  guidance = g * guidance_embeds_scale
  eps = nan_to_num(transformer(latents / sigma_data, scm, prompt, mask, guidance))
  pred = ((1-2s) x + (1-2s+2s^2) eps) / sqrt(s^2 + (1-s)^2) * sigma_data
  x0 = (0.267 latents - 0.964 pred) / sigma_data;  image = vae.decode(x0 / scaling_factor)
Common random numbers: every member uses the same latents (seed = epoch) and prompts
(unifed_es.py:163), so latents are drawn once and broadcast over members.

The multi-step sampler (models/SanaSprint.py:280-502 `SanaPipelineES`) follows below SanaOneStep; its math is
in that class's docstring.
"""
from __future__ import annotations

import math
from pathlib import Path
from typing import Any, List, NamedTuple, Optional, Sequence, Tuple

import torch

from .dcae import DCAEDecoder
from .lora import PopulationContext, set_population
from .sana import SANA_SPRINT_1_6B, SanaArch, SanaTransformer2DModel


class ESBaseModel:
    """models/baseEGG.py:14-77."""

    def __init__(self, model_name: str, device: str = "cuda:0", DTYPE: torch.dtype = torch.float32,
                 sigma_data: float = 0.5):
        self.model_name = str(model_name)
        self.device = str(device)
        self.DTYPE = DTYPE
        self.sigma_data = float(sigma_data)
        self.transformer: Optional[torch.nn.Module] = None

    def generate(self, *a, **k):
        raise NotImplementedError("Subclasses must implement generate()")

    def encode_prompts(self, *a, **k):
        raise NotImplementedError("Subclasses must implement encode_prompts()")


def load_prompts_from_txt(path, keep_comments: bool = False) -> List[str]:
    """models/SanaSprint.py:165-169: one prompt per line; blank lines and # lines are skipped.
    keep_comments: the loader of the pipeline class (models/SanaSprint.py:329-332), which skips blank lines only."""
    lines = Path(path).read_text(encoding="utf-8").splitlines()
    return [ln.strip() for ln in lines if ln.strip() and (keep_comments or not ln.strip().startswith("#"))]


class GemmaPromptEncoder:
    """The text side of SanaSprintPipeline on its own (diffusers `_get_gemma_prompt_embeds` + `encode_prompt`,
    clean_caption=False, restated from the published source — PARITY WITH DIFFUSERS UNPINNED, it is not
    importable here): the tokenizer and the Gemma-2 encoder (gemma2.py) of a local directory.  `model_name` is a
    diffusers model directory (text_encoder/ + tokenizer/); `text_encoder_path`, when given, is one directory
    that holds both the checkpoint and the tokenizer files and takes precedence.  Building it never
    instantiates the Sana transformer or the DC-AE."""

    MAX_SEQUENCE_LENGTH = 300

    def __init__(self, model_name, device: str, text_encoder_path: Optional[str] = None,
                 caption_channels: Optional[int] = None):
        if text_encoder_path:
            enc_dir = tok_dir = Path(str(text_encoder_path))
            named = str(text_encoder_path)
        else:
            enc_dir, tok_dir = Path(str(model_name)) / "text_encoder", Path(str(model_name)) / "tokenizer"
            named = str(model_name)
        if not enc_dir.is_dir() or not tok_dir.is_dir():
            raise FileNotFoundError(f"Sana text encoder {named!r}: not a local directory with "
                                    f"{'config.json, model.safetensors and the tokenizer files' if text_encoder_path else 'text_encoder/ and tokenizer/'}"
                                    f" of a Gemma-2 checkpoint (there is no hub access)")
        from . import checkpoints as ck
        arch = ck.gemma2_arch_from_config(ck.read_config(enc_dir))
        if caption_channels is not None and arch.hidden_size != int(caption_channels):
            raise ValueError(f"{enc_dir}: Gemma-2 hidden_size {arch.hidden_size} != caption_channels "
                             f"{int(caption_channels)}")
        from transformers import AutoTokenizer
        self.tokenizer = AutoTokenizer.from_pretrained(str(tok_dir))
        self.tokenizer.padding_side = "right"
        self.device = device
        self.encoder = ck.load_gemma2_encoder(enc_dir, device)

    @staticmethod
    def preprocess(prompts: Sequence[str]) -> List[str]:
        """`_text_preprocessing(clean_caption=False)`: lower-case, strip."""
        return [str(p).lower().strip() for p in prompts]

    @staticmethod
    def select_index(max_sequence_length: int = MAX_SEQUENCE_LENGTH) -> List[int]:
        """Position 0 (BOS), then the last max_sequence_length - 1 positions of the padded sequence."""
        return [0] + list(range(-max_sequence_length + 1, 0))

    def tokenize(self, prompts: Sequence[str], complex_human_instruction=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(input_ids, attention_mask) [B, max_length], right-padded, truncated, with special tokens.  max_length
        is 300, or with a complex_human_instruction list (joined with newlines and prefixed to every prompt)
        len(tokenizer.encode(chi)) + 300 - 2."""
        return tokenize_for_sana(self.tokenizer, prompts, complex_human_instruction, self.MAX_SEQUENCE_LENGTH)

    @torch.no_grad()
    def encode(self, prompts: Sequence[str], complex_human_instruction=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(prompt_embeds [B, 300, C] bf16 on the device, prompt_attention_mask [B, 300] int64 CPU).  Rows the
        mask marks as padding are zeros."""
        if self.encoder is None:
            raise RuntimeError("GemmaPromptEncoder: the encoder was dropped")
        ids, mask = self.tokenize(prompts, complex_human_instruction)
        lens = mask.sum(dim=-1)
        if not torch.equal(mask, (torch.arange(mask.shape[1])[None, :] < lens[:, None]).to(mask.dtype)):
            raise ValueError("GemmaPromptEncoder: the tokenizer did not pad on the right")
        h = self.encoder(ids, lens)                                   # [B, N = max(lens), C]; rows >= len: padding
        B, N, C = h.shape
        valid = (torch.arange(N)[None, :] < lens[:, None]).to(h.device)
        full = torch.zeros((B, mask.shape[1], C), dtype=h.dtype, device=h.device)
        full[:, :N] = h * valid[..., None]
        sel = self.select_index(self.MAX_SEQUENCE_LENGTH)
        return full[:, sel], mask[:, sel].to(torch.int64)

    @torch.no_grad()
    def encode_file(self, prompts_txt_path, encoded_save_path, batch_size: int = 4,
                    complex_human_instruction=None, keep_comments: bool = False) -> dict:
        """models/SanaSprint.py:195-277: the .txt's prompts -> {"prompts", "prompt_embeds" [P, 300, C] fp16 CPU,
        "prompt_attention_mask" [P, 300] int64 CPU}, saved with torch.save and returned."""
        prompts = load_prompts_from_txt(prompts_txt_path, keep_comments)
        if not prompts:
            raise ValueError(f"{prompts_txt_path}: no prompts (blank {'lines' if keep_comments else 'and # lines'} "
                             f"are skipped)")
        return self.encode_list(prompts, encoded_save_path, batch_size, complex_human_instruction)

    @torch.no_grad()
    def encode_list(self, prompts: Sequence[str], encoded_save_path, batch_size: int = 4,
                    complex_human_instruction=None) -> dict:
        """encode_file's payload for the given prompts, in their order, none dropped."""
        prompts = [str(p) for p in prompts]
        embeds, masks = [], []
        for start in range(0, len(prompts), max(int(batch_size), 1)):
            e, m = self.encode(self.preprocess(prompts[start:start + max(int(batch_size), 1)]),
                               complex_human_instruction)
            e16 = e.to(torch.float16)
            if not bool(torch.isfinite(e16).all()):
                raise RuntimeError(f"GemmaPromptEncoder: prompts {start}..{start + e.shape[0] - 1} do not fit fp16 "
                                   f"(max |x| = {float(e.float().abs().max()):.3e}); the saved format is float16")
            embeds.append(e16.cpu())
            masks.append(m.cpu())
        payload = {"prompts": prompts, "prompt_embeds": torch.cat(embeds), "prompt_attention_mask": torch.cat(masks)}
        enc = Path(encoded_save_path)
        enc.parent.mkdir(parents=True, exist_ok=True)
        torch.save(payload, enc)
        return payload

    def drop(self):
        self.encoder = None
        if torch.cuda.is_available():
            torch.cuda.empty_cache()


def tokenize_for_sana(tokenizer, prompts: Sequence[str], complex_human_instruction=None,
                      max_sequence_length: int = 300) -> Tuple[torch.Tensor, torch.Tensor]:
    """diffusers `_get_gemma_prompt_embeds`' tokenizer call (see GemmaPromptEncoder.tokenize)."""
    tokenizer.padding_side = "right"
    prompts = list(prompts)
    if not complex_human_instruction:
        max_length = max_sequence_length
    else:
        chi = "\n".join(complex_human_instruction)
        prompts = [chi + p for p in prompts]
        max_length = len(tokenizer.encode(chi)) + max_sequence_length - 2
    tok = tokenizer(prompts, padding="max_length", max_length=max_length, truncation=True, add_special_tokens=True,
                    return_tensors="pt")
    return tok.input_ids, tok.attention_mask


class _SanaStack(ESBaseModel):
    """What SanaOneStep and SanaPipelineES share: the transformer + DC-AE build and the prompt cache.
    Weights: `model_name` is a LOCAL diffusers-format directory
    (transformer/ + vae/, loaded by checkpoints.py; the architecture comes from its config.json files,
    `arch` / `vae_*` are ignored), or — only with synthetic_weights=True — anything, in which case
    the given architecture is built with seeded synthetic weights (throughput runs).
    Anything else raises FileNotFoundError: there is no hub access, and silently substituting random
    weights for a named checkpoint would produce plausible-looking but meaningless numbers."""

    KEEP_COMMENT_PROMPTS = False   # the prompt .txt loader keeps # lines (load_prompts_from_txt)

    def __init__(self, model_name: str = "Efficient-Large-Model/Sana_Sprint_1.6B_1024px_diffusers",
                 device: str = "cuda:0", DTYPE: torch.dtype = torch.float16, sigma_data: float = 0.5,
                 arch: SanaArch = SANA_SPRINT_1_6B, vae_widths=(128, 256, 512, 512, 1024, 1024),
                 vae_layers=(3, 3, 3, 3, 3, 3), weight_seed: int = 0, vae_chunk: int = 8,
                 synthetic_weights: bool = False, text_encoder_path: Optional[str] = None,
                 encode_only: bool = False):
        """text_encoder_path: one local directory with the Gemma-2 checkpoint and its tokenizer files, used by
        encode_prompts in place of model_name/text_encoder + model_name/tokenizer.  encode_only: build neither
        the transformer nor the DC-AE (an instance that exists to call encode_prompts)."""
        from . import checkpoints as C
        super().__init__(model_name, device, DTYPE, sigma_data)
        dev = torch.device(device)
        root = Path(str(model_name))
        self.text_encoder_path = str(text_encoder_path) if text_encoder_path else None
        self.tokenizer = self.text_encoder = self._prompt_encoder = None
        self.vae = None
        if encode_only:
            self.weights_source = "none (encode only)"
        elif C.is_local_model_dir(str(model_name)):
            arch = C.sana_arch_from_config(C.read_config(root / "transformer"))
            vkw = C.dcae_build_kwargs(C.read_config(root / "vae"))
            with torch.device(dev):
                self.transformer = SanaTransformer2DModel(arch)
                self.vae = DCAEDecoder(**vkw)
            C.load_sana_transformer(self.transformer, root / "transformer")
            C.load_dcae_decoder(self.vae, root / "vae")
            self.weights_source = str(root)
        elif synthetic_weights:
            with torch.device(dev):
                self.transformer = SanaTransformer2DModel(arch)
                self.vae = DCAEDecoder(arch.in_channels, widths=vae_widths, layers=vae_layers)
            self.transformer.init_weights(weight_seed)
            self.vae.init_weights(weight_seed + 1)
            self.weights_source = f"synthetic(seed={weight_seed})"
        else:
            why = ("exists but lacks transformer/ or vae/" if root.exists()
                   else "is not a local directory (no hub downloads offline)")
            raise FileNotFoundError(f"{type(self).__name__}: model_name {str(model_name)!r} {why}; pass a local diffusers "
                                    f"model directory, or synthetic_weights=True for seeded random weights")
        self.transformer_config = arch
        self.vae_chunk = vae_chunk
        self.ctx = PopulationContext()

    # ---- prompt cache (models/SanaSprint.py:165-277) --------------------------------
    def encode_prompts(self, prompts_txt_path, encoded_save_path, batch_size: int = 4, complex_human_instruction=None,
                       overwrite: bool = False):
        """models/SanaSprint.py:171-277.  An existing file loads unless overwrite; else the prompts of the .txt
        are encoded as SanaSprintPipeline.encode_prompt(clean_caption=False, max_sequence_length=300) does, by
        the Gemma-2 encoder and tokenizer of model_name/text_encoder + model_name/tokenizer (or of
        text_encoder_path), both local.  One difference from the reference: rows past a prompt's length are
        zeros here, where the reference keeps the model's output for the pad tokens; Sana's cross-attention
        masks those rows, so nothing downstream sees them."""
        enc = Path(encoded_save_path)
        if enc.is_file() and not overwrite:
            return torch.load(enc, map_location="cpu", weights_only=True)
        if self._prompt_encoder is None or self._prompt_encoder.encoder is None:
            cc = self.transformer_config.caption_channels if self.transformer is not None else None
            self._prompt_encoder = GemmaPromptEncoder(self.model_name, self.device, self.text_encoder_path, cc)
            self.tokenizer, self.text_encoder = self._prompt_encoder.tokenizer, self._prompt_encoder.encoder
        return self._prompt_encoder.encode_file(prompts_txt_path, enc, batch_size, complex_human_instruction,
                                                self.KEEP_COMMENT_PROMPTS)

    def encode_prompt_list(self, prompts: Sequence[str], encoded_save_path, batch_size: int = 4,
                           complex_human_instruction=None):
        """encode_prompts for prompts given as a list (a prompt table's column): every entry is encoded, in order,
        so row i of the file is prompts[i].  Always writes encoded_save_path."""
        if self._prompt_encoder is None or self._prompt_encoder.encoder is None:
            cc = self.transformer_config.caption_channels if self.transformer is not None else None
            self._prompt_encoder = GemmaPromptEncoder(self.model_name, self.device, self.text_encoder_path, cc)
            self.tokenizer, self.text_encoder = self._prompt_encoder.tokenizer, self._prompt_encoder.encoder
        return self._prompt_encoder.encode_list(prompts, Path(encoded_save_path), batch_size, complex_human_instruction)

    def drop_text_encoder(self):
        if self._prompt_encoder is not None:
            self._prompt_encoder.drop()
        self._prompt_encoder = None
        self.text_encoder = None


class SanaOneStep(_SanaStack):
    """models/SanaSprint.py:10-60: the one-step generator (build and prompt cache: _SanaStack)."""

    # ---- shared one-step math -------------------------------------------------------
    def _latents(self, b: int, seed: int, h: int, w: int) -> torch.Tensor:
        g = torch.Generator(device=self.device).manual_seed(int(seed))
        lat = torch.randn(b, self.transformer_config.in_channels, h, w, device=self.device, dtype=self.DTYPE,
                          generator=g)
        return lat * self.sigma_data

    @torch.no_grad()
    def _one_step(self, latents, prompt_embeds, prompt_attention_mask, guidance_scale, reps: int,
                  prompt_index: Optional[torch.Tensor] = None):
        """prompt_index (optional): [b] image -> row of prompt_embeds / mask, which then hold the
        distinct prompts only (the images of one prompt share its caption k / v, see sana.py)."""
        b = latents.shape[0]
        lmi = latents / self.sigma_data
        t = torch.tensor(1.571, device=self.device, dtype=torch.float32)
        timestep = t.expand(b)
        scm = torch.sin(timestep) / (torch.cos(timestep) + torch.sin(timestep))
        se = scm.view(-1, 1, 1, 1)
        guidance = torch.full((b,), guidance_scale, device=self.device, dtype=self.DTYPE)
        guidance = guidance * self.transformer_config.guidance_embeds_scale

        def rep(x):
            return x if reps == 1 else x.repeat(reps, *([1] * (x.ndim - 1)))  # member-major stacking

        enc_index = None
        if prompt_index is not None:
            u = prompt_embeds.shape[0]
            enc_index = (torch.arange(reps, device=self.device)[:, None] * u + prompt_index.to(self.device)[None, :]).reshape(-1)
        eps = self.transformer(rep(lmi.float()), rep(scm.float()), rep(prompt_embeds), rep(prompt_attention_mask),
                               rep(guidance.float()), enc_index=enc_index)
        eps = torch.nan_to_num(eps.float(), nan=0.0, posinf=0.0, neginf=0.0)
        # dtype semantics of models/SanaSprint.py:138-153: eps rounded to the latent dtype (fp16) before
        # the SCM combine, which promotes to fp32 through the fp32 scm tensor; 0.267 * latents is an fp16
        # product (python scalar x fp16 tensor) before the fp32 subtraction
        eps = eps.to(self.DTYPE)
        lmi_r, se_r = rep(lmi), rep(se)
        pred = ((1 - 2 * se_r) * lmi_r + (1 - 2 * se_r + 2 * se_r ** 2) * eps) / torch.sqrt(se_r ** 2 + (1 - se_r) ** 2)
        pred = pred.float() * self.sigma_data
        x0 = (rep(0.267 * latents) - 0.964 * pred) / self.sigma_data
        z = x0 / self.vae.scaling_factor
        imgs = [self.vae(z[s:s + self.vae_chunk]) for s in range(0, z.shape[0], self.vae_chunk)]
        return torch.cat(imgs), z

    # ---- reference API (single member: the transformer's own LoRA params) ------------
    @torch.no_grad()
    def generate(self, prompt_embeds, prompt_attention_mask, latents=None, seed: int = 0, guidance_scale: float = 1.0,
                 width_latent: int = 32, height_latent: int = 32, output_type: str = "pil"):
        """models/SanaSprint.py:60-164.  Returns (images, latents in VAE scale)."""
        set_population(self.transformer, None)
        if latents is None:
            latents = self._latents(prompt_embeds.shape[0], seed, height_latent, width_latent)
        imgs, z = self._one_step(latents, prompt_embeds, prompt_attention_mask, guidance_scale, reps=1)
        if output_type == "pt":
            return imgs, z
        return to_pil(imgs), z

    # ---- engine API -----------------------------------------------------------------
    @torch.no_grad()
    def generate_population(self, prompt_embeds, prompt_attention_mask, theta_pop: torch.Tensor, seed: int,
                            guidance_scale: float, width_latent: int, height_latent: int,
                            prompt_index: Optional[torch.Tensor] = None,
                            flat_seeds: Optional[Sequence[int]] = None) -> torch.Tensor:
        """All members of theta_pop [n, D] at once: returns VAE images [n*b, 3, H, W] (member-major).
        prompt_index: [b] image -> distinct-prompt row (prompt_embeds then holds the distinct prompts).
        flat_seeds: [b] per-image seeds: image i gets the latents of a one-image draw from Generator(flat_seeds[i])
        (every member the same ones) instead of its slice of one b-image draw from `seed`."""
        n = theta_pop.shape[0]
        self.ctx.theta_pop, self.ctx.n_members = theta_pop, n
        set_population(self.transformer, self.ctx)
        try:
            b = prompt_embeds.shape[0] if prompt_index is None else prompt_index.numel()
            if flat_seeds is None:
                latents = self._latents(b, seed, height_latent, width_latent)
            else:
                if len(flat_seeds) != b:
                    raise ValueError(f"flat_seeds has {len(flat_seeds)} entries for {b} images")
                latents = torch.cat([self._latents(1, int(s), height_latent, width_latent) for s in flat_seeds])
            imgs, _ = self._one_step(latents, prompt_embeds, prompt_attention_mask, guidance_scale, reps=n,
                                     prompt_index=prompt_index)
        finally:
            set_population(self.transformer, None)
            self.ctx.theta_pop = None
        return imgs


# ---------------------------------------------------------------------------------------
# Multi-step SCM sampler (models/SanaSprint.py:280-502 `SanaPipelineES`)
# ---------------------------------------------------------------------------------------

# True: the arithmetic between two forwards is one eggroll_scm_step launch; False: its torch form
# (_step_torch, about fifteen elementwise launches) — kept for A/B runs and as what the kernel is tested against
FUSE_SCM_STEP = True

SCM_MAX_TIMESTEPS = 1.57080
SCM_INTERMEDIATE_TIMESTEPS = 1.3
_ROUND_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def scm_timesteps(num_inference_steps: int, max_timesteps: float = SCM_MAX_TIMESTEPS,
                  intermediate_timesteps: Optional[float] = SCM_INTERMEDIATE_TIMESTEPS) -> List[float]:
    """SCMScheduler.set_timesteps: [max, intermediate, 0] (two steps only), or with intermediate_timesteps=None
    linspace(max, 0, steps + 1).  The sampler loops over all but the last."""
    steps = int(num_inference_steps)
    if steps < 1:
        raise ValueError(f"num_inference_steps must be >= 1, got {num_inference_steps}")
    if intermediate_timesteps is not None:
        if steps != 2:
            raise ValueError("Intermediate timesteps for SCM is not supported when num_inference_steps != 2.")
        return [float(max_timesteps), float(intermediate_timesteps), 0.0]
    return torch.linspace(float(max_timesteps), 0.0, steps + 1, dtype=torch.float64).tolist()


def scm_s(t: float) -> float:
    """The SCM timestep the transformer is conditioned on: sin t / (cos t + sin t)."""
    return math.sin(t) / (math.cos(t) + math.sin(t))


class ScmStepScalars(NamedTuple):
    """The scalars of one sampler step (eggroll_scm_step), fp64 on the host."""
    in_scale: float
    coef_m: float
    coef_eps: float
    cos_t: float
    sin_t: float
    cos_n: float
    sin_n_sd: float
    in_scale_next: float
    out_scale: float


def scm_step_scalars(t: float, n: float, sigma_data: float, out_scale: float = 1.0) -> ScmStepScalars:
    """Angular time t of this step, n of the next.  The pipeline feeds the transformer m = x / sigma_data * q with
    q = sqrt(s^2 + (1 - s)^2) and combines pred = ((1 - 2s) m + (1 - 2s + 2s^2) eps) / q * sigma_data; the
    scheduler takes x0 = cos t x - sin t pred and x_next = cos n x0 + sin n sigma_data noise."""
    s, sn = scm_s(t), scm_s(n)
    q, qn = math.sqrt(s * s + (1 - s) ** 2), math.sqrt(sn * sn + (1 - sn) ** 2)
    return ScmStepScalars(q / sigma_data, (1 - 2 * s) * sigma_data / q, (1 - 2 * s + 2 * s * s) * sigma_data / q,
                          math.cos(t), math.sin(t), math.cos(n), math.sin(n) * sigma_data, qn / sigma_data,
                          float(out_scale))


def _rnd(v: torch.Tensor, round_dtype: int) -> torch.Tensor:
    """fp32 -> the model dtype and back (round_dtype 0 none, 1 fp16, 2 bf16)."""
    if round_dtype == 0:
        return v.float()
    return v.to(torch.float16 if round_dtype == 1 else torch.bfloat16).float()


def _step_torch(x, eps, noise, sc: ScmStepScalars, round_dtype: int, members: int = 1, last: bool = False):
    """The torch form of eggroll_scm_step on the same fp32 scalars: (x_next, m_next, None), or on the last step
    (None, None, x0_out), each shaped like eps.  x: one member's elements (shared) or every member's."""
    c = ScmStepScalars(*[float(torch.tensor(v, dtype=torch.float32)) for v in sc])
    n = eps.numel() // members
    xm = x.float().reshape(-1, n)                                  # [1 or members, n]
    m = _rnd(xm * c.in_scale, round_dtype)
    pred = c.coef_m * m + c.coef_eps * _rnd(eps.float().reshape(members, n), round_dtype)
    x0 = c.cos_t * xm - c.sin_t * pred
    if last:
        return None, None, (x0 * c.out_scale).reshape(eps.shape)
    x_next = c.cos_n * x0 + c.sin_n_sd * noise.float().reshape(1, n)
    return x_next.reshape(eps.shape), _rnd(x_next * c.in_scale_next, round_dtype).reshape(eps.shape), None


class SanaPipelineES(_SanaStack):
    """models/SanaSprint.py:280-502: the multi-step Sana-Sprint sampler (num_inference_steps transformer
    forwards, two by default), with the population entry point of SanaOneStep.  The reference wraps diffusers'
    SanaSprintPipeline; the sampler here is restated from the published SanaSprintPipeline.__call__ and
    SCMScheduler — PARITY WITH DIFFUSERS UNPINNED, diffusers is not importable here:
      timesteps [1.57080, 1.3, 0] (SCMScheduler.set_timesteps); one Generator(seed) draws the fp32 initial
      latents (x sigma_data) and then one fp32 noise per step, the last included (its value is unused);
      per step at angular time t, s = sin t / (cos t + sin t), q = sqrt(s^2 + (1 - s)^2):
        m = DTYPE(x / sigma_data * q);  eps = transformer(m, DTYPE(s), prompt, mask, guidance)
        pred = ((1 - 2s) m + (1 - 2s + 2s^2) DTYPE(eps)) / q * sigma_data
        x0 = cos t x - sin t pred;  x = cos t' x0 + sin t' sigma_data noise   (t' the next time)
      image = vae.decode(x0 / sigma_data / scaling_factor) after the last step.
    Everything between two forwards is one eggroll_scm_step launch over all members (FUSE_SCM_STEP); the
    per-member state stays token-major [members * b, h * w, C] fp32, and the transformer and the decoder get
    NCHW views of it.  Two departures from the reference: the combine runs in fp32 where diffusers promotes
    fp16 operands, and width_latent / height_latent are honoured (the reference hard-codes 1024 px = 32 x 32).
    There is no nan_to_num (the pipeline has none; the engine masks a non-finite member).  Latents and step
    noise are common random numbers: the reference reseeds the generator for every member."""

    KEEP_COMMENT_PROMPTS = True   # models/SanaSprint.py:329-332

    def __init__(self, model_name: str = "Efficient-Large-Model/Sana_Sprint_1.6B_1024px_diffusers",
                 device: str = "cuda:0", DTYPE: torch.dtype = torch.float16, sigma_data: float = 0.5,
                 num_inference_steps: int = 2, arch: SanaArch = SANA_SPRINT_1_6B,
                 vae_widths=(128, 256, 512, 512, 1024, 1024), vae_layers=(3, 3, 3, 3, 3, 3), weight_seed: int = 0,
                 vae_chunk: int = 8, synthetic_weights: bool = False, text_encoder_path: Optional[str] = None,
                 encode_only: bool = False, max_timesteps: float = SCM_MAX_TIMESTEPS,
                 intermediate_timesteps: Optional[float] = SCM_INTERMEDIATE_TIMESTEPS):
        if DTYPE not in _ROUND_DTYPES:
            raise ValueError(f"SanaPipelineES: DTYPE {DTYPE} is not float32, float16 or bfloat16")
        self.timesteps = scm_timesteps(num_inference_steps, max_timesteps, intermediate_timesteps)
        self.num_inference_steps = int(num_inference_steps)
        super().__init__(model_name, device, DTYPE, sigma_data, arch=arch, vae_widths=vae_widths, vae_layers=vae_layers,
                         weight_seed=weight_seed, vae_chunk=vae_chunk, synthetic_weights=synthetic_weights,
                         text_encoder_path=text_encoder_path, encode_only=encode_only)

    def _draws(self, b: int, seed: int, h: int, w: int, image_seeds: Optional[Sequence[int]] = None):
        """(initial latents [b, C, h, w] fp32 x sigma_data, [one fp32 noise per step]) from one generator, in the
        pipeline's order.  image_seeds: image i has its own generator (its latents, then its step noises)."""
        C = self.transformer_config.in_channels

        def one(nb, sd):
            g = torch.Generator(device=self.device).manual_seed(int(sd))
            shape = (nb, C, h, w)
            lat = torch.randn(shape, device=self.device, dtype=torch.float32, generator=g) * self.sigma_data
            return lat, [torch.randn(shape, device=self.device, dtype=torch.float32, generator=g)
                         for _ in range(self.num_inference_steps)]
        if image_seeds is None:
            return one(b, seed)
        if len(image_seeds) != b:
            raise ValueError(f"image_seeds has {len(image_seeds)} entries for {b} images")
        parts = [one(1, s) for s in image_seeds]
        return (torch.cat([p[0] for p in parts]),
                [torch.cat([p[1][i] for p in parts]) for i in range(self.num_inference_steps)])

    def _step(self, x, eps, noise, sc: ScmStepScalars, round_dtype: int, members: int, last: bool):
        """(x_next, m_next, x0_out) of one sampler step, see _step_torch."""
        if not FUSE_SCM_STEP:
            return _step_torch(x, eps, noise, sc, round_dtype, members, last)
        from . import kernels as K
        new = lambda: torch.empty(eps.shape, dtype=torch.float32, device=eps.device)  # noqa: E731
        if last:
            z = new()
            K.scm_step(x, eps, None, sc, round_dtype, members, x0_out=z)
            return None, None, z
        x_next = x if x.numel() == eps.numel() else new()      # every member has its own x by now: in place
        m_next = new()
        K.scm_step(x, eps, noise, sc, round_dtype, members, x_next=x_next, m_next=m_next)
        return x_next, m_next, None

    @torch.no_grad()
    def _sample(self, draws, prompt_embeds, prompt_attention_mask, guidance_scale, reps: int,
                prompt_index: Optional[torch.Tensor] = None):
        """The sampler over reps members of b images: (images [reps * b, 3, H, W], final latents in VAE scale,
        an NCHW view).  prompt_index: as SanaOneStep._one_step."""
        lat, noises = draws
        b, C, h, w = lat.shape
        rd = _ROUND_DTYPES[self.DTYPE]
        tm = lambda t: t.permute(0, 2, 3, 1).reshape(b, h * w, C).contiguous()       # noqa: E731  token-major
        nchw = lambda t: t.view(-1, h, w, C).permute(0, 3, 1, 2)                     # noqa: E731  a view
        rep = lambda t: t if reps == 1 else t.repeat(reps, *([1] * (t.ndim - 1)))    # noqa: E731  member-major
        guidance = torch.full((b,), guidance_scale, device=self.device, dtype=self.DTYPE)
        guidance = rep((guidance * self.transformer_config.guidance_embeds_scale).float())
        enc_index = None
        if prompt_index is not None:
            u = prompt_embeds.shape[0]
            enc_index = (torch.arange(reps, device=self.device)[:, None] * u
                         + prompt_index.to(self.device)[None, :]).reshape(-1)
        pe, am = rep(prompt_embeds), rep(prompt_attention_mask)
        ts, steps = self.timesteps, self.num_inference_steps
        x = tm(lat)                                              # [b, hw, C]: shared by every member at step 0
        in_scale0 = float(torch.tensor(scm_step_scalars(ts[0], ts[1], self.sigma_data).in_scale, dtype=torch.float32))
        m = rep(_rnd(x * in_scale0, rd))
        z = None
        for i in range(steps):
            last = i == steps - 1
            sc = scm_step_scalars(ts[i], ts[i + 1], self.sigma_data,
                                  1.0 / (self.sigma_data * self.vae.scaling_factor) if last else 1.0)
            s = torch.full((b,), scm_s(ts[i]), device=self.device, dtype=torch.float32).to(self.DTYPE).float()
            eps = self.transformer(nchw(m), rep(s), pe, am, guidance, enc_index=enc_index)
            eps = eps.permute(0, 2, 3, 1).reshape(reps * b, h * w, C)   # proj_out's own layout: no copy
            if not eps.is_contiguous():
                eps = eps.contiguous()
            x, m, z = self._step(x, eps, None if last else tm(noises[i]), sc, rd, reps, last)
        zc = nchw(z)
        imgs = [self.vae(zc[s:s + self.vae_chunk]) for s in range(0, zc.shape[0], self.vae_chunk)]
        return torch.cat(imgs), zc

    # ---- reference API (single member: the transformer's own LoRA params) ------------
    @torch.no_grad()
    def generate_one_batch(self, prompt_embeds, prompt_attention_mask, seed: int = 0, guidance_scale: float = 1.0,
                           width_latent: int = 32, height_latent: int = 32, output_type: str = "pil",
                           image_seeds: Optional[Sequence[int]] = None):
        """models/SanaSprint.py:458-502: every prompt of the batch in one sampler run; (images, None).
        image_seeds (build-specific): one generator per image instead of one batched draw from `seed`."""
        set_population(self.transformer, None)
        draws = self._draws(prompt_embeds.shape[0], seed, height_latent, width_latent, image_seeds)
        imgs, _ = self._sample(draws, prompt_embeds.to(self.device), prompt_attention_mask.to(self.device),
                               guidance_scale, reps=1)
        return (imgs if output_type == "pt" else to_pil(imgs)), None

    @torch.no_grad()
    def generate(self, prompt_embeds, prompt_attention_mask, latents=None, seed: int = 0, guidance_scale: float = 1.0,
                 width_latent: int = 32, height_latent: int = 32, output_type: str = "pil"):
        """models/SanaSprint.py:431-453: a thin wrapper of generate_one_batch (`latents` is ignored, as there)."""
        return self.generate_one_batch(prompt_embeds, prompt_attention_mask, seed=seed, guidance_scale=guidance_scale,
                                       width_latent=width_latent, height_latent=height_latent, output_type=output_type)

    # ---- engine API -----------------------------------------------------------------
    @torch.no_grad()
    def generate_population(self, prompt_embeds, prompt_attention_mask, theta_pop: torch.Tensor, seed: int,
                            guidance_scale: float, width_latent: int, height_latent: int,
                            prompt_index: Optional[torch.Tensor] = None,
                            flat_seeds: Optional[Sequence[int]] = None) -> torch.Tensor:
        """SanaOneStep.generate_population's contract: all members of theta_pop [n, D] at once, VAE images
        [n*b, 3, H, W] (member-major); every step's forward uses prompt_index.  flat_seeds: [b] per-image seeds,
        image i draws its latents and step noises from its own Generator(flat_seeds[i]) (_draws' image_seeds)."""
        n = theta_pop.shape[0]
        self.ctx.theta_pop, self.ctx.n_members = theta_pop, n
        set_population(self.transformer, self.ctx)
        try:
            b = prompt_embeds.shape[0] if prompt_index is None else prompt_index.numel()
            seeds = None if flat_seeds is None else [int(s) for s in flat_seeds]
            imgs, _ = self._sample(self._draws(b, seed, height_latent, width_latent, seeds), prompt_embeds,
                                   prompt_attention_mask, guidance_scale, reps=n, prompt_index=prompt_index)
        finally:
            set_population(self.transformer, None)
            self.ctx.theta_pop = None
        return imgs


def to_pil(images: torch.Tensor) -> List[Any]:
    """PixArtImageProcessor.postprocess(output_type='pil')."""
    from PIL import Image
    arr = torch.round((images.float() / 2 + 0.5).clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
    return [Image.fromarray(a) for a in arr]
