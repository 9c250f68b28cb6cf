"""Evaluation on a prompt table (PartiPrompts): generate one image per prompt and candidate, score every
image with the reward models, report per Category and per Challenge.

The reference does this with two scripts: evaluate/run_benchmark.py (one image per prompt, from the base model
or a LoRA adapter directory, saved as <idx:04d>_<slug>.png) and evaluate/evalute_folder.py (a folder of such
images scored against the TSV; the text of benchmark_results/*).  Their conventions are restated here:

  * the TSV has a header row; its Prompt / Category / Challenge columns are found case-insensitively; row order
    is the prompt index;
  * file names are f"{idx:04d}_{slugify(prompt)}.png"; the index is read back from the digits before the first
    underscore;
  * the combined score mixes (aesthetic, text, no_artifacts, pickscore) with (0.3, 0.3, 0.2, 0.2), the
    evaluation script's default, not the training default;
  * the report averages one entry per prompt index, accumulated in Python floats in ascending index order.

On the population engine the base model and K checkpoints are K + 1 rows of theta_pop: `generate_and_score`
generates all candidates in one population-batched forward per pass, on the same prompts and the same per-image
seeds (common random numbers), and scores them in the same reward batches.  The reward models see exactly the
bytes a PNG would hold (kernels.images_to_u8 -> RewardModels.score_u8), so scoring in memory and scoring the
written folder (`evaluate_folder`) give the same numbers.

    python -m hyperscalees_t2i_amd.evaluate generate --encoded_path parti.pt --candidate base \\
        --candidate run1=es_runs/latest_lora --out_root eval_out --tsv_path PartiPrompts.tsv ...
    python -m hyperscalees_t2i_amd.evaluate score --images_dir eval_out/base --tsv_path PartiPrompts.tsv ...

PARITY WITH THE PUBLISHED NUMBERS IS UNPINNED: neither a PartiPrompts file nor the real weights are available
to the tests; what is pinned is the table / file-name / aggregation / report-text contract (tests/test_evaluate.py,
against values recorded from the reference's own functions) and the device path (tests/test_gpu_evaluate.py).
"""
from __future__ import annotations

import argparse
import csv
import inspect
import json
import re
import sys
import warnings
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch

REWARD_KEYS = ("clip_aesthetic", "clip_text", "no_artifacts", "pickscore", "combined")
DEFAULT_MIX_WEIGHTS = (0.3, 0.3, 0.2, 0.2)   # evalute_folder.py:60 (aesthetic, text, no_artifacts, pickscore)
IMAGE_SUFFIXES = {".png", ".jpg", ".jpeg"}
PNG_WORKERS = 8        # PNG encoding threads: fixed, never sized from the host's CPU count
TEXT_BATCH = 64        # prompts per text-tower batch


# ---------------------------------------------------------------------------------------
# prompt table and file names
# ---------------------------------------------------------------------------------------

@dataclass
class PromptTable:
    """The rows of a prompt TSV; row i is prompt index i."""
    prompts: List[str]
    categories: List[str]
    challenges: List[str]
    columns: Tuple[str, str, str]      # the header names the three columns were found under

    def __len__(self) -> int:
        return len(self.prompts)


def _find_column(fieldnames: Sequence[str], target: str) -> str:
    for name in fieldnames:
        if name.lower() == target.lower():
            return name
    raise ValueError(f"Could not find column '{target}' (case-insensitive) in TSV header: {list(fieldnames)}")


def read_prompt_table(tsv_path) -> PromptTable:
    """evalute_folder.py:198-212: a tab-separated file with a header row; ValueError on a missing column."""
    with Path(tsv_path).open("r", encoding="utf-8", newline="") as f:
        reader = csv.DictReader(f, delimiter="\t")
        if reader.fieldnames is None:
            raise ValueError("TSV file appears to have no header / fieldnames.")
        cols = tuple(_find_column(reader.fieldnames, t) for t in ("prompt", "category", "challenge"))
        rows = list(reader)
    return PromptTable([r[cols[0]] for r in rows], [r[cols[1]] for r in rows], [r[cols[2]] for r in rows], cols)


def slugify(text: str, max_len: int = 80) -> str:
    """run_benchmark.py:46-58: lower-case, runs of non-word characters -> one underscore, underscores stripped at
    both ends, cut to max_len (then trailing underscores stripped again), "prompt" if nothing is left."""
    text = re.sub(r"[^\w]+", "_", text.strip().lower()).strip("_")
    if len(text) > max_len:
        text = text[:max_len].rstrip("_")
    return text or "prompt"


def image_filename(idx: int, prompt: str) -> str:
    return f"{idx:04d}_{slugify(prompt)}.png"


def parse_index_from_filename(name: str) -> int:
    """evalute_folder.py:75-88: the digits before the first underscore; ValueError without them."""
    m = re.match(r"^(\d+)_", name)
    if not m:
        raise ValueError(f"Filename does not start with an index + underscore: {name}")
    return int(m.group(1))


# ---------------------------------------------------------------------------------------
# report
# ---------------------------------------------------------------------------------------

@dataclass
class GroupStats:
    """evalute_folder.py update_stats: a count and the running Python-float sum of each reward key."""
    count: int = 0
    sums: Dict[str, float] = field(default_factory=lambda: {k: 0.0 for k in REWARD_KEYS})

    def add(self, metrics: Dict[str, float]) -> None:
        self.count += 1
        for k in REWARD_KEYS:
            self.sums[k] += metrics[k]

    def means(self) -> Dict[str, float]:
        return {k: self.sums[k] / self.count for k in REWARD_KEYS}

    @classmethod
    def from_means(cls, count: int, means: Dict[str, float]) -> "GroupStats":
        return cls(int(count), {k: float(means[k]) * int(count) for k in REWARD_KEYS})


_GROUP_LINE = re.compile(r"^- (.*) \(n=\s*(\d+)\): aesthetic=(\S+), text=(\S+), no_artifacts=(\S+), pickscore=(\S+), "
                         r"combined=(\S+)$")
_OVERALL_NAMES = ("aesthetic_mean", "text_mean", "no_artifacts_mean", "pickscore_mean", "combined_mean")


@dataclass
class EvalReport:
    """Overall, per-category and per-challenge counts and means of the five reward keys."""
    overall: GroupStats = field(default_factory=GroupStats)
    by_category: Dict[str, GroupStats] = field(default_factory=dict)
    by_challenge: Dict[str, GroupStats] = field(default_factory=dict)
    mix_weights: Tuple[float, ...] = DEFAULT_MIX_WEIGHTS

    def add(self, category: Optional[str], challenge: Optional[str], metrics: Dict[str, float]) -> None:
        """One entry (one prompt index): evalute_folder.py:315-325."""
        self.overall.add(metrics)
        if category is not None:
            self.by_category.setdefault(category, GroupStats()).add(metrics)
        if challenge is not None:
            self.by_challenge.setdefault(challenge, GroupStats()).add(metrics)

    @classmethod
    def from_entries(cls, entries: Dict[int, Dict[str, float]], table: Optional[PromptTable] = None,
                     mix_weights: Sequence[float] = DEFAULT_MIX_WEIGHTS) -> "EvalReport":
        """entries: prompt index -> its five rewards (Python floats), added in ascending index order."""
        rep = cls(mix_weights=tuple(mix_weights))
        for idx in sorted(entries):
            rep.add(None if table is None else table.categories[idx], None if table is None else table.challenges[idx],
                    entries[idx])
        return rep

    @staticmethod
    def format_group(title: str, groups: Dict[str, GroupStats]) -> str:
        """print_group_stats' lines (without its leading blank line): groups sorted by key."""
        lines = [f"=== {title} ==="]
        for key in sorted(groups):
            st = groups[key]
            if st.count == 0:
                continue
            m = st.means()
            lines.append(f"- {key} (n={st.count:4d}): aesthetic={m['clip_aesthetic']:.4f}, text={m['clip_text']:.4f}, "
                         f"no_artifacts={m['no_artifacts']:.4f}, pickscore={m['pickscore']:.4f}, "
                         f"combined={m['combined']:.4f}")
        return "\n".join(lines)

    def format(self) -> str:
        """The report text of evalute_folder.py:344-356 in the layout of benchmark_results/* (no leading or
        trailing newline)."""
        if self.overall.count == 0:
            return "No valid images were evaluated. Nothing to report."
        m = self.overall.means()
        head = ["=== OVERALL ===", f"Total images evaluated: {self.overall.count}",
                f"  aesthetic_mean   = {m['clip_aesthetic']:.4f}", f"  text_mean        = {m['clip_text']:.4f}",
                f"  no_artifacts_mean= {m['no_artifacts']:.4f}", f"  pickscore_mean   = {m['pickscore']:.4f}",
                f"  combined_mean    = {m['combined']:.4f}"]
        return "\n\n".join(["\n".join(head), self.format_group("Per Category", self.by_category),
                            self.format_group("Per Challenge", self.by_challenge)])

    @classmethod
    def parse(cls, text: str) -> "EvalReport":
        """A report text (format(), benchmark_results/*) back into counts and means; the sums are mean * count."""
        rep, target = cls(), None
        overall: Dict[str, float] = {}
        count = 0
        for ln in text.splitlines():
            if ln.startswith("=== "):
                target = {"=== Per Category ===": rep.by_category, "=== Per Challenge ===": rep.by_challenge}.get(ln)
            elif ln.startswith("Total images evaluated:"):
                count = int(ln.split(":")[1])
            elif target is None and "=" in ln:
                name, val = ln.split("=")
                overall[name.strip()] = float(val)
            elif target is not None and ln.startswith("- "):
                g = _GROUP_LINE.match(ln)
                if not g:
                    raise ValueError(f"not a report group line: {ln!r}")
                target[g.group(1)] = GroupStats.from_means(int(g.group(2)),
                                                           dict(zip(REWARD_KEYS, map(float, g.groups()[2:]))))
        if count:
            rep.overall = GroupStats.from_means(count, {k: overall[n] for k, n in zip(REWARD_KEYS, _OVERALL_NAMES)})
        return rep

    def to_json(self) -> Dict[str, Any]:
        g = lambda st: {"count": st.count, **{f"{k}_mean": v for k, v in st.means().items()}} if st.count else \
            {"count": 0}                                                                         # noqa: E731
        return {"mix_weights": list(self.mix_weights), "overall": g(self.overall),
                "by_category": {k: g(self.by_category[k]) for k in sorted(self.by_category)},
                "by_challenge": {k: g(self.by_challenge[k]) for k in sorted(self.by_challenge)}}


# ---------------------------------------------------------------------------------------
# candidates
# ---------------------------------------------------------------------------------------

def _named_lora_params(backend) -> List[Tuple[str, torch.nn.Parameter]]:
    """(name, parameter) of the backend's theta, in collect_lora_params order."""
    params, _ = backend.collect_lora_params()
    names = {}
    for attr in ("transformer", "vae"):
        mod = getattr(backend.es_model, attr, None)
        if isinstance(mod, torch.nn.Module):
            names.update({id(p): f"{attr}.{n}" for n, p in mod.named_parameters()})
    return [(names[id(p)], p) for p in params]


def lora_b_mask(backend) -> torch.Tensor:
    """bool [D]: True inside the lora_B segments of the backend's theta."""
    return torch.cat([torch.full((p.numel(),), ".lora_B." in n, dtype=torch.bool) for n, p in _named_lora_params(backend)])


def _split_spec(spec: str) -> Tuple[str, str]:
    """"name=path" -> (name, path); a bare path is named after its directory (an adapter directory's own name, a
    meta file's parent directory)."""
    if "=" in spec and not Path(spec).exists():
        name, path = spec.split("=", 1)
        return name, path
    p = Path(spec)
    return (p.name if p.is_dir() or not p.parent.name else p.parent.name), spec


def load_candidates(backend, specs: Sequence[str]) -> Tuple[List[str], torch.Tensor]:
    """specs -> (names, theta_pop [n, D] fp32 on the backend's device).  A spec is "base" (the backend's theta
    with every lora_B segment zero: PEFT's untrained adapter, the LoRA term is exactly 0), an adapter directory
    (read through the backend's load_lora) or a latest_lora_meta.pt (load_latest_checkpoint); "name=path" names a
    candidate, otherwise the directory's / file's name does.  The backend's own LoRA parameters are left as they
    were.  FileNotFoundError on a missing path, ValueError on a theta of the wrong length."""
    from .es import flatten_params, unflatten_to_params
    from .es_step import load_latest_checkpoint
    params, shapes = backend.collect_lora_params()
    theta0 = flatten_params(params).detach().clone()
    names: List[str] = []
    rows: List[torch.Tensor] = []
    for spec in specs:
        spec = str(spec)
        if spec == "base":
            name, theta = "base", theta0.clone()
            theta[lora_b_mask(backend).to(theta.device)] = 0
        else:
            name, path = _split_spec(spec)
            p = Path(path)
            if not p.exists():
                raise FileNotFoundError(f"candidate {spec!r}: {p} does not exist")
            if p.is_dir():
                try:
                    backend.load_lora(p)
                    theta = flatten_params(params).detach().clone()
                finally:
                    unflatten_to_params(theta0, params, shapes)
            else:
                theta, _ = load_latest_checkpoint(p)
                if theta.numel() != theta0.numel():
                    raise ValueError(f"candidate {spec!r}: theta has {theta.numel()} elements, the backend's "
                                     f"{theta0.numel()}")
                theta = theta.to(theta0.device, theta0.dtype)
        base_name, k = name, 1
        while name in names:
            name, k = f"{base_name}_{k}", k + 1
        names.append(name)
        rows.append(theta.float())
    return names, torch.stack(rows).to(backend.device)


# ---------------------------------------------------------------------------------------
# generate and score
# ---------------------------------------------------------------------------------------

@dataclass
class EvalResult:
    """Per candidate and prompt: rewards[key] fp32 [n_candidates, n_prompts] (CPU), in the order of names /
    prompt_ids.  images: uint8 [n_candidates, n_prompts, H, W, 3] (CPU) with keep_images."""
    names: List[str]
    prompt_ids: List[int]
    prompts: List[str]
    rewards: Dict[str, torch.Tensor]
    mix_weights: Tuple[float, ...] = DEFAULT_MIX_WEIGHTS
    out_dirs: Optional[Dict[str, Path]] = None
    images: Optional[torch.Tensor] = None

    def entries(self, name: str) -> Dict[int, Dict[str, float]]:
        """prompt index -> the five rewards of candidate `name`, as Python floats."""
        c = self.names.index(name)
        return {pid: {k: float(self.rewards[k][c, j]) for k in REWARD_KEYS} for j, pid in enumerate(self.prompt_ids)}

    def report(self, name: str, table: Optional[PromptTable] = None) -> EvalReport:
        return EvalReport.from_entries(self.entries(name), table, self.mix_weights)


def compare(result: EvalResult, a: str, b: str) -> Dict[str, Dict[str, float]]:
    """Paired statistics of candidates a and b (same prompts, same seeds): per reward key the mean of b - a over
    the prompts and the share of prompts where b beats a."""
    ia, ib = result.names.index(a), result.names.index(b)
    out = {}
    for k in REWARD_KEYS:
        d = result.rewards[k][ib].double() - result.rewards[k][ia].double()
        out[k] = {"mean_diff": float(d.mean()) if d.numel() else 0.0,
                  "win_rate": float((d > 0).double().mean()) if d.numel() else 0.0}
    return out


def _text_features(rewards, texts: Sequence[str]) -> Dict[str, torch.Tensor]:
    """prompt_features of all texts, computed TEXT_BATCH prompts at a time (row i: texts[i])."""
    parts = [rewards.prompt_features(list(texts[s:s + TEXT_BATCH])) for s in range(0, len(texts), TEXT_BATCH)]
    return {"clip_aes": parts[0]["clip_aes"], "clip_neg": parts[0]["clip_neg"],
            "clip_prompt": torch.cat([p["clip_prompt"] for p in parts]),
            "pick_prompt": torch.cat([p["pick_prompt"] for p in parts])}


class _MixWeights:
    """rewards.mix_weights set for the length of an evaluation, then put back."""

    def __init__(self, rewards, mix_weights):
        from .rewards import split_mix_weights
        split_mix_weights(mix_weights)
        self.rewards, self.new = rewards, tuple(float(w) for w in mix_weights)

    def __enter__(self):
        self.old, self.rewards.mix_weights = self.rewards.mix_weights, self.new

    def __exit__(self, *exc):
        self.rewards.mix_weights = self.old


def _save_png(arr, path: Path) -> None:
    from PIL import Image
    Image.fromarray(arr).save(path)


@torch.no_grad()
def generate_and_score(backend, rewards, candidates: Tuple[Sequence[str], torch.Tensor],
                       prompt_ids: Optional[Sequence[int]] = None, max_prompts: Optional[int] = None,
                       prompts_per_pass: int = 8, seed_mode: str = "index", reference_batch_size: Optional[int] = None,
                       out_root=None, keep_images: bool = False, guidance_scale: Optional[float] = None,
                       mix_weights: Sequence[float] = DEFAULT_MIX_WEIGHTS) -> EvalResult:
    """candidates: (names, theta_pop [n, D]) of load_candidates.  Prompts are rows of the backend's encoded prompt
    file (backend.prompt_data; the reward texts are its "prompts" list): prompt_ids, default all, cut to
    max_prompts.  Per pass one generate_population over members_per_pass() candidates x prompts_per_pass prompts,
    converted by images_to_u8(imgs, backend.image_pil_mode) and scored by score_u8.
    seed_mode "index": the image of prompt i has the latents of a one-image draw from Generator(seed=i)
    (run_benchmark.py's --batch_size 1 default), however many prompts share a pass.  "batch": the reference's
    batched draw at --batch_size reference_batch_size: prompts [s, s + b) come from one b-image draw with
    seed = s (passes are then b prompts wide, and the prompts are the first max_prompts rows).
    out_root: writes out_root/<candidate>/<idx:04d>_<slug>.png from the scored bytes."""
    from . import kernels as K
    names, theta_pop = list(candidates[0]), candidates[1]
    if theta_pop.ndim != 2 or theta_pop.shape[0] != len(names):
        raise ValueError(f"candidates: {len(names)} names for theta_pop {tuple(theta_pop.shape)}")
    data = getattr(backend, "prompt_data", None)
    if not data or not data.get("prompts"):
        raise ValueError("generate_and_score: the backend has no encoded prompt file with a 'prompts' list")
    texts_all = list(data["prompts"])
    if seed_mode == "index":
        if "flat_seeds" not in inspect.signature(backend.generate_population).parameters:
            raise NotImplementedError(f"{type(backend).__name__}.generate_population takes no per-image seeds "
                                      f"(flat_seeds): seed_mode='index' is not available for this backend")
        width = max(int(prompts_per_pass), 1)
    elif seed_mode == "batch":
        if not reference_batch_size or int(reference_batch_size) < 1:
            raise ValueError("seed_mode='batch' needs reference_batch_size >= 1")
        if prompt_ids is not None:
            raise ValueError("seed_mode='batch' evaluates the first max_prompts rows (the seed of a draw is its "
                             "first row): prompt_ids must be None")
        width = int(reference_batch_size)
    else:
        raise ValueError(f"seed_mode must be 'index' or 'batch', got {seed_mode!r}")
    ids = list(range(len(texts_all))) if prompt_ids is None else [int(i) for i in prompt_ids]
    if max_prompts is not None:
        ids = ids[:max(int(max_prompts), 0)]
    if any(i < 0 or i >= len(texts_all) for i in ids):
        raise ValueError(f"prompt_ids outside the {len(texts_all)} encoded prompts")
    texts = [texts_all[i] for i in ids]
    n, P = len(names), len(ids)
    dev = theta_pop.device
    gs = float(backend.cfg.guidance_scale if guidance_scale is None else guidance_scale)
    per = backend.members_per_pass() or n
    pil_mode = int(getattr(backend, "image_pil_mode", 0))
    out = {k: torch.empty((n, P), dtype=torch.float32, device=dev) for k in REWARD_KEYS}
    kept: List[List[torch.Tensor]] = [[] for _ in range(n)]
    out_dirs = None
    if out_root is not None:
        out_dirs = {nm: Path(out_root) / nm for nm in names}
        for d in out_dirs.values():
            d.mkdir(parents=True, exist_ok=True)
    pending: list = []
    with _MixWeights(rewards, mix_weights), ThreadPoolExecutor(max_workers=PNG_WORKERS) as pool:
        feats = _text_features(rewards, texts) if P else None
        for s in range(0, P, width):
            chunk = ids[s:s + width]
            b = len(chunk)
            seeds = chunk if seed_mode == "index" else None
            for c0 in range(0, n, per):
                c1 = min(n, c0 + per)
                if seeds is None:
                    imgs = backend.generate_population(chunk, chunk[0], gs, theta_pop[c0:c1])
                else:
                    imgs = backend.generate_population(chunk, chunk[0], gs, theta_pop[c0:c1], flat_seeds=seeds)
                u8 = K.images_to_u8(imgs, pil_mode)                                   # [(c1 - c0) * b, H, W, 3]
                del imgs
                j = torch.arange(s, s + b, device=dev).repeat(c1 - c0)
                rew = rewards.score_u8(u8, j, feats)
                for k in REWARD_KEYS:
                    out[k][c0:c1, s:s + b] = rew[k].view(c1 - c0, b)
                if out_root is not None or keep_images:
                    host = u8.cpu().view(c1 - c0, b, *u8.shape[1:])                   # one device-to-host copy
                    if keep_images:
                        for c in range(c0, c1):
                            kept[c].append(host[c - c0])
                    if out_root is not None:
                        for f in pending:      # the previous pass's files: at most two passes of bytes in flight
                            f.result()
                        arr = host.numpy()
                        pending = [pool.submit(_save_png, arr[c - c0, q],
                                               out_dirs[names[c]] / image_filename(pid, texts_all[pid]))
                                   for c in range(c0, c1) for q, pid in enumerate(chunk)]
        for f in pending:
            f.result()
    images = torch.stack([torch.cat(k) for k in kept]) if keep_images and P else None
    return EvalResult(names, ids, texts, {k: v.cpu() for k, v in out.items()}, tuple(mix_weights), out_dirs, images)


# ---------------------------------------------------------------------------------------
# score a folder
# ---------------------------------------------------------------------------------------

def scan_images_dir(images_dir, num_rows: int) -> Dict[int, List[Path]]:
    """evalute_folder.py:223-241, 273-275: the .png / .jpg / .jpeg files (suffix case-insensitive) in sorted order,
    by prompt index; files without an index prefix and indices outside the table are skipped with a warning."""
    paths = sorted(p for p in Path(images_dir).iterdir() if p.suffix.lower() in IMAGE_SUFFIXES)
    by_idx: Dict[int, List[Path]] = {}
    for p in paths:
        try:
            by_idx.setdefault(parse_index_from_filename(p.name), []).append(p)
        except ValueError:
            warnings.warn(f"Skipping file without index prefix: {p.name}")
    for idx in sorted(by_idx):
        if idx < 0 or idx >= num_rows:
            warnings.warn(f"Image index {idx} exceeds TSV rows ({num_rows}), skipping.")
            del by_idx[idx]
    return by_idx


@torch.no_grad()
def score_folder(images_dir, table: PromptTable, rewards, image_batch: int = 64,
                 mix_weights: Sequence[float] = DEFAULT_MIX_WEIGHTS) -> Dict[int, Dict[str, float]]:
    """prompt index -> the five rewards (Python floats) of the folder's images of that index, averaged: images are
    decoded with PIL convert("RGB"), grouped by (H, W), uploaded as uint8 and scored by score_u8 with the row's
    prompt.  Unreadable files are skipped with a warning, and so is an index none of whose files could be read."""
    import numpy as np
    from PIL import Image
    by_idx = scan_images_dir(images_dir, len(table))
    dev = next(rewards.clip.parameters()).device
    decoded: Dict[Tuple[int, int], List[Tuple[int, Any]]] = {}
    for idx in sorted(by_idx):
        got = 0
        for p in by_idx[idx]:
            try:
                with Image.open(p) as im:
                    arr = np.asarray(im.convert("RGB"))
            except Exception as e:  # noqa: BLE001  (the reference skips whatever PIL cannot open)
                warnings.warn(f"Failed to open image {p}: {e}")
                continue
            decoded.setdefault(arr.shape[:2], []).append((idx, arr))
            got += 1
        if not got:
            warnings.warn(f"No valid images for index {idx}, skipping.")
    valid = sorted({idx for items in decoded.values() for idx, _ in items})
    if not valid:
        return {}
    row = {idx: j for j, idx in enumerate(valid)}
    per_image: Dict[int, List[torch.Tensor]] = {idx: [] for idx in valid}
    with _MixWeights(rewards, mix_weights):
        feats = _text_features(rewards, [table.prompts[i] for i in valid])
        for items in decoded.values():
            for s in range(0, len(items), max(int(image_batch), 1)):
                part = items[s:s + max(int(image_batch), 1)]
                u8 = torch.from_numpy(np.stack([a for _, a in part])).to(dev)
                rew = rewards.score_u8(u8, torch.tensor([row[i] for i, _ in part], device=dev), feats)
                vals = torch.stack([rew[k] for k in REWARD_KEYS], dim=1).cpu()          # [images, 5]
                for (idx, _), v in zip(part, vals):
                    per_image[idx].append(v)
    return {idx: dict(zip(REWARD_KEYS, (float(x) for x in torch.stack(per_image[idx]).mean(dim=0)))) for idx in valid}


def evaluate_folder(images_dir, tsv_path, rewards, image_batch: int = 64,
                    mix_weights: Sequence[float] = DEFAULT_MIX_WEIGHTS) -> EvalReport:
    """evalute_folder.py on the device: the report of a folder of <idx>_*.png / .jpg / .jpeg images against the
    TSV (see score_folder for what is scored and skipped)."""
    table = read_prompt_table(tsv_path)
    return EvalReport.from_entries(score_folder(images_dir, table, rewards, image_batch, mix_weights), table, mix_weights)


def encode_prompt_table(es_model, tsv_path, encoded_save_path, batch_size: int = 4) -> dict:
    """The Prompt column of the TSV, encoded in row order by the model's native prompt encoder into the encoded
    prompt file the backends read (row i = prompt index i).  Not through a prompts .txt: its loader drops blank
    and # lines, which would shift every later index."""
    return es_model.encode_prompt_list(read_prompt_table(tsv_path).prompts, encoded_save_path, batch_size=batch_size)


# ---------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------

def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m hyperscalees_t2i_amd.evaluate", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)

    def common(p):
        p.add_argument("--tsv_path", type=str, default=None, help="prompt TSV (Prompt / Category / Challenge)")
        p.add_argument("--mix_aes", type=float, default=DEFAULT_MIX_WEIGHTS[0])
        p.add_argument("--mix_txt", type=float, default=DEFAULT_MIX_WEIGHTS[1])
        p.add_argument("--mix_noart", type=float, default=DEFAULT_MIX_WEIGHTS[2])
        p.add_argument("--mix_pick", type=float, default=DEFAULT_MIX_WEIGHTS[3])
        p.add_argument("--clip_path", type=str, default=None, help="local openai/clip-vit-base-patch32 directory")
        p.add_argument("--pickscore_path", type=str, default=None, help="local yuvalkirstain/PickScore_v1 directory")
        p.add_argument("--synthetic_rewards", action="store_true", help="seeded random reward towers (no weights)")
        p.add_argument("--device", type=str, default="cuda:0")
        p.add_argument("--json", type=str, default=None, help="also write the report(s) as JSON to this file")

    g = sub.add_parser("generate", help="generate one image per prompt and candidate, and score them")
    common(g)
    g.add_argument("--model_name", type=str, default="Efficient-Large-Model/Sana_Sprint_1.6B_1024px_diffusers")
    g.add_argument("--backend_mode", choices=["one_step", "pipeline"], default="one_step")
    g.add_argument("--synthetic_weights", action="store_true")
    g.add_argument("--encoded_path", type=str, required=True, help="encoded prompt file (encode_prompt_table)")
    g.add_argument("--candidate", action="append", default=None,
                   help="'base', an adapter directory, a latest_lora_meta.pt, or name=path; repeatable (default base)")
    g.add_argument("--out_root", type=str, default=None, help="write <out_root>/<candidate>/<idx>_<slug>.png")
    g.add_argument("--guidance_scale", type=float, default=4.5)
    g.add_argument("--width_latent", type=int, default=32)
    g.add_argument("--height_latent", type=int, default=32)
    g.add_argument("--max_prompts", type=int, default=None)
    g.add_argument("--prompts_per_pass", type=int, default=8)
    g.add_argument("--seed_mode", choices=["index", "batch"], default="index")
    g.add_argument("--reference_batch_size", type=int, default=None)
    g.add_argument("--lora_r", type=int, default=2)
    g.add_argument("--lora_alpha", type=int, default=8)

    s = sub.add_parser("score", help="score a folder of <idx>_<slug> images against the TSV")
    common(s)
    s.add_argument("--images_dir", type=str, required=True)
    s.add_argument("--image_batch", type=int, default=64)
    return ap


def _rewards_from_args(a):
    from .rewards import RewardModels
    return RewardModels.build(a.device, clip_path=a.clip_path, pickscore_path=a.pickscore_path,
                              synthetic=a.synthetic_rewards)


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = build_parser().parse_args(argv)
    mix = (a.mix_aes, a.mix_txt, a.mix_noart, a.mix_pick)
    if a.command == "score":
        if not a.tsv_path:
            raise SystemExit("score: --tsv_path is required")
        reports = {Path(a.images_dir).name: evaluate_folder(a.images_dir, a.tsv_path, _rewards_from_args(a),
                                                            a.image_batch, mix)}
    else:
        from .backend import SanaBackend, SanaConfig
        cfg = SanaConfig(model_name=a.model_name, backend_mode=a.backend_mode, encoded_prompt_path=a.encoded_path,
                         guidance_scale=a.guidance_scale, width_latent=a.width_latent, height_latent=a.height_latent,
                         lora_r=a.lora_r, lora_alpha=a.lora_alpha, synthetic_weights=a.synthetic_weights)
        backend = SanaBackend(a.device, cfg)
        backend.init_and_attach_lora()
        cands = load_candidates(backend, a.candidate or ["base"])
        res = generate_and_score(backend, _rewards_from_args(a), cands, max_prompts=a.max_prompts,
                                 prompts_per_pass=a.prompts_per_pass, seed_mode=a.seed_mode,
                                 reference_batch_size=a.reference_batch_size, out_root=a.out_root, mix_weights=mix)
        table = read_prompt_table(a.tsv_path) if a.tsv_path else None
        reports = {nm: res.report(nm, table) for nm in res.names}
        for nm in res.names[1:]:
            print(f"[compare] {res.names[0]} -> {nm}: {json.dumps(compare(res, res.names[0], nm))}")
    for nm, rep in reports.items():
        print(f"\n##### {nm}\n{rep.format()}")
    if a.json:
        Path(a.json).write_text(json.dumps({nm: rep.to_json() for nm, rep in reports.items()}, indent=2))
    return 0


if __name__ == "__main__":
    sys.exit(main())
