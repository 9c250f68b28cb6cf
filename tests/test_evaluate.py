"""hyperscalees_t2i_amd.evaluate without a GPU: the prompt table, file names, aggregation and report text against
values recorded from the reference's own evaluate/evalute_folder.py (tests/golden/eval_golden.json, written by
tests/golden/make_golden_eval.py), the report layout against one of the reference's recorded result files
(tests/golden/eval_base_onestep.txt = benchmark_results/base_onestep), candidates on a tiny CPU backend, the
folder scan rules and the command line.

UNPINNED: slugify.  The reference's lives in evaluate/run_benchmark.py, which imports peft and cannot be imported
where the fixtures are generated; its cases below are written by hand from its source.
"""
import json
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

from hyperscalees_t2i_amd import evaluate as EV
from hyperscalees_t2i_amd.backend import SanaBackend, SanaConfig
from hyperscalees_t2i_amd.es import flatten_params
from hyperscalees_t2i_amd.sana import SanaArch

GOLDEN = Path(__file__).resolve().parent / "golden"
G = json.loads((GOLDEN / "eval_golden.json").read_text())
TINY = SanaArch(num_attention_heads=4, attention_head_dim=32, num_layers=2, num_cross_attention_heads=2,
                cross_attention_head_dim=64, caption_channels=2304)


@pytest.fixture()
def tsv(tmp_path):
    p = tmp_path / "prompts.tsv"
    p.write_text(G["tsv"], encoding="utf-8")
    return p


# ---------------------------------------------------------------------------------------
# table, file names
# ---------------------------------------------------------------------------------------

def test_prompt_table_matches_reference(tsv, tmp_path):
    t = EV.read_prompt_table(tsv)
    assert t.columns == (G["columns"]["prompt"], G["columns"]["category"], G["columns"]["challenge"])
    assert len(t) == len(G["rows"])
    for i, r in enumerate(G["rows"]):                      # row order is the prompt index
        assert (t.prompts[i], t.categories[i], t.challenges[i]) == (r["prompt"], r["category"], r["challenge"])
    assert G["missing_column_raises"]
    bad = tmp_path / "bad.tsv"
    bad.write_text("Prompt\tCategory\nx\ty\n")
    with pytest.raises(ValueError, match="challenge"):
        EV.read_prompt_table(bad)


def test_parse_index_matches_reference():
    for case in G["filenames"]:
        if case["index"] is None:
            with pytest.raises(ValueError):
                EV.parse_index_from_filename(case["name"])
        else:
            assert EV.parse_index_from_filename(case["name"]) == case["index"]


def test_slugify_cases_unpinned():
    assert EV.slugify("Two cats,  on a -- sofa!") == "two_cats_on_a_sofa"           # punctuation runs -> one _
    assert EV.slugify("  ...Hello, World...  ") == "hello_world"                      # stripped at both ends
    assert EV.slugify("Über-Café in Zürich 東京") == "über_café_in_zürich_東京"         # Unicode word characters kept
    assert EV.slugify("snake_case stays") == "snake_case_stays"
    long = "a" * 79 + " " + "b" * 20
    assert EV.slugify(long) == "a" * 79                                               # cut to 80, then _ stripped
    assert EV.slugify("x" * 100) == "x" * 80 and EV.slugify("x" * 100, max_len=10) == "x" * 10
    assert EV.slugify("") == "prompt" and EV.slugify("?!  --") == "prompt"
    assert EV.image_filename(7, "A red fox.") == "0007_a_red_fox.png"
    assert EV.image_filename(12345, "") == "12345_prompt.png"
    assert EV.parse_index_from_filename(EV.image_filename(41, "__x")) == 41


# ---------------------------------------------------------------------------------------
# aggregation and report text
# ---------------------------------------------------------------------------------------

def _ref_stats(st):
    return st["count"], {k: st[f"sum_{k}"] for k in EV.REWARD_KEYS}


def test_aggregates_and_group_text_match_reference(tsv):
    table = EV.read_prompt_table(tsv)
    entries = {int(i): m for i, m in G["metrics"].items()}           # the JSON holds them out of index order
    assert list(entries) != sorted(entries)
    rep = EV.EvalReport.from_entries(entries, table)
    assert tuple(G["default_mix_weights"]) == EV.DEFAULT_MIX_WEIGHTS == rep.mix_weights
    assert (rep.overall.count, rep.overall.sums) == _ref_stats(G["overall"])          # float sums: exact equality
    for got, want in ((rep.by_category, G["by_category"]), (rep.by_challenge, G["by_challenge"])):
        assert set(got) == set(want)
        for k in want:
            assert (got[k].count, got[k].sums) == _ref_stats(want[k]), k
    # print_group_stats prints a blank line, the title and the sorted groups
    assert "\n" + EV.EvalReport.format_group("Per Category", rep.by_category) + "\n" == G["group_text"]["Per Category"]
    assert "\n" + EV.EvalReport.format_group("Per Challenge", rep.by_challenge) + "\n" == G["group_text"]["Per Challenge"]
    js = rep.to_json()
    assert js["overall"]["count"] == 6 and list(js["by_category"]) == sorted(G["by_category"])
    assert js["by_challenge"]["Basic"]["pickscore_mean"] == G["by_challenge"]["Basic"]["sum_pickscore"] / 3
    json.dumps(js)


def test_report_format_regenerates_recorded_result_file():
    text = (GOLDEN / "eval_base_onestep.txt").read_text(encoding="utf-8")
    rep = EV.EvalReport.parse(text)
    assert rep.overall.count == 1631 and len(rep.by_category) == 12 and len(rep.by_challenge) == 11
    assert rep.by_category["Food & Beverage"].count == 74
    assert abs(rep.by_challenge["Writing & Symbols"].means()["pickscore"] - 21.7716) < 1e-9
    assert rep.format() == text                                       # byte for byte (the file has no final newline)
    assert rep.format().encode("utf-8") == (GOLDEN / "eval_base_onestep.txt").read_bytes()


def test_empty_report():
    rep = EV.EvalReport.from_entries({})
    assert rep.overall.count == 0 and "Nothing to report" in rep.format() and rep.to_json()["overall"] == {"count": 0}


# ---------------------------------------------------------------------------------------
# candidates
# ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def backend_cpu():
    cfg = SanaConfig(synthetic_weights=True, width_latent=4, height_latent=4, arch=TINY,
                     vae_widths=(16, 32, 32, 64, 64, 64), vae_layers=(1, 1, 1, 1, 1, 1))
    be = SanaBackend("cpu", cfg)
    be.init_and_attach_lora()
    return be


def test_load_candidates(backend_cpu, tmp_path):
    from hyperscalees_t2i_amd.es_step import save_latest_checkpoint
    be = backend_cpu
    params, shapes = be.collect_lora_params()
    theta = flatten_params(params).clone()
    be.save_lora(tmp_path / "run_a")
    meta = tmp_path / "run_b" / "latest_lora_meta.pt"
    theta_b = theta * 0.5 + 0.25
    save_latest_checkpoint(theta=theta_b, backend=be, lora_params=params, lora_shapes=shapes, save_dir=meta.parent,
                           meta_path=meta, epoch=3, stats={}, extra_meta={})
    from hyperscalees_t2i_amd.es import unflatten_to_params
    unflatten_to_params(theta, params, shapes)                         # save_latest_checkpoint wrote theta_b into them

    names, pop = EV.load_candidates(be, ["base", str(tmp_path / "run_a"), str(meta), f"again={tmp_path / 'run_a'}"])
    assert names == ["base", "run_a", "run_b", "again"]
    assert pop.shape == (4, theta.numel()) and pop.dtype == torch.float32
    assert torch.equal(pop[1], theta) and torch.equal(pop[3], theta)   # save_lora -> the same theta
    assert torch.equal(pop[2], theta_b)
    assert torch.equal(flatten_params(params), theta)                  # the backend's own parameters are untouched
    mask = EV.lora_b_mask(be)
    assert mask.shape == theta.shape and 0 < int(mask.sum()) < mask.numel()
    assert torch.equal(pop[0][~mask], theta[~mask])                    # base differs only inside the lora_B segments
    assert bool((pop[0][mask] == 0).all()) and bool((theta[mask] != 0).any())
    # the mask is the lora_B parameters, in theta order
    named = [(n, p) for n, p in be.es_model.transformer.named_parameters() if p.requires_grad]
    want = torch.cat([torch.full((p.numel(),), "lora_B" in n) for n, p in named])
    assert torch.equal(mask, want)
    # the same name twice gets a suffix
    assert EV.load_candidates(be, ["base", "base"])[0] == ["base", "base_1"]

    with pytest.raises(FileNotFoundError):
        EV.load_candidates(be, [str(tmp_path / "missing")])
    short = tmp_path / "short" / "latest_lora_meta.pt"
    short.parent.mkdir()
    torch.save({"theta_latest": theta[:-3].clone(), "epoch": 0}, short)
    with pytest.raises(ValueError, match="elements"):
        EV.load_candidates(be, [str(short)])
    assert torch.equal(flatten_params(params), theta)


def test_generate_and_score_argument_errors(backend_cpu):
    be = backend_cpu
    cands = EV.load_candidates(be, ["base"])
    with pytest.raises(ValueError, match="seed_mode"):
        EV.generate_and_score(be, None, cands, seed_mode="other")
    with pytest.raises(ValueError, match="reference_batch_size"):
        EV.generate_and_score(be, None, cands, seed_mode="batch")
    with pytest.raises(ValueError, match="prompt_ids"):
        EV.generate_and_score(be, None, cands, seed_mode="batch", reference_batch_size=2, prompt_ids=[1])
    with pytest.raises(ValueError, match="names"):
        EV.generate_and_score(be, None, (["a", "b"], cands[1]))

    class NoSeeds:
        prompt_data = {"prompts": ["x"]}

        def generate_population(self, flat_ids, seed, guidance_scale, theta_pop):
            raise AssertionError("not reached")

    with pytest.raises(NotImplementedError, match="flat_seeds"):
        EV.generate_and_score(NoSeeds(), None, cands, seed_mode="index")


# ---------------------------------------------------------------------------------------
# folder rules (no reward model: the scan, and the aggregation of several images per index)
# ---------------------------------------------------------------------------------------

def test_scan_images_dir_rules(tmp_path):
    for name in ("0001_b.png", "0001_a.PNG", "0000_x.JpEg", "0003_y.jpg", "0002_z.gif", "notes.txt", "cover.png",
                 "0009_outside.png", "_0004_lead.png"):
        (tmp_path / name).write_bytes(b"")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = EV.scan_images_dir(tmp_path, num_rows=7)
    assert {k: [p.name for p in v] for k, v in got.items()} == {0: ["0000_x.JpEg"], 1: ["0001_a.PNG", "0001_b.png"],
                                                                3: ["0003_y.jpg"]}
    msgs = sorted(str(x.message) for x in w)
    assert len(msgs) == 3 and any("cover.png" in m for m in msgs) and any("_0004_lead.png" in m for m in msgs)
    assert any("index 9" in m for m in msgs)                          # other suffixes are not even looked at


class _FakeRewards:
    """score_u8 stand-in: every reward key is the image's mean byte (+ its prompt row), so the test sees which
    images were scored with which row without a reward model."""
    mix_weights = (0.0, 0.0, 0.0, 1.0)

    def __init__(self):
        self.clip = torch.nn.Linear(1, 1)
        self.seen_mix = None
        self.texts = None

    def prompt_features(self, texts):
        self.texts = list(texts) if self.texts is None else self.texts + list(texts)
        n = len(texts)
        return {"clip_aes": torch.zeros(1), "clip_neg": torch.zeros(1), "clip_prompt": torch.zeros(n, 1),
                "pick_prompt": torch.zeros(n, 1)}

    def score_u8(self, u8, prompt_index, feats):
        self.seen_mix = self.mix_weights
        assert u8.dtype == torch.uint8 and u8.ndim == 4 and u8.shape[3] == 3
        assert feats["clip_prompt"].shape[0] == len(self.texts)
        v = u8.float().mean(dim=(1, 2, 3)) + 1000.0 * prompt_index.float()
        return {k: v.clone() for k in EV.REWARD_KEYS}


def test_score_folder_counts_an_index_once_and_skips(tmp_path, tsv, monkeypatch):
    from PIL import Image
    monkeypatch.setattr(EV, "TEXT_BATCH", 2)                          # three prompts: two text batches
    d = tmp_path / "imgs"
    d.mkdir()
    flat = lambda v, h=8, w=8: Image.fromarray(np.full((h, w, 3), v, np.uint8))  # noqa: E731
    flat(10).save(d / "0001_a.png")
    flat(30).save(d / "0001_b.png")                                   # index 1 twice: averaged into one entry
    flat(50, 6, 10).save(d / "0004_other_size.png")                   # another (H, W) group
    Image.fromarray(np.full((8, 8), 70, np.uint8)).save(d / "0005_gray.png")      # convert("RGB")
    (d / "0002_broken.png").write_bytes(b"not a png")                 # unreadable: skipped, and so is its index
    (d / "0099_outside.png").write_bytes(b"")
    (d / "readme.png").write_bytes(b"")
    rw = _FakeRewards()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        rep = EV.evaluate_folder(d, tsv, rw, image_batch=2)
    msgs = [str(x.message) for x in w]
    assert any("0002_broken.png" in m for m in msgs) and any("No valid images for index 2" in m for m in msgs)
    assert any("index 99" in m for m in msgs) and any("readme.png" in m for m in msgs)
    table = EV.read_prompt_table(tsv)
    assert rw.texts == [table.prompts[i] for i in (1, 4, 5)]           # that row's prompt, in index order
    assert rw.seen_mix == EV.DEFAULT_MIX_WEIGHTS and rw.mix_weights == (0.0, 0.0, 0.0, 1.0)   # set, then put back
    assert rep.overall.count == 3                                      # indices 1, 4, 5: one entry each
    want = [(10.0 + 30.0) / 2 + 0.0, 50.0 + 1000.0, 70.0 + 2000.0]
    assert rep.overall.sums["pickscore"] == want[0] + want[1] + want[2]
    assert rep.by_category[table.categories[1]].count == 1 and rep.by_challenge[table.challenges[5]].count == 1
    assert EV.EvalReport.parse(rep.format()).overall.count == 3


def test_compare_is_paired():
    r = EV.EvalResult(["a", "b"], [0, 1, 2, 3], ["p"] * 4,
                      {k: torch.tensor([[1.0, 2.0, 3.0, 4.0], [2.0, 2.0, 2.0, 6.0]]) for k in EV.REWARD_KEYS})
    c = EV.compare(r, "a", "b")
    assert set(c) == set(EV.REWARD_KEYS) and c["pickscore"] == {"mean_diff": 0.5, "win_rate": 0.5}
    assert EV.compare(r, "a", "a")["combined"] == {"mean_diff": 0.0, "win_rate": 0.0}
    assert r.entries("b")[3]["clip_text"] == 6.0 and r.report("a").overall.count == 4


# ---------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------

def test_cli_parsing():
    ap = EV.build_parser()
    a = ap.parse_args(["generate", "--encoded_path", "p.pt", "--candidate", "base", "--candidate", "r1=runs/a",
                       "--out_root", "out", "--backend_mode", "pipeline", "--max_prompts", "5", "--seed_mode", "batch",
                       "--reference_batch_size", "4", "--mix_pick", "0.5"])
    assert a.command == "generate" and a.candidate == ["base", "r1=runs/a"] and a.backend_mode == "pipeline"
    assert (a.max_prompts, a.seed_mode, a.reference_batch_size, a.out_root) == (5, "batch", 4, "out")
    assert (a.mix_aes, a.mix_txt, a.mix_noart, a.mix_pick) == (0.3, 0.3, 0.2, 0.5)
    d = ap.parse_args(["generate", "--encoded_path", "p.pt"])
    assert d.candidate is None and d.seed_mode == "index" and d.prompts_per_pass == 8 and d.guidance_scale == 4.5
    assert (d.width_latent, d.height_latent) == (32, 32)
    s = ap.parse_args(["score", "--images_dir", "imgs", "--tsv_path", "t.tsv"])
    assert s.command == "score" and s.images_dir == "imgs" and s.image_batch == 64
    assert (s.mix_aes, s.mix_txt, s.mix_noart, s.mix_pick) == EV.DEFAULT_MIX_WEIGHTS
    for bad in (["generate"], ["score", "--tsv_path", "t.tsv"], [], ["generate", "--encoded_path", "p", "--seed_mode", "x"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
