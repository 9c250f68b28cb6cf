"""The multi-step Sana-Sprint sampler's host side (pipeline.SanaPipelineES), no GPU: the scheduler's timestep
rule, the step scalars against their fp64 closed forms, the trigflow identity on the torch form of the step,
the backend's mode switch and the two prompt loaders."""
import math

import pytest
import torch

from hyperscalees_t2i_amd import pipeline as P
from hyperscalees_t2i_amd.backend import SanaBackend, SanaConfig


def test_timestep_rule():
    assert P.scm_timesteps(2) == [1.57080, 1.3, 0.0]
    with pytest.raises(ValueError, match="num_inference_steps != 2"):
        P.scm_timesteps(3)
    with pytest.raises(ValueError):
        P.scm_timesteps(1)
    for steps in (1, 2, 3, 4):
        got = P.scm_timesteps(steps, intermediate_timesteps=None)
        want = torch.linspace(1.57080, 0.0, steps + 1, dtype=torch.float64)
        assert len(got) == steps + 1 and got[0] == 1.57080 and got[-1] == 0.0
        assert torch.allclose(torch.tensor(got, dtype=torch.float64), want, rtol=0, atol=1e-15)


@pytest.mark.parametrize("t,n", [(1.57080, 1.3), (1.3, 0.0), (0.7, 0.2)])
def test_step_scalars_match_closed_forms(t, n):
    sd = 0.5
    sc = P.scm_step_scalars(t, n, sd, out_scale=3.0)
    s = math.tan(t) / (1.0 + math.tan(t))                      # sin t / (cos t + sin t)
    sn = math.tan(n) / (1.0 + math.tan(n))
    q2 = 1.0 - 2.0 * s + 2.0 * s * s                           # s^2 + (1 - s)^2
    close = lambda a, b: abs(a - b) <= 1e-12 * max(1.0, abs(b))  # noqa: E731
    assert close(P.scm_s(t), s)
    assert close(sc.in_scale, math.sqrt(q2) / sd)
    assert close(sc.coef_m, (1.0 - 2.0 * s) * sd / math.sqrt(q2))
    assert close(sc.coef_eps, math.sqrt(q2) * sd)              # (1 - 2s + 2s^2) / q = q
    assert close(sc.cos_t, math.cos(t)) and close(sc.sin_t, math.sin(t)) and close(sc.cos_n, math.cos(n))
    assert close(sc.sin_n_sd, math.sin(n) * sd)
    assert close(sc.in_scale_next, math.sqrt(1.0 - 2.0 * sn + 2.0 * sn * sn) / sd)
    assert sc.out_scale == 3.0
    # the in-scale times the two combine coefficients undo each other: pred(m = x in_scale, eps = 0) = (1 - 2s) x
    assert close(sc.in_scale * sc.coef_m, 1.0 - 2.0 * s)


@pytest.mark.parametrize("t", [1.57080, 1.3, 0.4])
@pytest.mark.parametrize("members", [1, 3])
def test_trigflow_identity_on_step_torch(t, members):
    """x = cos t x0 + sin t sd z with the network output whose combine is the exact velocity
    pred = -sin t x0 + cos t sd z: the step returns x0 (fp32 rounding of about ten operations), and with
    zero noise and next time 0 also x_next = x0."""
    sd, n = 0.5, 2 * 35 * 32
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(members, n, generator=g, dtype=torch.float64)
    z = torch.randn(members, n, generator=g, dtype=torch.float64)
    x = math.cos(t) * x0 + math.sin(t) * sd * z
    pred = -math.sin(t) * x0 + math.cos(t) * sd * z
    sc = P.scm_step_scalars(t, 0.0, sd, out_scale=1.0)
    x32 = x.float()
    m = x32 * float(torch.tensor(sc.in_scale, dtype=torch.float32))          # round_dtype 0: what the step computes
    eps = ((pred - sc.coef_m * m.double()) / sc.coef_eps).float()
    tol = 1e-5 * float(x0.abs().max())
    _, _, out = P._step_torch(x32, eps, None, sc, 0, members, last=True)
    assert out.shape == eps.shape and out.dtype == torch.float32
    assert float((out.double() - x0).abs().max()) <= tol
    x_next, m_next, none = P._step_torch(x32, eps, torch.zeros(n), sc, 0, members, last=False)
    assert none is None
    assert float((x_next.double() - x0).abs().max()) <= tol
    # next time 0: s = 0, q = 1, so the next model input is x_next / sd
    assert torch.equal(m_next, x_next * float(torch.tensor(1.0 / sd, dtype=torch.float32)))


def test_step_torch_rounding_points_and_shared_x():
    """round_dtype marks m, eps and m_next; a shared x (one member's elements) broadcasts over members."""
    g = torch.Generator().manual_seed(3)
    n, members = 70, 3
    x = torch.randn(n, generator=g)
    eps = torch.randn(members, n, generator=g)
    noise = torch.randn(n, generator=g)
    sc = P.scm_step_scalars(1.57080, 1.3, 0.5)
    for rd, dt in ((1, torch.float16), (2, torch.bfloat16)):
        xn, mn, _ = P._step_torch(x, eps, noise, sc, rd, members)
        assert torch.equal(mn, mn.to(dt).float())                               # representable in the model dtype
        xn_rep, mn_rep, _ = P._step_torch(x.repeat(members), eps, noise, sc, rd, members)
        assert torch.equal(xn, xn_rep) and torch.equal(mn, mn_rep)
        xn0, _, _ = P._step_torch(x, eps, noise, sc, 0, members)
        assert not torch.equal(xn, xn0)                                         # the rounding is live


def test_backend_mode_switch():
    be = SanaBackend("cpu", SanaConfig(backend_mode="pipeline", synthetic_weights=True))
    assert be.name == "sana_pipeline"
    assert SanaBackend("cpu", SanaConfig(synthetic_weights=True)).name == "sana_one_step"
    assert SanaConfig().num_inference_steps == 2
    with pytest.raises(ValueError, match="backend_mode"):
        SanaBackend("cpu", SanaConfig(backend_mode="bogus", synthetic_weights=True))


def test_prompt_loaders(tmp_path):
    txt = tmp_path / "prompts.txt"
    txt.write_text("a red cat\n\n# a comment\n   # indented\n an old man reading \nthe moon\n", encoding="utf-8")
    assert P.load_prompts_from_txt(txt) == ["a red cat", "an old man reading", "the moon"]
    assert P.load_prompts_from_txt(txt, keep_comments=True) == ["a red cat", "# a comment", "# indented",
                                                                "an old man reading", "the moon"]
    assert P.SanaPipelineES.KEEP_COMMENT_PROMPTS and not P.SanaOneStep.KEEP_COMMENT_PROMPTS


def test_pipeline_class_surface():
    """Built for encoding only it needs no weights: the constructor's scheduler checks and dtype rule."""
    es = P.SanaPipelineES("nowhere/model", device="cpu", encode_only=True)
    assert es.num_inference_steps == 2 and es.timesteps == [1.57080, 1.3, 0.0] and es.transformer is None
    with pytest.raises(ValueError):
        P.SanaPipelineES("nowhere/model", device="cpu", encode_only=True, num_inference_steps=3)
    es4 = P.SanaPipelineES("nowhere/model", device="cpu", encode_only=True, num_inference_steps=4,
                           intermediate_timesteps=None)
    assert len(es4.timesteps) == 5
    with pytest.raises(FileNotFoundError, match="SanaPipelineES"):
        P.SanaPipelineES("nowhere/model", device="cpu")
