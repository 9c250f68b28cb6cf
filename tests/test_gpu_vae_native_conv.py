"""The VAR VQVAE decoder and the Infinity BSQ-VAE decoder on libeggroll's conv (the halo kernel's wide class at
widths 160 / 320 / 640) and GroupNorm, against their previous routes (MIOpen, im2col, nn.GroupNorm): the golden
image of tests/golden/g11_var_model.npz judges both VAR paths, an fp32 run of the same weights judges both paths
at the real widths, and spies show which route every conv took.  Measured errors: DESIGN §3.3.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from hyperscalees_t2i_amd import kernels as K
from hyperscalees_t2i_amd.flux_vae import Conv, FluxVAEDecoder
from hyperscalees_t2i_amd.var import DConv2d, VARArch, VARClassGenerator, VQVAEDecode
from tests.test_var_model import ARCH, IMAGE_ABS, IMAGE_MEAN, _build

pytestmark = pytest.mark.gpu

# the native path may exceed the torch bf16 path's error against fp32 by this factor: both round the same operands
# to bf16 and differ in summation order and in the norm kernel's fp32 statistics only
REL_MARGIN = 1.5


def _spies(monkeypatch):
    """Counts of K.conv_nhwc and F.unfold calls, and the (kernel size, module / weight shape) of every
    nn.Conv2d.forward and F.conv2d call."""
    seen = {"conv_nhwc": 0, "unfold": 0, "conv2d_forward": [], "f_conv2d": []}
    conv_nhwc, unfold, fwd, conv2d = K.conv_nhwc, F.unfold, nn.Conv2d.forward, F.conv2d

    def s_conv_nhwc(*a, **k):
        seen["conv_nhwc"] += 1
        return conv_nhwc(*a, **k)

    def s_unfold(*a, **k):
        seen["unfold"] += 1
        return unfold(*a, **k)

    def s_fwd(self, x):
        seen["conv2d_forward"].append((tuple(self.kernel_size), self))
        return fwd(self, x)

    def s_conv2d(x, w, *a, **k):
        seen["f_conv2d"].append(tuple(w.shape))
        return conv2d(x, w, *a, **k)

    monkeypatch.setattr(K, "conv_nhwc", s_conv_nhwc)
    monkeypatch.setattr(F, "unfold", s_unfold)
    monkeypatch.setattr(nn.Conv2d, "forward", s_fwd)
    monkeypatch.setattr(F, "conv2d", s_conv2d)
    return seen


def _rel(y, ref):
    return float((y.float() - ref).norm() / ref.norm())


# ---------------------------------------------------------------------------------------------------
# VAR, golden
# ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("native", (True, False), ids=("native", "torch"))
def test_var_golden_image_both_paths(golden, dev, monkeypatch, native):
    """The reference's teacher-forced f_hat through fhat_to_img: within IMAGE_ABS / IMAGE_MEAN of the reference's
    image with the flag on and off.  On: every 3x3 decoder conv but conv_out (3 channels) is eligible and runs
    K.conv_nhwc, none reaches F.unfold or nn.Conv2d.forward.  Off: no K.conv_nhwc call."""
    d = golden("g11_var_model.npz")
    gen, _ = _build(dev, d["theta"])
    dec = gen.vae.decoder
    assert dec.native is True                      # the default
    dec.set_native(native)
    convs3 = [m for m in dec.modules() if isinstance(m, DConv2d) and m.kernel_size == (3, 3)]
    eligible = []
    for m in convs3:
        m.register_forward_pre_hook(lambda mod, args: eligible.append(mod) if mod.native_ok(args[0]) else None)
    f_hat = torch.from_numpy(d["f_hat"]).to(dev)
    seen = _spies(monkeypatch)
    img = (gen.vae.fhat_to_img(f_hat).float() + 1) * 0.5
    err = (img.clamp(0, 1) - torch.from_numpy(d["image"].astype(np.float32)).to(dev)).abs()
    print(f"[var golden image, {'native' if native else 'torch'} vae] max {float(err.max()):.4f} "
          f"mean {float(err.mean()):.5f}")
    assert float(err.max()) < IMAGE_ABS and float(err.mean()) < IMAGE_MEAN
    fwd3 = [m for ks, m in seen["conv2d_forward"] if ks == (3, 3)]
    if native:
        assert len(convs3) > 10 and [m for m in convs3 if m not in eligible] == [dec.conv_out]
        assert seen["conv_nhwc"] == len(eligible) == len(convs3) - 1
        assert seen["unfold"] == 0 and fwd3 == [dec.conv_out]
    else:
        assert eligible == [] and seen["conv_nhwc"] == 0
        assert seen["unfold"] > 0 and len(fwd3) > 1


def test_var_native_vae_conv_flag_reaches_decoder(dev):
    from hyperscalees_t2i_amd.backend import VarBackend, VarConfig
    assert VarConfig().native_vae_conv is True
    for flag in (False, True):
        be = VarBackend(str(dev), VarConfig(arch=ARCH, classes_per_gen=2, batches_per_gen=2, ckpt_dir="/nonexistent",
                                            synthetic_if_missing=True, native_vae_conv=flag))
        be.init_and_attach_lora()
        dec = be.es_model.vae.decoder
        assert dec.native is flag
        assert all(m.native is flag for m in dec.modules() if isinstance(m, (DConv2d, nn.GroupNorm)))
    assert VARClassGenerator(device=str(dev), arch=ARCH).vae.decoder.native is True
    be = VarBackend(str(dev), VarConfig(arch=ARCH, classes_per_gen=2, batches_per_gen=2, ckpt_dir="/nonexistent",
                                        synthetic_if_missing=True, native_vae_conv=False))
    be.init_and_attach_lora()
    imgs, _ = be.es_model.generate(seed=3, guidance_scale=4.0, class_ids=[3, 980], output_type="pt")
    assert imgs.shape == (2, 3, 256, 256) and torch.isfinite(imgs).all()


# ---------------------------------------------------------------------------------------------------
# VAR, real widths
# ---------------------------------------------------------------------------------------------------


def test_var_real_widths_native_vs_torch_vs_fp32(dev):
    """VQDecoder(160, (1, 1, 2, 2, 4), 2, 32), synthetic weights, z [2, 32, 16, 16]: two native decodes are
    bitwise equal, and the native path's relative L2 error against the same (bf16-rounded) weights run in fp32
    is at most REL_MARGIN x the torch bf16 path's."""
    vae = VQVAEDecode(VARArch()).to(dev)
    vae.init_weights(5)
    dec = vae.decoder.to(torch.bfloat16).to(memory_format=torch.channels_last)
    assert dec.conv_in.out_channels == 640 and dec.conv_out.in_channels == 160
    ref_dec = copy.deepcopy(dec).float()
    ref_dec.set_native(False)
    g = torch.Generator(device=dev).manual_seed(11)
    z = torch.randn(2, 32, 16, 16, generator=g, device=dev).bfloat16().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        ref = ref_dec(z.float())
        y_native = dec(z)
        assert torch.equal(y_native, dec(z))
        dec.set_native(False)
        y_torch = dec(z)
    assert y_native.shape == (2, 3, 256, 256)
    e_native, e_torch = _rel(y_native, ref), _rel(y_torch, ref)
    print(f"[var vae 160/320/640 vs fp32] rel L2 native {e_native:.5f}  torch bf16 {e_torch:.5f}")
    assert e_native <= REL_MARGIN * e_torch, (e_native, e_torch)


# ---------------------------------------------------------------------------------------------------
# Infinity (FluxVAEDecoder at the BSQ-VAE widths) and Z-Image
# ---------------------------------------------------------------------------------------------------


def _flux_fp32(dec, z):
    """FluxVAEDecoder.forward restated in fp32 NCHW torch ops on the module's (bf16-valued) weights."""
    def gn(m, x, silu=True):
        y = F.group_norm(x, m.groups, m.weight.float(), m.bias.float(), m.eps)
        return F.silu(y) if silu else y

    def conv(m, x):
        return F.conv2d(x, m.weight.float(), m.bias.float(), padding=m.ks // 2)

    def lin(m, x):
        return F.linear(x, m.weight.float(), m.bias.float())

    def res(r, x):
        h = conv(r.conv2, gn(r.norm2, conv(r.conv1, gn(r.norm1, x))))
        return h + (x if r.conv_shortcut is None else conv(r.conv_shortcut, x))

    def attn(a, x):
        B, C, H, W = x.shape
        n = gn(a.group_norm, x, False).flatten(2).transpose(1, 2)
        q, k, v = (lin(m, n)[:, None] for m in (a.to_q, a.to_k, a.to_v))
        o = F.scaled_dot_product_attention(q, k, v, scale=C ** -0.5)[:, 0]
        return x + lin(a.to_out[0], o).transpose(1, 2).reshape(B, C, H, W)

    x = conv(dec.conv_in, z.to(torch.bfloat16).float())
    x = res(dec.mid[2], attn(dec.mid[1], res(dec.mid[0], x)))
    for blk in dec.up_blocks:
        for r in blk.resnets:
            x = res(r, x)
        if blk.upsample is not None:
            x = conv(blk.upsample, F.interpolate(x, scale_factor=2, mode="nearest"))
    return conv(dec.conv_out, gn(dec.conv_norm_out, x))


def test_infinity_vae_native_vs_miopen_vs_fp32(dev, monkeypatch):
    """FluxVAEDecoder(14, (160, 320, 640, 640)), z [1, 14, 16, 16]: flag on against off under the rule of the VAR
    test, two native decodes bitwise equal, and with the flag on F.conv2d serves conv_in and conv_out only."""
    dec = FluxVAEDecoder(latent_channels=14, widths=(160, 320, 640, 640)).to(dev)
    dec.init_weights(3)
    g = torch.Generator(device=dev).manual_seed(12)
    z = torch.randn(1, 14, 16, 16, generator=g, device=dev)
    n3 = sum(1 for m in dec.modules() if isinstance(m, Conv) and m.ks == 3)
    with torch.no_grad():
        ref = _flux_fp32(dec, z)
        seen = _spies(monkeypatch)
        y_native = dec(z)
        assert seen["f_conv2d"] == [(640, 14, 3, 3), (3, 160, 3, 3)], seen["f_conv2d"]
        assert seen["conv_nhwc"] == n3 - 2
        assert torch.equal(y_native, dec(z))
        dec.set_native_wide_conv(False)
        seen["f_conv2d"].clear()
        seen["conv_nhwc"] = 0
        y_torch = dec(z)
        assert len(seen["f_conv2d"]) == n3 and seen["conv_nhwc"] == 0
    assert y_native.shape == (1, 3, 128, 128)
    e_native, e_torch = _rel(y_native, ref), _rel(y_torch, ref)
    print(f"[infinity vae 160/320/640 vs fp32] rel L2 native {e_native:.5f}  miopen bf16 {e_torch:.5f}")
    assert e_native <= REL_MARGIN * e_torch, (e_native, e_torch)


def test_zimage_vae_unchanged_by_flag(dev):
    """Z-Image's widths (128, 256, 512, 512) are power-of-two: their branch ignores the flag, bit for bit."""
    dec = FluxVAEDecoder().to(dev)
    dec.init_weights(2)
    g = torch.Generator(device=dev).manual_seed(13)
    z = torch.randn(1, 16, 16, 16, generator=g, device=dev)
    with torch.no_grad():
        y_on = dec(z)
        dec.set_native_wide_conv(False)
        y_off = dec(z)
    assert torch.equal(y_on, y_off)
