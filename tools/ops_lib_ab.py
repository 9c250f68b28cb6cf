"""A/B of two or more builds of libeggroll through the package's own op wrappers (kernels.py): the
global library handle is swapped between bound builds, each op's outputs are compared bitwise with the
first build's, then timed interleaved (median of rounds, HIP events on the launch stream).  Ops: the
epoch's row norms (Sana AdaLN on the fp32 stream with fp32 modulation, C = 2240; bf16 rows, C = 2240;
DC-AE RMSNorm + bias + fp32 residual, C = 512 and 1024), resid_layernorm (CLIP towers), the Z-Image q/k
norm + RoPE, the DC-AE decoder head and the DC-AE convs; small_cases adds one small case per remaining entry
point of the conv / nhwc / norm / qk / linattn / image units and per branch of their host-side kernel choices.
usage: python tools/ops_lib_ab.py <libA.so> <libB.so> [...] [--only=SUBSTRING] [--once]"""
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from hyperscalees_t2i_amd import _lib  # noqa: E402
from hyperscalees_t2i_amd import kernels as K  # noqa: E402
from es_lib_ab import bind, timed  # noqa: E402


def cases(dev, g):
    r = lambda *s, dt=torch.bfloat16, sc=1.0: (torch.randn(*s, device=dev, generator=g) * sc).to(dt)  # noqa: E731
    out = {}
    # Sana AdaLN: fp32 stream x [131072, 2240], fp32 (1 + scale) / shift per image (1024 rows each)
    x32 = r(131072, 2240, dt=torch.float32)
    ms, mh = r(128, 2240, dt=torch.float32, sc=0.1), r(128, 2240, dt=torch.float32, sc=0.1)
    out["adaln f32 131072x2240"] = lambda: K.rownorm(x32, 1e-6, layer=True, mscale=ms, mshift=mh, rows_per_group=1024)
    xb = r(131072, 2240)
    wb = r(2240, sc=0.5)
    out["rms bf16 131072x2240 +w"] = lambda: K.rownorm(xb, 1e-6, w=wb)
    for C, rows in ((512, 8 * 256 * 256), (512, 8 * 128 * 128), (1024, 8 * 128 * 128)):
        xc, wc, bc = r(rows, C), r(C, sc=0.5), r(C, sc=0.1)
        res0 = r(rows, C, dt=torch.float32)
        res = res0.clone()

        def f(xc=xc, wc=wc, bc=bc, res=res, res0=res0):
            res.copy_(res0)
            return K.rownorm(xc, 1e-5, w=wc, b=bc, res=res)
        out[f"dcae rms+res32 {rows}x{C}"] = f
        o32, sh = torch.empty_like(res0), torch.empty(rows, C, device=dev, dtype=torch.bfloat16)

        def f2(xc=xc, wc=wc, bc=bc, res0=res0, o32=o32, sh=sh):   # the product form, out of place (no copy timed)
            return K.rownorm(xc, 1e-5, w=wc, b=bc, res=res0, out=o32, shadow=sh)
        out[f"dcae rms+res32+shadow {rows}x{C}"] = f2
    # linear attention: Sana attn1 (separate q / k / v [B*N, 2240], 70 heads) and DC-AE planar [Q|K|V]
    qs, ks, vs = r(128 * 1024, 2240), r(128 * 1024, 2240), r(128 * 1024, 2240)
    out["linear_attention sana 128x1024 h70"] = lambda: K.linear_attention(qs, ks, vs, 128, 1024, 70, 32, False)
    for Bd, N, hd in ((8, 16384, 16), (8, 4096, 32), (8, 1024, 32)):
        flat = r(Bd * N, 3 * hd * 32)
        inner = hd * 32
        out[f"linear_attention dcae {Bd}x{N} h{hd}"] = (lambda flat=flat, inner=inner, Bd=Bd, N=N, hd=hd:
            K.linear_attention(flat, flat[:, inner:], flat[:, 2 * inner:], Bd, N, hd, 32, True))
    # DC-AE ResBlock conv2 + RMSNorm + residual (halo kernel, NORM epilogue): 128 ch at 1024^2, 256 ch at 512^2
    for Bc, Hc, Cc in ((8, 1024, 128), (8, 512, 256)):
        xc = r(Bc, Hc, Hc, Cc, sc=0.5)
        wpk = r(Cc, 9 * Cc, sc=(9 * Cc) ** -0.5)
        nwc, nbc, resc = r(Cc, sc=0.5), r(Cc, sc=0.1), r(Bc, Hc, Hc, Cc)
        out[f"conv3x3_rmsnorm {Bc}x{Hc}^2x{Cc}"] = (lambda xc=xc, wpk=wpk, nwc=nwc, nbc=nbc, resc=resc:
            K.conv3x3_rmsnorm_nhwc(xc, wpk, None, 1, 1e-6, nwc, nbc, resc))
    # DC-AE ResBlock conv1 (halo kernel): plain and bias + SiLU at the three product shapes
    for Bc, Hc, Cc in ((8, 1024, 128), (8, 512, 256), (8, 256, 512)):
        xc, wpk, bc = r(Bc, Hc, Hc, Cc, sc=0.5), r(Cc, 9 * Cc, sc=(9 * Cc) ** -0.5), r(Cc, sc=0.1)
        out[f"conv3x3 {Bc}x{Hc}^2x{Cc}"] = lambda xc=xc, wpk=wpk: K.conv3x3_nhwc(xc, wpk, None, 1)
        out[f"conv3x3 bias+silu {Bc}x{Hc}^2x{Cc}"] = (lambda xc=xc, wpk=wpk, bc=bc:
            K.conv3x3_nhwc(xc, wpk, bc, 1, "silu"))
    # flash attention (head dim 128): Z-Image's joint sequence (4 images x 4096+512 tokens x 30 heads) and a
    # ragged one (a partial key block, Nq not a multiple of the query tile)
    for Bf, Nf, Hf in ((4, 4608, 30), (2, 1000, 8)):
        qf, kf, vf = (r(Bf, Nf, Hf, 128, sc=0.5) for _ in range(3))
        out[f"flash_attention {Bf}x{Nf} h{Hf}"] = (lambda qf=qf, kf=kf, vf=vf:
            K.flash_attention(qf, kf, vf, 128 ** -0.5))
    # DC-AE up-blocks: 2x2 phase conv + sub-pixel interleave + bias + shortcut in one launch (the four product
    # shapes, 8 images; the 512->1024 one also on the fp32 stream with its bf16 shadow)
    from hyperscalees_t2i_amd.dcae import subpixel_phase_weights
    for Hs, Cin, Cout, f32 in ((512, 256, 128, False), (256, 512, 256, False), (128, 512, 512, False),
                               (64, 1024, 512, False), (64, 1024, 512, True)):
        xs = r(8, Hs, Hs, Cin, sc=0.5)
        w4 = subpixel_phase_weights(torch.randn(Cout, Cin, 3, 3, device=dev, generator=g) / (9 * Cin) ** 0.5)
        w4p = K.pack_conv3x3_weight(w4.to(torch.bfloat16).contiguous(memory_format=torch.channels_last), 1)
        bs = r(Cout, sc=0.1)
        if f32:
            src = r(8, Hs, Hs, Cin, dt=torch.float32)
            sh = torch.empty(8, 2 * Hs, 2 * Hs, Cout, device=dev, dtype=torch.bfloat16)
            out[f"conv2x2_subpixel f32 8x{Hs}^2 {Cin}->{Cout}"] = (lambda xs=xs, w4p=w4p, src=src, bs=bs, sh=sh:
                torch.cat([K.conv2x2_subpixel(xs, w4p, src, bias=bs, shadow=sh).flatten(), sh.float().flatten()]))
        else:
            out[f"conv2x2_subpixel 8x{Hs}^2 {Cin}->{Cout}"] = (lambda xs=xs, w4p=w4p, bs=bs:
                K.conv2x2_subpixel(xs, w4p, xs, bias=bs))
    # DC-AE multi-scale branch: 5x5 depthwise + grouped 1x1 (the three product shapes)
    for Hd, Cd in ((128, 1536), (64, 3072), (32, 3072)):
        xd = r(8, Hd, Hd, Cd, sc=0.5)
        wd = r(25, Cd, sc=0.2)
        pwd = r(Cd // 32, 32, 32, sc=1 / 6)
        out[f"~dwconv_pw5 8x{Hd}^2x{Cd}"] = lambda xd=xd, wd=wd, pwd=pwd: K.dwconv_pw_nhwc(xd, wd, pwd, 5)
    h0 = r(16 * 257, 1280, dt=torch.float32)
    h = h0.clone()
    y, w2, b2 = r(16 * 257, 1280), r(1280, sc=0.5), r(1280, sc=0.1)

    def rl():
        h.copy_(h0)
        return torch.cat([K.resid_layernorm_(h, y, w2, b2, 1e-5).float().flatten(), h.flatten()])
    out["resid_layernorm 4112x1280"] = rl
    out.update(small_cases(dev, r))
    return out


def small_cases(dev, r):
    """One small case per host-ladder branch and per entry point that the shapes above leave out (bitwise only:
    too small to time well).  In-place ops work on a fresh copy per call."""
    out = {}
    # rownorm: every step of the chunk ladder (16 ... 512 slots) in its three forms (bf16, fp32 x, fp32 out + bf16
    # shadow); resid_layernorm: 1, 2, 4, 8 chunks per lane
    for C in (128, 256, 512, 1024, 2048, 2240, 4096):
        x, w, res = r(96, C), r(C, sc=0.5), r(96, C, dt=torch.float32)
        out[f"rms bf16 96x{C}"] = lambda x=x, w=w: K.rownorm(x, 1e-6, w=w, act="silu")
        out[f"layer f32 96x{C}"] = lambda res=res, w=w: K.rownorm(res, 1e-6, layer=True, w=w)

        def rs(x=x, w=w, res=res):
            o, sh = torch.empty_like(res), torch.empty_like(x)
            K.rownorm(x, 1e-5, w=w, res=res, out=o, shadow=sh)
            return torch.cat([o.flatten(), sh.float().flatten()])
        out[f"rms+res32+shadow 96x{C}"] = rs
    for C in (512, 1024, 2048, 4096):
        h0, y, w, b = r(33, C, dt=torch.float32), r(33, C), r(C, sc=0.5), r(C, sc=0.1)

        def rl(h0=h0, y=y, w=w, b=b):
            h = h0.clone()
            return torch.cat([K.resid_layernorm_(h, y, w, b, 1e-5).float().flatten(), h.flatten()])
        out[f"resid_layernorm 33x{C}"] = rl
    # residual updates, bias + act
    xg, yg, gate = r(64, 320), r(64, 320), r(4, 320)
    out["gated_residual 64x320"] = lambda: K.gated_residual_(xg.clone(), yg, gate, 16)
    x32 = r(64, 320, dt=torch.float32)
    for nm, gt in (("bf16 gate", gate), ("f32 gate", gate.float()), ("no gate", None)):
        def gr(gt=gt):
            x, sh = x32.clone(), torch.empty(64, 320, device=dev, dtype=torch.bfloat16)
            K.gated_residual_f32_(x, yg, gt, 16, shadow=sh)
            return torch.cat([x.flatten(), sh.float().flatten()])
        out[f"gated_residual_f32 64x320 {nm}"] = gr
    bb = r(320, sc=0.1)
    for act in (None, "relu", "silu"):
        out[f"bias_act 64x320 {act}"] = lambda act=act: K.bias_act_(xg.clone(), bb, act)
    # scm_step: every rounding x eps dtype; 3 members of 1003 elements (the scalar form), 4 of 1024 (the vector form)
    sc = (0.5, 0.9, -0.4, 0.8, 0.6, 0.7, 0.35, 0.45, 2.0)
    for rd in (0, 1, 2):
        for edt in (torch.float32, torch.bfloat16):
            for mem, n in ((3, 1003), (4, 1024)):
                xs, es, nz = r(mem, n, dt=torch.float32), r(mem, n, dt=edt), r(n, dt=torch.float32)

                def scm(xs=xs, es=es, nz=nz, rd=rd, mem=mem):
                    o = [torch.empty_like(xs) for _ in range(3)]
                    K.scm_step(xs, es, nz, sc, rd, mem, *o)
                    return torch.cat([t.flatten() for t in o])
                out[f"scm_step rd{rd} {str(edt)[6:]} {mem}x{n}"] = scm
    # GroupNorm with and without SiLU
    xn, wn, bn = r(2, 9, 7, 64), r(64, sc=0.5), r(64, sc=0.1)
    for silu in (False, True):
        out[f"group_norm 2x9x7x64 silu={silu}"] = lambda silu=silu: K.group_norm_nhwc(xn, 32, wn, bn, 1e-6, silu)
    # depthwise convs: every KS x PRE_SILU x GLU instance (several channel slices, partial tiles), the 3x3 PW form
    xd, bd = r(2, 9, 37, 128, sc=0.5), r(128, sc=0.1)
    for ks in (3, 5):
        wd = r(ks * ks, 128, sc=0.2)
        for ps in (False, True):
            for glu in (False, True):
                out[f"dwconv{ks} silu={ps} glu={glu} 2x9x37x128"] = (lambda wd=wd, ks=ks, ps=ps, glu=glu:
                    K.dwconv_nhwc(xd, wd, bd, ks, ps, glu))
    w3, pw3 = r(9, 128, sc=0.2), r(4, 32, 32, sc=1 / 6)
    out["dwconv_pw3 2x9x37x128"] = lambda: K.dwconv_pw_nhwc(xd, w3, pw3, 3)
    # DC-AE shortcuts: rep = 4 Cout / Cin of 1, 2, 4 (the per-low-pixel kernel) and 8 (the per-output one)
    for cin, cout in ((64, 16), (64, 32), (32, 32), (32, 64)):
        xs, ys = r(2, 5, 7, cin), r(2, 10, 14, cout)
        y4, bs = r(2, 6, 8, 4 * cout), r(cout, sc=0.1)
        out[f"upshortcut_add {cin}->{cout}"] = lambda xs=xs, ys=ys: K.upshortcut_add_(ys.clone(), xs)
        out[f"subpixel_shortcut {cin}->{cout}"] = lambda xs=xs, y4=y4, bs=bs: K.subpixel_shortcut(y4, xs, bias=bs)
        if cout * 4 // cin <= 4:
            def sp32(xs=xs, y4=y4, bs=bs, cout=cout):
                sh = torch.empty(2, 10, 14, cout, device=dev, dtype=torch.bfloat16)
                o = K.subpixel_shortcut_f32(y4, xs.float(), bs, sh)
                return torch.cat([o.flatten(), sh.float().flatten()])
            out[f"subpixel_shortcut_f32 {cin}->{cout}"] = sp32
    # dense convs: every kernel instance the conv dispatch can launch.  Ragged shapes run the tap-staged kernel
    # under kernel 0 (ks 2; the 512 x 128 tile; 256 x 256 at px 1 and px 2); H = 16 with W = 32 (N = 128) or
    # W = 16 (N = 256) runs the halo kernel, and the tap-staged RMSNorm forms once more there under kernel 1
    for tag, shp, cout, ks, px, kerns in (("ks2", (1, 7, 10, 128), 128, 2, 1, (0,)),
                                          ("tall", (1, 7, 10, 128), 128, 3, 1, (0,)),
                                          ("px1", (1, 9, 12, 256), 256, 3, 1, (0,)),
                                          ("px2", (1, 7, 10, 128), 128, 3, 2, (0,)),
                                          ("halo tall", (1, 16, 32, 128), 128, 3, 1, (0, 1)),
                                          ("halo 256", (1, 16, 16, 256), 256, 3, 1, (0, 1))):
        xc = r(*shp, sc=0.5)
        wpk = K.pack_conv3x3_weight(r(cout, shp[3], ks, ks, sc=(ks * ks * shp[3]) ** -0.5), px)
        bc, nwc, nbc = r(cout, sc=0.1).repeat(px), r(cout, sc=0.5), r(cout, sc=0.1)
        resc = r(*shp[:3], cout)
        out[f"conv {tag} {shp}"] = lambda xc=xc, wpk=wpk, ks=ks, px=px: K.conv_nhwc(xc, wpk, None, ks, px)
        out[f"conv {tag} bias+silu {shp}"] = (lambda xc=xc, wpk=wpk, bc=bc, ks=ks, px=px:
            K.conv_nhwc(xc, wpk, bc, ks, px, "silu"))
        for kern in kerns if ks == 3 else ():
            out[f"conv_rmsnorm {tag} kernel {kern} {shp}"] = (
                lambda xc=xc, wpk=wpk, bc=bc, px=px, nwc=nwc, nbc=nbc, resc=resc, kern=kern:
                K.conv3x3_rmsnorm_nhwc(xc, wpk, bc, px, 1e-5, nwc, nbc, resc, kernel=kern))
    # conv2x2_subpixel: REP = 4 Cout / Cin of 1, 2, 4 with a bf16 and an fp32 shortcut source
    for cin in (256, 128, 64):
        xs, bs = r(2, 5, 7, cin, sc=0.5), r(64, sc=0.1)
        w4p = K.pack_conv3x3_weight(r(256, cin, 2, 2, sc=(4 * cin) ** -0.5), 1)
        out[f"conv2x2_subpixel {cin}->64"] = lambda xs=xs, w4p=w4p, bs=bs: K.conv2x2_subpixel(xs, w4p, xs, bias=bs)

        def spx32(xs=xs, w4p=w4p, bs=bs, src=r(2, 5, 7, cin, dt=torch.float32)):
            sh = torch.empty(2, 10, 14, 64, device=dev, dtype=torch.bfloat16)
            o = K.conv2x2_subpixel(xs, w4p, src, bias=bs, shadow=sh)
            return torch.cat([o.flatten(), sh.float().flatten()])
        out[f"conv2x2_subpixel f32 {cin}->64"] = spx32
    xh = r(2, 19, 21, 128)
    nw, nb, cw, cb = r(128, sc=0.5), r(128, sc=0.1), r(3, 128, 3, 3, sc=0.05), r(3, sc=0.1)
    out["dcae_head 2x19x21"] = lambda: K.dcae_head(xh, 1e-5, nw, nb, cw, cb)
    # linear attention: the fold with one head per block (odd head count), and 16 tiles per wave without head pairs
    for Bl, N, hd in ((64, 300, 33), (1, 8200, 2)):
        flat = r(Bl * N, 3 * hd * 32).abs()
        out[f"linear_attention planar {Bl}x{N} h{hd}"] = (lambda flat=flat, Bl=Bl, N=N, hd=hd:
            K.linear_attention(flat, flat[:, hd * 32:], flat[:, 2 * hd * 32:], Bl, N, hd, 32, False))
    # q / k preparation: Z-Image / Infinity (head dim 128, in place and into a cache), VAR, Gemma-2, Qwen3
    xq, wq = r(2 * 37, 3 * 128), r(128, sc=0.5)
    cs, sn = r(37, 64, dt=torch.float32), r(37, 64, dt=torch.float32)
    out["qk_norm_rope 74 rows h3"] = lambda: K.qk_norm_rope_(xq.clone(), wq, 1e-6, cs, sn, 3)
    hs, vin = r(3, dt=torch.float32), r(2 * 37, 3 * 128)

    def nrkv():
        x, kc = xq.clone(), torch.zeros(2, 50, 3 * 128, device=dev, dtype=torch.bfloat16)
        vc = torch.zeros_like(kc)
        K.qk_norm_rope_kv(x, wq, 1e-6, cs, sn, 3, hscale=hs, out=kc, rows_per_seq=37, row0=5, vin=vin, vout=vc)
        return torch.cat([x.flatten(), kc.flatten(), vc.flatten()])
    out["qk_norm_rope_kv 74 rows h3"] = nrkv
    qkv, qs = r(2 * 37, 3 * 4 * 64), r(4, dt=torch.float32)

    def l2kv():
        t = qkv.clone()
        kc = torch.zeros(2, 50, 4 * 64, device=dev, dtype=torch.bfloat16)
        vc = torch.zeros_like(kc)
        K.qk_l2norm_kv(t[:, :256], t[:, 256:512], t[:, 512:], 4, qscale=qs, kout=kc, vout=vc, rows_per_seq=37, row0=5)
        return torch.cat([t.flatten(), kc.flatten(), vc.flatten()])
    out["qk_l2norm_kv 74 rows h4"] = l2kv
    xg2, c2, s2 = r(2 * 37, 3 * 256), r(37, 128, dt=torch.float32), r(37, 128, dt=torch.float32)
    out["rope_half 2x37 h2"] = lambda: K.rope_half_(xg2.clone(), c2, s2, 2, 37, 2)
    wq3, wk3 = r(128, dt=torch.float32), r(128, dt=torch.float32)
    out["qk_norm_rope_half 2x37 h2+1"] = lambda: K.qk_norm_rope_half_(xq.clone(), wq3, wk3, 1e-6, cs, sn, 2, 37, 2, 1)
    # CLIP preprocessing of a bf16 decoder output
    from hyperscalees_t2i_amd.rewards import clip_pixels
    img = r(2, 3, 300, 260, sc=0.6)
    for mode in (0, 1, 2):
        out[f"clip_preprocess mode {mode} 2x300x260"] = lambda mode=mode: clip_pixels(img, mode)
    return out


def main(paths, rounds=7, only=None, once=False):
    libs = [bind(p) for p in paths]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    res = {}
    for name, fn in cases(dev, g).items():
        if only and only not in name:
            continue
        outs = []
        for lib in libs:
            _lib._lib = lib
            outs.append(fn().clone())
        torch.cuda.synchronize()
        same = [torch.equal(outs[0], o) for o in outs[1:]]
        us = [[] for _ in libs]
        for _ in range(0 if once else rounds):   # --once: each case once per build, for a kernel trace
            for i, lib in enumerate(libs):
                _lib._lib = lib
                us[i].append(timed(fn))
        res[name] = {"bitwise_equal_to_A": same, **{Path(p).name: round(statistics.median(u), 1)
                                                     for p, u in zip(paths, us) if u}}
        if name.startswith("~"):   # a numerics-changing A/B: report the largest relative difference instead
            res[name]["max_rel_diff_to_A"] = [float((o.float() - outs[0].float()).abs().max() /
                                                    outs[0].float().abs().max().clamp_min(1e-30)) for o in outs[1:]]
        print(json.dumps({name: res[name]}), flush=True)
        assert all(same) or name.startswith("~"), name
    print(json.dumps(res))


if __name__ == "__main__":
    only = next((a[7:] for a in sys.argv[1:] if a.startswith("--only=")), None)
    main([a for a in sys.argv[1:] if not a.startswith("--")], only=only, once="--once" in sys.argv)
