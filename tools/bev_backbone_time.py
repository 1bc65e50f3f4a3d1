#!/usr/bin/env python3
"""The BEV backbone + FPN neck (bev_backbone.py, csrc/deconv.hip), timed at the config-2 map: B = 8, 128 x 128,
256 channels, the default build (stages of 6 convolutions at 128 and 256 channels, upsampling 1 and 2 to 2 x 256 channels).
(a) The product transposed convolution, 256 -> 256, s = 2, 64 x 64 -> 128 x 128, written into its slice of the 512-channel concat:
    the fused launch (bevf_deconv_nhwc_*) against the composition the other kernels allow -- a 1x1 implicit-GEMM convolution to
    [M][s*s*Cout] (scale / shift / ReLU in its epilogue) plus a shuffle copy into the slice, written in torch --, fp32 and bf16, all
    four legs alternating in one process.  Median, min and max over the rounds; achieved TB/s (algorithmic bytes: x once, y once)
    and MFMA TF/s beside the arithmetic (17.2 GFLOP; 33.5 MB in + 134 MB out in fp32, half that in bf16).
(b) Every launch of the module's eval forward (engine.KernelTimer spans) and the whole module, fp32 and bf16.
usage: bev_backbone_time.py [rounds]   (prints one JSON object per measurement)"""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import bev_backbone, engine, synth

PEAK_HBM_GBS = 8000.0          # bench.py's
PEAK_F32_MFMA_TFLOPS = 157.3
PEAK_BF16_MFMA_TFLOPS = 2500.0


def timed_ab(fns, rounds=7, inner=20, warm=2):
    """(median, min, max) in us of each callable, measured in alternating rounds of one process."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for fn, t in zip(fns, ts):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) / inner * 1e3)
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in ts]


def deconv_legs(rounds, dev):
    B, H, W, Cin, Cout, s, Ct = 8, 64, 64, 256, 256, 2, 512
    M = B * H * W
    w = synth.normal((Cin, Cout, s, s), 1, 0.0, (2.0 / Cin) ** 0.5).to(dev)
    scale, shift = synth.uniform((Cout,), 2, 0.6, 1.2).to(dev), synth.normal((Cout,), 3, 0.0, 0.05).to(dev)
    legs, names, checks = [], [], []
    for dt, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        x = synth.normal((M * Cin,), 4).to(dev).to(dt)
        wp = L.deconv_pack(w, dt)
        # the composition's filter: rows n' = (i*s + j)*Cout + co of a 1x1 convolution, OHWI = [s*s*Cout][Cin]
        w1 = w.permute(2, 3, 1, 0).reshape(s * s * Cout, Cin).contiguous().to(dt).view(-1)
        sc4, sh4 = scale.repeat(s * s).contiguous(), shift.repeat(s * s).contiguous()
        mid = torch.empty(M * s * s * Cout, dtype=dt, device=dev)
        out_f = torch.zeros(M * s * s * Ct, dtype=dt, device=dev)
        out_c = torch.zeros(M * s * s * Ct, dtype=dt, device=dev)

        def fused(x=x, wp=wp, out=out_f):
            L.deconv_nhwc(x, wp, scale, shift, out[256:], N=B, H=H, W=W, Cin=Cin, x_cs=Cin, Cout=Cout, y_cs=Ct, s=s, relu=True)

        def composed(x=x, w1=w1, sc4=sc4, sh4=sh4, mid=mid, out=out_c):
            L.conv2d_nhwc(x, w1, sc4, sh4, mid, N=B, H=H, W=W, Cin=Cin, x_cs=Cin, Cout=s * s * Cout, y_cs=s * s * Cout, KH=1, KW=1,
                          stride=1, pad=0, relu=True)
            out.view(B, H, s, W, s, Ct)[..., 256:].copy_(mid.view(B, H, W, s, s, Cout).permute(0, 1, 3, 2, 4, 5))

        legs += [fused, composed]
        names += [f"bevf_deconv_nhwc_{tag} (fused)", f"1x1 conv + shuffle copy, {tag} (composition)"]
        checks.append((tag, fused, composed, out_f, out_c))
    for tag, fused, composed, out_f, out_c in checks:                  # the two routes compute the same map
        fused()
        composed()
        torch.cuda.synchronize()
        d = float((out_f.float() - out_c.float()).abs().max())
        print(json.dumps({"check": f"fused vs composition, {tag}", "max_abs_diff": d, "max_abs": float(out_c.float().abs().max())}), flush=True)
    flops = 2.0 * M * s * s * Cout * Cin
    res = timed_ab(legs, rounds)
    for name, (med, lo, hi) in zip(names, res):
        es = 2 if "bf16" in name else 4
        nbytes = float(es) * (M * Cin + M * s * s * Cout)
        print(json.dumps({"leg": name, "median_us": round(med, 1), "min_us": round(lo, 1), "max_us": round(hi, 1),
                          "algorithmic_mb": round(nbytes / 1e6, 1), "tb_per_s": round(nbytes / (med * 1e-6) / 1e12, 2),
                          "mfma_tf_per_s": round(flops / (med * 1e-6) / 1e12, 1)}), flush=True)
    for k, tag in ((0, "f32"), (2, "bf16")):
        (fm, _, _), (cm, clo, chi) = res[k], res[k + 1]
        keep = fm <= chi + (chi - clo)                                 # DESIGN 3.1c's rule: not above the other leg's max by more than its spread
        print(json.dumps({"verdict": tag, "fused_median_us": round(fm, 1), "composition_median_us": round(cm, 1),
                          "composition_min_max_us": [round(clo, 1), round(chi, 1)], "fused_kept": bool(keep)}), flush=True)


def module_legs(rounds, dev):
    B, H, W, C = 8, 128, 128, 256
    for dt, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        m = bev_backbone.BEVBackbone(C)
        synth.fill_state_dict_(m, 1)
        m = m.to(dev).to(dt).eval()
        x = synth.normal((B * H * W * C,), 5).to(dev).to(dt)
        run = lambda: m.forward_nhwc(x, B, H, W)
        with torch.no_grad():
            (med, lo, hi), = timed_ab([run], rounds, inner=5)
            timer = engine.KernelTimer()
            engine.set_timer(timer)
            for _ in range(5):
                run()
            torch.cuda.synchronize()
            engine.set_timer(None)
        print(json.dumps({"module": f"BEVBackbone default build, B = {B}, {H} x {W} x {C}, eval, {tag}, conv mode {engine.conv_mode()}",
                          "median_ms": round(med / 1e3, 3), "min_ms": round(lo / 1e3, 3), "max_ms": round(hi / 1e3, 3)}), flush=True)
        for name, d in timer.totals().items():
            n = d["launches"] / 5
            print(json.dumps({"span": name, "dtype": tag, "launches_per_forward": n, "ms_per_forward": round(d["ms"] / 5, 3),
                              "algorithmic_tf_per_s": round(d["flops"] / 5 / (d["ms"] / 5 * 1e-3) / 1e12, 1) if d["ms"] else None}),
                  flush=True)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 7
    if not torch.cuda.is_available():
        raise SystemExit("bev_backbone_time.py measures on the GPU: no 'cuda' device is visible")
    dev = torch.device("cuda")
    print(json.dumps({"peaks": {"hbm_gb_s": PEAK_HBM_GBS, "f32_mfma_tf_s": PEAK_F32_MFMA_TFLOPS, "bf16_mfma_tf_s": PEAK_BF16_MFMA_TFLOPS}}),
          flush=True)
    deconv_legs(rounds, dev)
    module_legs(max(3, rounds // 2), dev)


if __name__ == "__main__":
    main()
