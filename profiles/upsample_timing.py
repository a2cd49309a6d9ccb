"""Time per launch of rtowUpsampleDevice on the cover scene, 960 x 540 -> 1920 x 1080 and 1920 x 1080 -> 3840 x 2160, in each mode: POINT, BILINEAR, GUIDED without and
with the albedo demodulation (and BILINEAR with it).  The guides are the real ones - rtowTraceViewDevice and rtowShadeHitsDevice at both sizes with one view - because
the share of pixels that leave stage A decides how many taps a GUIDED launch reads; the colour is random (its values do not change the work).  In one process on one GPU.

Each call is bracketed by HIP events on the stream it is enqueued on (torch.cuda.Event, as profiles/trace_interval_timing.py); after `--warmup` untimed calls,
`--reps` timed calls per point: median, minimum and maximum.  `bytes_per_dst_pixel` counts every buffer the mode touches once (src buffers at their own size, outStage
not written), `tb_per_s` is that over the median.

`quality`: the parameter grid of the recommended values on the frames of tests/test_gpu_upsample.py's quality test (cover scene, 16 spp at 96 x 54 against 1024 spp at
192 x 108): mean squared error of each point over that of the POINT upsampling.

    python profiles/upsample_timing.py --out profiles/r09_upsample.json
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
rt = importlib.import_module("raytracing-in-one-weekend_amd")
abi = rt.abi
P, B, G, M, D = abi.RTOW_UPSAMPLE_POINT, abi.RTOW_UPSAMPLE_BILINEAR, abi.RTOW_UPSAMPLE_GUIDED, abi.RTOW_UPSAMPLE_MATCH_ENTITY, abi.RTOW_UPSAMPLE_DEMODULATE_ALBEDO
POINTS = [("point", P, 0), ("bilinear", B, 0), ("bilinear_demodulated", B, D), ("guided", G, M), ("guided_demodulated", G, M | D)]


def timed(stream, reps, warmup, call):
    for _ in range(warmup):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(stream)
        call()
        b.record(stream)
    stream.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return {"ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1]}


class Guides:
    """trace-view + shade-hits of `view` at w x h, resident"""

    def __init__(self, ctx, lib, dev, sp, view, env, w, h):
        n = w * h
        self.dist, self.ent = torch.empty(n, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        self.nrm, self.alb, rays = torch.empty(n * 3, device=dev), torch.empty(n * 3, device=dev), torch.empty(n * 8, device=dev)
        self.hits = abi.HitBuffers(self.dist.data_ptr(), self.ent.data_ptr(), self.nrm.data_ptr())
        p = abi.TraceViewParams(w, h, view, 0.0, 0)
        rt.lib.check(lib.rtowTraceViewDevice(ctx.handle, C.byref(p), C.byref(self.hits), rays.data_ptr(), sp), "rtowTraceViewDevice")
        surface = abi.SurfaceBuffers(self.alb.data_ptr(), None, None, None, None, None)
        sh = abi.ShadeHitsParams(env, 0, 0)
        rt.lib.check(lib.rtowShadeHitsDevice(ctx.handle, C.byref(sh), n, rays.data_ptr(), self.ent.data_ptr(), C.byref(surface), sp), "rtowShadeHitsDevice")


def timings(args, lib, dev, stream):
    S = rt.scenes
    scene = S.cover_scene()
    rows = []
    sp = C.c_void_p(stream.cuda_stream)
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        for (sw, sh), (dw, dh) in (((960, 540), (1920, 1080)), ((1920, 1080), (3840, 2160))):
            params = S.make_params(scene, sw, sh, spp=1, trace_depth=8, seed=1)
            ns, nd = sw * sh, dw * dh
            stream.wait_stream(torch.cuda.current_stream(dev))
            gs = Guides(ctx, lib, dev, sp, params.view, params.environment, sw, sh)
            gd = Guides(ctx, lib, dev, sp, params.view, params.environment, dw, dh)
            color = torch.rand(ns * 3, device=dev) * 2.0
            out, stage = torch.empty(nd * 3, device=dev), torch.empty(nd, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            stream.synchronize()
            row = {"src": [sw, sh], "dst": [dw, dh], "scene": "cover"}
            for name, mode, flags in POINTS:
                p = abi.UpsampleParams(sw, sh, dw, dh, mode, abi.UPSAMPLE_DEFAULT_NORMAL_SHARPNESS, abi.UPSAMPLE_DEFAULT_DEPTH_TOLERANCE, flags, 0)

                def call(stage_ptr=None):
                    rt.lib.check(lib.rtowUpsampleDevice(ctx.handle, C.byref(p), color.data_ptr(), C.byref(gs.hits), gs.alb.data_ptr(), C.byref(gd.hits), gd.alb.data_ptr(),
                                                        out.data_ptr(), stage_ptr, sp), "rtowUpsampleDevice")

                res = timed(stream, args.reps, args.warmup, call)
                guided, demod = mode == G, bool(flags & D)
                nbytes = nd * 12 + ns * 12 + (ns * 20 + nd * 20 if guided else 0) + (ns * 12 + nd * 12 if demod else 0)
                res["bytes_per_dst_pixel"] = nbytes / nd
                res["tb_per_s"] = nbytes / (res["ms_median"] * 1e-3) / 1e12
                if guided:
                    call(stage.data_ptr())
                    stream.synchronize()
                    res["stage_shares"] = [float((stage == k).float().mean()) for k in range(3)]
                row[name] = res
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def quality():
    import denoise_reference as dr
    import test_gpu_upsample as tg
    import upsample_reference as ur
    with rt.Context(0) as ctx:
        size, (c_src, _, _), ref, gs, gd = tg.quality_inputs(rt, ctx)
        (sw, sh), (dw, dh) = size
        mse = lambda x: float(np.mean((x.astype(np.float64) - ref) ** 2))
        point, _, _ = ur.upsample(sw, sh, dw, dh, ur.POINT, 0, 0.0, 0, c_src)
        base = mse(point)
        grid = []
        for flags in (M | D, D, M, 0):
            for sharp in (0, 2, 4, 6):
                for tol in (0.01, 0.05, 0.2):
                    got, stage = tg._device_upsample(rt, ctx, size, c_src, gs, gd, G, sharp, tol, flags)
                    grid.append({"normalSharpness": sharp, "depthTolerance": tol, "flags": flags, "mse_over_point": mse(got) / base,
                                 "stage_shares": [float((stage == k).mean()) for k in range(3)]})
        bil, _ = tg._device_upsample(rt, ctx, size, c_src, gs, gd, B, 0, 0.0, 0)
        bil_d, _ = tg._device_upsample(rt, ctx, size, c_src, gs, gd, B, 0, 0.0, D)
        # the recommended parameters, as the quality test runs them: on the noisy src frame with and without the demodulation, and on a denoised src frame
        rec = (abi.UPSAMPLE_DEFAULT_NORMAL_SHARPNESS, abi.UPSAMPLE_DEFAULT_DEPTH_TOLERANCE)
        got, stage = tg._device_upsample(rt, ctx, size, c_src, gs, gd, G, *rec, abi.UPSAMPLE_DEFAULT_FLAGS)
        plain, _ = tg._device_upsample(rt, ctx, size, c_src, gs, gd, G, *rec, abi.UPSAMPLE_DEFAULT_FLAGS & ~D)
        den = dr.denoise_reference(sw, sh, c_src, gs["normal"], gs["albedo"], abi.DENOISE_DEFAULT_ITERATIONS, abi.DENOISE_DEFAULT_NORMAL_SHARPNESS,
                                   abi.DENOISE_DEFAULT_COLOR_SIGMA, abi.DENOISE_DEFAULT_ALBEDO_SIGMA, abi.DENOISE_DEFAULT_FLAGS)
        den_point, _, _ = ur.upsample(sw, sh, dw, dh, ur.POINT, 0, 0.0, 0, den)
        den_guided, _ = tg._device_upsample(rt, ctx, size, den, gs, gd, G, *rec, abi.UPSAMPLE_DEFAULT_FLAGS)
    recommended = {"normalSharpness": rec[0], "depthTolerance": rec[1], "flags": abi.UPSAMPLE_DEFAULT_FLAGS, "mse_over_point": mse(got) / base,
                   "without_demodulation_over_point": mse(plain) / base, "stage_shares": [float((stage == k).mean()) for k in range(3)],
                   "denoised_src": {"point_mse": mse(den_point), "guided_over_point": mse(den_guided) / mse(den_point)}}
    best = min(grid, key=lambda g: g["mse_over_point"])
    best_both = min((g for g in grid if g["flags"] == M | D), key=lambda g: g["mse_over_point"])      # the recommended values: both flags are what the pass is for
    out = {"what": "cover scene, 16 spp (seed 1) at %d x %d upsampled to %d x %d against 1024 spp (seed 2) there; mean squared error over that of the POINT upsampling"
                   % (sw, sh, dw, dh), "point_mse": base, "bilinear_over_point": mse(bil) / base, "bilinear_demodulated_over_point": mse(bil_d) / base,
           "recommended": recommended, "guided_grid": grid, "best": best, "best_with_both_flags": best_both}
    print(json.dumps({k: v for k, v in out.items() if k != "guided_grid"}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_upsample.json"))
    args = ap.parse_args()
    lib = rt.lib.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    out = {"what": "rtowUpsampleDevice per launch, every mode, on the cover scene's own guides", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "warmup": args.warmup, "timing": "HIP events on the caller's stream around each call; median / min / max of reps",
           "recommended": {"normalSharpness": abi.UPSAMPLE_DEFAULT_NORMAL_SHARPNESS, "depthTolerance": abi.UPSAMPLE_DEFAULT_DEPTH_TOLERANCE,
                           "flags": abi.UPSAMPLE_DEFAULT_FLAGS},
           "rows": timings(args, lib, dev, stream)}
    if not args.no_quality:
        out["quality"] = quality()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
