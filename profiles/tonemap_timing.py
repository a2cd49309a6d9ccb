"""Device time of rtowMeterExposureDevice and rtowFinalizeToneMappedDevice at 1920 x 1080 and 3840 x 2160, in one process on one GPU, next to rtowFinalizeDevice on the
same buffers in the same run; and what the tone curve is for (`--quality`).

Timing: the cover scene under scenes.synthetic_sky() (an HDR sky with a sun), one sample per pixel, combined on the host into the float3 colour, normal and albedo
rtowFinalizeDevice takes.  rtowFinalizeDevice; rtowFinalizeToneMappedDevice with each curve and a metered state, and CLAMP without the guide pairs; the meter on the
rendered frame and on a constant frame (every pixel in one bin: all 64 lanes of a wave on one LDS word, the histogram's worst case).  Each call bracketed by HIP events
on the stream it is enqueued on; after `--warmup` untimed calls, `--reps` timed calls per point, the median reported, and its ratio to rtowFinalizeDevice's.

Quality (`--quality`): the same scene and sky at 192 x 108, 16 samples per pixel: the share of pixels with a saturated channel (a byte of 255) under CLAMP with
exposure 1 - which is rtowFinalizeDevice - and under ACES_FITTED with the recommended metering.  Recorded figures, not assertions.

    python profiles/tonemap_timing.py --quality --out profiles/r17_tonemap.json

Measured on an MI355X (profiles/r17_tonemap.json), 1920 x 1080 / 3840 x 2160, median of 20: rtowFinalizeDevice 0.0190 / 0.0744 ms; rtowFinalizeToneMappedDevice CLAMP
0.0201 / 0.0796 (1.06 / 1.07 x), ACES_FILM 0.0216 / 0.0841 (1.14 / 1.13 x), ACES_FITTED 0.0230 / 0.0915 (1.21 / 1.23 x), CLAMP without a state 0.0194 / 0.0793, ACES_FITTED
without the guide pairs 0.0142 / 0.0454.  The finalize stream is bound by its instruction count, so what a curve adds shows in full: ACES_FITTED's three correctly
rounded divisions and some sixty multiplies, adds and selects per pixel, next to nine byte conversions of about twenty instructions each, cost 21 to 23 % and no more.  rtowMeterExposureDevice 0.0194 / 0.0338 ms on the rendered frame, 0.0231 / 0.0437
on the constant one (1.19 / 1.29 x).  Quality: 2.57 % of the pixels saturate a channel under CLAMP at exposure 1, none under ACES_FITTED with the recommended metering
(exposure 0.389).
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
sys.path.insert(0, os.path.join(ROOT, "profiles"))
rt = importlib.import_module("raytracing-in-one-weekend_amd")
abi = rt.abi
from denoise_variance_timing import timed  # noqa: E402

CURVES = (("clamp", abi.TONE_CLAMP), ("aces_fitted", abi.TONE_ACES_FITTED), ("aces_film", abi.TONE_ACES_FILM))


def render(ctx, scene, w, h, spp):
    """the float3 colour, normal and albedo of one batch, combined on the host (sum / count; the inputs of the passes, not what is timed)"""
    p = rt.scenes.make_params(scene, w, h, spp=spp, trace_depth=8, seed=1, sky_type=abi.SKY_CUBEMAP)
    out = rt.sample_batch_host(ctx, p)
    count = np.maximum(out["color"][:, 3:4], 1)
    return [np.ascontiguousarray((out[k][:, :3] / count).astype(np.float32)) for k in ("color", "normal", "albedo")]


def exposure_params(w, h):
    return abi.ExposureParams(w, h, abi.EXPOSURE_DEFAULT_LOW_PERMILLE, abi.EXPOSURE_DEFAULT_HIGH_PERMILLE, abi.EXPOSURE_DEFAULT_COMPENSATION, abi.EXPOSURE_DEFAULT_MIN_STOPS,
                              abi.EXPOSURE_DEFAULT_MAX_STOPS, abi.EXPOSURE_DEFAULT_RATE, 0, 0)


def tone_params(n, curve, exposure=1.0):
    return abi.ToneMapParams(n, curve, exposure, 0, (C.c_int32 * 2)(0, 0))


def read_state(state):
    s = abi.ExposureState.from_buffer_copy(state.cpu().numpy().tobytes())
    return {"exposure": s.exposure, "stops": s.stops, "meanLog2": s.meanLog2, "valid": s.valid, "metered": s.metered, "ignored": s.ignored,
            "bins_hit": int(np.count_nonzero(np.ctypeslib.as_array(s.histogram)))}


def timing(ctx, lib, scene, args):
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    rows = []
    for w, h in ((1920, 1080), (3840, 2160)):
        n = w * h
        color, normal, albedo = [torch.from_numpy(x.reshape(-1)).to(dev) for x in render(ctx, scene, w, h, 1)]
        constant = torch.tensor([0.3, 0.6, 0.9], device=dev).repeat(n)
        outs = [torch.empty(n * 4, dtype=torch.uint8, device=dev) for _ in range(3)]
        scratch = torch.empty(abi.exposure_scratch_bytes(), dtype=torch.uint8, device=dev)
        state, state_constant = [torch.zeros(C.sizeof(abi.ExposureState), dtype=torch.uint8, device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        ep = exposure_params(w, h)

        def meter(frame, record):
            def call():
                rt.lib.check(lib.rtowMeterExposureDevice(ctx.handle, C.byref(ep), frame.data_ptr(), scratch.data_ptr(), record.data_ptr(), s), "rtowMeterExposureDevice")
            return call

        def finalize():
            rt.lib.check(lib.rtowFinalizeDevice(ctx.handle, n, color.data_ptr(), normal.data_ptr(), albedo.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                                outs[2].data_ptr(), s), "rtowFinalizeDevice")

        def tone(curve, guides=True, with_state=True):
            p = tone_params(n, curve)

            def call():
                rt.lib.check(lib.rtowFinalizeToneMappedDevice(ctx.handle, C.byref(p), state.data_ptr() if with_state else None, color.data_ptr(),
                                                              normal.data_ptr() if guides else None, albedo.data_ptr() if guides else None, outs[0].data_ptr(),
                                                              outs[1].data_ptr() if guides else None, outs[2].data_ptr() if guides else None, s), "rtowFinalizeToneMappedDevice")
            return call
        points = [("finalize_device", finalize), ("meter_rendered_frame", meter(color, state)), ("meter_constant_frame", meter(constant, state_constant))]
        points += [("tone_mapped_%s" % name, tone(curve)) for name, curve in CURVES]
        points += [("tone_mapped_clamp_no_state", tone(abi.TONE_CLAMP, with_state=False)), ("tone_mapped_aces_fitted_colour_only", tone(abi.TONE_ACES_FITTED, guides=False))]
        base = None
        for name, call in points:
            med, lo, hi = timed(stream, call, args.warmup, args.reps)
            base = med if name == "finalize_device" else base
            row = {"width": w, "height": h, "pass": name, "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "reps": args.reps,
                   "over_finalize_device": round(med / base, 3)}
            if name.startswith("meter"):
                stream.synchronize()
                row["state"] = read_state(state if "rendered" in name else state_constant)
            print(json.dumps(row), flush=True)
            rows.append(row)
        del color, normal, albedo, constant, outs, scratch, state, state_constant
    return rows


def quality(ctx, lib, scene):
    w, h, spp = 192, 108, 16
    n = w * h
    dev = torch.device("cuda:0")
    color, normal, albedo = [torch.from_numpy(x.reshape(-1)).to(dev) for x in render(ctx, scene, w, h, spp)]
    outs = [torch.empty(n * 4, dtype=torch.uint8, device=dev) for _ in range(3)]
    scratch = torch.empty(abi.exposure_scratch_bytes(), dtype=torch.uint8, device=dev)
    state = torch.zeros(C.sizeof(abi.ExposureState), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def saturated(curve, record):
        p = tone_params(n, curve)
        rt.lib.check(lib.rtowFinalizeToneMappedDevice(ctx.handle, C.byref(p), record, color.data_ptr(), normal.data_ptr(), albedo.data_ptr(), outs[0].data_ptr(),
                                                      outs[1].data_ptr(), outs[2].data_ptr(), None), "rtowFinalizeToneMappedDevice")
        ctx.synchronize()
        rgb = outs[0].cpu().numpy().reshape(n, 4)[:, :3]
        return round(float((rgb == 255).any(axis=1).mean()), 4)
    ep = exposure_params(w, h)
    rt.lib.check(lib.rtowMeterExposureDevice(ctx.handle, C.byref(ep), color.data_ptr(), scratch.data_ptr(), state.data_ptr(), None), "rtowMeterExposureDevice")
    ctx.synchronize()
    lum = color.cpu().numpy().reshape(n, 3) @ np.array([0.2126, 0.7152, 0.0722], np.float32)
    return {"protocol": "cover scene under scenes.synthetic_sky(), %d x %d, %d samples per pixel, sum / count on the host; share of pixels with a byte of 255 in a colour "
                        "channel" % (w, h, spp),
            "luminance_min_median_max": [round(float(x), 4) for x in (lum.min(), np.median(lum), lum.max())], "pixels_with_a_channel_above_1": round(float((color.cpu().numpy().reshape(n, 3) > 1).any(axis=1).mean()), 4),
            "saturated_share_clamp_exposure_1": saturated(abi.TONE_CLAMP, None),
            "saturated_share_aces_fitted_exposure_1": saturated(abi.TONE_ACES_FITTED, None),
            "saturated_share_aces_film_recommended_metering": saturated(abi.TONE_ACES_FILM, state.data_ptr()),
            "saturated_share_clamp_recommended_metering": saturated(abi.TONE_CLAMP, state.data_ptr()),
            "saturated_share_aces_fitted_recommended_metering": saturated(abi.TONE_ACES_FITTED, state.data_ptr()),
            "metered_state": read_state(state)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = rt.lib.load()
    meta = {"what": "rtowMeterExposureDevice and rtowFinalizeToneMappedDevice next to rtowFinalizeDevice on the same buffers, HIP events on the caller's stream, median of "
                    "%d after %d warm-up calls" % (args.reps, args.warmup), "device": torch.cuda.get_device_name(0), "library": os.path.relpath(rt.lib.LIB_PATH, ROOT)}
    scene = rt.scenes.cover_scene()
    sky = rt.scenes.synthetic_sky()
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        ctx.upload_sky_cubemap(sky.desc())
        if not args.no_timing:
            meta["rows"] = timing(ctx, lib, scene, args)
        if args.quality:
            meta["quality"] = quality(ctx, lib, scene)
            print(json.dumps(meta["quality"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(meta, f, indent=None, separators=(",", ":"))
            f.write("\n")


if __name__ == "__main__":
    main()
