"""Device time of rtowRectifyHistoryDevice at 1920 x 1080 and 3840 x 2160, radius 1 / 2 / 3, in one process on one GPU, next to rtowEstimateMomentsDevice with every
pixel qualifying (the same staging, 49 taps); and the parameter grid behind the recommended values.

Timing: the cover scene, its camera and the camera after a 2 % dolly; rtowTraceViewDevice at both views, rtowReprojectAccumDevice with its recommended values carries a
synthetic history of 64 samples per pixel (its holes are the pixels without history).  Three cases, out of place with moments, outKeep and outStats: no valid history
(zeroed accumulators: every tile leaves early), every pixel judged (the synthetic history itself, minTaps 2), the history the reprojection left.  Fresh colour: 4
samples per pixel of the history's colour with noise, so that all three outcomes occur.  Each call bracketed by HIP events on the stream it is enqueued on; after
`--warmup` untimed calls, `--reps` timed calls per point, the median reported.

Quality (`--quality`): tests/test_gpu_rectify_history.py's RectifyFrame (cover scene, 192 x 108, seeds 0 / 1000 / 2000; view A 16 x 4 spp with moments, a move, 4 x 1
spp of the new view; against 1024 spp) for its two moves, the 2 % dolly and the orbit.  Per move and seed the squared luminance error of the carried, the rectified
and the restarted frame, over all pixels, the pixels whose first hit is metal or glass and the rest, before and after rtowDenoiseVarianceDevice; the rectified frame
over the grid sigmaScale x relativeTolerance x radius x minTaps (guides as rtowEstimateMomentsDevice's recommended set).  The chosen point has the smallest sum, over
both moves and averaged over the seeds, of (rectified / carried) on the specular pixels and (rectified / carried) on the rest.

    python profiles/rectify_history_timing.py --quality --out profiles/r15_rectify_history.json
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
rt = importlib.import_module("raytracing-in-one-weekend_amd")
abi = rt.abi
from denoise_variance_timing import timed  # noqa: E402

GRID_SIGMA_SCALE = (0.5, 1.0, 2.0, 4.0)
GRID_RELATIVE_TOLERANCE = (0.0, 0.125, 0.25, 0.5)
GRID_RADIUS = (1, 2, 3)
GRID_MIN_TAPS = (2, 4, 9)


def timing(ctx, lib, args):
    import reproject_reference as rr
    S = rt.scenes
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    scene = S.cover_scene()
    ctx.upload_scene(scene.desc())
    rows = []
    for w, h in ((1920, 1080), (3840, 2160)):
        n = w * h
        pa = S.make_params(scene, w, h, spp=1, trace_depth=8, seed=1)
        cam = scene.camera
        position, target = np.asarray(cam["position"], np.float64), np.asarray(cam["target"], np.float64)
        focus = S.focus_distance(scene, np.asarray(cam["position"], np.float32), S._normalize(np.asarray(cam["target"], np.float32) - np.asarray(cam["position"], np.float32)))
        view_b = rr.make_view(tuple(position + 0.02 * (target - position)), tuple(target), w, h, vfov=cam["vfov"], focus=focus, up=tuple(cam["up"]))
        hits_a = ctx.trace_view(pa.view, w, h, want=("distance", "entityIndex"))
        hits_b = ctx.trace_view(view_b, w, h, want_rays=True)
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.float32).reshape(-1) if x.dtype != np.int32 else np.ascontiguousarray(x)).to(dev)
        rng = np.random.default_rng(3)
        base = rng.uniform(0.1, 2, (n, 3))
        shift = np.where(rng.random(n) < 0.7, 1.0, rng.uniform(1.2, 6.0, n))                       # three pixels in ten carry a mean the fresh samples refute
        history = np.concatenate([base * shift[:, None] * 64, np.full((n, 1), 64.0)], axis=1).astype(np.float32)
        fresh = np.concatenate([np.abs(base * (1 + 0.3 * rng.normal(size=(n, 3)))) * 4, np.full((n, 1), 4.0)], axis=1).astype(np.float32)
        lum = 0.2126 * history[:, 0] + 0.7152 * history[:, 1] + 0.0722 * history[:, 2]
        m16 = np.stack([lum / 4, (lum / 64) ** 2 * 16 + 0.5, np.full(n, 16.0)], axis=1).astype(np.float32)
        d = {"rays": t(hits_b["rays"]), "t": t(hits_b["distance"]), "e": t(hits_b["entityIndex"]), "n": t(hits_b["normal"]), "pt": t(hits_a["distance"]),
             "pe": t(hits_a["entityIndex"]), "history": t(history), "fresh": t(fresh), "m16": t(m16)}
        synthetic = [d["history"], torch.ones(n * 3, device=dev), torch.ones(n * 3, device=dev), torch.ones(n, device=dev)]
        carried = [torch.empty(n * 4, device=dev), torch.empty(n * 3, device=dev), torch.empty(n * 3, device=dev), torch.empty(n, device=dev)]
        zeros = [torch.zeros(n * 4, device=dev), torch.zeros(n * 3, device=dev), torch.zeros(n * 3, device=dev), torch.zeros(n, device=dev)]
        outs = [torch.empty(n * 4, device=dev), torch.empty(n * 3, device=dev), torch.empty(n * 3, device=dev), torch.empty(n, device=dev)]
        src = torch.empty(n, dtype=torch.int32, device=dev)
        out_m, keep, est = torch.empty(n * 3, device=dev), torch.empty(n, device=dev), torch.empty(n * 3, device=dev)
        stats = torch.zeros(4, dtype=torch.int32, device=dev)
        filled = torch.empty(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        s = stream.cuda_stream
        rp = abi.ReprojectParams(w, h, pa.view, abi.REPROJECT_DEFAULT_DEPTH_TOLERANCE, abi.REPROJECT_DEFAULT_MAX_HISTORY, abi.REPROJECT_DEFAULT_FLAGS, 0)
        hb, hp = abi.HitBuffers(d["t"].data_ptr(), d["e"].data_ptr(), None), abi.HitBuffers(d["pt"].data_ptr(), d["pe"].data_ptr(), None)
        ab = lambda bufs: abi.AccumBuffers(*[x.data_ptr() for x in bufs])
        ab_syn, ab_car, ab_zero, ab_out = ab(synthetic), ab(carried), ab(zeros), ab(outs)
        rt.lib.check(lib.rtowReprojectAccumDevice(ctx.handle, C.byref(rp), d["rays"].data_ptr(), C.byref(hb), C.byref(hp), C.byref(ab_syn), C.byref(ab_car),
                                                  src.data_ptr(), s), "rtowReprojectAccumDevice")
        stream.synchronize()
        holes = float((src < 0).float().mean().item())
        hits = abi.HitBuffers(d["t"].data_ptr(), d["e"].data_ptr(), d["n"].data_ptr())

        def rectify(radius, history_ab):
            p = abi.RectifyParams(w, h, radius, 2, abi.RECTIFY_DEFAULT_NORMAL_SHARPNESS, abi.RECTIFY_DEFAULT_DEPTH_TOLERANCE, abi.RECTIFY_DEFAULT_SIGMA_SCALE,
                                  abi.RECTIFY_DEFAULT_RELATIVE_TOLERANCE, abi.RECTIFY_DEFAULT_FLAGS, 0)

            def call():
                rt.lib.check(lib.rtowRectifyHistoryDevice(ctx.handle, C.byref(p), C.byref(history_ab), d["fresh"].data_ptr(), C.byref(hits), d["m16"].data_ptr(),
                                                          C.byref(ab_out), out_m.data_ptr(), keep.data_ptr(), stats.data_ptr(), s), "rtowRectifyHistoryDevice")
            return call
        ep = abi.EstimateMomentsParams(w, h, abi.ESTIMATE_MOMENTS_DEFAULT_MIN_BATCHES, abi.ESTIMATE_MOMENTS_DEFAULT_MIN_TAPS, abi.ESTIMATE_MOMENTS_DEFAULT_NORMAL_SHARPNESS,
                                       abi.ESTIMATE_MOMENTS_DEFAULT_DEPTH_TOLERANCE, abi.ESTIMATE_MOMENTS_DEFAULT_FLAGS, 0)

        def estimate_all():
            rt.lib.check(lib.rtowEstimateMomentsDevice(ctx.handle, C.byref(ep), d["fresh"].data_ptr(), C.byref(hits), None, est.data_ptr(), filled.data_ptr(), s),
                         "rtowEstimateMomentsDevice")
        points = []
        for radius in (1, 2, 3):
            points += [("rectify_no_valid_history_r%d" % radius, rectify(radius, ab_zero)), ("rectify_every_pixel_judged_r%d" % radius, rectify(radius, ab_syn)),
                       ("rectify_history_of_a_2_percent_dolly_r%d" % radius, rectify(radius, ab_car))]
        points.append(("estimate_moments_all_qualifying", estimate_all))
        for name, call in points:
            med, lo, hi = timed(stream, call, args.warmup, args.reps)
            row = {"width": w, "height": h, "pass": name, "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "reps": args.reps}
            if name.startswith("rectify"):
                stream.synchronize()
                row["judged_kept_cut_dropped"] = [int(x) for x in stats.cpu().numpy().view(np.uint32)]
                if "dolly" in name:
                    row["pixels_without_history"] = round(holes, 4)
            print(json.dumps(row), flush=True)
            rows.append(row)
        del d, synthetic, carried, zeros, outs, src, out_m, keep, est, stats, filled
    return rows


def quality(ctx):
    import test_gpu_rectify_history as tg
    guides = (abi.RECTIFY_DEFAULT_NORMAL_SHARPNESS, abi.RECTIFY_DEFAULT_DEPTH_TOLERANCE)
    flags = abi.RECTIFY_DEFAULT_FLAGS
    grid = [(sigma, rel, radius, taps) for sigma in GRID_SIGMA_SCALE for rel in GRID_RELATIVE_TOLERANCE for radius in GRID_RADIUS for taps in GRID_MIN_TAPS]
    cfg_of = lambda point: (point[2], point[3]) + guides + (point[0], point[1], flags)
    recommended = (abi.RECTIFY_DEFAULT_SIGMA_SCALE, abi.RECTIFY_DEFAULT_RELATIVE_TOLERANCE, abi.RECTIFY_DEFAULT_RADIUS, abi.RECTIFY_DEFAULT_MIN_TAPS)
    if recommended not in grid:
        grid.append(recommended)
    frames, ratios = [], {move: {p: [] for p in grid} for move in tg.MOVES}      # ratios[move][point] = per seed [specular, rest, all, and the three after denoising]
    for move in tg.MOVES:
        for seed in tg.SEEDS:
            frame = tg.RectifyFrame(rt, ctx, seed, move)
            try:
                fixed = {}
                for kind in ("carried", "restarted"):
                    noisy, den, _ = frame.frame(kind)
                    fixed[kind] = (frame.errors(noisy), frame.errors(den))
                base = fixed["carried"]
                for point in grid:
                    noisy, den, stats = frame.frame(cfg_of(point))
                    e, ed = frame.errors(noisy), frame.errors(den)
                    ratios[move][point].append([e[1] / base[0][1], e[2] / base[0][2], e[0] / base[0][0], ed[1] / base[1][1], ed[2] / base[1][2], ed[0] / base[1][0],
                                                stats.judged, stats.kept, stats.cut, stats.dropped])
                frames.append({"move": move, "seed": seed, "pixels_carried": round(frame.carried_share, 4), "specular_share": round(float(frame.specular.mean()), 4),
                               "mse_columns": ["all", "specular", "rest"],
                               "carried": list(fixed["carried"][0]), "carried_denoised": list(fixed["carried"][1]),
                               "restarted": list(fixed["restarted"][0]), "restarted_denoised": list(fixed["restarted"][1]),
                               "restarted_over_carried": [fixed["restarted"][0][k] / base[0][k] for k in range(3)],
                               "restarted_over_carried_denoised": [fixed["restarted"][1][k] / base[1][k] for k in range(3)]})
            finally:
                frame.free()
    mean = lambda move, point, col: float(np.mean([r[col] for r in ratios[move][point]]))
    total = lambda point: sum(mean(move, point, 0) + mean(move, point, 1) for move in tg.MOVES)
    best = min(grid, key=total)

    def describe(point):
        out = {"sigmaScale": point[0], "relativeTolerance": point[1], "radius": point[2], "minTaps": point[3], "ratio_sum": round(total(point), 4)}
        for move in tg.MOVES:
            rows = ratios[move][point]
            out[move] = {"columns": ["specular", "rest", "all", "specular_denoised", "rest_denoised", "all_denoised"],
                         "mean": [round(mean(move, point, c), 4) for c in range(6)], "per_seed": [[round(x, 4) for x in r[:6]] for r in rows],
                         "judged_kept_cut_dropped_per_seed": [r[6:] for r in rows]}
        return out
    sums = [total(p) for p in grid]
    return {"protocol": "cover scene, 192 x 108, seeds 0 / 1000 / 2000: view A 16 x 4 spp (seeds seed + 1 ..) with moments; dolly = 2 %% of the way to the target, orbit = "
                        "%g degrees about the target around the up axis; accumulators and moments reprojected (recommended); 4 x 1 spp (seeds seed + 201 ..) of the new "
                        "view from zero; against 1024 spp of the new view (seed + 9).  Squared luminance error of (a) carried history plus the fresh sums, (b) rectified "
                        "history plus the fresh sums, (c) the fresh sums alone; ratios are (b) / (a); specular = first hit is a dielectric or metallic >= 0.5 "
                        "(rtowShadeHitsDevice); denoised = rtowDenoiseVarianceDevice's recommended set with the frame's own moments (carried / rectified / restarted, the "
                        "fresh batches accumulated on top, rtowEstimateMomentsDevice's recommended set)" % tg.ORBIT_DEGREES,
            "orbit_degrees": tg.ORBIT_DEGREES, "frames": frames,
            "grid": {"sigmaScale": GRID_SIGMA_SCALE, "relativeTolerance": GRID_RELATIVE_TOLERANCE, "radius": GRID_RADIUS, "minTaps": GRID_MIN_TAPS,
                     "normalSharpness": guides[0], "depthTolerance": guides[1], "flags": flags},
            "grid_columns": ["sigmaScale", "relativeTolerance", "radius", "minTaps", "dolly_specular", "dolly_rest", "orbit_specular", "orbit_rest", "ratio_sum"],
            "grid_rows": [list(p) + [round(mean("dolly", p, 0), 4), round(mean("dolly", p, 1), 4), round(mean("orbit", p, 0), 4), round(mean("orbit", p, 1), 4),
                                     round(total(p), 4)] for p in grid],
            "ratio_sum_range": [round(min(sums), 4), round(max(sums), 4)],
            "chosen_smallest_ratio_sum": describe(best), "recommended_set_in_abi": describe(recommended)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = rt.lib.load()
    meta = {"what": "rtowRectifyHistoryDevice next to rtowEstimateMomentsDevice with every pixel qualifying, HIP events on the caller's stream, median of %d after %d "
                    "warm-up calls" % (args.reps, args.warmup), "device": torch.cuda.get_device_name(0), "library": os.path.relpath(rt.lib.LIB_PATH, ROOT)}
    with rt.Context(0) as ctx:
        if not args.no_timing:
            meta["rows"] = timing(ctx, lib, args)
        if args.quality:
            meta["quality"] = quality(ctx)
            print(json.dumps({k: v for k, v in meta["quality"].items() if not k.startswith("grid_")}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(meta, f, indent=None, separators=(",", ":"))
            f.write("\n")


if __name__ == "__main__":
    main()
