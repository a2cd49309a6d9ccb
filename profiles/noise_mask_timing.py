"""Device time of rtowNoiseMaskDevice at 1920 x 1080 and 3840 x 2160 in one process on one GPU, next to rtowReprojectMomentsDevice and rtowAccumulateMomentsDevice
with count 1 (passes of similar traffic, timed in the same run); and the parameter grid behind the recommended values (abi.NOISE_MASK_DEFAULT_*).

Timing: synthetic moments of 4 batches (means uniform in 0..2, deviations uniform in 0..1, one pixel in 64 without an estimate), so that the error spreads over a dozen
histogram bins as it does on a rendered frame; the pass without and with a budget (a quarter of the frame: the clear, the counting pass, the pick step and the masking
pass), dilate 0 and 3, with outError and outStats and with the mask alone; the gather over a source map that shifts the frame by one row; each call bracketed by HIP
events on the stream it is enqueued on; after `--warmup` untimed calls, `--reps` timed calls per point, the median reported.

Quality (`--quality`): tests/test_gpu_noise_mask.py's AdaptiveFrame - the cover scene at 192 x 108, 8 x 2 spp as a group with moments, then 4 refinement rounds of 4
list batches of 2 spp (rt.refine_noisy_pixels) - on three seeds, against 1024 spp.  The refined frame is compared with a uniform frame that got at least as many
samples in all, rounded up to whole batches, so the comparison never favours the feature.  Two ratios, refined over uniform: the squared error of the luminance, and
its relative squared error err^2 / (ref^2 + 2^-12).  Both error kinds; errorThreshold {0.0025, 0.01, 0.04} x luminanceFloor {2^-8, 2^-6, 2^-4} (relative only) x
dilate {0, 1, 2} x budget {n / 8, n / 4, n / 2}, UNKNOWN_QUALIFIES set.  The chosen point has the smallest sum of the two ratios, averaged over the seeds.

With `--ab-lib LABEL=PATH` (repeatable) the timing runs again in a child process that loads the library at PATH: builds of the same source with another cap on the
number of workgroups (kMaxBlocks in csrc/rtow_noise_mask.hip), which trades the statistics' device-wide atomics against the latency a workgroup's tile loop can hide.

    python profiles/noise_mask_timing.py --quality --out profiles/r14_noise_mask.json
"""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
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

GRID_THRESHOLD = (0.0025, 0.01, 0.04)
GRID_FLOOR = (2.0 ** -8, 2.0 ** -6, 2.0 ** -4)
GRID_DILATE = (0, 1, 2)
GRID_BUDGET_DIVISOR = (8, 4, 2)
START = (0, 0.01, 2.0 ** -6, 1, 4)          # relative, errorThreshold, luminanceFloor, dilate, budget divisor
SEEDS = (0, 1000, 2000)
ROUNDS, BATCHES = 4, 4


def timing(ctx, lib, args):
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    rows = []
    for w, h in ((1920, 1080), (3840, 2160)):
        n = w * h
        rng = np.random.default_rng(1)
        mean, spread = rng.uniform(0, 2, n).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32)
        m = np.stack([4 * mean, 4 * (mean * mean + spread * spread), np.full(n, 4, np.float32)], axis=1).astype(np.float32)
        m[::64, 2] = 1
        moments = torch.from_numpy(m.reshape(-1)).to(dev)
        color = torch.from_numpy(np.concatenate([rng.uniform(0, 2, (n, 3)) * 4, np.full((n, 1), 4.0)], axis=1).astype(np.float32).reshape(-1)).to(dev)
        source = torch.from_numpy(((np.arange(n, dtype=np.int64) + w) % n).astype(np.int32)).to(dev)
        mask, error = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, device=dev)
        stats, scratch = torch.empty(72, dtype=torch.int32, device=dev), torch.empty(72, dtype=torch.int32, device=dev)
        carried = torch.empty(n * 3, device=dev)
        torch.cuda.synchronize()
        s = stream.cuda_stream

        def noise(dilate, budget, full):
            p = abi.NoiseMaskParams(w, h, abi.NOISE_MASK_DEFAULT_ERROR_THRESHOLD, abi.NOISE_MASK_DEFAULT_LUMINANCE_FLOOR, dilate, budget, abi.NOISE_MASK_UNKNOWN_QUALIFIES, 0)

            def call():
                rt.lib.check(lib.rtowNoiseMaskDevice(ctx.handle, C.byref(p), moments.data_ptr(), mask.data_ptr(), error.data_ptr() if full else None,
                                                     stats.data_ptr() if full else None, scratch.data_ptr(), s), "rtowNoiseMaskDevice")
            return call

        def gather():
            rt.lib.check(lib.rtowReprojectMomentsDevice(ctx.handle, n, source.data_ptr(), moments.data_ptr(), abi.REPROJECT_MOMENTS_DEFAULT_MAX_BATCHES, carried.data_ptr(), s),
                         "rtowReprojectMomentsDevice")
        one = (C.c_void_p * 1)(color.data_ptr())

        def moments_one():
            rt.lib.check(lib.rtowAccumulateMomentsDevice(ctx.handle, n, 1, one, carried.data_ptr(), carried.data_ptr(), s), "rtowAccumulateMomentsDevice")
        points = [("noise_mask_dilate_%d_%s%s" % (d, "budget" if b else "no_budget", "" if full else "_mask_only"), noise(d, b, full))
                  for full in (True, False) for b in (0, n // 4) for d in (0, 3)]
        points += [("reproject_moments", gather), ("accumulate_moments_count_1", moments_one)]
        for name, call in points:
            med, lo, hi = timed(stream, call, args.warmup, args.reps)
            row = {"width": w, "height": h, "pass": name, "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "reps": args.reps}
            if name.startswith("noise_mask") and not name.endswith("mask_only"):
                stream.synchronize()
                st = stats.cpu().numpy().view(np.uint32)
                row.update(known=int(st[0]), unknown=int(st[1]), qualifying=int(st[2]), masked=int(st[3]), threshold=float(st[4:5].view(np.float32)[0]),
                           bins_in_use=int((st[8:] > 0).sum()))
            print(json.dumps(row), flush=True)
            rows.append(row)
        del moments, color, source, mask, error, stats, scratch, carried
    return rows


def quality(ctx, args):
    import test_gpu_noise_mask as tg
    w, h = 192, 108
    n = w * h
    points = [(0, t, f, d, b) for t in GRID_THRESHOLD for f in GRID_FLOOR for d in GRID_DILATE for b in GRID_BUDGET_DIVISOR]
    points += [(1, t, 0.0, d, b) for t in GRID_THRESHOLD for d in GRID_DILATE for b in GRID_BUDGET_DIVISOR]
    if args.quick:
        points = [START, (1, 0.01, 0.0, 1, 4)]
    per_point = {p: [] for p in points}
    base = []
    for seed in SEEDS:
        frame = tg.AdaptiveFrame(rt, ctx, w, h, seed=seed, most=ROUNDS * BATCHES)
        reference = frame.reference()
        first_abs, first_rel = tg.error_ratios(frame.acc, frame.acc, reference)
        err = (tg.luminance_of(frame.acc[0]) - reference) ** 2
        base.append({"seed": seed, "first_group_squared_error": float(err.mean()), "first_group_samples": float(frame.acc[0][:, 3].sum())})
        assert first_abs == 1.0 and first_rel == 1.0
        for p in points:
            absolute, threshold, floor, dilate, divisor = p
            acc, _, log = frame.refine(ROUNDS, BATCHES, ErrorThreshold=threshold, LuminanceFloor=floor, Dilate=dilate, MaxQualifying=n // divisor,
                                       Flags=abi.NOISE_MASK_UNKNOWN_QUALIFIES | (abi.NOISE_MASK_ABSOLUTE if absolute else 0))
            spent = float(acc[0][:, 3].astype(np.float64).sum())
            uniform, uniform_spent = frame.uniform(spent)
            assert uniform_spent >= spent
            r_abs, r_rel = tg.error_ratios(acc, uniform, reference)
            per_point[p].append([r_abs, r_rel, spent, uniform_spent, [int(s.qualifying) for s, _ in log], [int(l) for _, l in log]])
    mean = lambda p, k: float(np.mean([x[k] for x in per_point[p]]))
    score = lambda p: mean(p, 0) + mean(p, 1)
    best = min(points, key=score)

    def describe(p):
        return {"absolute": p[0], "errorThreshold": p[1], "luminanceFloor": p[2], "dilate": p[3], "budget": "n / %d" % p[4],
                "squared_error_ratio_mean": round(mean(p, 0), 4), "relative_squared_error_ratio_mean": round(mean(p, 1), 4),
                "squared_error_ratio_per_seed": [round(x[0], 4) for x in per_point[p]], "relative_squared_error_ratio_per_seed": [round(x[1], 4) for x in per_point[p]],
                "samples_refined_per_seed": [x[2] for x in per_point[p]], "samples_uniform_per_seed": [x[3] for x in per_point[p]],
                "qualifying_per_round_seed_0": per_point[p][0][4], "listed_per_round_seed_0": per_point[p][0][5]}
    recommended = (1 if abi.NOISE_MASK_DEFAULT_FLAGS & abi.NOISE_MASK_ABSOLUTE else 0, abi.NOISE_MASK_DEFAULT_ERROR_THRESHOLD,
                   0.0 if abi.NOISE_MASK_DEFAULT_FLAGS & abi.NOISE_MASK_ABSOLUTE else abi.NOISE_MASK_DEFAULT_LUMINANCE_FLOOR, abi.NOISE_MASK_DEFAULT_DILATE,
                   abi.NOISE_MASK_DEFAULT_BUDGET_DIVISOR)
    sums = [score(p) for p in points]
    return {"what": "cover scene %d x %d, seeds %s, 8 x 2 spp with moments, then %d rounds of %d list batches of 2 spp; refined over a uniform frame with at least as many "
                    "samples in all (whole batches), against 1024 spp; squared error of the luminance and its relative squared error err^2 / (ref^2 + 2^-12)"
                    % (w, h, list(SEEDS), ROUNDS, BATCHES),
            "first_group": base,
            "grid_columns": ["absolute", "errorThreshold", "luminanceFloor", "dilate", "budget_divisor", "squared_error_ratio_mean", "relative_squared_error_ratio_mean",
                             "squared_error_ratio_max_over_seeds", "relative_squared_error_ratio_max_over_seeds", "samples_refined_seed_0"],
            "grid": [list(p) + [round(mean(p, 0), 4), round(mean(p, 1), 4), round(max(x[0] for x in per_point[p]), 4), round(max(x[1] for x in per_point[p]), 4),
                                per_point[p][0][2]] for p in points],
            "ratio_sum_range": [round(min(sums), 4), round(max(sums), 4)],
            "points_with_both_ratios_below_0.95_on_every_seed": sum(1 for p in points if all(x[0] < 0.95 and x[1] < 0.95 for x in per_point[p])),
            "chosen_smallest_ratio_sum": describe(best), "starting_point": describe(START),
            "recommended_set_in_abi": describe(recommended) if recommended in per_point else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--quick", action="store_true", help="with --quality: the starting point and its ABSOLUTE twin only")
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--ab-lib", action="append", default=[], metavar="LABEL=PATH",
                    help="an A/B build of the library (the same source with another cap on the workgroups of the tile kernel): its timings are recorded next to the shipped library's")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = rt.lib.load()
    meta = {"what": "rtowNoiseMaskDevice next to rtowReprojectMomentsDevice and rtowAccumulateMomentsDevice (count 1), HIP events on the caller's stream, median of %d "
                    "after %d warm-up calls" % (args.reps, args.warmup), "device": torch.cuda.get_device_name(0), "library": os.path.relpath(rt.lib.LIB_PATH, ROOT)}
    with rt.Context(0) as ctx:
        if not args.no_timing:
            meta["rows"] = timing(ctx, lib, args)
        if args.quality:
            meta["quality"] = quality(ctx, args)
            print(json.dumps({k: v for k, v in meta["quality"].items() if k != "grid"}), flush=True)
    for item in args.ab_lib if not args.no_timing else []:
        label, path = item.split("=", 1)
        env = dict(os.environ, RTOW_LIB_PATH=os.path.abspath(path))
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--warmup", str(args.warmup)], env=env, capture_output=True, text=True,
                              timeout=300)
        assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
        rows = [json.loads(l) for l in proc.stdout.splitlines() if l.startswith("{") and '"pass"' in l]
        meta.setdefault("ab_rows", []).append({"label": label, "what": "the same source built with `constexpr unsigned kMaxBlocks = %s` in csrc/rtow_noise_mask.hip; same box, "
                                               "same run" % label, "rows": rows})
        for r in rows:
            if r["pass"].startswith("noise_mask") and not r["pass"].endswith("mask_only"):
                print(json.dumps(dict({k: r[k] for k in ("width", "height", "pass", "ms_median")}, library=label)), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(meta, f, indent=None, separators=(",", ":"))
            f.write("\n")


if __name__ == "__main__":
    main()
