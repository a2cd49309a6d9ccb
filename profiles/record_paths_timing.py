"""Device time of rtowRecordPathsDevice on the cover scene at 1920 x 1080, a list of every pixel, traceDepth 8, jitter on, white noise, zeroed accumulators, in one
process on one GPU - SELECT_INDEX with one sample per pixel, with and without `segments`, and SELECT_BRIGHTEST over 16 samples per pixel - next to, in the same run:
a 1-spp and a 16-spp rtowSampleBatchDevice of the same frame, and rtowTraceGuideViewDevice(maxBounces 8) writing hits and rays.

Each point is bracketed by HIP events on the stream it is enqueued on; after `--warmup` untimed calls, `--reps` timed calls per point, the median reported (the
sample batches' first calls also carry the per-scene preparation - camera-ray lists, cost map, threshold probes - which the warm-up absorbs).

    python profiles/record_paths_timing.py --out profiles/r18_record_paths.json
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

W, H, DEPTH = 1920, 1080, 8


def timing(ctx, lib, args):
    S = rt.scenes
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    scene = S.cover_scene()
    ctx.upload_scene(scene.desc())
    n = W * H
    words = torch.from_numpy(np.concatenate([np.array([n, 0, 0, 0], np.uint32), np.arange(n, dtype=np.uint32)]).view(np.int32)).to(dev)
    zeros = [torch.zeros(n * k, device=dev) for k in (4, 3, 3, 1)]
    outs = [torch.empty(n * k, device=dev) for k in (4, 3, 3, 1)]
    diag = torch.empty(n, device=dev)
    summaries = torch.empty(n * C.sizeof(abi.PathSummary) // 4, device=dev)
    segments = torch.empty(n * DEPTH * C.sizeof(abi.PathSegment) // 4, device=dev)
    hit = [torch.empty(n, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n * 3, device=dev)]
    rays = torch.empty(n * 8, device=dev)
    lst = abi.PixelList(words.data_ptr(), n)
    bi, bo = abi.AccumBuffers(*[x.data_ptr() for x in zeros]), abi.AccumBuffers(*[x.data_ptr() for x in outs])
    stream.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize(dev)

    def record(spp, select, with_segments):
        p = S.make_params(scene, W, H, spp=spp, trace_depth=DEPTH, jitter=True)
        rp = abi.RecordPathsParams(select, 0, 0, 0)

        def call():
            rt.lib.check(lib.rtowRecordPathsDevice(ctx.handle, C.byref(p), C.byref(rp), C.byref(lst), zeros[0].data_ptr(), zeros[3].data_ptr(), summaries.data_ptr(),
                                                   segments.data_ptr() if with_segments else None, sp), "rtowRecordPathsDevice")
        return call

    def batch(spp):
        p = S.make_params(scene, W, H, spp=spp, trace_depth=DEPTH, jitter=True)

        def call():
            rt.lib.check(lib.rtowSampleBatchDevice(ctx.handle, C.byref(p), C.byref(bi), C.byref(bo), diag.data_ptr(), sp, None), "rtowSampleBatchDevice")
        return call

    def guide():
        gp = abi.GuideParams(8, 0, 0)
        tv = abi.TraceViewParams(W, H, S.make_view(scene, W, H), 0.0, 0)
        gb = abi.guide_buffers({"distance": hit[0].data_ptr(), "entityIndex": hit[1].data_ptr(), "normal": hit[2].data_ptr(), "rays": rays.data_ptr()})

        def call():
            rt.lib.check(lib.rtowTraceGuideViewDevice(ctx.handle, C.byref(gp), C.byref(tv), C.byref(gb), sp), "rtowTraceGuideViewDevice")
        return call

    points = (("record_index_1spp_segments", record(1, abi.PATH_SELECT_INDEX, True)), ("record_index_1spp_summaries_only", record(1, abi.PATH_SELECT_INDEX, False)),
              ("record_brightest_16spp_segments", record(16, abi.PATH_SELECT_BRIGHTEST, True)), ("sample_batch_1spp", batch(1)), ("sample_batch_16spp", batch(16)),
              ("trace_guide_view_8_bounces", guide()))
    row = {"width": W, "height": H, "pixels": n, "traceDepth": DEPTH}
    for name, call in points:
        med, lo, hi = timed(stream, call, args.warmup, args.reps)
        row[name] = {"ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}
        print(name, json.dumps(row[name]), flush=True)
    stream.synchronize()
    ctx.synchronize()
    s = np.frombuffer(summaries.cpu().numpy().tobytes(), np.dtype(abi.PATH_SUMMARY_DTYPE))
    row["rays_per_pixel_of_the_brightest"] = round(float(s["segmentCount"].mean()), 3)
    row["rays_per_pixel_of_the_16spp_batch"] = round(float(diag.sum().item()) / n, 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = rt.lib.load()
    meta = {"what": "rtowRecordPathsDevice over every pixel of the cover scene at %d x %d, traceDepth %d, next to rtowSampleBatchDevice and rtowTraceGuideViewDevice of the "
                    "same frame; HIP events on the caller's stream, median of %d after %d warm-up calls" % (W, H, DEPTH, args.reps, args.warmup),
            "device": torch.cuda.get_device_name(0), "library": os.path.relpath(rt.lib.LIB_PATH, ROOT)}
    with rt.Context(0) as ctx:
        meta["row"] = timing(ctx, lib, args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(meta, f, indent=None, separators=(",", ":"))
            f.write("\n")


if __name__ == "__main__":
    main()
