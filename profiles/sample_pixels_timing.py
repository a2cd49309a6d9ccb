"""Device time of rtowSamplePixelsDevice against a full-frame rtowSampleBatchDevice on the cover scene: 1920 x 1080, 16 spp, trace depth 8, from zeroed inputs into
separate outputs.  The full frame first; then list launches over 100 % of the pixels and over 1 %, 10 % and 50 % of them, each share two ways - a centred rectangle
(whole 8 x 8 tiles, coherent 64-ticket pulls) and a seeded random mask (the same number of pixels scattered over the frame: what tile-incoherent lists cost) - every
list built by rtowBuildPixelListDevice, which is timed alone as well, into a list whose capacity is the whole frame (what a host that does not know the count
allocates: every list launch then runs one workgroup per CU), and an empty list for the fixed cost.  In one process on one GPU.

Each call is bracketed by HIP events on the stream it is enqueued on (torch.cuda.Event, as profiles/reproject_timing.py), so a list launch's time includes the copy of
the caller's list into the context's and the launch itself; after `--warmup` untimed calls, `--reps` timed calls per point: median, minimum and maximum, and the
ratio of the median to the full-frame launch's.

    python profiles/sample_pixels_timing.py --out profiles/r10_sample_pixels.json
"""
import argparse
import ctypes as C
import importlib
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
rt = importlib.import_module("raytracing-in-one-weekend_amd")
abi = rt.abi


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_sample_pixels.json"))
    args = ap.parse_args()
    lib = rt.lib.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    S = rt.scenes
    scene = S.cover_scene()
    w, h = args.width, args.height
    n = w * h
    rows = []
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        p = S.make_params(scene, w, h, spp=args.spp, trace_depth=args.depth, seed=1)
        f32 = lambda *shape: torch.zeros(*shape, device=dev)
        ins, outs = [f32(n, 4), f32(n, 3), f32(n, 3), f32(n)], [f32(n, 4), f32(n, 3), f32(n, 3), f32(n)]
        bi, bo = abi.AccumBuffers(*[x.data_ptr() for x in ins]), abi.AccumBuffers(*[x.data_ptr() for x in outs])
        words = torch.zeros(4 + n, dtype=torch.int32, device=dev)
        scratch = torch.zeros(abi.pixel_list_scratch_bytes(w, h) // 4, dtype=torch.int32, device=dev)
        lst = abi.PixelList(words.data_ptr(), n)
        params = (abi.SampleParams * 1)(p)
        stream.wait_stream(torch.cuda.current_stream(dev))
        torch.cuda.synchronize(dev)

        full = timed(stream, args.reps, args.warmup,
                     lambda: rt.lib.check(lib.rtowSampleBatchDevice(ctx.handle, C.byref(p), C.byref(bi), C.byref(bo), None, sp, None), "rtowSampleBatchDevice"))
        rows.append(dict({"what": "rtowSampleBatchDevice, full frame", "pixels": n, "share": 1.0}, **full))
        print(json.dumps(rows[-1]), flush=True)

        gen = torch.Generator(device=dev).manual_seed(7)
        noise = torch.rand(n, device=dev, generator=gen)
        cases = [("no pixel (an empty rectangle: the copy of the list and a launch that leaves at once)", 0.0, (8, 8, 8, 8), None), ("every pixel", 1.0, None, None)]
        for share in (0.01, 0.1, 0.5):
            rw, rh = int(round(w * math.sqrt(share) / 8)) * 8, int(round(h * math.sqrt(share) / 8)) * 8
            x0, y0 = (w - rw) // 2 // 8 * 8, (h - rh) // 2 // 8 * 8
            cases.append(("rectangle", share, (x0, y0, x0 + rw, y0 + rh), None))
            k = rw * rh                                             # the same number of pixels, scattered: the k smallest of n random numbers
            mask = torch.zeros(n, dtype=torch.uint8, device=dev)
            mask[torch.topk(noise, k, largest=False).indices] = 1
            cases.append(("random mask", share, None, mask))
        for kind, share, rect, mask in cases:
            x0, y0, x1, y1 = rect if rect else (0, 0, w, h)
            lp = abi.PixelListParams(w, h, x0, y0, x1, y1, 0, 1, 0.0, 0, 0)
            build = lambda: rt.lib.check(lib.rtowBuildPixelListDevice(ctx.handle, C.byref(lp), None, mask.data_ptr() if mask is not None else None, scratch.data_ptr(),
                                                                      C.byref(lst), sp), "rtowBuildPixelListDevice")
            tb = timed(stream, args.reps, args.warmup, build)
            listed = int(words[0].item()) & 0xffffffff
            tl = timed(stream, args.reps, args.warmup,
                       lambda: rt.lib.check(lib.rtowSamplePixelsDevice(ctx.handle, 1, params, C.byref(lst), C.byref(bi), C.byref(bo), None, sp, None), "rtowSamplePixelsDevice"))
            rt.lib.check(lib.rtowGetBatchStatus(ctx.handle), "rtowGetBatchStatus")
            row = {"what": "rtowSamplePixelsDevice, " + kind, "pixels": listed, "share": listed / n, "nominal_share": share, "rectangle": rect,
                   "list_launch": dict(tl, ratio_to_full_frame=tl["ms_median"] / full["ms_median"], per_pixel_cost_ratio=tl["ms_median"] / (full["ms_median"] * listed / n) if listed else None),
                   "builder_alone": tb}
            rows.append(row)
            print(json.dumps(row), flush=True)
    result = {"what": "rtowSamplePixelsDevice and rtowBuildPixelListDevice against a full-frame rtowSampleBatchDevice: cover scene, %d x %d, %d spp, trace depth %d"
                      % (w, h, args.spp, args.depth),
              "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "timing": "HIP events on the caller's stream around each call; median / min / max of reps; a list launch's time includes the copy of the caller's list",
              "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
