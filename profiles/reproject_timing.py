"""Device time of rtowReprojectAccumDevice at 1920 x 1080 and 3840 x 2160 on the cover scene: the view of the scene's camera and the same camera after a dolly of 2 % of the
way to its target, both traced with rtowTraceViewDevice, accumulators with sample counts around the recommended maxHistory.  In one process on one GPU.

Each call is bracketed by HIP events on the stream it is enqueued on (torch.cuda.Event, as profiles/trace_rays_timing.py); after `--warmup` untimed calls, `--reps` timed calls
per point: median, minimum and maximum are reported, with the bytes the pass moves per pixel (32 ray + 8 hit + 8 previous hit + 44 gathered + 44 + 4 written = 140) as GB/s.
rtowTraceViewDevice of the new view - the other call a camera move costs - is timed next to it.

    python profiles/reproject_timing.py --out profiles/r07_reproject.json
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
rt = importlib.import_module("raytracing-in-one-weekend_amd")
abi = rt.abi
BYTES_PER_PIXEL = 140


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_reproject.json"))
    args = ap.parse_args()
    lib = rt.lib.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    S = rt.scenes
    scene = S.cover_scene()
    rows = []
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        for w, h in ((1920, 1080), (3840, 2160)):
            n = w * h
            view_a = S.make_view(scene, w, h)
            position, target = np.asarray(scene.camera["position"], np.float64), np.asarray(scene.camera["target"], np.float64)
            scene.camera["position"] = tuple(position + 0.02 * (target - position))
            view_b = S.make_view(scene, w, h)
            scene.camera["position"] = tuple(position)
            f32 = lambda *shape: torch.empty(*shape, device=dev)
            dist, pdist, rays = f32(n), f32(n), f32(n * 8)
            ent, pent, source = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
            gen = torch.Generator(device=dev).manual_seed(1)
            count = torch.randint(1, 129, (n, 1), device=dev, generator=gen).float()
            prev = [torch.cat([torch.rand(n, 3, device=dev, generator=gen) * count, count], 1).contiguous(), (torch.rand(n, 3, device=dev, generator=gen) * count).contiguous(),
                    (torch.rand(n, 3, device=dev, generator=gen) * count).contiguous(), (torch.rand(n, 1, device=dev, generator=gen) * count).contiguous()]
            out = [f32(n, 4), f32(n, 3), f32(n, 3), f32(n)]
            hits, prev_hits = abi.HitBuffers(dist.data_ptr(), ent.data_ptr(), None), abi.HitBuffers(pdist.data_ptr(), pent.data_ptr(), None)
            pb, ob = abi.AccumBuffers(*[x.data_ptr() for x in prev]), abi.AccumBuffers(*[x.data_ptr() for x in out])
            ta, tb = abi.TraceViewParams(w, h, view_a, 0.0, 0), abi.TraceViewParams(w, h, view_b, 0.0, 0)
            rp = abi.ReprojectParams(w, h, view_a, abi.REPROJECT_DEFAULT_DEPTH_TOLERANCE, abi.REPROJECT_DEFAULT_MAX_HISTORY, abi.REPROJECT_DEFAULT_FLAGS, 0)
            stream.wait_stream(torch.cuda.current_stream(dev))
            torch.cuda.synchronize(dev)
            rt.lib.check(lib.rtowTraceViewDevice(ctx.handle, C.byref(ta), C.byref(prev_hits), None, sp), "rtowTraceViewDevice")
            trace = lambda: rt.lib.check(lib.rtowTraceViewDevice(ctx.handle, C.byref(tb), C.byref(hits), rays.data_ptr(), sp), "rtowTraceViewDevice")
            reproject = lambda: rt.lib.check(lib.rtowReprojectAccumDevice(ctx.handle, C.byref(rp), rays.data_ptr(), C.byref(hits), C.byref(prev_hits), C.byref(pb), C.byref(ob),
                                                                          source.data_ptr(), sp), "rtowReprojectAccumDevice")
            tt = timed(stream, args.reps, args.warmup, trace)
            tr = timed(stream, args.reps, args.warmup, reproject)
            carried = float((source >= 0).float().mean().item())
            row = {"width": w, "height": h, "pixels": n, "carried_share": carried, "bytes_per_pixel": BYTES_PER_PIXEL,
                   "reproject": dict(tr, gb_per_s=n * BYTES_PER_PIXEL / (tr["ms_median"] * 1e-3) / 1e9),
                   "trace_view_with_rays": tt}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del dist, pdist, rays, ent, pent, source, prev, out, count
    result = {"what": "rtowReprojectAccumDevice on the cover scene after a 2 % dolly, recommended parameters", "device": torch.cuda.get_device_name(0),
              "reps": args.reps, "warmup": args.warmup, "timing": "HIP events on the caller's stream around each call; median / min / max of reps", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
