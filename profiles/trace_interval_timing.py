"""Time per launch of rtowTraceRaysIntervalDevice / rtowTraceOcclusionDevice at 1920 x 1080 on the cover scene, 10 000 spheres and the 3 842-triangle mesh (mesh_scene(3)), on the
view's own rays (rtowTraceViewDevice's outRays) and on the same rays in shuffled (incoherent) order.  In one process on one GPU.  Per scene and order:

  * `nearest_null` next to `trace_rays`: the interval call with NULL intervals and rtowTraceRaysDevice on the same rays - the same results bit for bit, so the
    difference is what the interval form costs; the two calls ALTERNATE inside one timing loop;
  * `occlusion_null`: rtowTraceOcclusionDevice on the same rays - any-hit against the nearest walk, same rays, same (0, +inf);
  * `occlusion_segments`: segments from every first hit towards one fixed point L above the scene (origin = the hit point, direction = L - origin, interval
    (--segment-tmin, 1)); rays that missed carry an interval that is not traced; `nearest_segments` is the nearest form on those segments; each in a loop of its
    own, and once more alternating in one loop (`*_alternating`: every occlusion launch then follows a launch that wrote 20 bytes per ray);
  * `second_layer`: the nearest form on the view's rays with tMin = the next float above the first distance, tMax +inf (rays that missed: tMin = +inf).

Each call is bracketed by HIP events on the stream it is enqueued on (torch.cuda.Event, as profiles/trace_rays_timing.py); after `--warmup` untimed calls, `--reps`
timed calls per point: median, minimum and maximum.  The nearest forms write all three hit buffers.

    python profiles/trace_interval_timing.py --out profiles/r08_trace_interval.json
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


def timed(stream, reps, warmup, calls):
    """`calls`: {name: callable}; they alternate inside the loop, each between its own pair of events"""
    for _ in range(warmup):
        for call in calls.values():
            call()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for k in calls}
    for i in range(reps):
        for k, call in calls.items():
            a, b = ev[k][i]
            a.record(stream)
            call()
            b.record(stream)
    stream.synchronize()
    out = {}
    for k in calls:
        ms = sorted(a.elapsed_time(b) for a, b in ev[k])
        out[k] = {"ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--segment-tmin", type=float, default=1e-3, help="tMin of the occlusion segments, in units of (L - origin): keeps a segment off the surface it leaves")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_trace_interval.json"))
    args = ap.parse_args()
    lib = rt.lib.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    w, h = args.width, args.height
    n = w * h
    S = rt.scenes
    rows = []
    for name, make in (("cover", S.cover_scene), ("stress_10000", lambda: S.stress_scene(count=10000)), ("mesh_3", lambda: S.mesh_scene(3))):
        scene = make()
        view = S.make_view(scene, w, h)
        with rt.Context(0) as ctx:
            ctx.upload_scene(scene.desc())
            dist = torch.empty(n, device=dev)
            ent = torch.empty(n, dtype=torch.int32, device=dev)
            nrm = torch.empty(n * 3, device=dev)
            occ = torch.empty(n, dtype=torch.uint8, device=dev)
            view_rays = torch.empty(n * 8, device=dev)
            hits = abi.HitBuffers(dist.data_ptr(), ent.data_ptr(), nrm.data_ptr())
            p = abi.TraceViewParams(w, h, view, 0.0, 0)
            stream.wait_stream(torch.cuda.current_stream(dev))
            sp = C.c_void_p(stream.cuda_stream)
            rt.lib.check(lib.rtowTraceViewDevice(ctx.handle, C.byref(p), C.byref(hits), view_rays.data_ptr(), sp), "rtowTraceViewDevice")
            stream.synchronize()
            view_rays = view_rays.reshape(n, 8)
            first = dist.clone()
            hit = ent >= 0
            # segments towards one fixed point above the scene; a ray that missed gets an interval that is not traced
            target = torch.tensor(scene.camera["target"], dtype=torch.float32, device=dev)
            light = target + torch.tensor([3.0, 8.0, 2.0], device=dev)
            origin = view_rays[:, 0:3] + torch.where(hit, first, torch.zeros_like(first))[:, None] * view_rays[:, 4:7]
            seg_rays = torch.zeros(n, 8, device=dev)
            seg_rays[:, 0:3] = origin
            seg_rays[:, 4:7] = light[None, :] - origin
            seg_iv = torch.empty(n, 2, device=dev)
            seg_iv[:, 0] = torch.where(hit, torch.full_like(first, args.segment_tmin), torch.full_like(first, 1.0))
            seg_iv[:, 1] = torch.where(hit, torch.full_like(first, 1.0), torch.full_like(first, 0.0))
            layer_iv = torch.stack([torch.nextafter(first, torch.full_like(first, float("inf"))), torch.full_like(first, float("inf"))], dim=1).contiguous()
            perm = torch.from_numpy(np.random.default_rng(5).permutation(n)).to(dev)
            torch.cuda.synchronize(dev)
            row = {"scene": name, "entities": scene.entity_count, "rays": n, "hit_share": float(hit.float().mean())}
            for order in ("view_order", "shuffled"):
                pick = (lambda t: t) if order == "view_order" else (lambda t: t[perm].contiguous())
                rays, srays, siv, liv = pick(view_rays), pick(seg_rays), pick(seg_iv), pick(layer_iv)
                torch.cuda.synchronize(dev)
                check = rt.lib.check
                res = timed(stream, args.reps, args.warmup, {
                    "trace_rays": lambda: check(lib.rtowTraceRaysDevice(ctx.handle, n, rays.data_ptr(), C.byref(hits), sp), "rtowTraceRaysDevice"),
                    "nearest_null": lambda: check(lib.rtowTraceRaysIntervalDevice(ctx.handle, n, rays.data_ptr(), None, C.byref(hits), sp), "rtowTraceRaysIntervalDevice")})
                res.update(timed(stream, args.reps, args.warmup, {
                    "occlusion_null": lambda: check(lib.rtowTraceOcclusionDevice(ctx.handle, n, rays.data_ptr(), None, occ.data_ptr(), sp), "rtowTraceOcclusionDevice")}))
                assert torch.equal(occ != 0, pick(hit))                                # (0, +inf): occluded = the view's ray hit something
                res.update(timed(stream, args.reps, args.warmup, {
                    "occlusion_segments": lambda: check(lib.rtowTraceOcclusionDevice(ctx.handle, n, srays.data_ptr(), siv.data_ptr(), occ.data_ptr(), sp), "rtowTraceOcclusionDevice")}))
                res.update(timed(stream, args.reps, args.warmup, {
                    "nearest_segments": lambda: check(lib.rtowTraceRaysIntervalDevice(ctx.handle, n, srays.data_ptr(), siv.data_ptr(), C.byref(hits), sp), "rtowTraceRaysIntervalDevice")}))
                both = timed(stream, args.reps, args.warmup, {
                    "occlusion_segments_alternating": lambda: check(lib.rtowTraceOcclusionDevice(ctx.handle, n, srays.data_ptr(), siv.data_ptr(), occ.data_ptr(), sp), "rtowTraceOcclusionDevice"),
                    "nearest_segments_alternating": lambda: check(lib.rtowTraceRaysIntervalDevice(ctx.handle, n, srays.data_ptr(), siv.data_ptr(), C.byref(hits), sp), "rtowTraceRaysIntervalDevice")})
                res.update(both)
                assert torch.equal(occ != 0, ent >= 0)                                 # the two forms agree on the segments
                shadowed = float((occ != 0).float().sum() / max(1, int(hit.sum())))
                res.update(timed(stream, args.reps, args.warmup, {
                    "second_layer": lambda: check(lib.rtowTraceRaysIntervalDevice(ctx.handle, n, rays.data_ptr(), liv.data_ptr(), C.byref(hits), sp), "rtowTraceRaysIntervalDevice")}))
                second = float((ent >= 0).float().mean())
                for k in res:
                    res[k]["rays_per_s"] = n / (res[k]["ms_median"] * 1e-3)
                res["nearest_null_over_trace_rays"] = res["nearest_null"]["ms_median"] / res["trace_rays"]["ms_median"]
                res["occlusion_null_over_trace_rays"] = res["occlusion_null"]["ms_median"] / res["trace_rays"]["ms_median"]
                res["occlusion_segments_over_nearest_segments"] = res["occlusion_segments"]["ms_median"] / res["nearest_segments"]["ms_median"]
                res["segments_occluded_share_of_hits"] = shadowed
                res["second_layer_hit_share"] = second
                row[order] = res
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"what": "rtowTraceRaysIntervalDevice / rtowTraceOcclusionDevice at %d x %d next to rtowTraceRaysDevice on the same rays" % (w, h),
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "segment_tmin": args.segment_tmin,
           "timing": "HIP events on the caller's stream around each call; median / min / max of reps; trace_rays and nearest_null alternate in one loop", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
