"""Rays per second of rtowTraceViewDevice at 1920 x 1080 and of rtowTraceRaysDevice on the same rays in shuffled (incoherent) order, on the cover scene, 10 000 spheres
and the 250 882-triangle mesh - next to a loop over rtowProbeNearestHit (the host walk: the only query the library had before) on the same host over `--host-rays` of
those rays.  In one process on one GPU.

Each device call is bracketed by HIP events on the stream it is enqueued on (torch.cuda.Event, as profiles/denoise_timing.py); after `--warmup` untimed calls,
`--reps` timed calls per point: median, minimum and maximum are reported.  All three hit buffers are written.  The host loop is timed with the host clock around the
calls through ctypes (its call overhead is part of what a host pays per probe); it touches no device.

    python profiles/trace_rays_timing.py --out profiles/r07_trace_rays.json
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np
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
    ap.add_argument("--host-rays", type=int, default=10000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_trace_rays.json"))
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
            rays = torch.empty(n * 8, device=dev)
            hits = abi.HitBuffers(dist.data_ptr(), ent.data_ptr(), nrm.data_ptr())
            p = abi.TraceViewParams(w, h, view, 0.0, 0)
            stream.wait_stream(torch.cuda.current_stream(dev))
            sp = C.c_void_p(stream.cuda_stream)
            rt.lib.check(lib.rtowTraceViewDevice(ctx.handle, C.byref(p), C.byref(hits), rays.data_ptr(), sp), "rtowTraceViewDevice")
            stream.synchronize()
            coherent_ent = ent.cpu().numpy().copy()
            host_rays = rays.cpu().numpy().reshape(n, 8)
            perm = torch.from_numpy(np.random.default_rng(5).permutation(n)).to(dev)
            shuffled = rays.reshape(n, 8)[perm].contiguous()
            torch.cuda.synchronize(dev)
            tv = timed(stream, args.reps, args.warmup, lambda: rt.lib.check(lib.rtowTraceViewDevice(ctx.handle, C.byref(p), C.byref(hits), None, sp), "rtowTraceViewDevice"))
            tc = timed(stream, args.reps, args.warmup, lambda: rt.lib.check(lib.rtowTraceRaysDevice(ctx.handle, n, rays.data_ptr(), C.byref(hits), sp), "rtowTraceRaysDevice"))
            ts = timed(stream, args.reps, args.warmup, lambda: rt.lib.check(lib.rtowTraceRaysDevice(ctx.handle, n, shuffled.data_ptr(), C.byref(hits), sp), "rtowTraceRaysDevice"))
            assert np.array_equal(ent.cpu().numpy(), coherent_ent[perm.cpu().numpy()])          # the shuffled query answered the same rays
            # the host loop: every (n // host_rays)-th ray of the frame, so that it sees the whole view
            pick = np.arange(0, n, max(1, n // args.host_rays))[:args.host_rays]
            o3, d3, dd, ee = abi.Float3(), abi.Float3(), C.c_float(), C.c_int32()
            t0 = time.perf_counter()
            for k in pick:
                r = host_rays[k]
                o3.x, o3.y, o3.z, d3.x, d3.y, d3.z = r[0], r[1], r[2], r[4], r[5], r[6]
                lib.rtowProbeNearestHit(ctx.handle, C.byref(o3), C.byref(d3), 0.0, C.byref(dd), C.byref(ee))
            host_s = time.perf_counter() - t0
        host_rate = len(pick) / host_s
        row = {"scene": name, "entities": scene.entity_count, "rays": n, "hit_share": float((coherent_ent >= 0).mean()),
               "trace_view": dict(tv, rays_per_s=n / (tv["ms_median"] * 1e-3)),
               "trace_rays_view_order": dict(tc, rays_per_s=n / (tc["ms_median"] * 1e-3)),
               "trace_rays_shuffled": dict(ts, rays_per_s=n / (ts["ms_median"] * 1e-3)),
               "host_probe_loop": {"rays": int(len(pick)), "seconds": host_s, "rays_per_s": host_rate},
               "trace_view_over_host_loop": n / (tv["ms_median"] * 1e-3) / host_rate}
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"what": "rtowTraceViewDevice / rtowTraceRaysDevice at %d x %d against a host loop over rtowProbeNearestHit" % (w, h), "device": torch.cuda.get_device_name(0),
           "reps": args.reps, "warmup": args.warmup, "timing": "HIP events on the caller's stream around each call; median / min / max of reps", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
