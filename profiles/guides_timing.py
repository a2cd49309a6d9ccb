"""Device time of rtowTraceGuideViewDevice next to rtowTraceViewDevice at 1920 x 1080 and 3840 x 2160 on the cover scene (spheres; a quarter of the frame behind mirrors and
glass) and on textured_mesh_scene (triangles, image textures; its one perfectly specular material is the glass icosphere in the middle), and what the chain's guides are
worth to the denoiser.  In one process on one GPU.

Timing: each call is bracketed by HIP events on the stream it is enqueued on (torch.cuda.Event, as profiles/shade_hits_timing.py); after `--warmup` untimed calls, `--reps`
timed calls per point, the calls of a point alternating: median, minimum and maximum.  Both calls write the same four arrays (distance, entityIndex, normal, rays: 52 bytes
a pixel); the guide call is timed at maxBounces 0, 1 and 8 with those outputs, and once more at 8 with all of its outputs (73 bytes a pixel).  The ratio to the trace pass
and the mean of `bounces` are reported per point.

Guides: tests/guides_quality.py - the protocol of tests/test_gpu_denoise.py's quality test (cover scene, 192 x 108, 4 spp against 1024 spp, recommended parameters) under
combine's guides, first-hit guides and chain guides, for three seeds; the spread of chain / first-hit over the seeds is what the margin of the assertion in
tests/test_gpu_guides.py is held against.

    python profiles/guides_timing.py --out profiles/r11_guides.json
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
rt = importlib.import_module("raytracing-in-one-weekend_amd")
from guides_quality import guide_quality  # noqa: E402

abi = rt.abi


def timed(stream, reps, warmup, calls):
    """the calls alternate (a b c a b c ...), so that whatever else the machine does meets all of them alike; one result per call"""
    for _ in range(warmup):
        for call in calls:
            call()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in calls] for _ in range(reps)]
    for rep in ev:
        for (a, b), call in zip(rep, calls):
            a.record(stream)
            call()
            b.record(stream)
    stream.synchronize()
    out = []
    for k in range(len(calls)):
        ms = sorted(rep[k][0].elapsed_time(rep[k][1]) for rep in ev)
        out.append({"ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1]})
    return out


def time_scene(lib, stream, sp, dev, name, scene, args):
    rows = []
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        for w, h in ((1920, 1080), (3840, 2160)):
            n = w * h
            f = lambda c: torch.empty(n * c, device=dev)
            i = lambda: torch.empty(n, dtype=torch.int32, device=dev)
            dist, ent, nrm, rays, thr, path, bnc, end = f(1), i(), f(3), f(8), f(3), f(1), i(), torch.empty(n, dtype=torch.uint8, device=dev)
            tv = abi.TraceViewParams(w, h, rt.scenes.make_view(scene, w, h), 0.0, 0)
            hits = abi.HitBuffers(dist.data_ptr(), ent.data_ptr(), nrm.data_ptr())
            same = abi.guide_buffers({"distance": dist.data_ptr(), "entityIndex": ent.data_ptr(), "normal": nrm.data_ptr(), "rays": rays.data_ptr()})
            every = abi.guide_buffers({"distance": dist.data_ptr(), "entityIndex": ent.data_ptr(), "normal": nrm.data_ptr(), "rays": rays.data_ptr(), "throughput": thr.data_ptr(),
                                       "pathDistance": path.data_ptr(), "bounces": bnc.data_ptr(), "end": end.data_ptr()})
            stream.wait_stream(torch.cuda.current_stream(dev))
            torch.cuda.synchronize(dev)
            trace = lambda: rt.lib.check(lib.rtowTraceViewDevice(ctx.handle, C.byref(tv), C.byref(hits), rays.data_ptr(), sp), "rtowTraceViewDevice")
            guide = lambda p, out: (lambda: rt.lib.check(lib.rtowTraceGuideViewDevice(ctx.handle, C.byref(p), C.byref(tv), C.byref(out), sp), "rtowTraceGuideViewDevice"))
            depths = (0, 1, 8)
            params = [abi.GuideParams(mb, 0, 0) for mb in depths]
            mean_bounces = []
            for p in params:                                                       # (untimed, with `bounces`: its mean for this point)
                guide(p, every)()
                stream.synchronize()
                mean_bounces.append(float(bnc.float().mean().item()))
            cut_share = float((end == 2).float().mean().item())
            times = timed(stream, args.reps, args.warmup, [trace] + [guide(p, same) for p in params] + [guide(params[-1], every)])
            t_trace = times[0]
            row = {"scene": name, "entities": scene.entity_count, "width": w, "height": h, "pixels": n, "trace_view": t_trace, "guide_view": {}}
            for mb, t, mean in zip(depths, times[1:4], mean_bounces):
                row["guide_view"]["max_bounces_%d" % mb] = dict(t, over_trace_view=t["ms_median"] / t_trace["ms_median"], ms_over_trace_view=t["ms_median"] - t_trace["ms_median"],
                                                                mean_bounces=mean)
            row["guide_view"]["max_bounces_8_all_outputs"] = dict(times[4], over_trace_view=times[4]["ms_median"] / t_trace["ms_median"], cut_share_at_8=cut_share)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del dist, ent, nrm, rays, thr, path, bnc, end
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_guides.json"))
    args = ap.parse_args()
    lib = rt.lib.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    rows = []
    for name, scene in (("cover", rt.scenes.cover_scene()), ("textured_mesh", rt.scenes.textured_mesh_scene())):
        rows += time_scene(lib, stream, sp, dev, name, scene, args)
    quality = []
    with rt.Context(0) as ctx:
        for seed in (1, 11, 21):
            quality.append(guide_quality(rt, ctx, 192, 108, seed))
            print(json.dumps(quality[-1]), flush=True)
    ratios = [q["chain_guides"]["whole_frame_over_noisy"] / q["first_hit_guides"]["whole_frame_over_noisy"] for q in quality]
    spread = {"chain_over_first_hit_whole_frame": ratios, "spread": max(ratios) - min(ratios), "margin_of_the_test": 0.05}
    print(json.dumps(spread), flush=True)
    result = {"what": "rtowTraceGuideViewDevice: device time per call next to rtowTraceViewDevice, and the denoised error of a 4-spp cover frame under combine's, first-hit and "
                      "chain guides",
              "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "timing": "HIP events on the caller's stream around each call; median / min / max of reps", "rows": rows, "denoise_guides": quality, "seed_spread": spread}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
