"""Development helper: the table of the pruned camera-ray lists (csrc/rtow_camera_lists.hip.h) from the shipped code, through rtowGetCameraRayListStats.
Run on the GPU box:  python profiles/experiments/camera_list_lengths.py [--out FILE.json]
For the benchmark's scenes (bench.py --config 2 .. 5 where they are sphere scenes) at their frame sizes it prints, with whole lists (RTOW_CONTEXT_UNPRUNED_CAMERA_RAY_LISTS)
and with pruned ones: pixels with 0 .. 8 nodes, pixels without a list, nodes per list (mean) and pixels with 5 to 8 nodes.  One 1-sample batch builds the lists."""
import argparse, importlib, json, os, sys
sys.path.insert(0, os.getcwd())
rt = importlib.import_module("raytracing-in-one-weekend_amd")
S = rt.scenes
CASES = (("cover 1920x1080 pinhole", lambda: S.cover_scene(), 1920, 1080, None),
         ("cover 3840x2160 pinhole", lambda: S.cover_scene(), 3840, 2160, None),
         ("cover 1920x1080 aperture 0.1", lambda: S.cover_scene(), 1920, 1080, 0.1),
         ("moving 1920x1080", lambda: S.moving_scene(), 1920, 1080, None),
         ("stress 10 000 spheres 1920x1080", lambda: S.stress_scene(), 1920, 1080, None))
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for what, make, w, h, aperture in CASES:
        s = make()
        if aperture is not None:
            s.camera = dict(s.camera, aperture=aperture)
        p = S.make_params(s, w, h, spp=1, trace_depth=2)
        for label, flags in (("whole", rt.abi.CONTEXT_UNPRUNED_CAMERA_RAY_LISTS), ("pruned", 0)):
            with rt.Context(0, flags=flags) as ctx:
                ctx.upload_scene(s.desc())
                rt.sample_batch_host(ctx, p)
                st = ctx.camera_ray_list_stats()
            listed = sum(st["entries"])
            row = {"case": what, "lists": label, "pruned": st["pruned"], "entries": st["entries"], "no_list": st["no_list"], "owned": st["owned"],
                   "nodes_per_list_mean": round(sum(k * c for k, c in enumerate(st["entries"])) / max(listed, 1), 4), "pixels_with_5_to_8": sum(st["entries"][5:9])}
            rows.append(row)
            print("%-34s %-6s nodes/list %.3f  empty %8d  5..8 nodes %7d  no list %7d  | %s" % (what, label, row["nodes_per_list_mean"], st["entries"][0], row["pixels_with_5_to_8"],
                                                                                                  st["no_list"], st["entries"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
