"""Device time of rtowDenoiseDevice (the a-trous denoise pass) at 1920 x 1080 and 3840 x 2160 for 1..8 levels, in one process on one GPU.

Inputs: a random float3 colour frame with combine-like guides (unit normals in large flat areas, a sky block with zero normals, albedo in [0, 1]), the recommended
parameters apart from the level count.  Each call is bracketed by HIP events on the stream it is enqueued on (torch.cuda.Event, as profiles/adaptive_chain_ab.py);
after `--warmup` untimed calls, `--reps` timed calls per point, the median reported.  Effective GB/s counts what one level must move at the least - colour, normal
and albedo read once, colour written once: 48 B per pixel per level - so it is comparable with the streaming post passes, not a measure of the tap traffic.

    python profiles/denoise_timing.py --out profiles/r07_denoise.json
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


def frame(w, h, seed=0):
    rng = np.random.default_rng(seed)
    n = w * h
    c = rng.uniform(0, 2, (n, 3)).astype(np.float32)
    nrm = np.zeros((h, w, 3), np.float32)
    nrm[:, :, 2] = 1
    nrm[h // 2:, :, :] = (0, 1, 0)
    nrm[: h // 4, : w // 3] = 0
    a = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    return c, nrm.reshape(-1, 3), a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = rt.lib.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    rows = []
    with rt.Context(0) as ctx:
        for w, h in ((1920, 1080), (3840, 2160)):
            n = w * h
            ins = [torch.from_numpy(x.reshape(-1)).to(dev) for x in frame(w, h)]
            out = torch.empty(n * 3, device=dev)
            scratch = torch.empty(abi.denoise_scratch_bytes(w, h) // 4, device=dev)
            stream.wait_stream(torch.cuda.current_stream(dev))
            for levels in range(1, 9):
                p = abi.DenoiseParams(w, h, levels, abi.DENOISE_DEFAULT_NORMAL_SHARPNESS, abi.DENOISE_DEFAULT_COLOR_SIGMA, abi.DENOISE_DEFAULT_ALBEDO_SIGMA,
                                      abi.DENOISE_DEFAULT_FLAGS, 0)

                def call():
                    rt.lib.check(lib.rtowDenoiseDevice(ctx.handle, C.byref(p), ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), scratch.data_ptr(),
                                                       out.data_ptr(), stream.cuda_stream), "rtowDenoiseDevice")
                for _ in range(args.warmup):
                    call()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
                for a, b in ev:
                    a.record(stream)
                    call()
                    b.record(stream)
                stream.synchronize()
                ms = sorted(a.elapsed_time(b) for a, b in ev)
                med = ms[len(ms) // 2]
                row = {"width": w, "height": h, "levels": levels, "ms_median": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                       "ms_per_level": round(med / levels, 4), "effective_GBps": round(48.0 * n * levels / (med * 1e-3) / 1e9, 1), "reps": args.reps}
                print(json.dumps(row), flush=True)
                rows.append(row)
    if args.out:
        meta = {"what": "rtowDenoiseDevice, HIP events on the caller's stream, median of %d after %d warm-up calls" % (args.reps, args.warmup),
                "device": torch.cuda.get_device_name(0), "params": "recommended (normalSharpness %d, colorSigma %g, albedoSigma %g, demodulate), levels 1..8"
                % (abi.DENOISE_DEFAULT_NORMAL_SHARPNESS, abi.DENOISE_DEFAULT_COLOR_SIGMA, abi.DENOISE_DEFAULT_ALBEDO_SIGMA), "rows": rows}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
