"""What the guides of rtowTraceGuideViewDevice are worth to the denoiser: one quality run, shared by tests/test_gpu_guides.py (its assertion) and
profiles/guides_timing.py (the figures of profiles/r11_guides.json)."""
import numpy as np

F = np.float32


def guide_quality(rt, ctx, w, h, seed):
    """tests/test_gpu_denoise.py's quality protocol - cover scene, 4 spp (seed) against 1024 spp (seed + 1), trace depth 8, both combined on the device, rtowDenoiseDevice
    with the recommended parameters - under three guide pairs: combine's own normal and albedo; the first hit's (rtowTraceViewDevice's normal, rtowShadeHitsDevice's
    albedo); the chain's (rtowTraceGuideViewDevice's normal, rtowShadeHitsDevice's albedo on its rays).  Squared errors relative to the noisy frame's, on the whole frame and
    on the pixels whose first hit is perfectly specular."""
    a = rt.abi
    scene = rt.scenes.cover_scene()
    n = w * h
    ctx.upload_scene(scene.desc())
    combined = []
    for spp, s in ((4, seed), (1024, seed + 1)):
        p = rt.scenes.make_params(scene, w, h, spp=spp, trace_depth=8, seed=s)
        acc = rt.sample_batch_host(ctx, p, want_diag=False)
        ins = [rt.DeviceBuffer(ctx).upload(acc[k]) for k in ("color", "normal", "albedo")]
        outs = [rt.DeviceBuffer(ctx, n * 12) for _ in range(3)]
        cj = rt.CombineJob(ctx, (w, h))
        cj.InputColor, cj.InputNormal, cj.InputAlbedo = ins
        cj.OutputColor, cj.OutputNormal, cj.OutputAlbedo = outs
        rt.lib.check(cj.Schedule().Complete(), "rtowCombineDevice")
        ctx.synchronize()
        combined.append([o.download(F, (n, 3)) for o in outs])
        for b in ins + outs:
            b.free()
    (c4, n4, a4), (reference, _, _) = combined
    first = ctx.trace_view(p.view, w, h, want_rays=True, want=("entityIndex", "normal"))
    first_surface = ctx.shade_hits(first["rays"], first["entityIndex"], p.environment, outputs=("albedo", "materialInfo"))
    chain = ctx.trace_guide_view(p.view, w, h, a.GUIDE_DEFAULT_MAX_BOUNCES, want=("entityIndex", "normal", "rays", "bounces", "end"))
    chain_albedo = ctx.shade_hits(chain["rays"], chain["entityIndex"], p.environment, outputs=("albedo",))["albedo"]

    def denoise(normal, albedo):
        bufs = [rt.DeviceBuffer(ctx).upload(np.ascontiguousarray(x, dtype=F)) for x in (c4, normal, albedo)]
        out, scratch = rt.DeviceBuffer(ctx, n * 12), rt.DeviceBuffer(ctx, a.denoise_scratch_bytes(w, h))
        dj = rt.DenoiseJob(ctx, w, h)
        dj.InputColor, dj.InputNormal, dj.InputAlbedo, dj.Scratch, dj.OutputColor = bufs[0], bufs[1], bufs[2], scratch, out
        rt.lib.check(dj.Schedule().Complete(), "rtowDenoiseDevice")
        ctx.synchronize()
        res = out.download(F, (n, 3))
        for b in bufs + [out, scratch]:
            b.free()
        return res

    specular = (first_surface["materialInfo"] != a.MATERIAL_INFO_MISS) & ((first_surface["materialInfo"] & a.MATERIAL_INFO_PERFECT_SPECULAR) != 0)
    mse = lambda x, mask=slice(None): float(np.mean((x.astype(np.float64)[mask] - reference[mask]) ** 2))
    frames = {"combine_guides": denoise(n4, a4), "first_hit_guides": denoise(first["normal"], first_surface["albedo"]), "chain_guides": denoise(chain["normal"], chain_albedo)}
    out = {"scene": "cover", "width": w, "height": h, "spp": 4, "reference_spp": 1024, "seed": seed, "noisy_mse": mse(c4), "noisy_mse_on_specular_first_hits": mse(c4, specular),
           "perfect_specular_first_hit_share": float(specular.mean()), "mean_bounces": float(chain["bounces"].mean()), "cut_share": float((chain["end"] == 2).mean())}
    for k, frame in frames.items():
        assert np.isfinite(frame).all(), k
        out[k] = {"whole_frame_over_noisy": mse(frame) / out["noisy_mse"], "specular_first_hits_over_noisy": mse(frame, specular) / out["noisy_mse_on_specular_first_hits"]}
    return out
