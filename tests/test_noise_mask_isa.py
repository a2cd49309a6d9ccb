"""CPU: resource usage of the compiled noise-mask kernels (csrc/rtow_noise_mask.hip), checked by cross-compiling for gfx950 with csrc/Makefile's flags - the method of
tests/test_temporal_moments_isa.py.  Only the compiler's resource-usage remarks are read.

The pass streams 12 bytes per pixel in and a byte (and a float) out, and its staging loads are hidden by occupancy like those of the estimate pass: every
instantiation of the tile kernel must stay without scratch (private segment 0, no spill) and within 64 VGPRs, at 8 waves per SIMD as the remark reports it - a figure
that counts its LDS: the 72 x 12 plane of e, the 70 x 10 plane of "qualifies" and the workgroup's statistics."""
import os
import subprocess

from test_denoise_isa import CSRC, FLAGS
from test_upsample_isa import _usage


def test_noise_mask_kernels_have_no_scratch_and_at_most_64_vgprs(tmp_path):
    src = os.path.join(CSRC, "rtow_noise_mask.hip")
    proc = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + [src, "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "rtow_noise_mask.o")],
                          capture_output=True, text=True, cwd=CSRC)
    assert proc.returncode == 0, proc.stderr[-3000:]
    usage = _usage(proc.stderr)
    tile = [k for k in usage if "noise_mask_kernel" in k]
    assert len(usage) == 4 and len(tile) == 3 and any("noise_pick_kernel" in k for k in usage), sorted(usage)      # count + mask, count only, mask only; the pick step
    for name, u in sorted(usage.items()):
        print(name, u)
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (name, u)
        assert u["vgprs"] + u["agprs"] <= 64, (name, u)
        assert u["occupancy"] >= 8, (name, u)
        if name in tile:
            assert 72 * 12 * 4 <= u["lds"] <= 160 * 1024 // 8, (name, u)      # the staged plane of e at least, and room for 8 workgroups of 4 waves per CU
        else:
            assert u["lds"] == 0, (name, u)
