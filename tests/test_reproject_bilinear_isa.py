"""CPU: resource usage of the compiled four-tap reprojection kernels (csrc/rtow_reproject_bilinear.hip), checked by cross-compiling for gfx950 with
csrc/Makefile's flags.

The pass is a gather of up to four scattered records of the previous frame per pixel, whose latency only occupancy hides.  Both kernels of the unit - with and
without moments - must stay without scratch and without a spilled register of either kind, within the sibling's 64 VGPRs (AGPRs included), at 8 waves per SIMD.
Resource counts only: the test does not read instructions."""
import os
import subprocess

from test_reproject_isa import CSRC, FLAGS, _usage


def test_bilinear_reproject_kernels_have_no_scratch_no_spill_and_at_most_64_vgprs(tmp_path):
    src = os.path.join(CSRC, "rtow_reproject_bilinear.hip")
    proc = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + [src, "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "rtow_reproject_bilinear.o")],
                          capture_output=True, text=True, cwd=CSRC)
    assert proc.returncode == 0, proc.stderr[-3000:]
    usage = _usage(proc.stderr)
    kernels = {k: v for k, v in usage.items() if "reproject_bilinear_kernel" in k}
    assert len(kernels) == 2 and len(usage) == 2, sorted(usage)                   # with and without moments, and nothing else in the unit
    for name, u in usage.items():
        print(name, u)
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (name, u)
        assert u["vgprs"] + u["agprs"] <= 64, (name, u)
        assert u["occupancy"] >= 8, (name, u)
    with_moments = [u for k, u in usage.items() if "ILb1E" in k][0]
    without = [u for k, u in usage.items() if "ILb0E" in k][0]
    assert without["vgprs"] < with_moments["vgprs"], "a call without moments pays no registers for them"
