"""CPU: resource usage of the compiled variance-guided denoise kernels (csrc/rtow_denoise_variance.hip), checked by cross-compiling for gfx950 with csrc/Makefile's
flags - the method of tests/test_denoise_isa.py.

The variance level reads 25 taps of four streams per pixel from L2 / MALL, like the plain level with one more 4-byte load per tap: what hides that latency is
occupancy.  Every kernel of the unit (the moments pass, the initial variance, the level) must stay without scratch (private segment 0, no spill) and within 64
VGPRs, so that 8 waves per SIMD stay possible: the variance state fits (the level measures 52 VGPRs next to the plain level's 47)."""
import os
import subprocess

from test_denoise_isa import CSRC, FLAGS, _usage


def test_variance_kernels_have_no_scratch_and_at_most_64_vgprs(tmp_path):
    src = os.path.join(CSRC, "rtow_denoise_variance.hip")
    proc = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + [src, "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "rtow_denoise_variance.o")],
                          capture_output=True, text=True, cwd=CSRC)
    assert proc.returncode == 0, proc.stderr[-3000:]
    usage = _usage(proc.stderr)
    kernels = {k: v for k, v in usage.items() if "_kernel" in k}
    assert len(kernels) == 3 and all(any(part in k for k in kernels) for part in ("accumulate_moments", "initial_variance", "denoise_variance_level")), sorted(usage)
    for name, u in kernels.items():
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (name, u)
        assert u["vgprs"] + u["agprs"] <= 64, (name, u)
        assert u["occupancy"] >= 8, (name, u)
