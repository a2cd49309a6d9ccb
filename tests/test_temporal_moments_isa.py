"""CPU: resource usage of the compiled temporal-moments kernels (csrc/rtow_moments_temporal.hip), checked by cross-compiling for gfx950 with csrc/Makefile's flags -
the method of tests/test_denoise_isa.py.  Only the compiler's resource-usage remarks are read.

The gather's scattered 12-byte read and the estimate's staging loads are hidden by occupancy, like the taps of the neighbouring post passes: every kernel of the
unit must stay without scratch (private segment 0, no spill) and within 64 VGPRs, at 8 waves per SIMD as the remark reports it - for the estimate that figure
counts its LDS (six planes of the 70 x 10 halo region, 16800 bytes, next to the workgroup reduction's).  The planes are declared in the kernel; their geometry, the
staging and the tap loop are csrc/rtow_guided_halo.hip.h's, which csrc/rtow_rectify_history.hip shares (tests/test_rectify_history_isa.py)."""
import os
import subprocess

from test_denoise_isa import CSRC, FLAGS
from test_upsample_isa import _usage


def test_temporal_moments_kernels_have_no_scratch_and_at_most_64_vgprs(tmp_path):
    src = os.path.join(CSRC, "rtow_moments_temporal.hip")
    proc = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + [src, "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "rtow_moments_temporal.o")],
                          capture_output=True, text=True, cwd=CSRC)
    assert proc.returncode == 0, proc.stderr[-3000:]
    usage = _usage(proc.stderr)
    assert len(usage) == 2 and all(any(part in k for k in usage) for part in ("reproject_moments_kernel", "estimate_moments_kernel")), sorted(usage)
    for name, u in sorted(usage.items()):
        print(name, u)
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (name, u)
        assert u["vgprs"] + u["agprs"] <= 64, (name, u)
        assert u["occupancy"] >= 8, (name, u)
        if "estimate" in name:
            assert 70 * 10 * 24 <= u["lds"] <= 160 * 1024 // 8, (name, u)      # the staged halo region, and room for 8 workgroups of 4 waves per CU
        else:
            assert u["lds"] == 0, (name, u)
