"""CPU: resource usage of the compiled history-rectification kernel (csrc/rtow_rectify_history.hip), checked by cross-compiling for gfx950 with csrc/Makefile's flags -
the method of tests/test_temporal_moments_isa.py.  Only the compiler's resource-usage remarks are read.

The staging loads and the reads of a pixel's own history are hidden by occupancy, like the taps of the neighbouring post passes: the kernel must stay without scratch
(private segment 0) and without spills - a scalar register parked in a VGPR lane counts as one; the kernel reads the pointers it hands to the staging
(csrc/rtow_guided_halo.hip.h's, inlined) and its write-phase pointers from the kernel arguments tile by tile so that none is - within 64 VGPRs, at 8 waves per SIMD as
the remark reports it.  That figure counts its LDS: six planes of the 70 x 10 halo region, 16800 bytes, declared in the kernel, next to the workgroup's four
counters."""
import os
import subprocess

from test_denoise_isa import CSRC, FLAGS
from test_upsample_isa import _usage


def test_rectify_history_kernel_has_no_scratch_no_spills_and_at_most_64_vgprs(tmp_path):
    src = os.path.join(CSRC, "rtow_rectify_history.hip")
    proc = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + [src, "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "rtow_rectify_history.o")],
                          capture_output=True, text=True, cwd=CSRC)
    assert proc.returncode == 0, proc.stderr[-3000:]
    usage = _usage(proc.stderr)
    assert len(usage) == 1 and "rectify_history_kernel" in next(iter(usage)), sorted(usage)
    for name, u in usage.items():
        print(name, u)
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (name, u)
        assert u["vgprs"] + u["agprs"] <= 64, (name, u)
        assert u["occupancy"] >= 8, (name, u)
        assert 70 * 10 * 24 <= u["lds"] <= 160 * 1024 // 8, (name, u)      # the staged halo region, and room for 8 workgroups of 4 waves per CU


def test_makefile_builds_the_unit_without_contraction():
    text = open(os.path.join(CSRC, "Makefile"), encoding="utf-8").read()
    assert "rtow_rectify_history.o" in text and "-ffp-contract=off" in text
