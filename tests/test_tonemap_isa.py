"""CPU: resource usage of the compiled metering and tone-mapped finalize kernels (csrc/rtow_tonemap.hip), checked by cross-compiling for gfx950 with csrc/Makefile's
flags - the method of tests/test_upsample_isa.py.  Only the compiler's resource-usage remarks are read.

The unit holds exactly five kernels: the histogram, the resolve, and one finalize kernel per tone curve (the curve is a template parameter, so CLAMP carries no ACES
code).  None may use scratch or spill - a scalar register parked in a VGPR lane counts as a spill.  The finalize kernels stream like finalize_kernel and hide their
loads the same way, so the occupancy the compiler reports for them must not be below what it reports for finalize_kernel when rtow_kernels.hip is compiled the same
way, here, in the same test."""
import os
import re
import subprocess

from test_upsample_isa import CSRC, FLAGS, _usage


def _compile(name, tmp_path):
    proc = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + [os.path.join(CSRC, name + ".hip"), "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / (name + ".o"))],
                          capture_output=True, text=True, cwd=CSRC)
    assert proc.returncode == 0, proc.stderr[-3000:]
    return _usage(proc.stderr)


def test_tonemap_kernels_have_no_scratch_no_spills_and_the_occupancy_of_finalize(tmp_path):
    usage = _compile("rtow_tonemap", tmp_path)
    histogram = [k for k in usage if "exposure_histogram_kernel" in k]
    resolve = [k for k in usage if "exposure_resolve_kernel" in k]
    finalize = {k: v for k, v in usage.items() if "tonemap_finalize_kernel" in k}
    assert len(histogram) == 1 and len(resolve) == 1, sorted(usage)
    # tonemap_finalize_kernel<CURVE>: CLAMP, ACES_FITTED, ACES_FILM (Itanium mangling: ILi<curve>EE)
    assert sorted(re.search(r"tonemap_finalize_kernelILi(\d)EE", k).group(1) for k in finalize) == ["0", "1", "2"], sorted(usage)
    assert len(usage) == 5, sorted(usage)                                  # exactly the kernels of the unit: the table builder stays in rtow_kernels.hip
    for name, u in sorted(usage.items()):
        print(name, u)
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (name, u)
    assert usage[histogram[0]]["lds"] == 4 * 256 * 4, usage[histogram[0]]  # a private 256-bin row per wave
    plain = [v for k, v in _compile("rtow_kernels", tmp_path).items() if re.search(r"\d+finalize_kernelE", k)]
    assert len(plain) == 1, "finalize_kernel of rtow_kernels.hip"
    print("finalize_kernel", plain[0])
    for name, u in finalize.items():
        assert u["occupancy"] >= plain[0]["occupancy"], (name, u, plain[0])


def test_makefile_builds_the_unit_without_contraction():
    text = open(os.path.join(CSRC, "Makefile"), encoding="utf-8").read()
    assert "rtow_tonemap.o" in text and "-ffp-contract=off" in text
