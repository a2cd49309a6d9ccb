"""CPU: resource usage of the compiled bloom kernels (csrc/rtow_bloom.hip), checked by cross-compiling for gfx950 with csrc/Makefile's flags - the method of
tests/test_tonemap_isa.py.  Only the compiler's resource-usage remarks are read.

The unit holds exactly five kernels: the prefilter with and without the Karis average (a template parameter, so the plain form carries no weight plane and no
division), the downsample, the upsample and the composite.  None may use scratch or spill - a scalar register parked in a VGPR lane counts as a spill.  The prefilter's
LDS is what its source comment states: 1300 words a plane, four planes with the flag and three without; the other kernels use none."""
import os
import re
import subprocess

from test_upsample_isa import CSRC, FLAGS, _usage

PLANE_WORDS = 130 * 10                                                     # the 64 x 4 tile of mip 1 reads 130 x 10 source pixels


def test_bloom_kernels_have_no_scratch_no_spills_and_the_stated_lds(tmp_path):
    proc = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + [os.path.join(CSRC, "rtow_bloom.hip"), "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "rtow_bloom.o")],
                          capture_output=True, text=True, cwd=CSRC)
    assert proc.returncode == 0, proc.stderr[-3000:]
    usage = _usage(proc.stderr)
    prefilter = {re.search(r"bloom_prefilter_kernelILb(\d)EE", k).group(1): v for k, v in usage.items() if "bloom_prefilter_kernel" in k}
    rest = {name: [v for k, v in usage.items() if re.search(r"\d+%sE" % name, k)] for name in ("bloom_downsample_kernel", "bloom_upsample_kernel", "bloom_composite_kernel")}
    assert sorted(prefilter) == ["0", "1"], sorted(usage)                  # bloom_prefilter_kernel<KARIS> (Itanium mangling: ILb<flag>EE)
    assert all(len(v) == 1 for v in rest.values()), sorted(usage)
    assert len(usage) == 5, sorted(usage)                                  # exactly the kernels of the unit
    for name, u in sorted(usage.items()):
        print(name, u)
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (name, u)
    assert prefilter["1"]["lds"] == 4 * PLANE_WORDS * 4 == 20800, prefilter["1"]
    assert prefilter["0"]["lds"] == 3 * PLANE_WORDS * 4 == 15600, prefilter["0"]
    source = open(os.path.join(CSRC, "rtow_bloom.hip"), encoding="utf-8").read()
    assert "20800 bytes" in source and "15600 bytes" in source, "the figures the unit's own comment states"
    for name, (u,) in rest.items():
        assert u["lds"] == 0, (name, u)


def test_makefile_builds_the_unit_without_contraction():
    text = open(os.path.join(CSRC, "Makefile"), encoding="utf-8").read()
    assert "rtow_bloom.o" in text and "-ffp-contract=off" in text
