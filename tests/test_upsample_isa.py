"""CPU: resource usage of the compiled upsampling kernels (csrc/rtow_upsample.hip), checked by cross-compiling for gfx950 with csrc/Makefile's flags.

The pass is a gather: four to sixteen scattered reads of the rendered frame and its guides per displayed pixel, whose latency only occupancy hides.  Every kernel of
the unit - POINT, BILINEAR and GUIDED, the latter two with and without the albedo demodulation - must stay without scratch (private segment 0, no spill) and within
64 VGPRs + AGPRs, so that 8 waves per SIMD stay possible.  What was built is printed."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing-in-one-weekend_amd", "csrc")
FLAGS = ["-std=c++17", "-O3", "-fPIC", "-fvisibility=hidden", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "-x", "hip"]   # csrc/Makefile's


def _usage(remarks):
    out = {}
    for block in re.split(r"remark: (?:[^\n]*?: )?Function Name: ", remarks)[1:]:
        name = block.split(" [")[0].strip()
        fields = {}
        for key, tag in (("vgprs", r"\bVGPRs"), ("agprs", "AGPRs"), ("scratch", r"ScratchSize \[bytes/lane\]"), ("occupancy", r"Occupancy \[waves/SIMD\]"),
                         ("sgpr_spill", "SGPRs Spill"), ("vgpr_spill", "VGPRs Spill"), ("lds", r"LDS Size \[bytes/block\]")):
            m = re.search(tag + r": (\d+)", block)
            assert m, (name, key)
            fields[key] = int(m.group(1))
        out[name] = fields
    return out


def test_upsample_kernels_have_no_scratch_and_at_most_64_vgprs(tmp_path):
    src = os.path.join(CSRC, "rtow_upsample.hip")
    proc = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + [src, "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "rtow_upsample.o")],
                          capture_output=True, text=True, cwd=CSRC)
    assert proc.returncode == 0, proc.stderr[-3000:]
    usage = _usage(proc.stderr)
    kernels = {k: v for k, v in usage.items() if "upsample_kernel" in k}
    # upsample_kernel<MODE, DEMOD>: POINT, BILINEAR x 2, GUIDED x 2 (Itanium mangling: ILi<mode>ELb<demod>EE)
    assert sorted(re.search(r"ILi(\d)ELb(\d)EE", k).groups() for k in kernels) == [("0", "0"), ("1", "0"), ("1", "1"), ("2", "0"), ("2", "1")], sorted(usage)
    assert len(kernels) == len(usage), sorted(usage)                  # every kernel of the unit is held to the budget
    for name, u in sorted(kernels.items()):
        print(name, u)
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (name, u)
        assert u["vgprs"] + u["agprs"] <= 64, (name, u)
        assert u["occupancy"] >= 8, (name, u)
        assert u["lds"] == 0, (name, u)
