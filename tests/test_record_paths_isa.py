"""CPU: resource usage of the compiled path-recording kernels (csrc/rtow_record_paths.hip), checked by cross-compiling for gfx950 with csrc/Makefile's flags.

The unit holds a whole sample path in one lane - camera ray, walk, scatter, fold - under three noise sources and three scene bases: nine kernels.  The lanes' emission /
attenuation stacks live in the caller's segment slots (or the context's block), never in private arrays, so every kernel must stay without scratch and without a
spilled VGPR or SGPR.  Registers and occupancy are printed, not capped: nobody has measured what the pass needs."""
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
                         ("sgpr_spill", "SGPRs Spill"), ("vgpr_spill", "VGPRs Spill")):
            m = re.search(tag + r": (\d+)", block)
            assert m, (name, key)
            fields[key] = int(m.group(1))
        out[name] = fields
    return out


def test_record_paths_kernels_have_no_scratch_and_no_spill(tmp_path):
    src = os.path.join(CSRC, "rtow_record_paths.hip")
    proc = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + [src, "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "rtow_record_paths.o")],
                          capture_output=True, text=True, cwd=CSRC)
    assert proc.returncode == 0, proc.stderr[-3000:]
    usage = _usage(proc.stderr)
    kernels = {k: v for k, v in usage.items() if "record_paths_kernel" in k}
    assert len(kernels) == 9, sorted(usage)            # three scene bases x three noise sources
    assert len(usage) == len(kernels), sorted(usage)   # the sample-kernel header the unit includes instantiates nothing
    for name, u in sorted(kernels.items()):
        print(name, u)
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (name, u)
