"""GPU: the TEST stage's sphere test with the run's reciprocal (csrc/rtow_hit_tests.hip.h, sphere_hit_shared_rcp / sphere_root_quotient) against sphere_hit on the same
operands: the hit flag and the bits of t, 2^25 rays and spheres and 2^25 root triples (tests/native/sphere_quotient_parity.hip, whose head lists the operand families).
No mismatch - and every kind of case the sweep is there for must have come up, which the program reports by count."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kinds of case that must occur, per part.  Part 1 goes through the whole function: a finite numerator of 2^65 and more (biased exponent 192) and a redo that ends
# in a hit cannot come out of its arithmetic (the program's head says why) - part 2, on the part behind the square root, has both.
COMMON = ["hits", "quotients from the reciprocal", "second root taken", "cold redo entered", "numerator exponent 63", "numerator exponent 64", "numerator exponent 191",
          "a exponent 95", "a exponent 96", "a exponent 159", "a exponent 160", "a zero", "a subnormal", "a infinite", "a NaN"]
NEEDED = {1: COMMON + ["numerator infinite", "negative discriminants", "zero discriminants", "origins inside", "origins on the sphere", "origins outside"],
          2: COMMON + ["numerator exponent 192", "cold redo hits"]}


def test_shared_reciprocal_sphere_test_equals_sphere_hit():
    src = os.path.join(ROOT, "tests", "native", "sphere_quotient_parity.hip")
    csrc = os.path.join(ROOT, "raytracing-in-one-weekend_amd", "csrc")
    newest = max(os.path.getmtime(p) for p in [src] + [os.path.join(csrc, h) for h in ("rtow_hit_tests.hip.h", "rtow_vecmath.hip.h", "rtow_exactmath.hip.h", "rtow_kernels.h")])
    out_dir = os.path.join(ROOT, "tests", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "sphere_quotient_parity")
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-value", "-Wno-unused-function",
                        "-x", "hip", src, "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "part 1 rays and spheres 33554432: 0 mismatches" in r.stdout and "part 2 root triples 33554432: 0 mismatches" in r.stdout and "total 0 mismatches" in r.stdout, r.stdout
    counts = {(int(m.group(1)), m.group(2)): int(m.group(3)) for m in re.finditer(r"^part (\d) (.+?) (\d+)$", r.stdout, re.M)}
    for part, kinds in NEEDED.items():
        for kind in kinds:
            assert counts[(part, kind)] > 0, (part, kind, r.stdout)
