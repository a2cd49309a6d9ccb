"""CPU: the ABI of rtowTraceGuideRaysDevice / rtowTraceGuideViewDevice (include/rtow.h, added after API version 12 without changing it) - the layouts of RtowGuideParams and
RtowGuideBuffers as g++ sees the header against the ctypes mirrors and the explicit-layout C# structs of INTEGRATION.md section 1, the exported symbols, the numpy view of
the outputs, and the argument validation that needs no device.  (A context cannot be created without a device, so only the NULL-context path of the validation is reachable
here; tests/test_gpu_guides.py walks every other case with a real context.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "raytracing-in-one-weekend_amd", "csrc", "librtow_hip.so")

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "rtow.h"
int main(void)
{
    printf("%zu %zu %zu %zu\n", sizeof(RtowGuideParams), offsetof(RtowGuideParams, maxBounces), offsetof(RtowGuideParams, flags), offsetof(RtowGuideParams, reserved));
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(RtowGuideBuffers), offsetof(RtowGuideBuffers, hits), offsetof(RtowGuideBuffers, rays), offsetof(RtowGuideBuffers, throughput),
           offsetof(RtowGuideBuffers, pathDistance), offsetof(RtowGuideBuffers, bounces), offsetof(RtowGuideBuffers, end));
    return 0;
}
"""
EXPECTED = {"GuideParams": [12, 0, 4, 8], "GuideBuffers": [64, 0, 24, 32, 40, 48, 56]}
C_NAMES = {"GuideParams": "RtowGuideParams", "GuideBuffers": "RtowGuideBuffers"}
ENTRIES = ("rtowTraceGuideRaysDevice", "rtowTraceGuideViewDevice")


def _probe(tmp_path):
    src, exe = tmp_path / "guide_layout.c", tmp_path / "guide_layout"
    src.write_text(PROBE)
    subprocess.run(["g++", "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    return {k: [int(x) for x in line.split()] for k, line in zip(("GuideParams", "GuideBuffers"), lines)}


def _mirror(rt, name):
    S = getattr(rt.abi, name)
    return [C.sizeof(S)] + [getattr(S, f[0]).offset for f in S._fields_]


def test_struct_layouts_match_the_ctypes_mirrors(rt, tmp_path):
    seen = _probe(tmp_path)
    for name, want in EXPECTED.items():
        assert seen[name] == want == _mirror(rt, name), (name, seen[name], _mirror(rt, name))
    a = rt.abi
    assert [f[0] for f in a.GuideParams._fields_] == ["maxBounces", "flags", "reserved"]
    assert [f[0] for f in a.GuideBuffers._fields_] == ["hits", "rays", "throughput", "pathDistance", "bounces", "end"]
    assert a.GuideBuffers._fields_[0][1] is a.HitBuffers
    # the numpy view of the outputs, in the struct's order (hits member by member), and the helper that fills the struct from it
    assert list(a.GUIDE_OUTPUTS) == ["distance", "entityIndex", "normal", "rays", "throughput", "pathDistance", "bounces", "end"]
    sizes = {k: np.dtype(d).itemsize * w for k, (d, w) in a.GUIDE_OUTPUTS.items()}
    assert sizes == {"distance": 4, "entityIndex": 4, "normal": 12, "rays": 32, "throughput": 12, "pathDistance": 4, "bounces": 4, "end": 1}
    b = a.guide_buffers({k: 0x1000 * (i + 1) for i, k in enumerate(a.GUIDE_OUTPUTS)})
    assert [b.hits.distance, b.hits.entityIndex, b.hits.normal, b.rays, b.throughput, b.pathDistance, b.bounces, b.end] == [0x1000 * (i + 1) for i in range(8)]
    only = a.guide_buffers({"end": 0x40})
    assert only.end == 0x40 and not any([only.hits.distance, only.hits.entityIndex, only.hits.normal, only.rays, only.throughput, only.pathDistance, only.bounces])
    assert (a.GUIDE_END_SKY, a.GUIDE_END_SURFACE, a.GUIDE_END_CUT, a.GUIDE_MAX_BOUNCES, a.GUIDE_DEFAULT_MAX_BOUNCES) == (0, 1, 2, 64, 8)


def test_the_csharp_binding_declares_the_same_layouts(rt):
    doc = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    for name, c_name in C_NAMES.items():
        m = re.search(r"\[StructLayout\(LayoutKind\.Explicit,\s*Size\s*=\s*(\d+)\)\]\s*public\s+(?:unsafe\s+)?struct\s+" + c_name + r"\s*(?://[^\n]*)?\s*\{(.*?)\}", doc, flags=re.S)
        assert m, "INTEGRATION.md section 1 declares %s with an explicit layout" % c_name
        fields = re.findall(r"\[FieldOffset\((\d+)\)\]\s*public\s+([\w\*]+)\s+(\w+)\s*;", m.group(2))
        S = getattr(rt.abi, name)
        assert int(m.group(1)) == C.sizeof(S), c_name
        assert [(n.lower(), int(off)) for off, _, n in fields] == [(f[0].lower(), getattr(S, f[0]).offset) for f in S._fields_], c_name
    for entry, n_args in zip(ENTRIES, (6, 5)):
        bind = re.search(r'EntryPoint\s*=\s*"' + entry + r'"[^\]]*\]\s*[^\n]*\n\s*public\s+static\s+extern\s+[^(]+\(([^)]*)\)', doc)
        assert bind, "INTEGRATION.md binds " + entry
        assert len([a for a in bind.group(1).split(",")]) == n_args, entry


def test_the_library_exports_the_calls_without_a_version_change(rt):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r"\bT " + name + "$", out, flags=re.M), name
        assert name in rt.abi.EXPORTED_SYMBOLS
    assert rt.lib.load().rtowGetApiVersion() == rt.abi.RTOW_API_VERSION == 12
    assert callable(rt.Context.trace_guide_rays) and callable(rt.Context.trace_guide_view)


def test_invalid_arguments_are_rejected_without_a_device(rt):
    lib = rt.lib.load()
    a = rt.abi
    bad = a.RTOW_ERROR_INVALID_VALUE
    fake = 0x10000                                                                 # never dereferenced: validation fails first
    out = a.guide_buffers({k: fake * (i + 1) for i, k in enumerate(a.GUIDE_OUTPUTS)})
    params = a.GuideParams(8, 0, 0)
    view = a.TraceViewParams(8, 8, a.View(), 0.0, 0)
    assert lib.rtowTraceGuideRaysDevice(None, None, 0, None, None, None) == bad
    assert lib.rtowTraceGuideRaysDevice(None, C.byref(params), 4, fake, C.byref(out), None) == bad           # no context
    assert lib.rtowTraceGuideViewDevice(None, None, None, None, None) == bad
    assert lib.rtowTraceGuideViewDevice(None, C.byref(params), C.byref(view), C.byref(out), None) == bad     # no context
