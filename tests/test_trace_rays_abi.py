"""CPU: the ABI of rtowTraceRaysDevice / rtowTraceViewDevice (include/rtow.h, added after API version 12 without changing it) - the layouts of RtowRay, RtowHitBuffers
and RtowTraceViewParams as g++ sees the header against the ctypes mirrors and the explicit-layout C# structs of INTEGRATION.md section 1, the exported symbols, and the
argument validation that needs no device.  (A context cannot be created without a device, so only the NULL-context path of the validation is reachable here;
tests/test_gpu_trace_rays.py walks every other case with a real context.)"""
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
    printf("%zu %zu %zu %zu %zu\n", sizeof(RtowRay), offsetof(RtowRay, origin), offsetof(RtowRay, time), offsetof(RtowRay, direction), offsetof(RtowRay, pad));
    printf("%zu %zu %zu %zu\n", sizeof(RtowHitBuffers), offsetof(RtowHitBuffers, distance), offsetof(RtowHitBuffers, entityIndex), offsetof(RtowHitBuffers, normal));
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(RtowTraceViewParams), offsetof(RtowTraceViewParams, width), offsetof(RtowTraceViewParams, height),
           offsetof(RtowTraceViewParams, view), offsetof(RtowTraceViewParams, time), offsetof(RtowTraceViewParams, reserved));
    return 0;
}
"""
EXPECTED = {"Ray": [32, 0, 12, 16, 28], "HitBuffers": [24, 0, 8, 16], "TraceViewParams": [104, 0, 4, 8, 96, 100]}
C_NAMES = {"Ray": "RtowRay", "HitBuffers": "RtowHitBuffers", "TraceViewParams": "RtowTraceViewParams"}


def _probe(tmp_path):
    src, exe = tmp_path / "trace_layout.c", tmp_path / "trace_layout"
    src.write_text(PROBE)
    subprocess.run(["g++", "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    return {k: [int(x) for x in line.split()] for k, line in zip(("Ray", "HitBuffers", "TraceViewParams"), lines)}


def _mirror(rt, name):
    S = getattr(rt.abi, name)
    return [C.sizeof(S)] + [getattr(S, f[0]).offset for f in S._fields_]


def test_struct_layouts_match_the_ctypes_mirrors(rt, tmp_path):
    seen = _probe(tmp_path)
    for name, want in EXPECTED.items():
        assert seen[name] == want == _mirror(rt, name), (name, seen[name], _mirror(rt, name))
    assert [f[0] for f in rt.abi.Ray._fields_] == ["origin", "time", "direction", "pad"]
    assert [f[0] for f in rt.abi.HitBuffers._fields_] == ["distance", "entityIndex", "normal"]
    assert [f[0] for f in rt.abi.TraceViewParams._fields_] == ["width", "height", "view", "time", "reserved"]
    d = np.dtype(rt.abi.RAY_DTYPE)
    assert d.itemsize == 32 and [d.fields[k][1] for k in ("origin", "time", "direction", "pad")] == [0, 12, 16, 28]


def test_the_csharp_binding_declares_the_same_layouts(rt):
    doc = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    for name, c_name in C_NAMES.items():
        m = re.search(r"\[StructLayout\(LayoutKind\.Explicit,\s*Size\s*=\s*(\d+)\)\]\s*public\s+(?:unsafe\s+)?struct\s+" + c_name + r"\s*(?://[^\n]*)?\s*\{(.*?)\}", doc, flags=re.S)
        assert m, "INTEGRATION.md section 1 declares %s with an explicit layout" % c_name
        fields = re.findall(r"\[FieldOffset\((\d+)\)\]\s*public\s+([\w\*]+)\s+(\w+)\s*;", m.group(2))
        S = getattr(rt.abi, name)
        assert int(m.group(1)) == C.sizeof(S), c_name
        assert [(n.lower(), int(off)) for off, _, n in fields] == [(f[0].lower(), getattr(S, f[0]).offset) for f in S._fields_], c_name
    for entry, n_args in (("rtowTraceRaysDevice", 5), ("rtowTraceViewDevice", 5)):
        bind = re.search(r'EntryPoint\s*=\s*"' + entry + r'"[^\]]*\]\s*[^\n]*\n\s*public\s+static\s+extern\s+[^(]+\(([^)]*)\)', doc)
        assert bind, "INTEGRATION.md binds " + entry
        assert len([a for a in bind.group(1).split(",")]) == n_args, entry


def test_the_library_exports_the_queries_without_a_version_change(rt):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for name in ("rtowTraceRaysDevice", "rtowTraceViewDevice"):
        assert re.search(r"\bT " + name + "$", out, flags=re.M), name
        assert name in rt.abi.EXPORTED_SYMBOLS
    assert rt.lib.load().rtowGetApiVersion() == rt.abi.RTOW_API_VERSION == 12


def test_invalid_arguments_are_rejected_without_a_device(rt):
    lib = rt.lib.load()
    a = rt.abi
    bad = a.RTOW_ERROR_INVALID_VALUE
    fake = [0x10000 * k for k in range(1, 6)]          # never dereferenced: validation fails first
    hits = a.HitBuffers(fake[0], fake[1], fake[2])
    none = a.HitBuffers(None, None, None)
    good = a.TraceViewParams(8, 8, a.View(), 0.0, 0)
    assert lib.rtowTraceRaysDevice(None, 0, None, None, None) == bad
    assert lib.rtowTraceRaysDevice(None, 4, fake[3], C.byref(hits), None) == bad                 # no context
    assert lib.rtowTraceRaysDevice(None, -1, fake[3], C.byref(hits), None) == bad
    assert lib.rtowTraceRaysDevice(None, 4, fake[3], C.byref(none), None) == bad
    assert lib.rtowTraceViewDevice(None, None, None, None, None) == bad
    assert lib.rtowTraceViewDevice(None, C.byref(good), C.byref(hits), None, None) == bad        # no context
    for p in (a.TraceViewParams(0, 8, a.View(), 0.0, 0), a.TraceViewParams(8, -1, a.View(), 0.0, 0), a.TraceViewParams(65536, 32768, a.View(), 0.0, 0),
              a.TraceViewParams(8, 8, a.View(), 0.0, 1)):
        assert lib.rtowTraceViewDevice(None, C.byref(p), C.byref(hits), None, None) == bad
