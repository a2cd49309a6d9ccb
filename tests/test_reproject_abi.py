"""CPU: the ABI of rtowReprojectAccumDevice (include/rtow.h, added after API version 12 without changing it) - RtowReprojectParams' layout as g++ sees the
header against the ctypes mirror and the explicit-layout C# struct of INTEGRATION.md section 1, the exported symbol, and every refusal of the argument
validation, which needs no device.  (A context cannot be created without a device, so each refusal is reached here with a NULL context, which is itself one;
tests/test_gpu_reproject.py walks them again with a real context and shows that nothing was enqueued.)"""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "raytracing-in-one-weekend_amd", "csrc", "librtow_hip.so")
NAMES = ["width", "height", "previousView", "depthTolerance", "maxHistory", "flags", "reserved"]

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "rtow.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(RtowReprojectParams), offsetof(RtowReprojectParams, width), offsetof(RtowReprojectParams, height),
           offsetof(RtowReprojectParams, previousView), offsetof(RtowReprojectParams, depthTolerance), offsetof(RtowReprojectParams, maxHistory),
           offsetof(RtowReprojectParams, flags), offsetof(RtowReprojectParams, reserved), (int)RTOW_REPROJECT_MATCH_ENTITY);
    return 0;
}
"""


def test_reproject_params_layout_matches_the_ctypes_mirror(rt, tmp_path):
    src, exe = tmp_path / "reproject_layout.c", tmp_path / "reproject_layout"
    src.write_text(PROBE)
    subprocess.run(["g++", "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    seen = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = rt.abi.ReprojectParams
    assert [f[0] for f in P._fields_] == NAMES
    assert [C.sizeof(P)] + [getattr(P, n).offset for n in NAMES] == seen[:8] == [112, 0, 4, 8, 96, 100, 104, 108]
    assert P._fields_[2][1] is rt.abi.View and P._fields_[3][1] is C.c_float and P._fields_[4][1] is C.c_int32
    assert seen[8] == rt.abi.RTOW_REPROJECT_MATCH_ENTITY == 1
    a = rt.abi
    assert (a.REPROJECT_DEFAULT_DEPTH_TOLERANCE, a.REPROJECT_DEFAULT_MAX_HISTORY, a.REPROJECT_DEFAULT_FLAGS) == (0.01, 64, a.RTOW_REPROJECT_MATCH_ENTITY)


def test_the_csharp_binding_declares_the_same_layout(rt):
    doc = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    m = re.search(r"\[StructLayout\(LayoutKind\.Explicit,\s*Size\s*=\s*(\d+)\)\]\s*public\s+(?:unsafe\s+)?struct\s+RtowReprojectParams\s*\{(.*?)\}", doc, flags=re.S)
    assert m, "INTEGRATION.md section 1 declares RtowReprojectParams with an explicit layout"
    fields = re.findall(r"\[FieldOffset\((\d+)\)\]\s*public\s+(\w+)\s+(\w+)\s*;", m.group(2))
    P = rt.abi.ReprojectParams
    assert int(m.group(1)) == C.sizeof(P) == 112
    assert [(name.lower(), int(off)) for off, _, name in fields] == [(f[0].lower(), getattr(P, f[0]).offset) for f in P._fields_]
    assert [t for _, t, _ in fields] == ["int", "int", "RtowView", "float", "int", "int", "int"]
    bind = re.search(r'EntryPoint\s*=\s*"rtowReprojectAccumDevice"[^\]]*\]\s*[^\n]*\n\s*public\s+static\s+extern\s+[^(]+\(([^)]*)\)', doc)
    assert bind, "INTEGRATION.md binds rtowReprojectAccumDevice"
    args = [a.strip() for a in bind.group(1).split(",")]
    assert len(args) == 9 and args[1].startswith("ref RtowReprojectParams") and args[3].startswith("ref RtowHitBuffers") and args[4].startswith("ref RtowHitBuffers")


def test_the_library_exports_the_pass_without_a_version_change(rt):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rtowReprojectAccumDevice$", out, flags=re.M)
    assert "rtowReprojectAccumDevice" in rt.abi.EXPORTED_SYMBOLS
    assert rt.lib.load().rtowGetApiVersion() == rt.abi.RTOW_API_VERSION == 12


def _view(rt):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import reproject_reference as rr
    return rr.make_view((0.0, 1.0, 6.0), (0.0, 0.0, 0.0), 8, 8)


def test_invalid_arguments_are_rejected_without_a_device(rt):
    lib = rt.lib.load()
    a = rt.abi
    bad = a.RTOW_ERROR_INVALID_VALUE
    view = _view(rt)
    n = 64
    base = 0x100000                                  # never dereferenced: validation fails first
    addr = {k: base + 0x1000 * i for i, k in enumerate(("rays", "d", "e", "pd", "pe", "pc", "pn", "pa", "ps", "oc", "on", "oa", "os", "src"))}

    def call(ctx=None, params=(8, 8, view, 0.01, 64, 1, 0), **over):
        p = {**addr, **over}
        hits, prev_hits = a.HitBuffers(p["d"], p["e"], None), a.HitBuffers(p["pd"], p["pe"], None)
        prev, out = a.AccumBuffers(p["pc"], p["pn"], p["pa"], p["ps"]), a.AccumBuffers(p["oc"], p["on"], p["oa"], p["os"])
        return lib.rtowReprojectAccumDevice(ctx, C.byref(a.ReprojectParams(*params)), p["rays"], C.byref(hits), C.byref(prev_hits), C.byref(prev), C.byref(out),
                                            p["src"], None)

    assert lib.rtowReprojectAccumDevice(None, None, None, None, None, None, None, None, None) == bad
    assert call() == bad                                                              # no context
    for name in addr:                                                                 # a NULL ray array / required member (outSource alone may be NULL)
        assert call(**{name: None}) == bad, name
    flat = a.View()                                                                   # all zero: LF, HR and VU are 0
    nan_view = _view(rt)
    nan_view.horizontal.x = float("nan")
    for params in ((0, 8, view, 0.01, 64, 1, 0), (8, -1, view, 0.01, 64, 1, 0), (65536, 32768, view, 0.01, 64, 1, 0), (8, 8, view, -0.01, 64, 1, 0),
                   (8, 8, view, float("nan"), 64, 1, 0), (8, 8, view, float("inf"), 64, 1, 0), (8, 8, view, 0.01, 0, 1, 0), (8, 8, view, 0.01, -5, 1, 0),
                   (8, 8, view, 0.01, 64, 2, 0), (8, 8, view, 0.01, 64, -1, 0), (8, 8, view, 0.01, 64, 1, 1), (8, 8, flat, 0.01, 64, 1, 0),
                   (8, 8, nan_view, 0.01, 64, 1, 0)):
        assert call(params=params) == bad, params[:2] + params[3:]
    # an output on a buffer the pass gathers from, or on another output (partial overlaps included)
    for over in ({"oc": addr["pc"]}, {"on": addr["pc"] + n * 16 - 4}, {"os": addr["ps"] + 4}, {"src": addr["pa"]}, {"oa": addr["pd"]}, {"src": addr["pe"]},
                 {"oc": addr["on"] - 8}, {"src": addr["os"]}, {"oa": addr["on"] + n * 12 - 4}):
        assert call(**over) == bad, over
