"""CPU: the ABI of rtowMeterExposureDevice and rtowFinalizeToneMappedDevice (include/rtow.h, added after API version 12 without changing it) - the exported symbols,
sizeof and the offsets of RtowExposureParams, RtowExposureState and RtowToneMapParams as g++ sees the header against the ctypes mirrors and the explicit-layout C#
structs, the bindings of INTEGRATION.md, the package's job classes and recommended values, and every refusal that needs no device."""
import ctypes as C
import math
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "raytracing-in-one-weekend_amd", "csrc", "librtow_hip.so")
NAMES = ("rtowMeterExposureDevice", "rtowFinalizeToneMappedDevice")
EXPOSURE_FIELDS = ("width", "height", "lowPermille", "highPermille", "compensation", "minStops", "maxStops", "rate", "flags", "reserved")
EXPOSURE_FLOATS = ("compensation", "minStops", "maxStops", "rate")
STATE_FIELDS = ("exposure", "stops", "targetStops", "meanLog2", "valid", "metered", "ignored", "reserved", "histogram")
STATE_FLOATS = ("exposure", "stops", "targetStops", "meanLog2")
TONE_FIELDS = ("pixelCount", "curve", "exposure", "flags", "reserved")

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "rtow.h"
#define O(T, f) printf(" %zu", offsetof(T, f))
int main(void)
{
    printf("%zu", sizeof(RtowExposureParams));
    O(RtowExposureParams, width); O(RtowExposureParams, height); O(RtowExposureParams, lowPermille); O(RtowExposureParams, highPermille); O(RtowExposureParams, compensation);
    O(RtowExposureParams, minStops); O(RtowExposureParams, maxStops); O(RtowExposureParams, rate); O(RtowExposureParams, flags); O(RtowExposureParams, reserved);
    printf(" %zu", sizeof(RtowExposureState));
    O(RtowExposureState, exposure); O(RtowExposureState, stops); O(RtowExposureState, targetStops); O(RtowExposureState, meanLog2); O(RtowExposureState, valid);
    O(RtowExposureState, metered); O(RtowExposureState, ignored); O(RtowExposureState, reserved); O(RtowExposureState, histogram);
    printf(" %zu", sizeof(RtowToneMapParams));
    O(RtowToneMapParams, pixelCount); O(RtowToneMapParams, curve); O(RtowToneMapParams, exposure); O(RtowToneMapParams, flags); O(RtowToneMapParams, reserved);
    printf(" %d %d %d %zu %d\n", (int)RTOW_TONE_CLAMP, (int)RTOW_TONE_ACES_FITTED, (int)RTOW_TONE_ACES_FILM, (size_t)RTOW_EXPOSURE_SCRATCH_BYTES, (int)RTOW_API_VERSION);
    return 0;
}
"""


def _csharp_struct(doc, name):
    cs = re.search(r"\[StructLayout\(LayoutKind\.Explicit,\s*Size\s*=\s*(\d+)\)\]\s*public\s+(?:unsafe\s+)?struct\s+%s\s*\{(.*?)\n    \}" % name, doc, flags=re.S)
    assert cs, name
    fields = re.findall(r"\[FieldOffset\((\d+)\)\]\s*public\s+((?:fixed\s+)?\w+)\s+(\w+)(?:\[(\d+)\])?;", cs.group(2))
    return int(cs.group(1)), [(int(o), t, n[0].lower() + n[1:], int(k) if k else 1) for o, t, n, k in fields]


def test_the_three_structs_have_one_layout_in_c_in_ctypes_and_in_the_csharp_binding(rt, tmp_path):
    src, exe = tmp_path / "tonemap_structs.c", tmp_path / "tonemap_structs"
    src.write_text(PROBE)
    subprocess.run(["g++", "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    seen = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    a = rt.abi
    P, S, T = a.ExposureParams, a.ExposureState, a.ToneMapParams
    assert seen[0] == C.sizeof(P) == 40
    assert tuple(f[0] for f in P._fields_) == EXPOSURE_FIELDS
    assert seen[1:11] == [getattr(P, f).offset for f in EXPOSURE_FIELDS] == list(range(0, 40, 4))
    assert seen[11] == C.sizeof(S) == 1056
    assert tuple(f[0] for f in S._fields_) == STATE_FIELDS
    assert seen[12:21] == [getattr(S, f).offset for f in STATE_FIELDS] == list(range(0, 36, 4)) and C.sizeof(S) - S.histogram.offset == 256 * 4
    assert seen[21] == C.sizeof(T) == 24
    assert tuple(f[0] for f in T._fields_) == TONE_FIELDS
    assert seen[22:27] == [getattr(T, f).offset for f in TONE_FIELDS] == [0, 4, 8, 12, 16]
    assert seen[27:30] == [a.RTOW_TONE_CLAMP, a.RTOW_TONE_ACES_FITTED, a.RTOW_TONE_ACES_FILM] == [a.TONE_CLAMP, a.TONE_ACES_FITTED, a.TONE_ACES_FILM] == [0, 1, 2]
    assert seen[30] == a.exposure_scratch_bytes() == 256 * 256 * 4 and seen[31] == 12
    doc = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    size, fields = _csharp_struct(doc, "RtowExposureParams")
    assert size == 40
    assert fields == [(o, "float" if f in EXPOSURE_FLOATS else "int", f, 1) for o, f in zip(range(0, 40, 4), EXPOSURE_FIELDS)]
    size, fields = _csharp_struct(doc, "RtowExposureState")
    assert size == 1056
    assert fields == [(o, "float" if f in STATE_FLOATS else "uint", f, 1) for o, f in zip(range(0, 32, 4), STATE_FIELDS[:8])] + [(32, "fixed uint", "histogram", 256)]
    size, fields = _csharp_struct(doc, "RtowToneMapParams")
    assert size == 24
    assert fields == [(0, "int", "pixelCount", 1), (4, "int", "curve", 1), (8, "float", "exposure", 1), (12, "int", "flags", 1), (16, "fixed int", "reserved", 2)]
    curve = re.search(r"enum\s+RtowToneCurve\s*\{([^}]*)\}", doc).group(1)
    assert [x.strip() for x in curve.split(",")] == ["Clamp = 0", "AcesFitted = 1", "AcesFilm = 2"]


def test_the_library_exports_both_passes_without_a_version_change(rt):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s$" % name, out, flags=re.M), name
        assert name in rt.abi.EXPORTED_SYMBOLS
    assert rt.lib.load().rtowGetApiVersion() == rt.abi.RTOW_API_VERSION == 12


def test_the_csharp_binding_declares_the_entry_points_and_the_frame_loop():
    doc = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rtow.h"), encoding="utf-8").read(), flags=re.S)
    for name, count in zip(NAMES, (6, 10)):
        decl = re.search(r"RTOW_API\s+int\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert decl and len(decl.group(1).split(",")) == count, name
        bind = re.search(r'EntryPoint\s*=\s*"%s"[^\]]*\]\s*[^\n]*\n\s*public\s+static\s+extern\s+[^(]+\(([^)]*)\)' % name, doc)
        assert bind, "INTEGRATION.md binds " + name
        args = [x.strip() for x in bind.group(1).split(",")]
        assert len(args) == count, (name, args)
        if name == NAMES[0]:
            assert args[1].startswith("ref RtowExposureParams") and args[4].startswith("RtowExposureState*")
        else:
            assert args[1].startswith("ref RtowToneMapParams") and args[2].startswith("RtowExposureState*")
    loop = doc[doc.index("Auto-exposure and a tone curve in the finalize"):]
    at = 0
    for step in ("CombineDevice", "MeterExposureDevice", "FinalizeToneMappedDevice"):
        at = loop.find("RtowContext." + step, at)
        assert at >= 0, "the frame loop, in its order: " + step


def test_the_package_exports_the_jobs_and_the_recommended_values(rt):
    a = rt.abi
    assert rt.ExposureJob is rt.host.ExposureJob and rt.ToneMapJob is rt.host.ToneMapJob and "ExposureJob" in rt.__all__ and "ToneMapJob" in rt.__all__
    p = rt.ExposureJob(None, 96, 54).params()
    assert (p.width, p.height, p.lowPermille, p.highPermille, p.flags, p.reserved) == (96, 54, a.EXPOSURE_DEFAULT_LOW_PERMILLE, a.EXPOSURE_DEFAULT_HIGH_PERMILLE, 0, 0)
    assert (a.EXPOSURE_DEFAULT_LOW_PERMILLE, a.EXPOSURE_DEFAULT_HIGH_PERMILLE, a.EXPOSURE_DEFAULT_MIN_STOPS, a.EXPOSURE_DEFAULT_MAX_STOPS) == (500, 950, -8, 8)
    assert p.compensation == a.EXPOSURE_DEFAULT_COMPENSATION == C.c_float(math.log2(0.18)).value
    assert (p.minStops, p.maxStops, p.rate) == (-8.0, 8.0, 1.0) and a.EXPOSURE_DEFAULT_RATE == 1.0 and a.EXPOSURE_BINS == 256
    q = rt.ExposureJob(None, 8, 4, LowPermille=0, HighPermille=1000, Compensation=0.0, MinStops=-1, MaxStops=2, Rate=0.25).params()
    assert (q.lowPermille, q.highPermille, q.compensation, q.minStops, q.maxStops, q.rate) == (0, 1000, 0.0, -1.0, 2.0, 0.25)
    t = rt.ToneMapJob(None, 5184).params()
    assert (t.pixelCount, t.curve, t.exposure, t.flags, list(t.reserved)) == (5184, a.TONE_DEFAULT_CURVE, 1.0, 0, [0, 0])
    assert a.TONE_DEFAULT_CURVE == a.TONE_ACES_FITTED and a.TONE_DEFAULT_EXPOSURE == 1.0 and a.TONE_CURVES == (0, 1, 2)
    t = rt.ToneMapJob(None, 7, Curve=a.TONE_ACES_FILM, Exposure=0.5).params()
    assert (t.curve, t.exposure) == (2, 0.5)


def test_invalid_arguments_are_rejected_without_a_device(rt):
    """What can be refused without a device: a context exists only on a GPU, and the context is what both calls check first, so these are the calls without one (the
    addresses are never dereferenced) - with arguments that are otherwise good, and with each rejection of the validation lists on top.  The same rejections WITH a
    context - which is where each of them decides - are in tests/test_gpu_tonemap.py."""
    lib = rt.lib.load()
    a = rt.abi
    bad = a.RTOW_ERROR_INVALID_VALUE
    fake = [0x1000000 * k for k in range(1, 12)]
    nan, inf = float("nan"), float("inf")
    good = [8, 8, 500, 950, -2.5, -8.0, 8.0, 1.0, 0, 0]

    def meter(values=good, color=fake[0], scratch=fake[1], state=fake[2], params=True):
        p = a.ExposureParams(*values)
        return lib.rtowMeterExposureDevice(None, C.byref(p) if params else None, color, scratch, state, None)

    assert meter() == bad                                                  # no context
    assert lib.rtowMeterExposureDevice(None, None, None, None, None, None) == bad
    assert meter(params=False) == bad and meter(color=None) == bad and meter(scratch=None) == bad and meter(state=None) == bad
    for index, value in ((0, 0), (1, -1), (0, 65536), (2, -1), (2, 951), (3, 1001), (4, nan), (4, inf), (4, -inf), (5, -32.5), (5, 8.5), (6, 32.5), (5, nan), (6, nan),
                         (7, nan), (7, -0.25), (7, 1.25), (8, 1), (9, 1)):
        p = list(good)
        p[index] = value
        if (index, value) == (0, 65536):
            p[1] = 65536                                                   # width * height beyond INT32_MAX
        assert meter(p) == bad, (index, value)
    assert meter(scratch=fake[0] + 4) == bad and meter(state=fake[0] + 8 * 8 * 12 - 4) == bad and meter(state=fake[1] + 256 * 256 * 4 - 4) == bad      # forbidden overlaps

    def tone(values=(64, 1, 1.0, 0, (0, 0)), state=fake[3], ins=fake[4:7], outs=fake[7:10], params=True):
        p = a.ToneMapParams(values[0], values[1], values[2], values[3], (C.c_int32 * 2)(*values[4]))
        return lib.rtowFinalizeToneMappedDevice(None, C.byref(p) if params else None, state, ins[0], ins[1], ins[2], outs[0], outs[1], outs[2], None)

    assert tone() == bad                                                   # no context
    assert lib.rtowFinalizeToneMappedDevice(None, None, None, None, None, None, None, None, None, None) == bad
    assert tone(params=False) == bad and tone(ins=[None, fake[5], fake[6]]) == bad and tone(outs=[None, fake[8], fake[9]]) == bad
    assert tone(ins=[fake[4], None, fake[6]]) == bad and tone(outs=[fake[7], fake[8], None]) == bad                # half a guide pair
    for values in ((0, 1, 1.0, 0, (0, 0)), (-1, 1, 1.0, 0, (0, 0)), (64, 3, 1.0, 0, (0, 0)), (64, -1, 1.0, 0, (0, 0)), (64, 1, -0.5, 0, (0, 0)), (64, 1, nan, 0, (0, 0)),
                   (64, 1, inf, 0, (0, 0)), (64, 1, 1.0, 1, (0, 0)), (64, 1, 1.0, 0, (1, 0)), (64, 1, 1.0, 0, (0, 1))):
        assert tone(values) == bad, values
    assert tone(outs=[fake[4] + 64 * 12 - 4, fake[8], fake[9]]) == bad and tone(outs=[fake[7], fake[7] + 64 * 4 - 4, fake[9]]) == bad      # an input, another output
    assert tone(outs=[fake[7], fake[8], fake[3] + 1052]) == bad            # the state
