"""CPU: what a context's caches are valid for (csrc/rtow_launch_cache.h), decided without a device.

(i)   tests/native/launch_cache_host.cpp under the address and undefined-behaviour sanitizers, as a stand-alone program (nothing is loaded into Python): a fresh Keyed
      holds nothing, a single changed member of either key is a different key, drop empties it, and decodeSchedulerKnob over every word.
(ii)  decodeSchedulerKnob through a plain ctypes shim against the packing of RtowContextOptions.schedulerTune[7] written out here, for every word in [-1, 65536].
(iii) The source rule.  Every `A.<field>` that primary_candidates_kernel reads is in the table below, as a member of the lists' key - then the key's builder reads it -
      or as fixed by rtowUploadScene, which the key's scene serial covers.  A field the kernel reads later fails here until someone decides where it belongs."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing-in-one-weekend_amd", "csrc")
HEADER = os.path.join(CSRC, "rtow_launch_cache.h")
GXX = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"]


# ------------------------------------------------------------------ (i) ------------------------------------------------------------------
def test_launch_cache_host_program_runs_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "launch_cache_host")
    src = os.path.join(ROOT, "tests", "native", "launch_cache_host.cpp")
    build = subprocess.run(GXX + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr


def test_the_header_is_host_only():
    includes = re.findall(r"^#include\s+[<\"]([^>\"]+)[>\"]", open(HEADER).read(), re.M)
    assert [i for i in includes if "/" in i or i.endswith(".h")] == ["../../include/rtow.h"], includes      # standard headers beside it, nothing of HIP, nothing of csrc


# ------------------------------------------------------------------ (ii) -----------------------------------------------------------------
DEFAULT_WORD = 3
REFUSED_LOW_NIBBLES = (5, 6, 7, 9, 10, 11, 12, 13, 14, 15)       # of a word in 1 .. 65 535; every word from 65 536 on is refused whatever its low nibble


def knob(given):
    """schedulerTune[7] as rtowCreateContext takes it: None for a refused word, else (word, ticketMapSide, regroupMode, orderByTotal, slotBlockOverride, pixelGateOverride)"""
    if given >= 65536 or (given > 0 and given % 16 in REFUSED_LOW_NIBBLES):
        return None
    word = given if given > 0 else DEFAULT_WORD
    if word % 16 == 0:
        word += DEFAULT_WORD                                      # only the upper fields given: the default side
    side = word % 16
    return (word, {1: 0, 3: 1, 2: 2, 4: 4, 8: 8}[side], word // 16 % 4, word // 64 % 2, word // 256 % 16, word // 4096 % 16)


@pytest.fixture(scope="module")
def shim():
    out_dir = os.path.join(ROOT, "tests", "build")
    os.makedirs(out_dir, exist_ok=True)
    src, so = os.path.join(ROOT, "tests", "native", "launch_cache_shim.cpp"), os.path.join(out_dir, "liblaunch_cache_shim.so")
    deps = [src, HEADER, os.path.join(ROOT, "include", "rtow.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(GXX + ["-O1", "-fPIC", "-shared", src, "-o", so], check=True, capture_output=True)
    lib = C.CDLL(so)
    lib.shim_decode_scheduler_knob.argtypes = [C.c_int, C.POINTER(C.c_int)]
    lib.shim_decode_scheduler_knob.restype = C.c_int
    return lib


def test_scheduler_knob_decodes_like_the_packing_for_every_word(shim):
    refused = 0
    for given in range(-1, 65537):
        out = (C.c_int * 6)(*([-77] * 6))
        ok = shim.shim_decode_scheduler_knob(given, out)
        want = knob(given)
        if want is None:
            refused += 1
            assert ok == 0 and list(out) == [-77] * 6, given
        else:
            assert ok == 1 and tuple(out) == want, (given, list(out), want)
    assert refused == 4096 * len(REFUSED_LOW_NIBBLES) + 1
    assert knob(-1) == knob(0) == knob(3) == (3, 1, 0, 0, 0, 0)
    assert knob(16) == (19, 1, 1, 0, 0, 0) and knob(0x4000) == (0x4003, 1, 0, 0, 0, 4) and knob(0x0201) == (0x0201, 0, 0, 0, 2, 0) and knob(64 + 8) == (72, 8, 0, 1, 0, 0)


# ------------------------------------------------------------------ (iii) ----------------------------------------------------------------
UPLOAD = "fixed by upload"
# A.<field> of primary_candidates_kernel -> the launch fields the key's builder reads for it, or UPLOAD (the scene serial of the key covers it)
KERNEL_INPUTS = {
    "totalWork": ("width", "height", "sliceOffset", "sliceDivider"),       # the owned pixels of the frame and slice
    "width": ("width",),
    "sliceOffset": ("sliceOffset",),
    "sliceDivider": ("sliceDivider",),
    "view": ("view",),
    "sizeX": ("sizeX",),
    "sizeY": ("sizeY",),
    "subPixelJitter": ("subPixelJitter",),
    "sceneBlob": UPLOAD,        # ctx->dScene: written by rtowUploadScene alone
    "wideCodes": UPLOAD,        # ctx->wideCodes: set by rtowUploadScene alone
    "layout": UPLOAD,           # ctx->scene.layout - but for exactTies, below
}


def _body(text, opening):
    """the text between the line that matches `opening` and the first line that is a closing brace alone"""
    at = re.search(opening, text, re.M)
    assert at, opening
    return text[at.end():text.index("\n}\n", at.end())]


def test_every_input_of_the_camera_list_kernel_is_in_the_key_or_fixed_by_the_upload():
    kernel = _body(open(os.path.join(CSRC, "rtow_kernels.hip")).read(), r"^__global__ void .*\bprimary_candidates_kernel\(SampleKernelArgs A, uint2\* __restrict__ out, int prune\)\n\{\n")
    read = set(re.findall(r"\bA\.(\w+)", kernel))
    assert read == set(KERNEL_INPUTS), ("not in the table", sorted(read - set(KERNEL_INPUTS)), "no longer read", sorted(set(KERNEL_INPUTS) - read))
    assert re.search(r"\bprune\b", kernel)
    builder = _body(open(HEADER).read(), r"^template <typename Launch> CameraListKey cameraListKey\(uint64_t sceneSerial, const Launch& a, bool prune\)\n\{\n")
    built_from = set(re.findall(r"\ba\.(\w+)", builder))
    for field, where in KERNEL_INPUTS.items():
        if where != UPLOAD:
            assert set(where) <= built_from, (field, where, sorted(built_from))
    assert re.search(r"\bsceneSerial\b", builder) and re.search(r"\bprune\b", builder)
    # the one part of `layout` that is not fixed by the upload: launches rewrite exactTies (the tie watch, the fix-up and the list launches), so the kernel must not read it
    assert "const SceneLayout& L = A.layout;" in kernel
    layout_read = set(re.findall(r"\bL\.(\w+)", kernel))
    assert layout_read and "exactTies" not in layout_read, sorted(layout_read)
    api = open(os.path.join(CSRC, "rtow_api.hip")).read()
    rewritten = set(re.findall(r"\b[ar]\.layout\.(\w+)\s*=[^=]", api))
    assert rewritten == {"exactTies"}, sorted(rewritten)
    assert not (rewritten & layout_read)
    # and what the table calls fixed by the upload reaches a launch from the context alone
    for line in ("a.sceneBlob = ctx->dScene;", "a.layout = ctx->scene.layout;", "a.wideCodes = ctx->wideCodes ? 1 : 0;"):
        assert line in api, line


def test_no_hand_kept_cache_configuration_is_left_in_the_sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".h", ".hip", ".cpp")):
            text = open(os.path.join(CSRC, name)).read()
            for word in ("pixCand", "orderValid", "orderW", "tunePendingScene"):
                assert word not in text, (name, word)
