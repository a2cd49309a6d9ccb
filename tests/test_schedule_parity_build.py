"""CPU: tests/native/schedule_parity.hip - the test-only program around csrc/rtow_schedule.hip.h that tests/test_gpu_schedule.py loads on the GPU box - still
cross-compiles for gfx950 with the product's flags and exports its three entry points.  A change to the header that breaks the program shows here, without a GPU;
the result is not loaded."""
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_schedule as gpu_side  # noqa: E402


def test_schedule_parity_cross_compiles():
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "libschedule_parity.so")
        proc = gpu_side.build_schedule_parity(so)
        assert proc.returncode == 0, proc.stderr[-3000:]
        symbols = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
        for name in ("schedule_chunk_order", "schedule_regroup", "schedule_init_map"):
            assert " T " + name in symbols, symbols
        # the launchers keep the library's hidden visibility: loading this next to librtow_hip.so cannot rebind either one's calls
        assert "launchRegroupTickets" not in symbols
