"""CPU: the camera move of the hole-filling test (tests/test_gpu_sample_pixels.py, tests/pixel_list_holes.py) leaves holes, and fewer than half the frame - by the
numpy restatement of the reprojection on the oracle's first hits, so that the GPU test's two bounds are known to hold before it runs."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pixel_list_holes as ph  # noqa: E402


def test_the_dolly_leaves_holes_in_less_than_half_the_frame(rt, oracle):
    holes = ph.holes_on_the_cpu(rt, oracle)
    share = holes.mean()
    print("hole filling: %d of %d pixels (%.3f) carry nothing after the move" % (holes.sum(), holes.size, share))
    assert holes.size == ph.W * ph.H
    assert 0 < holes.sum() and share < 0.5
    assert holes.sum() >= 64                 # more than one 64-ticket pull of the sample kernel
