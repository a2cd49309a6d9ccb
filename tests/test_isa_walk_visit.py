"""CPU: the vector instructions of one COMPILED sign-ordered node visit (the headline kernels <true, 0, 4 | 8, 0, 0, false, 0>; helpers and compile step of
tests/test_isa_walk_loop.py, whose own bound of 50 stays where it is).

The visit went from 50 to 44 vector instructions when three things that computed nothing the result needs left it (rtow_sample_kernel.hip.h, finishVisit / listLeaves /
popSlot): the leaf codes arrive ready to store (two inversions per visit), an empty stack pops the sentinel -1 by itself (a compare and a select), and the sign-ordered
loop tests a child with two compares instead of a min and a compare (two min).  Nothing in the source holds the compiler to that, so this reads the ISA: the loop is still
ONE basic block with one branch, no exec-mask save and the one traversal-stack store, and it has at most kVisitValu vector instructions.
"""
import pytest

from test_isa_walk_loop import walk_loops  # noqa: F401  (the module-scoped fixture: both units compiled once for this module)

kVisitValu = 44      # the count this build reaches, loop test included (50 before)


@pytest.mark.parametrize("hw", [4, 8])
def test_sign_ordered_visit_vector_instructions(walk_loops, hw):  # noqa: F811
    loops = walk_loops[(0, hw)]
    print(hw, loops)
    assert len(loops) == 2, loops
    ordered = min(loops, key=lambda l: l["instructions"])      # the sign-ordered loop is the shorter one (test_isa_walk_loop.py)
    assert ordered["blocks"] == 1 and ordered["branches"] == 1 and ordered["saveexec"] == 0, ordered
    assert ordered["stores"] == 1, ordered
    assert ordered["valu"] <= kVisitValu, ordered
