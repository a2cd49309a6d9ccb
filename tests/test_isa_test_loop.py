"""CPU: the vector instructions of one COMPILED exact sphere test (the TEST loop of the headline kernels <true, 0 | 1, 4 | 8, 0, 0, false, 0>; compile step and
kernel parser of tests/test_isa_walk_loop.py).

Every quotient t = n / a of a TEST run divides by the run's a = dot(rd, rd), so the loop takes it from the run's correctly rounded reciprocal in three instructions
(rtow_hit_tests.hip.h, sphere_hit_shared_rcp / sphere_root_quotient: v_mul, v_fma, v_fmac - exact_div_step), one quotient a candidate, and keeps hipcc's IEEE expansion
for the operands outside exact_div3's ranges only.  Before that the expansion (12 vector instructions and a class test) sat on the path every wave takes - 53 vector
instructions an iteration, 67 as soon as one lane of the wave took the second root, whose own expansion followed the first.  Nothing in the source holds the compiler
to the short form, so this reads the ISA.

The loop: the innermost natural loop (control-flow graph of the kernel, dominators) that holds the candidate load `ds_read_u16` and a `ds_read_b128` (the sphere) and
no LDS store (the box walks pop with a 16-bit read and load nodes 128 bits at a time too, but they store their stack).  Its basic blocks that hold a `v_div_scale_f32`
or a `v_sqrt_f32` are the fallbacks; the others are what a wave of ordinary rays executes.  Asserted for all four kernels:

  * the other blocks hold the quotient: `v_mul_f32 q, y, n`, `v_fma_f32 r, -a, q, n`, `v_fmac_f32 q, r, y` with y and a written nowhere in the loop (the run's);
  * the loop still holds the fallback division: a `v_div_scale_f32` whose divisor is that same a;
  * the other blocks add up to at most kTestValu vector instructions, the count this build reaches.  The natural loop takes in every block of the iteration, the
    rarely entered ones too (the rank rule of a tie, its mark, the accepted hit): 48 / 50 in the static-sphere kernels, 57 in the moving-sphere ones.  Their
    predecessors have 45 / 46 and 54 by the same count, but there the count leaves out the division every candidate with a positive numerator pays (13 more vector
    instructions in that block: 58 / 59 and 67 on the ordinary path, and 12 more for the second root's division as soon as one lane of the wave takes it).  A
    hand count along the ordinary path alone, without the rare blocks, gave 53 for the static-sphere kernels' predecessors.

What the count can and cannot see: a block is a fallback by what it CONTAINS, so an IEEE division that came back onto the path every wave takes would take its block
out of the sum instead of raising it, and the bound alone would hold on the predecessors too (45 <= 48).  The first assertion is what tells the builds apart - the one
quotient from the run's reciprocal must stand in a block without a division - and the bound then holds that path's length.

Mnemonics, block structure and register names only.
"""
import os
import re
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

from test_isa_walk_loop import UNITS, _compile, kernel_items

BRANCH = re.compile(r"s_cbranch_\w+|s_branch\b")
# vector instructions of the blocks without a fallback, per (kind, hw): static spheres 4 / 8 words, moving spheres 4 / 8 words
kTestValu = {(0, 4): 48, (0, 8): 50, (1, 4): 57, (1, 8): 57}


def basic_blocks(items):
    """the kernel as basic blocks: [{"labels": [...], "insts": [...], "succ": [block indices]}]"""
    blocks = [{"labels": [], "insts": []}]
    for kind, text in items:
        if kind in ("label", "block"):
            if blocks[-1]["insts"]:
                blocks.append({"labels": [], "insts": []})
            if kind == "label":
                blocks[-1]["labels"].append(text)
            continue
        blocks[-1]["insts"].append(text)
        if BRANCH.match(text) or text.startswith(("s_endpgm", "s_setpc_b64", "s_swappc_b64")):
            blocks.append({"labels": [], "insts": []})
    if not blocks[-1]["insts"]:
        blocks.pop()
    at = {lab: i for i, b in enumerate(blocks) for lab in b["labels"]}
    for i, b in enumerate(blocks):
        lastInst = b["insts"][-1]
        succ = []
        if BRANCH.match(lastInst):
            succ.append(at[lastInst.split()[-1]])
        if not lastInst.startswith(("s_branch", "s_endpgm", "s_setpc_b64")) and i + 1 < len(blocks):
            succ.append(i + 1)
        b["succ"] = succ
    return blocks


def dominators(blocks):
    """immediate-dominator-free form: dom[i] = set of blocks that dominate block i (iterative data flow over a reverse post-order)"""
    n = len(blocks)
    pred = [[] for _ in range(n)]
    for i, b in enumerate(blocks):
        for s in b["succ"]:
            pred[s].append(i)
    order, seen, stack = [], {0}, [(0, iter(blocks[0]["succ"]))]
    while stack:
        node, it = stack[-1]
        nxt = next((s for s in it if s not in seen), None)
        if nxt is None:
            order.append(node)
            stack.pop()
        else:
            seen.add(nxt)
            stack.append((nxt, iter(blocks[nxt]["succ"])))
    order.reverse()
    dom = {0: {0}}
    changed = True
    while changed:
        changed = False
        for i in order[1:]:
            ps = [dom[p] for p in pred[i] if p in dom]
            new = set.intersection(*ps) | {i} if ps else {i}
            if dom.get(i) != new:
                dom[i] = new
                changed = True
    return dom, pred


def natural_loops(blocks):
    """head block -> the set of blocks of its natural loop (back edges latch -> head with head dominating latch, merged per head)"""
    dom, pred = dominators(blocks)
    loops = {}
    for latch, b in enumerate(blocks):
        for head in b["succ"]:
            if latch in dom and head in dom[latch]:
                body = loops.setdefault(head, {head})
                work = [latch]
                while work:
                    x = work.pop()
                    if x not in body:
                        body.add(x)
                        work.extend(pred[x])
    return loops


def exact_test_loop(items):
    blocks = basic_blocks(items)
    found = []
    for head, body in natural_loops(blocks).items():
        insts = [t for i in body for t in blocks[i]["insts"]]
        if any(t.startswith("ds_read_u16") for t in insts) and any(t.startswith("ds_read_b128") for t in insts) and not any(t.startswith("ds_write") for t in insts):
            found.append(body)
    assert found, "no loop with the candidate load, a 128-bit LDS load and no LDS store"
    body = min(found, key=len)
    return [blocks[i]["insts"] for i in sorted(body)]


def _regs(operand):
    """vector registers an operand names: v7 -> {7}, v[82:85] -> {82 .. 85}, anything else -> {}"""
    m = re.fullmatch(r"-?\|?v(\d+)\|?", operand)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", operand)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()


def _operands(inst):
    return [o.strip() for o in inst.split(None, 1)[1].split(",")] if " " in inst else []


def written_vgprs(loop):
    out = set()
    for b in loop:
        for t in b:
            if t.startswith(("v_", "ds_read", "global_load", "buffer_load", "scratch_load", "flat_load")) and not t.startswith("v_cmp"):
                out |= _regs(_operands(t)[0])
    return out


def shared_reciprocal_quotients(loop, hot):
    """(y, a) register pairs of every v_mul / v_fma / v_fmac quotient in the `hot` blocks whose reciprocal y and divisor a are written nowhere in the loop"""
    written = written_vgprs(loop)
    out = []
    for b in hot:
        for i, t in enumerate(b):
            if not t.startswith("v_mul_f32"):
                continue
            q, x0, x1 = _operands(t)[:3]
            for j in range(i + 1, min(i + 4, len(b))):
                if not b[j].startswith("v_fma_f32"):
                    continue
                r, na, fq, n = _operands(b[j])[:4]
                if not (na.startswith("-") and fq == q and n in (x0, x1)):
                    continue
                y = x1 if n == x0 else x0
                a = na[1:]
                for k in range(j + 1, min(j + 4, len(b))):
                    if b[k].startswith("v_fmac_f32") and _operands(b[k])[:3] in ([q, r, y], [q, y, r]):
                        if _regs(y) and _regs(a) and not (_regs(y) | _regs(a)) & written:
                            out.append((y, a))
    return out


@pytest.fixture(scope="module")
def exact_test_loops():
    with tempfile.TemporaryDirectory() as tmp:
        dirs = {u: os.path.join(tmp, u) for u in UNITS}
        for d in dirs.values():
            os.makedirs(d)
        with ThreadPoolExecutor(2) as pool:
            asm = dict(zip(dirs, pool.map(lambda u: _compile(u, dirs[u]), dirs)))
    out = {}
    for unit, kind in UNITS.items():
        kernels = kernel_items(asm[unit])
        for hw in (4, 8):
            out[(kind, hw)] = exact_test_loop(kernels[(1, kind, hw, 0, 0, 0, 0)])
    return out


@pytest.mark.parametrize("kind,hw", [(0, 4), (0, 8), (1, 4), (1, 8)])
def test_exact_test_loop_takes_its_quotient_from_the_runs_reciprocal(exact_test_loops, kind, hw):
    loop = exact_test_loops[(kind, hw)]
    fallback = [b for b in loop if any(t.startswith(("v_div_scale_f32", "v_sqrt_f32")) for t in b)]
    hot = [b for b in loop if b not in fallback]
    valu = sum(1 for b in hot for t in b if t.startswith("v_"))
    quotients = shared_reciprocal_quotients(loop, hot)
    scales = [_operands(t) for b in loop for t in b if t.startswith("v_div_scale_f32")]
    print((kind, hw), "blocks", len(loop), "fallback blocks", len(fallback), "VALU outside them", valu, "VALU in all", sum(1 for b in loop for t in b if t.startswith("v_")),
          "quotients (y, a)", quotients, "v_div_scale_f32", len(scales))
    assert len(quotients) == 1, "one quotient a candidate, from the run's reciprocal, outside the fallback blocks"
    a = quotients[0][1]
    # v_div_scale_f32 vdst, sdst, src0, divisor, numerator: the fallback n / a divides by the quotient's own a
    assert any(ops[3] == a for ops in scales), ("the loop has lost its IEEE fallback for n / a", scales)
    assert valu <= kTestValu[(kind, hw)], valu
