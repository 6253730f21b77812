"""The burst emit of the headline kernel as the compiler leaves it, checked without a device: step_fast<true, 2, 6, 3, 32, 32>
cross-compiled with the recipe of tests/test_fast_codegen.py.  The interior iterations of common.h's burst_emit are a ds_read_b32, the four
byte-to-float converts and one streaming 16-byte store on a scalar base -- a vector compare or a 64-bit vector add in that loop is the
per-lane bookkeeping coming back -- and the instance as a whole issues fewer vector instructions than the commit before the helper."""
import os
import re

from tests import test_fast_codegen as F

KERNEL = "_Z9step_fastILb1ELi2ELi6ELi3ELi32ELi32E"
PARENT_VECTOR = 985     # v_* instructions of the instance before burst_emit, the versioned agent loop and philox_uniform (same recipe, same count)
FINAL_VECTOR = 953      # ... of this build: 996 with the burst helper alone (three copies of its body), 1 021 with the two windows of the agent loop,
                        # 953 once the sweep's blocks lost their uniform moves, reloads, and a multiplication and an exclusive-or each


def _body(tmp_path):
    F._compile(tmp_path, F.HEADLINE, extra=("-save-temps=obj",))
    asm = [p for p in os.listdir(tmp_path) if p.endswith(".s")]
    assert asm, os.listdir(tmp_path)
    text = "".join(open(os.path.join(tmp_path, p)).read() for p in asm)
    m = re.search(r"^%s\w*:" % KERNEL, text, re.M)
    assert m, "the headline instance is not in the assembly"
    body = text[m.end():]
    lines = [ln.strip() for ln in body[:body.index("s_endpgm")].splitlines()]
    return [ln for ln in lines if ln and not ln.startswith((";", "//"))]


def _loops_with(lines, pattern):
    """[first, last] line ranges of the innermost loops (a label and the last backward branch to it) that hold a line matching ``pattern``."""
    labels = {ln[:-1].split(":")[0]: i for i, ln in enumerate(lines) if re.match(r"^\.LBB\d+_\d+:", ln)}
    loops = []
    for i, ln in enumerate(lines):
        m = re.match(r"^s_cbranch_\w+ (\.LBB\d+_\d+)", ln) or re.match(r"^s_branch (\.LBB\d+_\d+)", ln)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            loops.append((labels[m.group(1)], i))
    out = []
    for i, ln in enumerate(lines):
        if re.search(pattern, ln):
            holding = [lp for lp in loops if lp[0] <= i <= lp[1]]
            if holding:
                out.append(min(holding, key=lambda lp: lp[1] - lp[0]))
    return sorted(set(out))


def test_burst_loop_has_no_vector_compare_and_no_64_bit_vector_add(tmp_path):
    lines = _body(tmp_path)
    stores = [ln for ln in lines if re.match(r"^global_store_dwordx4 .* nt$", ln)]
    assert stores, "no streaming 16-byte store in the headline instance"
    loops = _loops_with(lines, r"^global_store_dwordx4 .* nt$")
    assert loops, "no loop holds the streaming 16-byte store"
    for first, last in loops:
        loop = lines[first:last + 1]
        print("\n".join(loop))
        assert not [ln for ln in loop if ln.startswith("v_cmp")], "a vector compare in the burst loop"
        assert not [ln for ln in loop if ln.startswith("v_lshl_add_u64")], "a 64-bit vector add in the burst loop"
        # the store takes the scalar-base form: a 32-bit lane offset next to a scalar register pair
        assert [ln for ln in loop if re.match(r"^global_store_dwordx4 v\d+, v\[\d+:\d+\], s\[\d+:\d+\]", ln)], "the burst store has a vector base"


def test_vector_instruction_count_is_below_the_parents(tmp_path):
    lines = _body(tmp_path)
    n = sum(ln.startswith("v_") for ln in lines)
    print("vector instructions:", n)
    assert FINAL_VECTOR < PARENT_VECTOR
    assert n <= FINAL_VECTOR, (n, FINAL_VECTOR)
