"""What the compiler makes of the learner kernels (policy.h, ppo_loss.h, iqn_loss.h, returns.h, reduce_stage1/2), checked without a
device: the kernel headers as one small translation unit with explicit instantiations, cross-compiled for gfx950.  These kernels share
their row arithmetic (categorical.h) and their workgroup reduction (block_reduce.h); what sharing could silently change is what no test
of the results on one shape would see --

* registers: a helper that costs a VGPR, a byte of scratch or a wave of occupancy in one instance;
* fp contract: ``#pragma clang fp contract(off)`` is lexical, so a helper without its own pragma fuses a product into a sum on behalf of
  a kernel that promises not to -- and a helper WITH the pragma un-fuses the moments of returns.h, which have always run contracted.

Bounds: ``tools/regs.py`` rows of the commit before the helpers were shared (6e388b5), reproduced with this very recipe on that tree."""
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as G

ROOT = G.ROOT
CHAIN = (*G.JIT_PARTS, "block_reduce.h", "small_kernels.h", "returns.h", "categorical.h", "policy.h", "ppo_loss.h", "iqn_loss.h")
SYSTEM = ("hip/hip_runtime.h", "stdint.h", "stddef.h", "algorithm", "type_traits")
INSTANCES = (
    "policy_sample_kernel<4, false, true>(const PolicyParams)",
    "policy_sample_kernel<16, true, false>(const PolicyParams)",
    "policy_sample_kernel<0, false, false>(const PolicyParams)",
    "ppo_loss_kernel<4, false, true>(const PpoLossParams)",
    "ppo_loss_kernel<16, true, true>(const PpoLossParams)",
    "ppo_loss_kernel<0, false, false>(const PpoLossParams)",
    "iqn_loss_kernel<64, true>(const IqnLossParams)",
    "iqn_loss_kernel<8, false>(const IqnLossParams)",
    "returns_kernel<2, false>(const ReturnsParams)",
    "returns_kernel<1, false>(const ReturnsParams)",
    "returns_normalize_all_kernel<false>(const ReturnsParams)",
)
# kernel -> (part of its mangled name, VGPRs, occupancy) on the parent; the non-template kernels come along with the headers
PARENT = {
    "policy_sample_kernel<4,false,true>": ("20policy_sample_kernelILi4ELb0ELb1EE", 62, 7),
    "policy_sample_kernel<16,true,false>": ("20policy_sample_kernelILi16ELb1ELb0EE", 93, 5),
    "policy_sample_kernel<0,false,false>": ("20policy_sample_kernelILi0ELb0ELb0EE", 78, 6),
    "ppo_loss_kernel<4,false,true>": ("15ppo_loss_kernelILi4ELb0ELb1EE", 107, 4),
    "ppo_loss_kernel<16,true,true>": ("15ppo_loss_kernelILi16ELb1ELb1EE", 156, 3),
    "ppo_loss_kernel<0,false,false>": ("15ppo_loss_kernelILi0ELb0ELb0EE", 101, 4),
    "ppo_loss_merge_kernel": ("21ppo_loss_merge_kernel", 19, 8),
    "iqn_loss_kernel<64,true>": ("15iqn_loss_kernelILi64ELb1EE", 51, 7),
    "iqn_loss_kernel<8,false>": ("15iqn_loss_kernelILi8ELb0EE", 49, 8),
    "iqn_loss_merge_kernel": ("21iqn_loss_merge_kernel", 11, 8),
    "returns_kernel<2,false>": ("14returns_kernelILi2ELb0EE", 63, 7),
    "returns_kernel<1,false>": ("14returns_kernelILi1ELb0EE", 67, 7),
    "returns_normalize_all_kernel<false>": ("28returns_normalize_all_kernelILb0EE", 28, 8),
    "reduce_stage1": ("13reduce_stage1", 14, 8),
    "reduce_stage2": ("13reduce_stage2", 12, 8),
}
# every operation of these is rounded on its own (include/sgw.h states the arithmetic term by term)
UNCONTRACTED = ("policy_sample_kernel<4,false,true>", "policy_sample_kernel<16,true,false>", "policy_sample_kernel<0,false,false>",
                "ppo_loss_kernel<4,false,true>", "ppo_loss_kernel<16,true,true>", "ppo_loss_kernel<0,false,false>", "ppo_loss_merge_kernel",
                "iqn_loss_kernel<64,true>", "iqn_loss_kernel<8,false>")


def _compile(tmp, out, *flags):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.isfile(hipcc):
        pytest.fail("no hipcc: the kernels cannot be cross-compiled")
    csrc = os.path.join(ROOT, "sorrel_amd", "csrc")
    src = "".join(f"#include <{h}>\n" for h in SYSTEM) + '#include "' + os.path.join(ROOT, "include", "sgw.h") + '"\n'
    src += "".join(f'#include "{os.path.join(csrc, n)}"\n' for n in CHAIN)
    src += "".join(f"template __global__ void {i};\n" for i in INSTANCES)
    tu = tmp / "learner_tu.hip"
    tu.write_text(src)
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", *flags, "-o", str(tmp / out), str(tu)]
    run = subprocess.run(cmd, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    return run.stderr


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """mangled name -> the compiler's resource-usage remarks of that kernel"""
    remarks = _compile(tmp_path_factory.mktemp("learner_obj"), "tu.o", "-c", "-Rpass-analysis=kernel-resource-usage")
    keys = (("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"),
            ("spill_v", r"VGPRs Spill: (\d+)"))
    table, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = table.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for key, pat in keys:
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
    return table


@pytest.fixture(scope="module")
def ir(tmp_path_factory):
    """mangled name -> the lines of that function's body in the device IR"""
    tmp = tmp_path_factory.mktemp("learner_ir")
    _compile(tmp, "tu.ll", "-emit-llvm", "-S")
    table, cur = {}, None
    for line in (tmp / "tu.ll").read_text().splitlines():
        m = re.match(r"define .*@(\w+)\(", line)
        if m:
            cur = table.setdefault(m.group(1), [])
        elif line.startswith("}"):
            cur = None
        elif cur is not None:
            cur.append(line)
    return table


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """mangled name -> the instruction lines of that kernel in the device assembly"""
    tmp = tmp_path_factory.mktemp("learner_isa")
    _compile(tmp, "tu.s", "-S")
    table, cur = {}, None
    for line in (tmp / "tu.s").read_text().splitlines():
        m = re.match(r"(_Z\w+):", line)
        if m:
            cur = table.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and line.startswith("\t") and not line.startswith("\t."):
            cur.append(line.strip())
    return table


def _float_ops(body):
    """(fmul / fadd / fsub / fdiv instructions carrying the contract flag, those without it)"""
    count = [0, 0]
    for line in body:
        m = re.search(r"= (?:fmul|fadd|fsub|fdiv) ((?:[a-z]+ )*)", line)
        if m:
            count["contract" not in m.group(1).split()] += 1
    return count


def _one(table, part):
    found = [k for k in table if part in k]
    assert len(found) == 1, (part, found)
    return table[found[0]]


@pytest.mark.parametrize("kernel", sorted(PARENT))
def test_registers_scratch_and_occupancy(usage, kernel):
    part, vgpr, occupancy = PARENT[kernel]
    u = _one(usage, part)
    print(kernel, u)
    assert u["scratch"] == 0, u
    assert u["spill_v"] == 0, u
    assert u["vgpr"] <= vgpr, u
    assert u["occupancy"] >= occupancy, u


@pytest.mark.parametrize("kernel", UNCONTRACTED)
def test_no_operation_may_contract(ir, kernel):
    flagged, plain = _float_ops(_one(ir, PARENT[kernel][0]))
    print(kernel, flagged, "of", flagged + plain)
    assert plain > 0, "no float operation found: the IR is not what this test reads"
    assert flagged == 0, (flagged, plain)


@pytest.mark.parametrize("kernel, rows", [("policy_sample_kernel<4,false,true>", 1), ("ppo_loss_kernel<4,false,true>", 1), ("ppo_loss_kernel<16,true,true>", 8)])
def test_vec_rows_are_read_sixteen_bytes_at_a_time(isa, kernel, rows):
    """cat_load_row reads a float32 row as four scalars off a pointer it declares 16-byte aligned and leaves it to the backend to make one
    load of them (HIP's float4 reached the backend as two halves before); a float64 row as 16-byte vectors.  Either way the kernel holds
    NA / 4 (NA / 2) 16-byte loads; nothing else in these kernels loads 16 bytes."""
    body = _one(isa, PARENT[kernel][0])
    assert sum(line.startswith("global_load_dwordx4") for line in body) == rows, [line for line in body if line.startswith("global_load")]


def test_returns_moments_stay_contracted(ir):
    """returns_kernel's body is compiled with contract off for the discount recurrence; moments_push, a helper, never was: the mean and the
    standard deviation it yields are the bits of fused operations.  Exactly the recurrence's 16 operations (a product and a sum for each of
    kReturnsChunk = 8 turns) are unflagged."""
    flagged, plain = _float_ops(_one(ir, PARENT["returns_kernel<2,false>"][0]))
    print(flagged, "of", flagged + plain)
    assert flagged > 0
    assert plain == 16
