"""What the compiler makes of the headline kernel, checked without a device: step_fast<true, 2, 6, 3, 32, 32> cross-compiled for gfx950
the way tools/quick_regs.py does (the specialiser's translation unit + one explicit instantiation, down to an object file, so the
assembler sees the inline assembly too).  The kernel is bound by vector issue at 8 waves per SIMD: a register over the budget, a byte of
scratch or another scalar spilled into vector lanes (v_writelane / v_readlane are vector instructions) is a regression no test of the
results would see."""
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as G

ROOT = G.ROOT
HEADLINE = "step_fast<true, 2, 6, 3, 32, 32>"
# SGPRs the commit before the shared Philox pass spilled in this instance (measured from that build with this very recipe)
PARENT_SGPR_SPILL = 28


def _compile(tmp_path, instance, extra=()):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.isfile(hipcc):
        pytest.fail("no hipcc: the kernel cannot be cross-compiled")
    csrc = os.path.join(ROOT, "sorrel_amd", "csrc")
    src = "#include <hip/hip_runtime.h>\n#include <stdint.h>\n#include <stddef.h>\n#include \"" + os.path.join(ROOT, "include", "sgw.h") + "\"\n"
    src += "".join(f'#include "{os.path.join(csrc, n)}"\n' for n in G.JIT_PARTS)
    src += f"template __global__ void {instance}(const Params);\n"
    tu = tmp_path / "tu.hip"
    tu.write_text(src)
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           *extra, "-o", str(tmp_path / "tu.o"), str(tu)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stderr


def _usage(remarks, mangled_part):
    """The resource-usage remarks of the one kernel whose mangled name contains ``mangled_part``."""
    keys = (("vgpr", r" VGPRs: (\d+)"), ("sgpr", r"[^ ]SGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
            ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("spill_s", r"SGPRs Spill: (\d+)"), ("spill_v", r"VGPRs Spill: (\d+)"))
    found, cur = [], None
    for line in remarks.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)} if mangled_part in m.group(1) else None
            if cur is not None:
                found.append(cur)
            continue
        if cur is None:
            continue
        for key, pat in keys:
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
    assert len(found) == 1, [f["name"] for f in found]
    assert all(k in found[0] for k, _ in keys), found[0]
    return found[0]


def test_headline_instance_registers_scratch_and_spills(tmp_path):
    u = _usage(_compile(tmp_path, HEADLINE), "9step_fastILb1ELi2ELi6ELi3ELi32ELi32E")
    print(u)
    assert u["occupancy"] == 8, u
    assert u["vgpr"] <= 64, u
    assert u["scratch"] == 0, u
    assert u["spill_v"] == 0, u
    assert u["spill_s"] <= PARENT_SGPR_SPILL, u


def test_agent_loop_records_are_single_lane_writes(tmp_path):
    """The agent loop's per-lane records (reward; moved / bad type) leave scalar registers through v_writelane with the lane in M0 -- the form
    the helper in common.h emits -- and the reward total is one unconditional v_add_f64."""
    _compile(tmp_path, HEADLINE, extra=("-save-temps=obj",))
    asm = [p for p in os.listdir(tmp_path) if p.endswith(".s")]
    assert asm, os.listdir(tmp_path)
    text = "".join(open(os.path.join(tmp_path, p)).read() for p in asm)
    body = text[text.index("_Z9step_fastILb1ELi2ELi6ELi3ELi32ELi32E"):]
    assert len(re.findall(r"v_writelane_b32 v\d+, s\d+, m0", body)) >= 2, "the loop's records are not single-lane writes"
    assert len(re.findall(r"v_add_f64", body)) == 1, "the reward total is more than one add"
