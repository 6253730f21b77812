"""What the compiler makes of the two kernels of ``sgw_iqn_backward`` (iqn_backward.h, over iqn_forward.h's device functions), checked without
a device: the headers as one small translation unit, cross-compiled for gfx950 (the recipe of ``tests/test_learner_codegen.py``).

* no scratch and no spills in either kernel (iqn_bwd_rows_kernel holds three GEMMs' staging; its tile loop keeps L opaque so that their
  loop-invariant addresses are not hoisted into registers it does not have), two waves per SIMD for the 512-thread rows kernel;
* the rows kernel's LDS is iqn_quantile_kernel's three images (below the 160 KiB of a CU), the weight-gradient kernel uses none;
* every float operation is rounded on its own (``#pragma clang fp contract(off)`` reaches the shared device functions);
* no atomics; the weight-gradient kernel is one chain of 32x32x2 matrix instructions per tile, kBwdAhead of them per loop body."""
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as G
from tests.test_learner_codegen import SYSTEM, _float_ops, _one

ROOT = G.ROOT
CHAIN = (*G.JIT_PARTS, "iqn_forward.h", "iqn_backward.h")
ROWS, WGRAD = "19iqn_bwd_rows_kernel", "16iqn_wgrad_kernel"
AHEAD = 8


def _compile(tmp, out, *flags):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.isfile(hipcc):
        pytest.fail("no hipcc: the kernels cannot be cross-compiled")
    csrc = os.path.join(ROOT, "sorrel_amd", "csrc")
    src = "".join(f"#include <{h}>\n" for h in SYSTEM) + '#include "' + os.path.join(ROOT, "include", "sgw.h") + '"\n'
    src += "".join(f'#include "{os.path.join(csrc, n)}"\n' for n in CHAIN)
    tu = tmp / "backward_tu.hip"
    tu.write_text(src)
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", *flags, "-o", str(tmp / out), str(tu)]
    run = subprocess.run(cmd, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    return run.stderr


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    remarks = _compile(tmp_path_factory.mktemp("backward_obj"), "tu.o", "-c", "-Rpass-analysis=kernel-resource-usage")
    keys = (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
            ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("spill_v", r"VGPRs Spill: (\d+)"), ("spill_s", r"SGPRs Spill: (\d+)"),
            ("lds", r"LDS Size \[bytes/block\]: (\d+)"))
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
    tmp = tmp_path_factory.mktemp("backward_ir")
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
    tmp = tmp_path_factory.mktemp("backward_isa")
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


def test_rows_kernel_resources(usage):
    u = _one(usage, ROWS)
    print(u)
    assert u["scratch"] == 0 and u["spill_v"] == 0, u
    assert u["occupancy"] >= 2, u                                                # 512 threads = two waves per SIMD
    assert u["lds"] == 4 * (64 * 257 + 64 * 65 + 256 * 33 + 64 + 64), u          # X, Cb, Wl, tau_s, state_s
    assert u["lds"] <= 160 * 1024


def test_wgrad_kernel_resources(usage):
    u = _one(usage, WGRAD)
    print(u)
    assert u["scratch"] == 0 and u["spill_v"] == 0, u
    assert u["lds"] == 0, u
    assert u["vgpr"] + u["agpr"] <= 128 and u["occupancy"] >= 4, u                # a tile's 16 accumulators and 4 x kBwdAhead operands


@pytest.mark.parametrize("kernel", [ROWS, WGRAD])
def test_no_operation_may_contract(ir, kernel):
    flagged, plain = _float_ops(_one(ir, kernel))
    print(kernel, flagged, "of", flagged + plain)
    assert flagged == 0, (flagged, plain)
    if kernel == ROWS:
        assert plain > 0, "no float operation found: the IR is not what this test reads"


@pytest.mark.parametrize("kernel", [ROWS, WGRAD])
def test_no_atomics(isa, kernel):
    body = _one(isa, kernel)
    assert body and not [line for line in body if "atomic" in line]


def test_wgrad_is_one_chain_of_matrix_instructions_and_reads_memory_directly(isa):
    body = _one(isa, WGRAD)
    mfma = [line for line in body if line.startswith("v_mfma_f32_32x32x2")]
    assert len(mfma) == AHEAD, mfma                                              # the unrolled loop body; nothing else multiplies
    assert not [line for line in body if line.startswith("ds_")]
    assert sum(line.startswith("global_load_dword ") for line in body) >= 2 * AHEAD


def test_rows_kernel_runs_every_product_on_the_matrix_unit(isa):
    body = _one(isa, ROWS)
    mfma = [line for line in body if line.startswith("v_mfma_f32_32x32x2")]
    # three GEMMs (embedding, noisy, dz), each with the two-row-tile and the one-row-tile loop over a staged tile of 32 k; the embedding's
    # K = 64 is a constant, so both of its k-tiles are laid out
    assert len(mfma) == 4 * (2 * 16 + 16), len(mfma)
