"""CPU tests of ``sgw_noisy_weights`` (sorrel_amd/csrc/noisy.h): the definition of its keyed normals restated in NumPy holds the conditions
the GPU test asks of the device's draws (so that test cannot fail on a bound the definition itself misses), the refusals (all come before
any launch: no device is needed), and what the compiler makes of the kernel, cross-compiled for gfx950."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as G
from sorrel_amd import _native as N
from tests import learner_common as LK
from tests import noisy_common as NC
from tests.test_learner_codegen import SYSTEM, _float_ops, _one

FORWARD, BACKWARD = "noisy_kernelILb0EE", "noisy_kernelILb1EE"


# ------------------------------------------------------------------------------------------------------------------ the definition
def test_the_stat_key_holds_the_conditions_with_room_for_the_devices_error():
    """2^20 draws of the GPU test's fixed key: mean, variance and range, each with the device's error allowance (2^-16 per element) to spare."""
    x = NC.keyed_normals(*NC.STAT_KEY, NC.STAT_COUNT)
    mean_cap, var_cap = NC.stat_bounds(NC.STAT_COUNT)
    mean, var, top = float(x.mean()), float(x.var()), float(np.abs(x).max())
    print(mean, var, top)
    slack = NC.EPS_CAP
    assert abs(mean) + slack <= mean_cap
    assert abs(var - 1.0) + 2 * slack * float(np.abs(x).mean()) + slack * slack <= var_cap
    assert top + slack <= NC.EPS_MAX
    # the two halves of a pair are uncorrelated, and so are neighbouring pairs
    assert abs(float(np.mean(x[0::2] * x[1::2]))) <= 5.0 / np.sqrt(x.size / 2)
    assert abs(float(np.mean(x[:-2] * x[2:]))) <= 5.0 / np.sqrt(x.size - 2)


@pytest.mark.parametrize("key", (NC.BASE_KEY,) + NC.OTHER_KEYS)
def test_every_drawn_key_gives_finite_normals_in_range_and_keys_differ(key):
    n = max(NC.COUNTS)
    x = NC.keyed_normals(*key, n)
    assert np.isfinite(x).all() and float(np.abs(x).max()) + NC.EPS_CAP <= NC.EPS_MAX
    for count in NC.COUNTS:                   # a shorter tensor is a prefix: element i depends on (key, i) alone
        assert np.array_equal(NC.keyed_normals(*key, count), x[:count])
    if key != NC.BASE_KEY:
        base = NC.keyed_normals(*NC.BASE_KEY, n)
        assert (np.abs(base - x) > 4 * NC.EPS_CAP).mean() > 0.9       # the device's draws will differ too


def test_box_muller_extremes():
    """u1 = 2^-24 gives the largest radius, below EPS_MAX; u1 = 1 gives radius 0 (no log of 0 anywhere)."""
    assert np.sqrt(-2.0 * np.log(2.0 ** -24)) < NC.EPS_MAX
    assert np.sqrt(-2.0 * np.log(np.float64(((0xFFFFFFFF >> 8) + 1)) * 2.0 ** -24)) == 0.0


def test_the_stream_has_a_number_of_its_own_and_the_binding_and_the_restatement_use_it():
    text = open(os.path.join(G.ROOT, "include", "sgw.h")).read()
    number = int(re.search(r"^enum \{ SGW_STREAM_NOISE = (\d+) \};", text, flags=re.M)[1])
    others = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+SGW_STREAM_([A-Z_]+)\s+(\d+)u?\b", text, flags=re.M)}
    assert len(others) == 12 and number not in others.values() and number < 16          # (four bits of the counter word hold the stream)
    assert N.STREAM_NOISE == number == 12
    assert N.NOISY_MAX_JOBS == int(re.search(r"^#define SGW_NOISY_MAX_JOBS (\d+)", text, flags=re.M)[1]) >= 24


# ------------------------------------------------------------------------------------------------------------------ refusals
def _good(mode):
    """A descriptor the library would launch (never handed over unchanged: every test breaks one field first).  The pointers are never read."""
    if mode == N.NOISY_FORWARD:
        jobs = [dict(weight=0x1000, sigma=0x2000, out_eff=0x3000, out_eps=0x4000, count=5, tensor_id=k) for k in range(3)]
    else:
        jobs = [dict(grad_eff=0x1000, eps_in=0x2000, out_grad_sigma=0x3000, count=5) for _ in range(3)]
    return NC.desc(mode, jobs, seed=1, draw=2)


def _refused(d, word):
    fn = N.load().sgw_noisy_weights
    assert fn(C.byref(d), None) == N.EINVAL
    err = N.load().sgw_last_error().decode()
    assert word in err, err


def test_refuses_null_descriptor(built):
    assert N.load().sgw_noisy_weights(None, None) == N.EINVAL
    assert b"desc is NULL" in N.load().sgw_last_error()


@pytest.mark.parametrize("field", ["weight", "sigma", "out_eff"])
def test_forward_refuses_null_required_pointer(built, field):
    d = _good(N.NOISY_FORWARD)
    setattr(d.jobs[1], field, None)
    _refused(d, "job 1: weight, sigma and out_eff must not be NULL")


@pytest.mark.parametrize("field", ["grad_eff", "eps_in", "out_grad_sigma"])
def test_backward_refuses_null_required_pointer(built, field):
    d = _good(N.NOISY_BACKWARD)
    setattr(d.jobs[2], field, None)
    _refused(d, "job 2: grad_eff, eps_in and out_grad_sigma must not be NULL")


def test_refuses_the_other_modes_pointers(built):
    d = _good(N.NOISY_FORWARD)
    d.jobs[0].grad_eff = 0x5000
    _refused(d, "must be NULL (forward)")
    d = _good(N.NOISY_BACKWARD)
    d.jobs[0].out_eff = 0x5000
    _refused(d, "must be NULL (backward)")


def test_refuses_counts_ids_jobs_modes_reserved_and_alignment(built):
    for change, word in (({"count": -1}, "count = -1"), ({"count": (1 << 32) + 1}, "outside [0, 2^32]"), ({"tensor_id": -1}, "tensor_id = -1"),
                         ({"tensor_id": 1 << 28}, "tensor_id"), ({"reserved": 1}, "reserved"), ({"weight": 0x1002}, "misaligned"),
                         ({"out_eps": 0x4001}, "misaligned")):
        d = _good(N.NOISY_FORWARD)
        for key, value in change.items():
            setattr(d.jobs[1], key, value)
        _refused(d, word)
    for change, word in (({"num_jobs": N.NOISY_MAX_JOBS + 1}, "num_jobs = 25"), ({"num_jobs": -1}, "num_jobs = -1"), ({"mode": 2}, "unknown mode 2"),
                         ({"reserved0": 1}, "reserved"), ({"reserved1": 1}, "reserved")):
        for mode in (N.NOISY_FORWARD, N.NOISY_BACKWARD):
            d = _good(mode)
            for key, value in change.items():
                setattr(d, key, value)
            _refused(d, word)


def test_nothing_to_do_is_ok_without_a_device(built):
    """num_jobs == 0 and jobs of count 0 launch nothing: SGW_OK with no device in sight."""
    fn = N.load().sgw_noisy_weights
    for mode in (N.NOISY_FORWARD, N.NOISY_BACKWARD):
        d = _good(mode)
        d.num_jobs = 0
        assert fn(C.byref(d), None) == N.OK
        d = _good(mode)
        for k in range(3):
            d.jobs[k].count = 0
        assert fn(C.byref(d), None) == N.OK
    assert N.NOISY_MAX_JOBS >= 24


def test_jobs_past_num_jobs_are_ignored(built):
    d = _good(N.NOISY_FORWARD)
    for k in range(3):
        d.jobs[k].count = 0
    d.jobs[5].count = -7                       # not a job of this call
    assert N.load().sgw_noisy_weights(C.byref(d), None) == N.OK


# ------------------------------------------------------------------------------------------------------------------ codegen
def _compile(tmp, out, *flags):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.isfile(hipcc):
        pytest.fail("no hipcc: the kernels cannot be cross-compiled")
    csrc = os.path.join(G.ROOT, "sorrel_amd", "csrc")
    src = "".join(f"#include <{h}>\n" for h in SYSTEM) + '#include "' + os.path.join(G.ROOT, "include", "sgw.h") + '"\n'
    src += "".join(f'#include "{os.path.join(csrc, n)}"\n' for n in (*G.JIT_PARTS, "noisy.h"))
    src += "template __global__ void noisy_kernel<false>(const NoisyParams);\ntemplate __global__ void noisy_kernel<true>(const NoisyParams);\n"
    tu = tmp / "noisy_tu.hip"
    tu.write_text(src)
    run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", *flags, "-o", str(tmp / out), str(tu)],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    return run.stderr


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    remarks = _compile(tmp_path_factory.mktemp("noisy_obj"), "tu.o", "-c", "-Rpass-analysis=kernel-resource-usage")
    keys = (("vgpr", r" VGPRs: (\d+)"), ("sgpr", r" SGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
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
    tmp = tmp_path_factory.mktemp("noisy_ir")
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
    tmp = tmp_path_factory.mktemp("noisy_isa")
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


@pytest.mark.parametrize("kernel", [FORWARD, BACKWARD])
def test_no_scratch_no_lds_no_spills(usage, kernel):
    u = _one(usage, kernel)
    print(kernel, u)
    assert u["scratch"] == 0 and u["spill_v"] == 0 and u["spill_s"] == 0, u
    assert u["lds"] == 0, u
    assert u["occupancy"] >= 4, u


@pytest.mark.parametrize("kernel", [FORWARD, BACKWARD])
def test_no_operation_may_contract(ir, kernel):
    """``w + s * eps`` stays a rounded product and a sum: no float operation of the kernel carries the contract flag ..."""
    flagged, plain = _float_ops(_one(ir, kernel))
    print(kernel, flagged, "of", flagged + plain)
    assert plain > 0, "no float operation found: the IR is not what this test reads"
    assert flagged == 0, (flagged, plain)


def test_the_sum_is_an_add_of_a_rounded_product(isa):
    """... and the assembly of the forward holds four v_mul_f32 / v_add_f32 pairs where the effective weights are formed and stores only
    dwords; the backward has no fused multiply-add at all."""
    fwd, bwd = _one(isa, FORWARD), _one(isa, BACKWARD)
    assert not [line for line in bwd if re.match(r"v_(fma|mad|mac|fmac|pk_fma)", line)], bwd
    assert sum(line.startswith("v_mul_f32") for line in bwd) == 4
    for body in (fwd, bwd):
        stores = [line for line in body if line.startswith(("global_store", "flat_store", "buffer_store"))]
        assert stores and all(line.startswith("global_store_dword ") for line in stores), stores
        assert not [line for line in body if "atomic" in line]
        assert not [line for line in body if line.startswith(("ds_", "scratch_"))]


def test_host_twin_of_the_bit_rule(tmp_path):
    """The rule itself on the host, under the kernel's own pragma: ``w + (s * e)`` with the product rounded differs from the fused result for
    operands chosen so, and equals NumPy's two roundings."""
    src = tmp_path / "twin.c"
    src.write_text("#include <stdio.h>\n#include <math.h>\n#include <string.h>\n"
                   "int main(void){\n#pragma STDC FP_CONTRACT OFF\n volatile float w = -1.0f, s = 1.0f + 0x1p-12f, e = 1.0f + 0x1p-12f;\n"
                   " float p = s * e; float two = w + p; float one = fmaf(s, e, w); unsigned a, b; memcpy(&a, &two, 4); memcpy(&b, &one, 4);\n"
                   ' printf("%u %u\\n", a, b); return 0;}\n')
    exe = tmp_path / "twin"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-o", str(exe), str(src), "-lm"], check=True)
    two, one = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    w, s, e = np.float32(-1.0), np.float32(1.0 + 2.0 ** -12), np.float32(1.0 + 2.0 ** -12)
    want = LK.bits(np.array([w + (s * e)], np.float32))[0]
    assert two == int(want)
    assert one != two                          # the operands do tell the two apart: tests/test_gpu_noisy_weights.py uses them
