"""The learner clock without a GPU (``sgw_learn_clock`` and the four calls that read or advance it; ``PyTorchIQN.capture_train_step`` and
``updates_per_call``): every refusal of the clocked calls with its text (validation precedes the launch, so no device is needed) and one
inherited refusal per call, the binding against the header, what the compiler makes of the new kernels cross-compiled for gfx950 (the recipe
of ``tests/test_learner_codegen.py``), and the host-side rules of the learner: no capture on a CPU model, a failed capture leaves the eager
state, ``updates_per_call`` steps equal as many single calls."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

import __graft_entry__ as G
from sorrel_amd import _native as N
from tests import iqn_learner_common as LC
from tests import learner_common as LK
from tests import noisy_common as NC
from tests.test_iqn_forward_cpu import good_desc as forward_desc
from tests.test_learner_codegen import SYSTEM, _float_ops, _one
from tests.test_sample_cpu import good_desc as sample_desc

CLOCK = 0x10000                # never followed: every call below is refused, or launches nothing
NOISY, QUANTILE, ADVANCE = "20noisy_clocked_kernel", "27iqn_quantile_clocked_kernel", "26learn_clock_advance_kernel"
SAMPLE = tuple(f"26sample_rows_clocked_kernelILi{v}ELb{u}EE" for v in (1, 4) for u in (0, 1))


# ------------------------------------------------------------------------------------------------------------------ refusals
def noisy_desc():
    return NC.desc(N.NOISY_FORWARD, [dict(weight=0x1000, sigma=0x2000, out_eff=0x3000, out_eps=0x4000, count=5, tensor_id=k) for k in range(3)], seed=1)


def _forward():
    d = forward_desc()
    d.n = 5                    # (a call that would launch, were it accepted)
    return d


def _sample():
    d = sample_desc()
    d.n = 5
    return d


def refused(name, d, clock, word):
    lib = N.load()
    assert getattr(lib, name)(C.byref(d) if d is not None else None, clock, None) == N.EINVAL
    err = lib.sgw_last_error().decode()
    assert word in err and name in err, err


CALLS = (("sgw_noisy_weights_clocked", noisy_desc), ("sgw_iqn_forward_clocked", _forward), ("sgw_sample_clocked", _sample))


@pytest.mark.parametrize("name,make", CALLS, ids=[c[0] for c in CALLS])
def test_refuses_a_null_descriptor_a_null_clock_and_a_misaligned_clock(built, name, make):
    refused(name, None, CLOCK, "desc is NULL")
    refused(name, make(), None, "clock is NULL")
    for off in (1, 2, 4, 7):
        refused(name, make(), CLOCK + off, "misaligned clock")


def test_advance_refuses_a_null_and_a_misaligned_clock(built):
    lib = N.load()
    assert lib.sgw_learn_clock_advance(None, None) == N.EINVAL and b"sgw_learn_clock_advance: clock is NULL" in lib.sgw_last_error()
    assert lib.sgw_learn_clock_advance(CLOCK + 4, None) == N.EINVAL and b"sgw_learn_clock_advance: misaligned clock" in lib.sgw_last_error()


def test_refuses_the_scalars_the_clock_replaces(built):
    d = noisy_desc()
    d.draw = 3
    refused("sgw_noisy_weights_clocked", d, CLOCK, "draw = 3 must be 0")
    d = noisy_desc()
    d.draw = 1 << 32
    refused("sgw_noisy_weights_clocked", d, CLOCK, "must be 0")
    d = _forward()
    d.turn = 7
    refused("sgw_iqn_forward_clocked", d, CLOCK, "turn = 7 must be 0")
    d = _forward()
    d.taus = 4096
    refused("sgw_iqn_forward_clocked", d, CLOCK, "taus must be NULL")
    for change in ({"starts": 4096, "envs": 4096}, {"starts": 4096}, {"envs": 4096}):
        d = _sample()
        for key, value in change.items():
            setattr(d, key, value)
        refused("sgw_sample_clocked", d, CLOCK, "starts and envs must be NULL")


def test_the_unclocked_checks_still_run(built):
    """One inherited refusal per call, under the clocked call's name; the sampler's bound is checked against the ring as ``num_starts`` is."""
    d = noisy_desc()
    d.jobs[1].sigma = None
    refused("sgw_noisy_weights_clocked", d, CLOCK, "job 1: weight, sigma and out_eff must not be NULL")
    d = noisy_desc()
    d.mode = N.NOISY_BACKWARD          # (the forward's pointers in backward mode)
    refused("sgw_noisy_weights_clocked", d, CLOCK, "grad_eff, eps_in and out_grad_sigma must not be NULL")
    d = _forward()
    d.layer_size = 257
    refused("sgw_iqn_forward_clocked", d, CLOCK, "layer_size")
    d = _forward()
    d.num_envs = 0
    refused("sgw_iqn_forward_clocked", d, CLOCK, "num_envs")
    d = _sample()
    d.num_starts = 15                  # upper bound + n_frames past the capacity
    refused("sgw_sample_clocked", d, CLOCK, "capacity")
    d = _sample()
    d.num_starts = 0
    refused("sgw_sample_clocked", d, CLOCK, "num_starts")


def test_nothing_to_do_is_ok_without_a_device(built):
    lib = N.load()
    d = noisy_desc()
    d.num_jobs = 0
    assert lib.sgw_noisy_weights_clocked(C.byref(d), CLOCK, None) == N.OK
    assert lib.sgw_iqn_forward_clocked(C.byref(forward_desc()), CLOCK, None) == N.OK          # n == 0
    assert lib.sgw_sample_clocked(C.byref(sample_desc()), CLOCK, None) == N.OK


# ------------------------------------------------------------------------------------------------------------------ the binding
def test_the_binding_mirrors_the_struct_and_the_four_prototypes(tmp_path):
    assert C.sizeof(N.SgwLearnClock) == 32 and C.alignment(N.SgwLearnClock) == 8
    assert [(f, getattr(N.SgwLearnClock, f).offset) for f, _ in N.SgwLearnClock._fields_] == [("count", 0), ("num_starts", 8), ("reserved", 16)]
    got = LK.c_layout(tmp_path, [("sgw_learn_clock", ["count", "num_starts", "reserved"])])["sgw_learn_clock"]
    assert got == {"sizeof": 32, "count": 0, "num_starts": 8, "reserved": 16}
    text = open(os.path.join(G.ROOT, "include", "sgw.h")).read()
    for name, desc in (("sgw_noisy_weights", "sgw_noisy_weights_desc"), ("sgw_iqn_forward", "sgw_iqn_forward_desc"), ("sgw_sample", "sgw_sample_desc")):
        assert f"int {name}_clocked(const {desc}* desc, const sgw_learn_clock* clock, void* stream);" in text
        assert len(N.PROTOTYPES[name + "_clocked"][1]) == len(N.PROTOTYPES[name][1]) + 1
    assert "int sgw_learn_clock_advance(sgw_learn_clock* clock, void* stream);" in text
    assert N.PROTOTYPES["sgw_learn_clock_advance"] == (C.c_int, [C.c_void_p, C.c_void_p])


# ------------------------------------------------------------------------------------------------------------------ codegen
def _compile(tmp, out, *flags):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.isfile(hipcc):
        pytest.fail("no hipcc: the kernels cannot be cross-compiled")
    csrc = os.path.join(G.ROOT, "sorrel_amd", "csrc")
    src = "".join(f"#include <{h}>\n" for h in SYSTEM) + '#include "' + os.path.join(G.ROOT, "include", "sgw.h") + '"\n'
    src += "".join(f'#include "{os.path.join(csrc, n)}"\n' for n in (*G.JIT_PARTS, "sample.h", "iqn_forward.h", "noisy.h"))
    src += "".join(f"template __global__ void sample_rows_clocked_kernel<{v}, {u}>(const SampleParams, const sgw_learn_clock*);\n"
                   f"template __global__ void sample_rows_kernel<{v}, {u}>(const SampleParams);\n" for v in (1, 4) for u in ("false", "true"))
    src += "template __global__ void noisy_kernel<false>(const NoisyParams);\n"
    tu = tmp / "clock_tu.hip"
    tu.write_text(src)
    run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", *flags, "-o", str(tmp / out), str(tu)],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    return run.stderr


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    remarks = _compile(tmp_path_factory.mktemp("clock_obj"), "tu.o", "-c", "-Rpass-analysis=kernel-resource-usage")
    keys = (("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"),
            ("spill_v", r"VGPRs Spill: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"))
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
    tmp = tmp_path_factory.mktemp("clock_ir")
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


# kernel -> (its unclocked twin, the least occupancy both must reach)
TWINS = {NOISY: ("12noisy_kernelILb0EE", 4), QUANTILE: ("19iqn_quantile_kernel", 2), ADVANCE: ("19sample_count_kernel", 8),
         **{k: (k.replace("26sample_rows_clocked_kernel", "18sample_rows_kernel"), 7) for k in SAMPLE}}


@pytest.mark.parametrize("kernel", sorted(TWINS))
def test_no_scratch_no_spills_and_the_twins_registers(usage, kernel):
    twin, occupancy = TWINS[kernel]
    u = _one(usage, kernel)
    print(kernel, u)
    assert u["scratch"] == 0 and u["spill_v"] == 0, u
    assert u["occupancy"] >= occupancy, u
    t = _one(usage, twin)                       # the clock costs no vector register and no LDS
    assert u["vgpr"] <= t["vgpr"] and u["lds"] == t["lds"], (u, t)


@pytest.mark.parametrize("kernel", [NOISY, QUANTILE])
def test_no_operation_may_contract_where_the_twin_promises_it(ir, kernel):
    flagged, plain = _float_ops(_one(ir, kernel))
    print(kernel, flagged, "of", flagged + plain)
    assert plain > 0, "no float operation found: the IR is not what this test reads"
    assert flagged == 0, (flagged, plain)


# ------------------------------------------------------------------------------------------------------------------ the learner's host rules
def test_capture_on_a_cpu_model_and_below_the_gate_raises():
    model = LC.fill_memory(LC.make_model(LC.SHAPES[0], "cpu"))
    with pytest.raises(RuntimeError, match="on the CPU"):
        model.capture_train_step()
    assert model._recorded is None and model.steps_done == 0
    model.release_train_step()                  # (nothing to drop: not an error)


def test_a_failed_capture_leaves_the_eager_state(monkeypatch):
    """The recorded body raises at its first call, after host-side effects and before any device work (the warm-up, the graph and the capture
    guard are stood in for: there is no device here): the counters are put back, nothing is recorded, the optimiser counts as before, and
    the eager step runs with the bits of a model that never tried."""
    import contextlib

    from sorrel_amd import capture

    model = LC.fill_memory(LC.make_model(LC.SHAPES[0], "cpu"))
    twin = LC.fill_memory(LC.make_model(LC.SHAPES[0], "cpu"))
    before = (model.steps_done, model.memory.idx, model.memory.size)
    entered = []

    def body(batch, taus, noise, clock=None):
        assert clock == model._clock.data_ptr() and batch is None and taus is None and noise is None
        model.steps_done += 1
        model.memory.idx += 1
        model.memory.size -= 1
        raise RuntimeError("boom")

    @contextlib.contextmanager
    def recording(graph):
        entered.append(graph)
        yield graph

    with monkeypatch.context() as m:
        m.setattr(model, "device", torch.device("cuda:0"))
        m.setattr(model, "_clock", torch.zeros((4,), dtype=torch.int64))
        m.setattr(model, "_warm_up", lambda steps, clock: None)
        m.setattr(torch.cuda, "CUDAGraph", object)
        m.setattr(capture, "recording", recording)
        m.setattr(model, "_train_step_device", body)
        with pytest.raises(RuntimeError, match="boom"):
            model.capture_train_step()
    assert len(entered) == 1
    assert model._recorded is None and not model.optimizer.device_step
    assert (model.steps_done, model.memory.idx, model.memory.size) == before
    torch.manual_seed(11)
    a = model.train_step()
    torch.manual_seed(11)
    b = twin.train_step()
    assert float(a) == float(b) and model.steps_done == twin.steps_done == 1
    LC.same_state(LC.get_state(model), LC.get_state(twin))


def test_gate_closed_raises_on_a_device_model_without_touching_the_device(monkeypatch):
    model = LC.make_model(LC.SHAPES[0], "cpu")
    monkeypatch.setattr(model, "device", torch.device("cuda:0"))
    with pytest.raises(RuntimeError, match="gate is closed"):
        model.capture_train_step()


@pytest.mark.parametrize("shape", LC.SHAPES, ids=LC.tag_of)
def test_updates_per_call_on_the_cpu_path_equals_single_calls(shape):
    a = LC.fill_memory(LC.make_model(shape, "cpu"))
    b = LC.fill_memory(LC.make_model(shape, "cpu"))
    assert a.updates_per_call == 1
    a.updates_per_call = 3
    torch.manual_seed(77)
    last = a.train_step()
    torch.manual_seed(77)
    singles = [b.train_step() for _ in range(3)]
    assert a.steps_done == b.steps_done == 3
    assert float(last) == float(singles[-1]) and len({float(x) for x in singles}) == 3
    LC.same_state(LC.get_state(a), LC.get_state(b))
    # with overrides: exactly one step
    case = LC.load_fixture()[LC.tag_of(shape)]
    a.train_step(**LC.step_args(case["steps"][0], "cpu"))
    assert a.steps_done == 4
