"""CPU tests of the drop-in boundary: the C-ABI library loads and exports every symbol include/sgw.h declares, and the whole ctypes
binding agrees with the header -- every struct mirror's layout, every function's prototype, every constant.
No compute calls are made (there is no GPU in the build container)."""
import ctypes as C
import os
import re

import pytest

from tests import helpers as H
from tests import learner_common as LK
from sorrel_amd import _native as N

HEADER = os.path.join(H.ROOT, "include", "sgw.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sgw_[a-z_0-9]+)\s*\(", text)))


def test_header_declares_what_binding_expects():
    assert set(declared_symbols()) == set(N.EXPORTS)


def header_macros():
    """Every numeric macro of the header: ``{"SGW_X": value}`` (decimal or hex, an ``u`` suffix and parentheses allowed)."""
    return {m.group(1): int(m.group(2), 0)
            for m in re.finditer(r"^#define\s+(SGW_[A-Z_0-9]+)\s+\(?(-?(?:0x[0-9A-Fa-f]+|\d+))u?\)?(?=\s)", open(HEADER).read(), flags=re.M)}


# numeric macros of the header the binding has no name for, and why
UNMIRRORED = {"SGW_STREAM_" + name: "a stream only the kernels and the oracle draw from (its number is checked against the oracle's below)"
              for name in ("SPAWN", "SPAWN_KIND", "ACTION", "PLACE", "DENSE", "DENSE_KIND", "TAG_INIT", "EXPLORE")}


def test_constants_match_the_header():
    """The binding's constants are the header's macros (the header is the interface): every ``SGW_<NAME>`` whose ``<NAME>`` the binding
    has holds the header's value, and every other numeric macro is on ``UNMIRRORED`` with its reason."""
    macros = header_macros()
    assert len(macros) >= 97
    for name, value in macros.items():
        if hasattr(N, name[4:]):
            assert getattr(N, name[4:]) == value, name
    assert {name for name in macros if not hasattr(N, name[4:])} == set(UNMIRRORED)
    flags = [macros[k] for k in macros if k.startswith("SGW_STEP_")]
    assert len(set(flags)) == len(flags) == 7 and all(f & (f - 1) == 0 for f in flags)      # distinct single bits
    # the counter-RNG streams: the oracle's numbering is the header's (tests compare draws made by either)
    from oracle import gridstep_oracle as O
    for name in ("SPAWN", "SPAWN_KIND", "ACTION", "PLACE", "DENSE", "DENSE_KIND", "TAG_INIT", "EXPLORE"):
        assert getattr(O, "STREAM_" + name) == macros["SGW_STREAM_" + name], name


def _c_kind(decl):
    """An argument or return type of the header as what the calling convention sees: pointer, double, or an integer's width."""
    if "*" in decl:
        return "pointer"
    words = decl.replace("const", "").split()
    return {"double": "double", "int64_t": "int64", "int32_t": "int32", "uint32_t": "int32", "int": "int32", "void": None}[words[0]]


def _ctypes_kind(t):
    if t is None:
        return None
    if t in (C.c_void_p, C.c_char_p) or hasattr(t, "contents"):
        return "pointer"
    return "double" if t is C.c_double else {4: "int32", 8: "int64"}[C.sizeof(t)]


def test_prototypes_match_the_header():
    """Every function of the binding's table against the header's declaration: the argument count, per argument pointer / double /
    4-byte / 8-byte integer, and the return type."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = {name: (ret, [a for a in args.split(",") if a.strip() != "void"])
                for ret, name, args in re.findall(r"([A-Za-z_][\w \*]*?)\b(sgw_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text)}
    assert set(declared) == set(N.PROTOTYPES) == set(N.EXPORTS) and len(declared) >= 67
    for name, (restype, argtypes) in N.PROTOTYPES.items():
        ret, args = declared[name]
        assert [_ctypes_kind(t) for t in argtypes] == [_c_kind(a) for a in args], name
        assert _ctypes_kind(restype) == _c_kind(ret), name
        if "*" not in ret:
            assert restype is {"int": C.c_int, "int64_t": C.c_int64, "void": None}[ret.strip()], name
        assert all(t not in (C.c_float, C.c_longdouble) for t in argtypes), name


def test_load_sets_every_prototype(built):
    lib = N.load()
    for name, (restype, argtypes) in N.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_workspace_raises_for_an_error_code_and_holds_at_least_one_element(built):
    lib = N.load()
    assert lib.sgw_ppo_loss_workspace_bytes(-1) == N.EINVAL
    with pytest.raises(ValueError, match="n ="):
        N.workspace(lib.sgw_ppo_loss_workspace_bytes(-1), "cpu")
    assert [N.workspace(n, "cpu").numel() for n in (0, 1, 8, 9, 24)] == [1, 1, 1, 2, 3]


def test_value_action_is_argmax_or_the_engines_uniform_draw():
    """oracle.value_action -- the checker of SGW_ACT_QF32 -- against its definition: np.argmax (first maximum; NaN counts as one)
    unless u32(EXPLORE, agent) < floor(epsilon * 2**32), then the action random_actions takes for that (env, turn, agent)
    (sorrel/models/pytorch/iqn.py:294-309 with the counter RNG in place of `random`)."""
    import numpy as np
    from oracle import gridstep_oracle as O

    spec = O.treasurehunt_spec(9, 9, 3, 2, seed=77)
    nact = len(spec.action_dy)
    rng = np.random.default_rng(0)
    assert O.value_action(spec, 0, 0, 1, 0, [1.0, 3.0, 3.0, 2.0]) == 1                 # first maximum
    assert O.value_action(spec, 0, 0, 1, 0, [1.0, np.nan, 9.0, np.nan]) == 1           # NaN counts as the maximum
    assert O.value_action(spec, 0, 0, 1, 0, [-np.inf] * nact) == 0
    explored = 0
    for env in range(40):
        for turn in range(1, 6):
            q = rng.standard_normal(nact).astype(np.float32)
            rnd = O.random_actions(spec, env, 3, turn)
            for a in range(spec.num_agents):
                assert O.value_action(spec, env, 3, turn, a, q, 0.0) == int(np.argmax(q))
                assert O.value_action(spec, env, 3, turn, a, q, 1.0) == int(rnd[a])
                u = int(O.rng_u32(spec.seed, env, 3, turn, O.STREAM_EXPLORE, a))
                want = int(rnd[a]) if u < O.prob_threshold(0.3) else int(np.argmax(q))
                assert O.value_action(spec, env, 3, turn, a, q, 0.3) == want
                explored += u < O.prob_threshold(0.3)
    assert 120 < explored < 240                                                         # ~0.3 of 600 draws


def test_library_exports_every_declared_symbol(built):
    lib = N.load()   # dlopen only (after torch, so one HIP runtime is mapped): no HIP call, works without a GPU
    for name in declared_symbols():
        assert hasattr(lib, name), f"libsgw.so does not export {name}"


def test_library_has_gfx950_code_object(built):
    data = open(N.LIB_PATH, "rb").read()
    assert b"gfx950" in data
    assert b"step_kernel" in data


def test_every_struct_layout_matches_c(tmp_path):
    """Every ``ctypes.Structure`` of the binding (found by introspection: a new mirror is covered as it is added) against the C
    compiler's view of the struct its docstring names: ``sizeof``, ``offsetof`` of every field, and the field names in the header's
    declaration order.  One compile for all of them."""
    mirrors = {}
    for cls in vars(N).values():
        if isinstance(cls, type) and issubclass(cls, C.Structure) and cls is not C.Structure:
            named = re.search(r"``struct (sgw_\w+)``", cls.__doc__ or "")
            assert named, f"{cls.__name__}'s docstring does not name the struct it mirrors"
            mirrors[named.group(1)] = cls
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    bodies = dict(re.findall(r"typedef struct (sgw_\w+) \{(.*?)\} \1;", text, flags=re.S))
    assert set(bodies) == set(mirrors) and len(mirrors) >= 14
    got = LK.c_layout(tmp_path, [(cname, [f for f, _ in cls._fields_]) for cname, cls in mirrors.items()])
    for cname, cls in mirrors.items():
        fields = [f for f, _ in cls._fields_]
        declared = [re.sub(r"\[.*", "", f.split("*")[-1].split()[-1]) for d in bodies[cname].split(";") if d.strip() for f in d.split(",")]
        assert declared == fields, cname
        assert got[cname]["sizeof"] == C.sizeof(cls), cname
        for f in fields:
            assert got[cname][f] == getattr(cls, f).offset, (cname, f)


def test_pure_host_helpers_agree_with_spec(built):
    from sorrel_amd.spec import treasurehunt_spec

    lib = N.load()
    for (h, w, a, r, want) in ((16, 16, 4, 2, 3476), (32, 32, 8, 3, 13592), (128, 128, 64, 5, 251984)):
        spec = treasurehunt_spec(h, w, a, r)
        cfg = spec.to_config(1)
        # SURVEY.md 8(d) per-env-step algorithmic bytes for C2 / C3 / C5
        assert lib.sgw_algorithmic_bytes_per_env_step(C.byref(cfg)) == want == spec.algorithmic_bytes_per_env_step()
        assert lib.sgw_grid_bytes_per_env(C.byref(cfg)) == 2 * h * w
        assert lib.sgw_obs_elems_per_env(C.byref(cfg)) == a * 6 * (2 * r + 1) ** 2


def test_engine_fails_loudly_without_gpu():
    import torch

    from sorrel_amd.engine import GridEngine
    from sorrel_amd.spec import treasurehunt_spec

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(N.SgwError):
        GridEngine(treasurehunt_spec(16, 16, 4, 2), 8, device="cuda")
    with pytest.raises(N.SgwError):
        GridEngine(treasurehunt_spec(16, 16, 4, 2), 8, device="cpu")


def test_missing_library_fails_loudly(monkeypatch):
    """No built extension -> SgwError naming the build command; nothing else is tried."""
    monkeypatch.setattr(N, "_lib", None)
    monkeypatch.setattr(N, "LIB_PATH", "/nonexistent/libsgw.so")
    with pytest.raises(N.SgwError, match="no CPU fallback"):
        N.load()
