"""The instance ledger: one case per (prebuilt kernel instance of libsgw.so, role it is launched in), for the seven turn-kernel templates
step_fast / step_big / step_kernel / step_fast_rows / phase_rows / observe_rows / phase_kernel.  tests/test_instance_ledger.py proves on
the CPU that every case plans the instance it claims, that the cases cover the library, and that no case is vacuous on the oracle;
tests/test_gpu_instances.py launches every case against the C oracle, bit for bit.  Not collected by pytest; imports nothing of the GPU.

Every case runs with ``jit = 0`` (the prebuilt instances only).  Instances are selected the way a user's world would select them -- table
shape, map size, agent count -- and otherwise by the forcing options the GPU tests already use (FORCING_OPTIONS below)."""
import dataclasses
import functools

import numpy as np

from sorrel_amd import _native as N
from tests import helpers as H

TEMPLATES = ("step_fast", "step_big", "step_kernel", "step_fast_rows", "phase_rows", "observe_rows", "phase_kernel")

# how an instance gets launched -> the field of sgw_plan that names it (None: only sgw_launch_info does)
ROLE_KEY = {"step": "kernel", "plain": "kernel_plain", "rollout": "kernel_rollout", "walk": "kernel_walk", "phase_rows": "kernel_phase",
            "observe_rows": "kernel_observe_rows", "sweep_rows": None, "phase_kernel": None}

# the only options a case may set besides jit = 0, with every value the sweep of test_instance_ledger.py gives them
# (the default first)
FORCING_OPTIONS = {"group": (0, 16, 32, 64), "force_generic": (0, 1), "fast_rules": (1, 0), "pack3": (1, 0), "stage": (1, 0),
                   "big_threads": (0, 256, 512), "big_walk_blocks": (0, 3), "phase_kernel": (-1, 0, 1), "phase_rows": (1, 0)}

# Instances of the library that no plan can name, each with the line of sorrel_amd/csrc/plan.h that shadows it.  (Empty: the sweep of
# test_instance_ledger.py finds a world and an option set for every one of the 107.)
UNREACHABLE = []   # [((template, args), "the shadowing line of plan.h", "why")]


@dataclasses.dataclass
class World:
    spec: object                 # sorrel_amd.spec.WorldSpec
    start: object = None         # (grid [L, H, W], pos [A, 2]) of one env that every env begins from; None: sgw_reset builds the map


# ----------------------------------------------------------------------------- the worlds
def th(h, w, a, r, seed=7):
    """Treasurehunt: two layers, six one-hot channels."""
    from sorrel_amd.spec import treasurehunt_spec

    return World(treasurehunt_spec(h, w, a, r, spawn_prob=0.08, seed=seed, dense_prob=0.3))


def move(h, w, layers, channels, a, r, seed=9):
    """Plain movers under any other (layers, channels) one-hot table."""
    from tests.gpu_common import _move_world

    return World(_move_world(h, w, layers, channels, a, r, seed))


def tag(h, w, a, r, channels=4, seed=None):
    """The Tag example's tables (one layer, four channels) on any map; ``channels`` > 4 appends empty channels (another table shape).
    ``seed``: big maps are sparse -- one under which the flag changes hands within the case's turns."""
    from tests.gpu_common import _tag_spec

    ws = _tag_spec(h, w, a, r)
    if seed is not None:
        ws = dataclasses.replace(ws, seed=seed)
    if channels != 4:
        app = np.zeros((len(ws.appearance), channels))
        app[:, :4] = ws.appearance
        ws = dataclasses.replace(ws, num_channels=channels, appearance=app)
    return World(ws)


def not_onehot(world):
    """The same world under a table that is not one-hot (as tag_72x72_r3_float of tests/test_gpu_kernels.py): the float64 layer-sum path."""
    ws = world.spec
    app = np.asarray(ws.appearance, dtype=np.float64) * 1.0
    t = ws.agent_type[0]
    app[t, int(np.argmax(app[t]))] = 2.5
    app[1 if t != 1 else 2, 0] += 0.25
    return World(dataclasses.replace(ws, appearance=app), world.start)


def cleanup_golden(name):
    """A Cleanup fixture as stored: three layers, nine channels, the map the reference's host code populated."""
    d, spec = H.load_golden(name)
    return World(H.world_spec(spec), (d["grid0"][0].copy(), d["pos0"][0].copy()))


def cleanup(h, w, a, beam=3, r=3, channels=9, seed=5):
    """Cleanup's layered rule set on any map (the river / land / orchard thirds of tests/test_gpu_kernels.py), agents on random distinct
    cells of the middle layer.  ``channels`` > 9: another table shape."""
    d, spec = H.load_golden("cleanup_15x16")
    ws = H.world_spec(spec)
    ws = dataclasses.replace(ws, height=h, width=w, num_agents=a, agent_type=[ws.agent_type[0]] * a, beam_radius=beam, vision_radius=r)
    if channels != 9:
        app = np.zeros((len(ws.appearance), channels))
        app[:, :9] = ws.appearance
        ws = dataclasses.replace(ws, num_channels=channels, appearance=app)
    g = np.zeros((3, h, w), np.uint8)
    g[:, 0, :] = g[:, -1, :] = 2
    g[:, :, 0] = g[:, :, -1] = 2
    g[0, 1:h // 3, 1:-1] = 3
    g[0, h // 3:2 * h // 3, 1:-1] = 1
    g[0, 2 * h // 3:h - 1, 1:-1] = 5
    rng = np.random.default_rng(seed)
    cells = rng.permutation((h - 2) * (w - 2))[:a]
    pos = np.stack([cells // (w - 2) + 1, cells % (w - 2) + 1], axis=1).astype(np.uint8)
    for y, x in pos:
        g[1, y, x] = ws.agent_type[0]
    return World(ws, (g, pos))


def rgb(h, w, a, r, tagged=False):
    """Integer colour tables behind clip / 255 (three channels), bright enough that the layers of a cell add up past 255."""
    d, spec = H.load_golden("rgb_treasurehunt")
    ws = H.world_spec(spec)
    if tagged:
        d2, spec2 = H.load_golden("tag_11x11_default")
        wt = H.world_spec(spec2)
        app = np.zeros((len(wt.appearance), 3))
        for t in range(len(app)):
            app[t] = [(37 * t) % 256, (91 * t + 5) % 256, 300 if t else 200]       # (one layer: a colour above 255 is what clips)
        return World(dataclasses.replace(wt, height=h, width=w, num_agents=a, vision_radius=r, agent_type=[wt.agent_type[0]] * a, num_channels=3,
                                         appearance=app, obs_post=1))
    app = np.asarray(ws.appearance, dtype=np.float64).copy()
    app[app > 0] = 255.0
    app[0] = [200.0, 180.0, 90.0]
    return World(dataclasses.replace(ws, height=h, width=w, num_agents=a, vision_radius=r, agent_type=[ws.agent_type[0]] * a, appearance=app,
                                     spawn_prob=[0.08 if p else 0.0 for p in ws.spawn_prob], dense_prob=0.3))


@dataclasses.dataclass
class Entry:
    id: str
    world: object                # () -> World
    num_envs: int
    options: dict                # always with jit = 0
    role: str
    instance: tuple              # (template, args) as tests/helpers.canonical_instance spells it
    turns: int = 6

    @functools.lru_cache(maxsize=None)
    def _built(self):
        return self.world()

    def __hash__(self):
        return hash(self.id)

    def built(self) -> World:
        return self._built()

    def config(self, num_envs=None, first=0):
        """The sgw_config the engine of this case is created with (spec.alloc_grid pads the env stride to 16 bytes)."""
        ws = self.built().spec
        cfg = ws.to_config(self.num_envs if num_envs is None else num_envs, first)
        cfg.grid_env_stride = (ws.layers * ws.height * ws.width + 15) // 16 * 16
        return cfg


def _inst(text):
    tmpl, args = text.split("<")
    return tmpl, tuple(a.strip() for a in args.rstrip(">").split(","))


ENTRIES = []


def case(id, world, num_envs, role, instance, turns=6, **options):
    assert set(options) <= set(FORCING_OPTIONS), options
    ENTRIES.append(Entry(id, world, num_envs, dict(options, jit=0), role, _inst(instance), turns))


F = "false"
# ----------------------------------------------------------------------------- step_fast: 28
_th_rt = lambda: th(14, 18, 3, 2)                      # a run-time map: 504 bytes per env, 37 envs: last workgroup holds one env
case("fast_th_runtime_stage", _th_rt, 37, "step", "step_fast<true,2,6,0,0,0,false,false,true,false,false,false>", 8)
case("fast_th_runtime_plain", _th_rt, 37, "plain", "step_fast<true,2,6,0,0,0,false,false,false,false,false,false>", 8)
case("fast_th_runtime_rollout", _th_rt, 37, "rollout", "step_fast<true,2,6,0,0,0,false,false,true,true,false,false>")
case("fast_th_runtime_unstaged", lambda: th(13, 17, 4, 3, seed=8), 37, "step", "step_fast<true,2,6,0,0,0,false,false,false,false,false,false>", 8, stage=0)
case("fast_c2", lambda: th(16, 16, 4, 2, seed=11), 37, "step", "step_fast<true,2,6,2,16,16,false,false,false,false,false,false>", 8)
case("fast_c2_rollout", lambda: th(16, 16, 4, 2, seed=11), 37, "rollout", "step_fast<true,2,6,2,16,16,false,false,false,true,false,false>")
case("fast_c3", lambda: th(32, 32, 8, 3, seed=12), 37, "step", "step_fast<true,2,6,3,32,32,false,false,false,false,false,false>", 8)
case("fast_c3_rollout", lambda: th(32, 32, 8, 3, seed=12), 37, "rollout", "step_fast<true,2,6,3,32,32,false,false,false,true,false,false>")
_mv = lambda: move(12, 14, 3, 7, 4, 2)                 # three layers, seven channels: 3-bit packed counters
case("fast_move_p3", _mv, 37, "step", "step_fast<true,0,0,0,0,0,false,false,true,false,true,false>", 8)
case("fast_move_plain", _mv, 37, "plain", "step_fast<true,0,0,0,0,0,false,false,false,false,false,false>", 8)
case("fast_move_bytes", _mv, 37, "step", "step_fast<true,0,0,0,0,0,false,false,true,false,false,false>", 8, pack3=0)
case("fast_move_12_channels", lambda: move(13, 12, 2, 12, 5, 3), 37, "step", "step_fast<true,0,0,0,0,0,false,false,true,false,false,false>", 8)   # > 10 channels: no 3-bit counters
case("fast_move_float", lambda: not_onehot(th(14, 18, 3, 2, seed=13)), 37, "step", "step_fast<false,0,0,0,0,0,false,false,false,false,false,false>", 8)
_tg = lambda: tag(12, 13, 5, 3)
case("fast_tag_p3", _tg, 37, "step", "step_fast<true,0,0,0,0,0,true,false,true,false,true,false>", 10)
case("fast_tag_plain", _tg, 37, "plain", "step_fast<true,0,0,0,0,0,true,false,false,false,false,false>", 10)
case("fast_tag_bytes", _tg, 37, "step", "step_fast<true,0,0,0,0,0,true,false,true,false,false,false>", 10, pack3=0)
case("fast_tag_float", lambda: not_onehot(tag(12, 13, 5, 3)), 37, "step", "step_fast<false,0,0,0,0,0,true,false,false,false,false,false>", 10)
case("fast_tag_32x32", lambda: tag(32, 32, 12, 3), 37, "step", "step_fast<true,1,4,3,32,32,true,false,false,false,false,false>", 10)
_cl = lambda: cleanup_golden("cleanup_15x16")
case("fast_cleanup_p3", _cl, 37, "step", "step_fast<true,0,0,0,0,0,false,true,true,false,true,false>", 10)
case("fast_cleanup_p3_plain", _cl, 37, "plain", "step_fast<true,0,0,0,0,0,false,true,false,false,true,false>", 10)
case("fast_cleanup_p3_rollout", _cl, 37, "rollout", "step_fast<true,3,9,0,0,0,false,true,true,true,true,false>")
case("fast_cleanup_bytes", _cl, 37, "step", "step_fast<true,0,0,0,0,0,false,true,true,false,false,false>", 10, pack3=0)
case("fast_cleanup_bytes_plain", _cl, 37, "plain", "step_fast<true,0,0,0,0,0,false,true,false,false,false,false>", 10, pack3=0)
case("fast_cleanup_bytes_rollout", _cl, 37, "rollout", "step_fast<true,3,9,0,0,0,false,true,true,true,false,false>", pack3=0)
case("fast_cleanup_as_shipped", lambda: cleanup_golden("cleanup_21x31_default"), 37, "step", "step_fast<true,3,9,5,21,31,false,true,true,false,true,false>", 10)
_cl10 = lambda: cleanup(13, 14, 4, beam=2, r=2, channels=10)     # the rule set under a ten-channel table: the run-time-table turn loop
case("fast_rules_p3_rollout", _cl10, 37, "rollout", "step_fast<true,0,0,0,0,0,false,true,true,true,true,false>")
case("fast_rules_bytes_rollout", _cl10, 37, "rollout", "step_fast<true,0,0,0,0,0,false,true,true,true,false,false>", pack3=0)
case("fast_cleanup_float", lambda: not_onehot(cleanup_golden("cleanup_13x12_r2")), 37, "step", "step_fast<false,0,0,0,0,0,false,true,false,false,false,false>", 10)
case("fast_rgb", lambda: rgb(12, 13, 3, 3), 37, "step", "step_fast<true,0,3,0,0,0,false,false,true,false,false,true>", 8)
case("fast_rgb_tag", lambda: rgb(14, 12, 5, 3, tagged=True), 37, "step", "step_fast<true,0,3,0,0,0,true,false,true,false,false,true>", 10)

# ----------------------------------------------------------------------------- step_big: 17 (a 48x48x2 world, 4 608 bytes per env, selects it by itself)
_b5 = lambda: th(48, 48, 8, 5, seed=21)                # 8 agents x 121 window cells <= 2 048: four waves
_b5w = lambda: th(48, 50, 40, 5, seed=22)              # 40 agents: eight waves
case("big_c5_256", _b5, 5, "step", "step_big<true,2,6,5,false,false,false,256,false>")
case("big_c5_256_walk", _b5, 7, "walk", "step_big<true,2,6,5,false,true,false,256,false>", big_walk_blocks=3)
case("big_c5_rollout", _b5, 5, "rollout", "step_big<true,2,6,5,true,false,false,512,false>")
case("big_c5_512", _b5w, 5, "step", "step_big<true,2,6,5,false,false,false,512,false>")
case("big_c5_512_walk", _b5w, 7, "walk", "step_big<true,2,6,5,false,true,false,512,false>", big_walk_blocks=3)
_bm = lambda: move(50, 52, 2, 5, 6, 3, seed=23)
_bmw = lambda: move(52, 50, 2, 5, 44, 3, seed=24)      # 44 agents x 49 cells > 2 048
case("big_move_256", _bm, 6, "step", "step_big<true,0,0,0,false,false,false,256,false>")
case("big_move_256_walk", _bm, 7, "walk", "step_big<true,0,0,0,false,true,false,256,false>", big_walk_blocks=3)
case("big_move_512", _bmw, 5, "step", "step_big<true,0,0,0,false,false,false,512,false>")
case("big_move_512_walk", _bmw, 7, "walk", "step_big<true,0,0,0,false,true,false,512,false>", big_walk_blocks=3)
_bf = lambda: not_onehot(th(48, 48, 7, 3, seed=25))
case("big_float", _bf, 6, "step", "step_big<false,0,0,0,false,false,false,512,false>")
case("big_float_rollout", _bf, 5, "rollout", "step_big<false,0,0,0,true,false,false,512,false>")
case("big_float_walk", _bf, 7, "walk", "step_big<false,0,0,0,false,true,false,512,false>", big_walk_blocks=3)
case("big_tag_r4_256", lambda: tag(66, 64, 20, 4, seed=5), 6, "step", "step_big<true,1,4,4,false,false,true,256,false>", 10)
case("big_tag_r4_512", lambda: tag(66, 64, 40, 4, seed=2), 6, "step", "step_big<true,1,4,4,false,false,true,512,false>", 10)
case("big_tag_r3_256", lambda: tag(64, 66, 30, 3, seed=1), 6, "step", "step_big<true,0,0,0,false,false,true,256,false>", 10)
case("big_tag_r3_512", lambda: tag(65, 65, 60, 3, seed=1), 6, "step", "step_big<true,0,0,0,false,false,true,512,false>", 10)
case("big_tag_float", lambda: not_onehot(tag(66, 64, 40, 3, seed=2)), 6, "step", "step_big<false,0,0,0,false,false,true,512,false>", 10)

# ----------------------------------------------------------------------------- step_kernel: 53
_sm = {   # small worlds for the packed (16 / 32 lanes per env) and the wave-per-env generic kernel
    "th_r2": lambda: th(11, 13, 3, 2, seed=31), "th_r3": lambda: th(13, 15, 4, 3, seed=32), "move": lambda: move(9, 13, 1, 4, 4, 2, seed=33),
    "float": lambda: not_onehot(th(12, 11, 3, 2, seed=34)), "cleanup": lambda: cleanup_golden("cleanup_13x12_r2"),
    "cleanup_float": lambda: not_onehot(cleanup_golden("cleanup_13x12_r2")), "tag_r2": lambda: tag(12, 11, 5, 2), "tag_r3": lambda: tag(13, 12, 5, 3),
    "tag_r4": lambda: tag(12, 14, 5, 4), "tag_11x11": lambda: tag(11, 11, 5, 4), "tag_c5": lambda: tag(12, 13, 5, 2, channels=5),
    "tag_float": lambda: not_onehot(tag(11, 12, 5, 2)),
}
for G, E in ((16, 45), (32, 33), (64, 21)):
    o = {"group": G} if G != 64 else {"force_generic": 1}
    sk = lambda args, G=G: f"step_kernel<{G},{args},64,false>"
    case(f"sk{G}_th", _sm["th_r3"], E, "step", sk("true,2,6,0,0,0,0,false"), 8, **o)
    case(f"sk{G}_th_rollout", _sm["th_r3"], E, "rollout", sk("true,2,6,0,0,0,0,true"), **o)
    case(f"sk{G}_move", _sm["move"], E, "step", sk("true,0,0,0,0,0,0,false"), 8, **o)
    case(f"sk{G}_move_rollout", _sm["move"], E, "rollout", sk("true,0,0,0,0,0,0,true"), **o)
    case(f"sk{G}_float", _sm["float"], E, "step", sk("false,0,0,0,0,0,0,false"), 8, **o)
    case(f"sk{G}_float_rollout", _sm["float"], E, "rollout", sk("false,0,0,0,0,0,0,true"), **o)
    case(f"sk{G}_cleanup", _sm["cleanup"], E, "step", sk("true,0,0,2,0,0,0,false"), 10, **o)
    case(f"sk{G}_cleanup_float", _sm["cleanup_float"], E, "step", sk("false,0,0,2,0,0,0,false"), 10, **o)
    case(f"sk{G}_tag", _sm["tag_r2"], E, "step", sk("true,1,4,1,0,0,0,false"), 10, **o)
    case(f"sk{G}_tag_5_channels", _sm["tag_c5"], E, "step", sk("true,0,0,1,0,0,0,false"), 10, **o)
    case(f"sk{G}_tag_float", _sm["tag_float"], E, "step", sk("false,0,0,1,0,0,0,false"), 10, **o)
case("sk16_th_r2", _sm["th_r2"], 45, "step", "step_kernel<16,true,2,6,0,2,0,0,false,64,false>", 8, group=16)
case("sk16_th_r2_rollout", _sm["th_r2"], 45, "rollout", "step_kernel<16,true,2,6,0,2,0,0,true,64,false>", group=16)
case("sk32_tag_r3", _sm["tag_r3"], 33, "step", "step_kernel<32,true,1,4,1,3,0,0,false,64,false>", 10, group=32)
case("sk32_tag_r4", _sm["tag_r4"], 33, "step", "step_kernel<32,true,1,4,1,4,0,0,false,64,false>", 10, group=32)
case("sk32_tag_11x11", _sm["tag_11x11"], 33, "step", "step_kernel<32,true,1,4,1,4,11,11,false,64,false>", 10, group=32)
case("sk32_tag_11x11_rollout", _sm["tag_11x11"], 33, "rollout", "step_kernel<32,true,1,4,1,4,11,11,true,64,false>", group=32)
# a workgroup per env (worlds above 4 KiB forced off step_big / the RULES kernel)
_g256 = {"th": lambda: th(48, 48, 6, 3, seed=41), "move": lambda: move(48, 50, 2, 5, 6, 3, seed=42), "float": lambda: not_onehot(th(48, 48, 5, 3, seed=43)),
         "cleanup": lambda: cleanup(40, 48, 8), "cleanup_float": lambda: not_onehot(cleanup(40, 48, 8)), "tag": lambda: tag(66, 64, 48, 3, seed=2),
         "tag_c5": lambda: tag(66, 64, 48, 3, channels=5, seed=2), "tag_float": lambda: not_onehot(tag(66, 64, 48, 3, seed=2))}
for name, args, T in (("th", "true,2,6,0", 8), ("move", "true,0,0,0", 8), ("float", "false,0,0,0", 8), ("cleanup", "true,0,0,2", 10), ("cleanup_float", "false,0,0,2", 10),
                      ("tag", "true,1,4,1", 10), ("tag_c5", "true,0,0,1", 10), ("tag_float", "false,0,0,1", 10)):
    case(f"sk256_{name}", _g256[name], 7, "step", f"step_kernel<256,{args},0,0,0,false,64,false>", T, force_generic=1)
# more than 64 agents: 65 on a 12x12 map (100 interior cells), 128-entry per-agent arrays
_many = {"move": lambda: th(12, 12, 65, 2, seed=51), "float": lambda: not_onehot(th(12, 12, 65, 2, seed=52)), "tag": lambda: tag(12, 12, 65, 2),
         "tag_float": lambda: not_onehot(tag(12, 12, 65, 2)), "cleanup": lambda: cleanup(12, 12, 65, beam=2, r=2), "cleanup_float": lambda: not_onehot(cleanup(12, 12, 65, beam=2, r=2))}
for name, args in (("move", "true,0,0,0"), ("float", "false,0,0,0"), ("tag", "true,0,0,1"), ("tag_float", "false,0,0,1"), ("cleanup", "true,0,0,2"), ("cleanup_float", "false,0,0,2")):
    case(f"many_{name}", _many[name], 9, "step", f"step_kernel<256,{args},0,0,0,false,128,false>", 6)

# ----------------------------------------------------------------------------- the phase and row kernels: 9
_rows = {2: lambda: th(14, 18, 3, 2, seed=61), 3: lambda: th(32, 32, 8, 3, seed=62), 5: lambda: th(12, 14, 3, 5, seed=63)}
for r, mk in _rows.items():
    case(f"phase_rows_r{r}", mk, 37, "phase_rows", f"phase_rows<2,2,{r}>")
    case(f"observe_rows_r{r}", mk, 37, "observe_rows", f"observe_rows<2,2,{r}>")
case("sweep_rows_c3", _rows[3], 37, "sweep_rows", "step_fast_rows<2,6,3,32,32,false,false>")
case("phase_kernel_onehot", lambda: th(48, 48, 6, 4, seed=64), 7, "phase_kernel", "phase_kernel<true>")      # no phase_rows<2, 2, 4> in the library
case("phase_kernel_float", lambda: not_onehot(th(48, 48, 6, 3, seed=65)), 7, "phase_kernel", "phase_kernel<false>")


def actions_for(entry, t):
    """The actions of turn ``t``: None where the exercise lets the device draw them (step / rollout / walk), else a fixed random table."""
    if entry.role in ("step", "rollout", "walk"):
        return None
    ws = entry.built().spec
    rng = np.random.default_rng(1000 + t)
    return rng.integers(0, len(ws.action_dy), size=(entry.num_envs, ws.num_agents), dtype=np.uint8)


FIRST_ENV, EPOCH = 3, 1


def begin_oracle(entry):
    """The C oracle at the start of the case's exercise."""
    w = entry.built()
    co = H.COracle(w.spec, entry.num_envs, first_env_id=FIRST_ENV)
    if w.start is None:
        co.reset(EPOCH)
    else:
        co.grid[...], co.pos[...], co.total[...] = w.start[0], w.start[1], 0
    return co


def oracle_turn(entry, co, t):
    """Turn ``t`` of the case on the oracle; returns its status word."""
    acts = actions_for(entry, t)
    return co.step(EPOCH, t, random_actions=True) if acts is None else co.step(EPOCH, t, actions=acts)
