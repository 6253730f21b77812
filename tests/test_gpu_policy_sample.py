"""``sgw_policy_sample`` on the device: the reference's fixture (``tests/golden/policy``) through the C ABI and through
``GridEngine.policy_sample``; a grid of action counts (every bucket and the generic loop), row counts around the wave and the tile,
strides, a base the 16-byte loads must step aside for, ``idx`` with repeats, keys that cross a Philox word and a counter -- all against the
NumPy restatement (``tests/policy_common.py``, itself pinned by the fixture in ``tests/test_policy_cpu.py``); more row tiles than
workgroups; invalid rows and the bytes around every output; and a sampling policy through the four turn loops of the environment.

Bounds.  Actions are compared for equality.  Log-probabilities and entropies are held to ONE float32 ulp of the reference / the
restatement: the values are float64 results rounded once, and the device's ``log`` / ``exp`` may differ from NumPy's in the last float64
bit (after at most 256 terms of one sign that is below 2^-44 relative: it can move a float32 rounding by one step, not two).  In logits
mode the weights themselves carry that last-bit difference, so equal actions are demanded only after asserting ON THE RESTATEMENT that
every threshold keeps 2^-40 S from every running sum.  No expectation comes from the kernel."""
import ctypes as C

import numpy as np
import pytest

from sorrel_amd import _native as N
from tests import policy_common as PC
from tests.gpu_common import torch_cuda  # noqa: F401
from tests.learner_common import DEV, Guarded

pytestmark = pytest.mark.gpu

META, SETS = PC.load_fixture()


def abi_sample(torch, x, *, logits=False, stride=None, misalign=False, idx=None, num_envs, agent0=0, seed=0, first_env=0, epoch=0, turn=0,
               want_lp=True, want_ent=True):
    """One ``sgw_policy_sample`` call over the host rows ``x [n, na]`` (float32 / float64), laid out as the caller describes; every output
    sits inside guards, which must come back untouched.  Returns (actions, log_probs or None, entropy or None)."""
    lib = N.load()
    n, na = x.shape
    stride = na if stride is None else stride
    host = np.full((n, stride), 0.015625, x.dtype)             # (what lies between the rows is a valid weight: reading it would change results)
    host[:, :na] = x
    flat = torch.from_numpy(np.concatenate([np.zeros(1, x.dtype), host.ravel()])).to(DEV)
    dist = flat[1:] if misalign else flat[1:].clone()
    assert not misalign or dist.data_ptr() % 16 == x.dtype.itemsize          # (the 16-byte loads must step aside)
    acts = Guarded(torch, n, np.int64)
    lps = Guarded(torch, n, np.float32) if want_lp else None
    ents = Guarded(torch, n, np.float32) if want_ent else None
    d = N.SgwPolicyDesc()
    d.dist = dist.data_ptr()
    keep = None
    if idx is not None:
        keep = torch.from_numpy(np.asarray(idx, np.int64)).to(DEV)
        d.idx = keep.data_ptr()
    d.out_actions = acts.ptr
    d.out_log_probs = lps.ptr if lps else None
    d.out_entropy = ents.ptr if ents else None
    d.n, d.num_envs, d.row_stride, d.num_actions = n, num_envs, stride, na
    d.seed, d.first_env, d.epoch, d.turn, d.agent0 = seed, first_env, epoch, turn, agent0
    d.dist_type = N.POLICY_F64 if x.dtype == np.float64 else N.POLICY_F32
    d.mode = N.POLICY_LOGITS if logits else N.POLICY_PROBS
    rc = lib.sgw_policy_sample(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == N.OK, lib.sgw_last_error()
    torch.cuda.synchronize()
    for g in (acts, lps, ents):
        assert g is None or g.intact(), "bytes outside an output were written"
    return acts.numpy(), lps.numpy() if lps else None, ents.numpy() if ents else None


def check(got, want, ctx):
    acts, lps, ents = got
    wa, wl, we = want
    assert np.array_equal(acts, wa), (ctx, "actions", np.flatnonzero(acts != wa)[:8])
    if lps is not None:
        assert PC.ulps(lps, wl).max() <= 1, (ctx, "log-probabilities", int(PC.ulps(lps, wl).max()))
    if ents is not None:
        assert PC.ulps(ents, we).max() <= 1, (ctx, "entropies", int(PC.ulps(ents, we).max()))


# ------------------------------------------------------------------------------------------------------------- the reference's fixture
@pytest.mark.parametrize("bits", (64, 32))
def test_fixture_through_the_abi(torch_cuda, bits):
    for tag, s in SETS.items():
        got = abi_sample(torch_cuda, s[f"probs{bits}"], idx=s["idx"], num_envs=META["num_envs"], seed=META["seed"], first_env=META["first_env"],
                         epoch=META["epoch"], turn=META["turn"])
        check(got, (s[f"actions{bits}"], s[f"ref_lp{bits}"], s[f"ref_ent{bits}"]), (tag, bits))


@pytest.mark.parametrize("bits", (64, 32))
def test_fixture_through_grid_engine_policy_sample(torch_cuda, bits):
    torch = torch_cuda
    from sorrel_amd.models import ActionProbs
    from sorrel_amd.spec import treasurehunt_spec
    from tests.gpu_common import make_engine

    eng = make_engine(treasurehunt_spec(8, 8, 2, 2, seed=META["seed"]), META["num_envs"], first=META["first_env"])
    for tag, s in SETS.items():
        probs = torch.from_numpy(s[f"probs{bits}"]).to(DEV)
        idx = torch.from_numpy(s["idx"]).to(DEV)
        acts, lps, ents = eng.policy_sample(ActionProbs(probs), idx=idx, epoch=META["epoch"], turn=META["turn"])
        check((acts.cpu().numpy(), lps.cpu().numpy(), ents.cpu().numpy()), (s[f"actions{bits}"], s[f"ref_lp{bits}"], s[f"ref_ent{bits}"]), (tag, bits))
        # out=: the caller's tensors are the ones written; a bare tensor counts as probabilities; False = not wanted
        oa = torch.full_like(acts, -1)
        ol = torch.full_like(lps, 7.0)
        ra, rl, re_ = eng.policy_sample(probs, idx=idx, epoch=META["epoch"], turn=META["turn"], out_actions=oa, out_log_probs=ol, out_entropy=False)
        assert ra is oa and rl is ol and re_ is None and torch.equal(oa, acts) and torch.equal(ol, lps)
    # the engine's own epoch / turn are the defaults, agent = the key of one agent's [E] rows
    eng.epoch, eng.turn = 5, 9
    s = SETS["4"]
    probs = torch.from_numpy(s["probs32"][:META["num_envs"]]).to(DEV)
    acts, lps, ents = eng.policy_sample(ActionProbs(probs), agent=6)
    u = PC.draws(META["seed"], META["first_env"], np.arange(META["num_envs"]), 5, 9, 6)
    check((acts.cpu().numpy(), lps.cpu().numpy(), ents.cpu().numpy()), PC.restate(s["probs32"][:META["num_envs"]], False, u)[:3], "defaults")
    with pytest.raises(ValueError):
        eng.policy_sample(probs.to(torch.float16))
    with pytest.raises(ValueError):
        eng.policy_sample(probs, out_actions=torch.zeros(3, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):                         # a ring without bound replay rows: which row the turn fills is unknown
        eng.turn_policy_sample(0, ActionProbs(probs), torch.zeros(META["num_envs"], dtype=torch.int64, device=DEV),
                               torch.zeros((4, META["num_envs"]), dtype=torch.float32, device=DEV))


# ------------------------------------------------------------------------------------------------------------- a grid against the restatement
def rows_of(rng, n, na, logits, dtype):
    if logits:
        x = rng.integers(-32, 33, size=(n, na)).astype(np.float64) / 8.0
        x[rng.random((n, na)) < 0.15] = -np.inf
        x[np.arange(n), rng.integers(0, na, size=n)] = rng.integers(-8, 9, size=n) / 8.0      # (never a row of -inf alone)
    else:
        x = rng.integers(0, 9, size=(n, na)).astype(np.float64)
        x[rng.random((n, na)) < 0.3] = 0.0
        x[np.arange(n), rng.integers(0, na, size=n)] += 1.0                                  # (never an all-zero row)
        x /= 1024.0                                                                            # multiples of 2^-10: every sum is exact
    return x.astype(dtype)


@pytest.mark.parametrize("na", (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 256))
def test_grid_against_the_restatement(torch_cuda, na):
    rng = np.random.default_rng(9000 + na)
    case = 0
    for n in (1, 63, 64, 65, 257):
        for logits in (False, True):
            for dtype, wider, misalign, use_idx in ((np.float32, False, False, False), (np.float32, True, False, True), (np.float32, False, True, False),
                                                    (np.float64, False, False, True), (np.float64, True, False, False)):
                case += 1
                agent0 = (0, 3, 4, 127)[case % 4]
                num_envs = n if agent0 == 127 else max(1, n // 3)          # rows run over several agents: 3 -> 4 crosses a Philox word, 4 a counter
                seed, first_env = int(rng.integers(0, 1 << 63)), int(rng.integers(0, 1 << 20))
                epoch, turn = int(rng.integers(0, 1 << 28)), int(rng.integers(0, 1 << 32))
                idx = None
                if use_idx:                                                 # repeats and any order, every agent key that exists
                    idx = rng.integers(0, num_envs * 128, size=n).astype(np.int64)
                    idx[n // 2] = idx[0]
                    idx[-1] = num_envs * 128 - 1
                x = rows_of(rng, n, na, logits, dtype)
                env, agent = PC.keys_of_rows(n, num_envs, agent0, idx)
                want = PC.restate(x, logits, PC.draws(seed, first_env, env, epoch, turn, agent))
                assert not want[3]["bad"].any()
                if logits:
                    assert PC.margin(want[3]) >= PC.MARGIN
                stride = na + (3 if wider else 0) if not (wider and na % 4 == 0) else na + 4   # (a wider stride that keeps 16-byte rows, too)
                got = abi_sample(torch_cuda, x, logits=logits, stride=stride, misalign=misalign, idx=idx, num_envs=num_envs, agent0=agent0, seed=seed,
                                 first_env=first_env, epoch=epoch, turn=turn)
                check(got, want[:3], dict(na=na, n=n, logits=logits, dtype=dtype.__name__, stride=stride, misalign=misalign, idx=use_idx, agent0=agent0))


def test_more_row_tiles_than_workgroups(torch_cuda):
    n = PC.max_blocks() * 256 + 3
    rng = np.random.default_rng(77)
    x = rows_of(rng, n, 2, False, np.float32)
    num_envs = n // 2 + 1
    env, agent = PC.keys_of_rows(n, num_envs, 3)
    want = PC.restate(x, False, PC.draws(11, 5, env, 2, 40, agent))
    check(abi_sample(torch_cuda, x, num_envs=num_envs, agent0=3, seed=11, first_env=5, epoch=2, turn=40), want[:3], "strided tiles")
    assert len(set(want[0][-260:].tolist())) == 2            # (the rows of the last, strided-to tile do take both actions)


# ------------------------------------------------------------------------------------------------------------- invalid rows
@pytest.mark.parametrize("na", (3, 8, 20))
def test_invalid_rows_get_255_and_nan_and_their_neighbours_are_untouched(torch_cuda, na):
    rng = np.random.default_rng(na)
    n = 70
    x = rows_of(rng, n, na, False, np.float64)
    x[5, 1] = -0.25
    x[6, 0] = np.nan
    x[20] = 0.0
    x[63, na - 1] = np.inf                                     # S is not finite
    x[64, 0], x[64, 2] = 0.5, -0.0                             # (a negative zero is no negative weight)
    bad = [5, 6, 20, 63]
    u = PC.draws(3, 0, np.arange(n), 1, 2, 9)
    for dtype in (np.float64, np.float32):
        want = PC.restate(x.astype(dtype), False, u)
        assert np.flatnonzero(want[3]["bad"]).tolist() == bad
        got = abi_sample(torch_cuda, x.astype(dtype), num_envs=n, agent0=9, seed=3, epoch=1, turn=2)
        check(got, want[:3], ("probs", dtype.__name__))
        assert (got[0][bad] == 255).all() and np.isnan(got[1][bad]).all() and np.isnan(got[2][bad]).all()
        assert (np.delete(got[0], bad) < na).all() and np.isfinite(np.delete(got[1], bad)).all() and np.isfinite(np.delete(got[2], bad)).all()
    y = rows_of(rng, n, na, True, np.float64)
    y[7, 0] = np.inf
    y[8] = -np.inf
    y[9, 1] = np.nan
    y[64] = -np.inf
    y[64, 2] = 0.5                                             # one finite logit: probability 1
    want = PC.restate(y, True, u)
    assert np.flatnonzero(want[3]["bad"]).tolist() == [7, 8, 9] and PC.margin(want[3]) >= PC.MARGIN and want[0][64] == 2
    got = abi_sample(torch_cuda, y, logits=True, num_envs=n, agent0=9, seed=3, epoch=1, turn=2)
    check(got, want[:3], "logits")
    # idx entries that name no (env, agent) pair: that row alone is refused
    idx = np.arange(n, dtype=np.int64)
    idx[3], idx[4], idx[66] = -1, n * 128, -n
    env, agent = PC.keys_of_rows(n, n, idx=idx)
    want = PC.restate(x, False, PC.draws(3, 0, np.maximum(env, 0), 1, 2, np.clip(agent, 0, 127)))
    for k in (3, 4, 66):
        want[0][k], want[1][k], want[2][k] = 255, np.nan, np.nan
    check(abi_sample(torch_cuda, x, idx=idx, num_envs=n, seed=3, epoch=1, turn=2), want[:3], "idx")
    # NULL out_log_probs / out_entropy: nothing but the actions is written (and they are the same actions)
    only = abi_sample(torch_cuda, x, idx=idx, num_envs=n, seed=3, epoch=1, turn=2, want_lp=False, want_ent=False)
    assert only[1] is None and only[2] is None and np.array_equal(only[0], want[0])
    one = abi_sample(torch_cuda, x, idx=idx, num_envs=n, seed=3, epoch=1, turn=2, want_lp=True, want_ent=False)
    check(one, (want[0], want[1], None), "log-probabilities alone")


# ------------------------------------------------------------------------------------------------------------- through the environment
def test_sampling_policy_through_every_turn_loop(torch_cuda):
    """Treasurehunt 8x8, 2 agents, 5x5 windows, 65 envs, 6 turns; the model is a fixed linear layer + softmax that returns ``ActionProbs``,
    the memories are ``RolloutBuffer``s.  Generic hooks, fast loop, a recorded turn replayed, ``speculate_turns = "always"`` (declined: the
    eager loop plays) and the older per-launch protocol give the same bits, and what they stored is the restatement of the stored windows'
    probabilities; the same model over an ordinary ``Buffer`` (fast loop) stores the same actions and nothing else."""
    torch = torch_cuda
    from sorrel_amd.buffers import Buffer, RolloutBuffer
    from sorrel_amd.models import ActionProbs, BaseModel
    from tests.gpu_common import make_env

    E, A, T, CAP = 65, 2, 6, 8

    class Softmax(BaseModel):
        def __init__(self, input_size, action_space, k, ring):
            super().__init__(input_size, action_space, memory_size=0, num_envs=E, device=DEV)
            self.memory = ring(capacity=CAP, obs_shape=tuple(input_size), num_envs=E, device=DEV)
            g = torch.Generator().manual_seed(31 + k)
            # multiples of 1/8 against one-hot windows: the logits are exact in any order of summation
            self.weight = (torch.randint(-8, 9, (int(np.prod(input_size)), action_space), generator=g).float() / 8.0).to(DEV)

        def probs(self, state):
            return torch.softmax(state.reshape(state.shape[0], -1) @ self.weight, dim=1)

        def take_action(self, state):
            return ActionProbs(self.probs(state))

    def build(mode, ring=RolloutBuffer):
        made = []

        def factory(input_size, action_space):
            made.append(Softmax(input_size, action_space, len(made), ring))
            return made[-1]

        env = make_env(8, 8, A, 2, E, p=0.05, seed=21, model_factory=factory)
        env.fast_policy_loop = mode not in ("generic", "per_launch")
        env.patch_windows = mode != "per_launch"                                # (the older protocol: a window rendered per act launch)
        env.speculate_turns = "always" if mode == "speculative" else False
        return env

    envs = {mode: build(mode) for mode in ("generic", "fast", "recorded", "speculative", "per_launch")}
    assert envs["fast"].turn_plan()["loop"] == "fast" and envs["generic"].turn_plan()["loop"] == "generic"
    plain = build("plain", Buffer)
    assert envs["speculative"].turn_plan()["loop"] != "speculative"            # declined: a sampling policy plays the eager loop
    cap = envs["recorded"].capture_turn(warmup=2, force=True)
    assert cap is not None, envs["recorded"].capture_error
    rec = envs["recorded"].agents[0].model.memory
    for t in range(T):
        for mode, env in list(envs.items()) + [("plain", plain)]:
            if mode == "recorded" and t < 2:
                continue                                                       # (its two warm-up turns were real turns)
            env.take_turn()
        if t == 3:      # two consecutive replays (turns 3 and 4): two different ring rows, two different draws
            torch.cuda.synchronize()
            assert cap.turns_replayed == 2 and rec.idx == 4
            assert not torch.equal(rec.log_probs[2], rec.log_probs[3]) and not torch.equal(rec.actions[2], rec.actions[3])
            assert not rec.log_probs[4:].any()                                 # (the rows of later turns are still empty)
    torch.cuda.synchronize()
    assert cap.turns_replayed == T - 2 and envs["speculative"].__dict__.get("speculation_passes", 0) == 0
    ref = envs["generic"]
    assert ref.turn == T and all(env.turn == T for env in envs.values())
    for mode, env in envs.items():
        for name in ("grid", "agent_pos", "total_reward"):
            assert torch.equal(getattr(ref.world, name), getattr(env.world, name)), (mode, name)
        assert torch.equal(ref.rewards, env.rewards) and torch.equal(ref.actions, env.actions), mode
        for a in range(A):
            ma, mb = ref.agents[a].model.memory, env.agents[a].model.memory
            assert (mb.idx, mb.size) == (T, T) and isinstance(mb, RolloutBuffer), (mode, a)
            for name in ("states", "actions", "rewards", "dones", "log_probs"):
                assert torch.equal(getattr(ma, name), getattr(mb, name)), (mode, a, name)
        env.raise_on_status()
    # what was stored is the restatement of the stored windows' probabilities: float64 on the host, keyed by (seed, env, epoch, turn, agent)
    eng = ref._engine
    for a in range(A):
        model = ref.agents[a].model
        mem = model.memory
        for t in range(T):
            probs = model.probs(mem.states[t]).cpu().numpy()                   # (the same device arithmetic on the same exact logits)
            u = PC.draws(int(eng.spec.seed), eng.first_env_id, np.arange(E), ref.epoch, t + 1, a)
            actions, lp, _ent, info = PC.restate(probs, False, u)
            assert not info["bad"].any()
            assert np.array_equal(mem.actions[t].cpu().numpy(), actions), (a, t)
            assert PC.ulps(mem.log_probs[t].cpu().numpy(), lp).max() <= 1, (a, t)
        assert not mem.log_probs[T:].any() and not mem.actions[T:].any()
        # the actions the engine recorded are the sampled ones
        assert torch.equal(ref.actions[:, a].to(torch.int64), mem.actions[T - 1])
    # the same model with an ordinary Buffer stores the actions only -- the same ones, the draw being keyed
    for a in range(A):
        mp = plain.agents[a].model.memory
        assert type(mp) is Buffer and not hasattr(mp, "log_probs")
        assert torch.equal(mp.actions, ref.agents[a].model.memory.actions) and torch.equal(mp.states, ref.agents[a].model.memory.states)
    assert torch.equal(plain.world.grid, ref.world.grid)
