/*
 * sgw.h -- C ABI of the MI355X batched gridworld step/observation engine.
 *
 * Sorrel (social-ai-uoft/sorrel v1.4.0) is pure Python and has no FFI; the
 * interface a maintainer would bind is its class-based plugin API.  Each entry
 * point below names the reference interface it replaces for a batch of E
 * independent environments (paths relative to the reference root):
 *
 *   sgw_create      Environment.__init__ / setup_agents       sorrel/environment.py:36-54
 *                   + OneHotObservationSpec.__init__/generate_map
 *                                                             sorrel/observation/observation_spec.py:128-173
 *                   + Entity attribute table                  sorrel/entities/entity.py:29-39
 *                   + ActionSpec / MovingAgent.movement table sorrel/action/action_spec.py:23-26,
 *                                                             sorrel/agents/agent.py:187-213
 *   sgw_reset       Environment.reset -> Gridworld.create_world + populate_environment
 *                                                             sorrel/environment.py:72-79,
 *                                                             sorrel/worlds/gridworld.py:47-65,
 *                                                             sorrel/examples/treasurehunt/env.py:114-147
 *   sgw_observe     OneHotObservationSpec.observe -> visual_field -> shift
 *                                                             sorrel/observation/observation_spec.py:175-205,
 *                                                             sorrel/observation/visual_field.py:9-101,
 *                                                             sorrel/utils/helpers.py:48-77
 *   sgw_observe_full  ObservationSpec(full_view=True).observe  sorrel/observation/observation_spec.py:197-203,
 *                                                             sorrel/observation/visual_field.py:41-55
 *   sgw_step        Environment.take_turn                     sorrel/environment.py:81-93
 *                   -> Entity.transition sweep                sorrel/examples/treasurehunt/entities.py:69-85
 *                   -> Agent.transition (pov, act, reward)    sorrel/agents/agent.py:155-173
 *                   -> MovingAgent.act -> Gridworld.move      sorrel/agents/agent.py:215-225,
 *                                                             sorrel/worlds/gridworld.py:95-122
 *   sgw_observe_rows / sgw_act   Agent.transition of a policy-driven agent: pov, then act
 *                                                             sorrel/agents/agent.py:155-173, 215-225
 *   sgw_rollout     the turn loop of run_experiment           sorrel/environment.py:160-166
 *   sgw_reduce_metrics  world.total_reward read-out           sorrel/environment.py:193-199
 *
 * Conventions
 *   - every function returns 0 on success or a negative SGW_E* code and never
 *     throws; sgw_last_error() returns the message of the calling thread's
 *     last failure;
 *   - all array arguments are DEVICE pointers owned by the caller (PyTorch);
 *     the library owns only the engine handle, its constant tables and a small
 *     reduction workspace;
 *   - all kernels are enqueued asynchronously on the HIP stream passed as `stream`
 *     (a hipStream_t, NULL = default stream).  The calls that block the host are:
 *     sgw_create / sgw_destroy (allocate and upload the constant tables with blocking
 *     copies), sgw_get_status, sgw_get_step_time_ms and sgw_get_step_times_ms (they
 *     wait for the events / the status word they read), and -- only while timing is
 *     enabled with sgw_set_timing -- every 4096th sgw_step / sgw_observe, which waits
 *     for its oldest pair of events when the event pool wraps;
 *   - one engine per device, not thread-safe per engine (the reference is
 *     single-threaded);
 *   - there is no CPU fallback: without a HIP device every launch fails.
 *
 * Tensor layouts (C order, per-env contiguous)
 *   grid          uint8  [E][L][H][W]   entity TYPE id per cell (env e starts at e * grid_env_stride)
 *   agent_pos     uint8  [E][A][2]      (y, x) of each agent on `agent_layer`
 *   actions       uint8  [E][A]         action index per agent
 *   obs           float  [E][A][C][V][V], V = 2*vision_radius+1
 *   rewards       float  [E][A]
 *   total_reward  double [E]            world.total_reward (float64, agent order)
 */
#ifndef SGW_H
#define SGW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGW_MAX_TYPES 32
#define SGW_MAX_CHANNELS 16
#define SGW_MAX_CHOICES 8
#define SGW_MAX_ACTIONS 16
#define SGW_MAX_AGENTS 128 /* round 6 (64 before): up to 64 agents every kernel family applies (lane = agent on the wave- / workgroup-per-env kernels); 65..128 run on
                            * the ticket-ordered workgroup-per-env generic kernel, whatever the world's size (the reference steps any list: sorrel/environment.py:92-93) */
#define SGW_MAX_LAYERS 7   /* numpy sums <= 7 layers left to right; 8+ pairwise */
#define SGW_MAX_DIM 256    /* positions are uint8 */

/* entity transition rules (Entity.transition plugins the device can run) */
#define SGW_RULE_NONE 0
#define SGW_RULE_SPAWN 1   /* w.p. p replace own cell by one of n types, uniformly */
#define SGW_RULE_BECOME_IF 2 /* become rule_become if the cell of layer rule_layer in the same column holds a type in
                             * rule_mask; rule_layer < 0 = always (timers).  Cleanup: Pollution, Apple, beams
                             * (sorrel/examples/cleanup/entities.py:57-66,94-105, agents.py:190-205).  Columns are
                             * swept in ndenumerate order: a lower layer has already transitioned, a higher has not. */

#define SGW_NO_BORDER 255

/* observation post-processing (sgw_config.obs_post) */
/* action kinds (sgw_config.action_kind), SGW_AGENT_RULE_CLEANUP */
#define SGW_ACTION_MOVE 0
#define SGW_ACTION_CLEAN 1
#define SGW_ACTION_ZAP 2

#define SGW_OBS_POST_NONE 0            /* OneHotObservationSpec: the layer sum itself */
#define SGW_OBS_POST_CLIP255_DIV255 1  /* RGBObservationSpec: np.clip(obs, 0, 255) / 255 (observation_spec.py:483) */

/* counter-RNG stream ids: u32 = Philox4x32-10(ctr = {index>>2, turn, env, epoch<<4|stream},
 * key = {seed lo, seed hi})[index & 3] */
#define SGW_STREAM_SPAWN 0
#define SGW_STREAM_SPAWN_KIND 1
#define SGW_STREAM_ACTION 2
#define SGW_STREAM_PLACE 3
#define SGW_STREAM_DENSE 4
#define SGW_STREAM_DENSE_KIND 5
#define SGW_STREAM_TAG_INIT 6
#define SGW_STREAM_EXPLORE 7           /* index = agent: the epsilon test of SGW_ACT_QF32 (sgw_turn_epsilon) */
#define SGW_STREAM_VALUE 8             /* index = layer-major cell index of the TARGET cell (the spawn stream's index), turn = the turn in
                                        * flight: which of its two values a type with value_alt_prob > 0 is worth this turn */
#define SGW_STREAM_SAMPLE 9            /* sgw_sample's drawn indices: epoch 0, turn / env = the low / high word of the draw counter */
#define SGW_STREAM_POLICY 10u          /* (unsigned, as the flags are: it is or-ed into a 32-bit counter word) index = agent, turn = the turn in flight: the uniform sgw_policy_sample draws an action with (SGW_STREAM_EXPLORE's layout) */

/* what Agent.act does (sgw_config.agent_rule) */
#define SGW_AGENT_RULE_MOVE 0 /* MovingAgent.act: reward = value of the target, then move (sorrel/agents/agent.py:215-225) */
#define SGW_AGENT_RULE_CLEANUP 2 /* CleanupAgent.act: move (turning the agent) or fire a clean / zap beam; reward summed over
                                  * all layers of the target cell (sorrel/examples/cleanup/agents.py:93-177);
                                  * needs sgw_bind_agent_dir */
#define SGW_AGENT_RULE_TAG 1  /* TagAgent.act: move, tag the first adjacent NotIt agent, reward for not being it
                               * (sorrel/examples/tag/agents.py:76-106); needs sgw_bind_agent_state */

/* sgw_step flags */
#define SGW_STEP_SWEEP 1u           /* run the entity-transition sweep first */
#define SGW_STEP_RANDOM_ACTIONS 2u  /* draw actions from STREAM_ACTION and STORE them to `actions` */
#define SGW_STEP_NO_OBS 4u          /* do not write observations (obs may be NULL) */
#define SGW_STEP_OBS_NEXT 8u        /* policy-driven (phased) stepping: do NOT write the observations of the stepped
                                     * agents; instead write the observation of agent `agent_end` (if < num_agents) from
                                     * the grid AFTER the moves of [agent_begin, agent_end) -- exactly what that agent's
                                     * pov() sees next (sorrel/agents/agent.py:167), so a policy turn costs 1 + A
                                     * launches instead of 1 + 2A */
#define SGW_STEP_OBS_NEXT_PACKED 16u /* with SGW_STEP_OBS_NEXT: `obs` is NOT the [E][A][C][V][V] tensor but one window per env,
                                     * [E][C][V][V] contiguous, which receives agent `agent_end`'s observation -- e.g. the
                                     * slot of that agent's replay buffer its pov() is about to be stored in
                                     * (sorrel/agents/agent.py:155-173: state = pov(); ...; add_memory(state, ...)), so the
                                     * observation is written once, where it will live */
#define SGW_STEP_NO_MOVE 32u         /* nobody acts: the entity sweep (with SGW_STEP_SWEEP) and the windows of [agent_begin, agent_end)
                                     * from the grid after it -- step 1 + 2 of a policy-driven turn in one launch when the windows
                                     * live in the [E][A][C][V][V] tensor (see sgw_act).  No rewards, no totals, no auto-reset;
                                     * SGW_STEP_RANDOM_ACTIONS / SGW_STEP_OBS_NEXT do not combine with it */
#define SGW_STEP_OBS_AGENT_MAJOR 64u /* `obs` is [A][E][C][V][V] (agent-major: agent a's windows of all envs are one contiguous [E][C*V*V] row, the shape a
                                     * replay ring row and a batched policy want) instead of [E][A][C][V][V].  Whole-turn calls (agent range 0 .. A, no
                                     * SGW_STEP_OBS_NEXT) of engines with SGW_CAP_OBS_AGENT_MAJOR -- the workgroup-per-env kernels (worlds above
                                     * 4 KiB): with SGW_STEP_NO_MOVE that is the sweep AND every agent's pre-move window into such rows in one launch */
#define SGW_STEP_DEFAULT (SGW_STEP_SWEEP)

/* error codes */
#define SGW_OK 0
#define SGW_EINVAL (-1)   /* rejected configuration / argument */
#define SGW_EHIP (-2)     /* HIP runtime error */
#define SGW_ENOMEM (-3)

/* bits of the device status word (sgw_get_status) */
#define SGW_STATUS_OOB_MOVE 1   /* an agent targeted a cell outside the grid (reference: IndexError / wrap) */
#define SGW_STATUS_BAD_ACTION 2 /* action index >= num_actions */
#define SGW_STATUS_BAD_TYPE 4   /* grid holds a type id >= num_types */
#define SGW_STATUS_BAD_POS 8    /* an agent position outside the grid was passed in (treated as (0, 0): memory-safe, result undefined) */

typedef struct sgw_config {
    int32_t height, width, layers;
    int32_t num_agents, vision_radius;
    int32_t num_types, num_channels, num_actions;
    int32_t agent_layer;   /* layer (z) every agent lives on */
    int32_t default_type;  /* Gridworld.default_entity: refills vacated cells */
    int32_t fill_type;     /* ObservationSpec.fill_entity_kind: out-of-bounds appearance */
    int32_t obs_post;      /* SGW_OBS_POST_*: applied to the float64 layer sum before the float32 cast */
    int8_t action_dy[SGW_MAX_ACTIONS]; /* in {-1,0,1}; (0,0) for non-move action names */
    int8_t action_dx[SGW_MAX_ACTIONS];
    uint8_t agent_type[SGW_MAX_AGENTS];
    double type_value[SGW_MAX_TYPES];     /* Entity.value */
    uint8_t type_passable[SGW_MAX_TYPES]; /* Entity.passable */
    uint8_t type_rule[SGW_MAX_TYPES];     /* SGW_RULE_* (Entity.has_transitions + transition) */
    double spawn_prob[SGW_MAX_TYPES];
    uint8_t spawn_count[SGW_MAX_TYPES];
    uint8_t spawn_choice[SGW_MAX_TYPES][SGW_MAX_CHOICES];
    double appearance[SGW_MAX_TYPES][SGW_MAX_CHANNELS]; /* ObservationSpec.entity_map[kind of type] */
    /* reset layout (populate_environment): per-layer fill and border types,
     * optional Bernoulli pre-seeding of the agent layer's interior, agents on
     * distinct interior cells */
    uint8_t layer_fill_type[8];
    uint8_t layer_border_type[8]; /* SGW_NO_BORDER = none */
    double dense_prob;
    uint8_t dense_count;
    uint8_t dense_choice[SGW_MAX_CHOICES];
    uint8_t agent_rule;     /* SGW_AGENT_RULE_*: what Agent.act does */
    uint8_t tag_it_type;    /* SGW_AGENT_RULE_TAG: type of an agent that is "it" (kind "It") */
    uint8_t tag_notit_type; /*                     ... that is not (kind "NotIt") */
    uint8_t reserved1[4];
    uint64_t seed;
    uint64_t first_env_id; /* global id of local env 0 (multi-GPU sharding) */
    int64_t num_envs;      /* E on this device */
    double tag_reward;     /* SGW_AGENT_RULE_TAG: TagAgent.reward_per_turn */
    /* SGW_RULE_BECOME_IF parameters, per type */
    int8_t rule_layer[SGW_MAX_TYPES];
    uint8_t rule_become[SGW_MAX_TYPES];
    uint32_t rule_mask[SGW_MAX_TYPES];
    /* SGW_AGENT_RULE_CLEANUP parameters */
    uint8_t action_kind[SGW_MAX_ACTIONS];
    int32_t beam_radius;
    uint8_t clean_beam_type; /* type of a freshly fired beam (its timer = a chain of SGW_RULE_BECOME_IF types) */
    uint8_t zap_beam_type;
    uint8_t reserved2[2];
    uint32_t beam_block_mask;    /* bit t: no beam is placed on a beam-layer cell holding type t (walls) */
    int32_t reward_total_factor; /* how many times act's reward enters total_reward (0 = 1; Cleanup = 2) */
    int64_t grid_env_stride; /* bytes between consecutive envs in `grid`; 0 = dense (L*H*W).  A stride that is a
                              * multiple of 16 lets worlds of any byte count use the 16-byte load/store kernels */
    /* Drawn values (0.3; a pure suffix: every field above keeps its offset).  An entity whose value is redrawn every turn between two
     * outcomes (Deck.transition, sorrel/examples/iowa/entities.py:45-70): a type with value_alt_prob[t] > 0 is worth type_value_alt[t]
     * when u32(SGW_STREAM_VALUE, index = cell) < floor(value_alt_prob[t] * 2^32) (SGW_RULE_SPAWN's threshold convention), else
     * type_value[t].  The draw is a function of (seed, env, epoch, turn, cell): it is made when an agent targets the cell and never
     * stored.  SGW_AGENT_RULE_MOVE only, not on agent types; all zero = no type draws. */
    double type_value_alt[SGW_MAX_TYPES];
    double value_alt_prob[SGW_MAX_TYPES];
} sgw_config;

typedef struct sgw_engine sgw_engine;

int sgw_create(const sgw_config* cfg, sgw_engine** out);
void sgw_destroy(sgw_engine* eng);

int sgw_reset(sgw_engine* eng, uint8_t* grid, uint8_t* agent_pos, double* total_reward,
              uint32_t epoch, void* stream);

/* Stateless observation of agents [agent_begin, agent_end) from the current
 * grid; obs rows of other agents are left untouched. */
int sgw_observe(sgw_engine* eng, const uint8_t* grid, const uint8_t* agent_pos, float* obs,
                int32_t agent_begin, int32_t agent_end, void* stream);

/* The whole map as an observation -- ObservationSpec(full_view=True).observe -> visual_field(location=None)
 * (sorrel/observation/observation_spec.py:140-142,197-203, sorrel/observation/visual_field.py:41-55): `out`
 * [E][C][H][W] (float, or uint8 with SGW_OBS_U8) receives every cell's appearance summed over the layers; no window, no
 * fill entity, the same for every agent. */
int sgw_observe_full(sgw_engine* eng, const uint8_t* grid, void* out, void* stream);

/* One take_turn for every env.  `turn` is Environment.turn AFTER its increment
 * (1 for the first turn of an epoch).  Agents [agent_begin, agent_end) are
 * stepped sequentially; pass (0, num_agents) for a whole turn.  A policy-driven
 * loop that must reproduce "agent i+1 observes agent i's move" calls
 * sgw_step once per agent with SGW_STEP_SWEEP only on the first call. */
int sgw_step(sgw_engine* eng, uint8_t* grid, uint8_t* agent_pos, uint8_t* actions, float* obs,
             float* rewards, double* total_reward, uint32_t epoch, uint32_t turn,
             int32_t agent_begin, int32_t agent_end, uint32_t flags, void* stream);

/* ---- Policy-driven turns without re-rendering (round 3) ----------------------------------------------------------
 * The reference's agent loop is pov -> get_action -> act, one agent after another (sorrel/agents/agent.py:155-173), and
 * agent j's pov shows the moves of agents < j.  A move changes at most two cells of the agent layer, so instead of
 * rendering a window per agent and launch:
 *   1. sgw_step(agent_begin = agent_end = 0, SGW_STEP_SWEEP | SGW_STEP_NO_OBS)      the entity sweep alone
 *   2. sgw_observe_rows(...)  (or sgw_observe into the [E][A][C][V][V] tensor)       EVERY agent's window, once
 *      (1 + 2 in ONE launch when the windows live in the tensor: sgw_step(0, A, SGW_STEP_SWEEP | SGW_STEP_NO_MOVE))
 *   3. per agent a, in order: policy(window a) -> actions[:, a];  sgw_act(a)         move agent a AND rewrite, in the
 *      windows of the agents after a that contain them, the <= 2 cells its move changed
 * gives every agent exactly the window the reference's pov() would build, at the cost of one fused turn plus A tiny
 * launches.  `rows[a]` (a HOST array of num_agents DEVICE pointers) is where agent a's window lives: element
 * rows[a][e * env_stride + (c * V + i) * V + j] for env e -- a row of that agent's replay buffer (env_stride = C*V*V) or
 * slot a of the observation tensor (rows[a] = obs + a*C*V*V, env_stride = A*C*V*V); element type = sgw_set_obs_format's.
 * sgw_observe_rows needs SGW_CAP_OBSERVE_ROWS (one-hot float32 windows of an instantiated layers / channels / radius),
 * sgw_act (SGW_CAP_ACT) serves every agent rule -- MovingAgent.act, TagAgent.act (the tagger's and its victim's cells are
 * repaired too; agent_state / state_at_pov kept as by sgw_step) and CleanupAgent.act (beam cells too; agent_dir kept) --
 * for any appearance table and float32 or uint8 windows; rows entries of agents
 * <= `agent` are ignored by sgw_act, NULL entries (or rows == NULL) are skipped.
 * sgw_act's optional extras keep the host out of the agent loop: `agent_action` (device, [E], element type
 * `action_kind`) is read INSTEAD of actions[:, agent] -- the policy's output tensor as it is, no narrowing copy; the
 * uint8 record actions[:, agent] is still written -- and `reward_row` (float [E]) / `action_row` (int64 [E]) receive a
 * second copy of the rewards / the actions: the rows of the agent's replay buffer (sorrel/buffers.py:46-63 stores
 * int64 actions and float32 rewards), so add_memory has nothing left to copy.  All three may be NULL.
 * sgw_act never runs the in-stream reset of sgw_set_auto_reset (that belongs to whole-turn sgw_step / sgw_rollout calls):
 * a policy-driven epoch loop resets with sgw_reset, as Environment.run_experiment does. */
#define SGW_CAP_OBSERVE_ROWS 1
#define SGW_CAP_ACT 2
#define SGW_CAP_RESOLVE 4      /* sgw_turn_resolve (speculative policy turns): plain movers, impassable agent types, float32 windows, at most 64 agents
                                * (any other rule set or agent count: sgw_verify_rows) */
#define SGW_CAP_OBS_AGENT_MAJOR 8   /* sgw_step accepts SGW_STEP_OBS_AGENT_MAJOR */
#define SGW_CAP_SWEEP_ROWS 16       /* sgw_sweep_observe_rows: steps 1 and 2 of the patched-window protocol in ONE launch (round 6: every kernel family where the
                                     * in-process specialiser is available; without hipRTC the headline's prebuilt instance only) */
#define SGW_ACT_U8 0
#define SGW_ACT_I32 1
#define SGW_ACT_I64 2
/* SGW_ACT_QF32: `agent_action` is the policy's VALUE output, float32 [E][num_actions] (contiguous): the act takes the first index
 * of the row's maximum itself (np.argmax / torch.argmax; a NaN counts as the maximum, as in both) -- the greedy half of the
 * reference's take_action (sorrel/models/pytorch/iqn.py:294-309: `random.random() > epsilon` -> argmax of the action values, else a
 * uniform action), one launch less per agent in a recorded turn.  The other half under the turn protocol (sgw_turn_act /
 * sgw_turn_act_rows): with probability epsilon[agent] (sgw_turn_epsilon; 0 until set) the action is the engine's own uniform draw
 * for (env, turn, agent) -- the action SGW_STEP_RANDOM_ACTIONS would take, stream SGW_STREAM_ACTION -- decided by
 * u32(SGW_STREAM_EXPLORE, index = agent) < floor(epsilon * 2^32).  sgw_act has no turn of its own: it reads epoch, turn in flight
 * (= completed + 1) and epsilon from the same device state, which its caller keeps current with sgw_turn_set (epsilon 0, the
 * default, needs neither).  The action taken is recorded in actions[:, agent] (uint8) and the replay row (int64) as for the
 * other kinds. */
#define SGW_ACT_QF32 3
int sgw_capabilities(sgw_engine* eng);
int sgw_observe_rows(sgw_engine* eng, const uint8_t* grid, const uint8_t* agent_pos, void* const* rows, int64_t env_stride,
                     int32_t agent_begin, int32_t agent_end, void* stream);
int sgw_act(sgw_engine* eng, uint8_t* grid, uint8_t* agent_pos, uint8_t* actions, void* const* rows, int64_t env_stride,
            float* rewards, double* total_reward, int32_t agent, const void* agent_action, int32_t action_kind,
            float* reward_row, int64_t* action_row, void* stream);
/* Steps 1 and 2 of that protocol in one launch (SGW_CAP_SWEEP_ROWS; float32 windows): the entity sweep of Environment.take_turn
 * (sorrel/environment.py:84-90; flags = SGW_STEP_SWEEP, or 0 for none) and then EVERY agent's window of the grid after the sweep
 * (Agent.pov, sorrel/agents/agent.py:158) into rows[a] + env * env_stride, env_stride == C * V * V + the bound row tail exactly; the tail
 * (sgw_bind_row_tail: what TagAgent.pov / CleanupObservation.observe append) is written behind every window.  Round 5: the wave-per-env
 * kernel's compile-time-shape instances of plain movers; round 6: every family -- step_big<..., ROWS>, the chunk-staging instances
 * (step_fast_rowsx), the generic kernel (step_kernel<..., ROWS>), Tag's whole-env instances -- as instances of their own.  Same
 * results as sgw_step(SGW_STEP_SWEEP | SGW_STEP_NO_OBS, agents [0, 0)) followed by sgw_observe_rows; the grid is read once and the
 * windows leave as the step kernel's one burst per env (config 3 at 65 536 envs: 183 us in two launches). */
int sgw_sweep_observe_rows(sgw_engine* eng, uint8_t* grid, const uint8_t* agent_pos, void* const* rows, int64_t env_stride,
                           uint32_t epoch, uint32_t turn, uint32_t flags, void* stream);

/* `num_turns` whole take_turns (all agents, in order) with one call -- Environment.run_experiment's inner loop
 * `while turn < max_turns: take_turn()` (sorrel/environment.py:160-166) for actions that need no host in between: drawn
 * on device (SGW_STEP_RANDOM_ACTIONS) or given up front.  Turn t of the call (t = 0 .. num_turns-1, Environment.turn =
 * first_turn + t) reads / writes its actions, observations and rewards `t * *_turn_stride` ELEMENTS after the pointers
 * passed (a stride of 0 makes every turn overwrite the same tensor; a ring of replay slots passes the slot size); grid,
 * agent_pos and total_reward hold the state after the last turn.  Where the step kernel supports it the turns run
 * inside ONE launch with the env's grid resident in LDS from turn to turn (no grid read / write-back and no kernel
 * boundary between turns); elsewhere the call is a loop of sgw_step launches.  Results are identical either way, and
 * identical to num_turns calls of sgw_step.  With sgw_set_auto_reset armed an epoch boundary inside the range is
 * honoured (the turn counter restarts at 1 in epoch + 1). */
int sgw_rollout(sgw_engine* eng, uint8_t* grid, uint8_t* agent_pos, uint8_t* actions, float* obs, float* rewards,
                double* total_reward, uint32_t epoch, uint32_t first_turn, uint32_t num_turns, int64_t obs_turn_stride,
                int64_t actions_turn_stride, int64_t rewards_turn_stride, uint32_t flags, void* stream);

/* out (device, 4 doubles) = { sum(total_reward), sum(total_reward^2), E, 0 },
 * summed in a fixed order (bitwise reproducible). */
int sgw_reduce_metrics(sgw_engine* eng, const double* total_reward, double* out, void* stream);

/* Per-env agent state: the CURRENT entity type of every agent, uint8 [E][A] (Tag: It / NotIt; it
 * survives resets, as TagAgent.it does).  Once bound, sgw_reset places the agents with these types
 * and sgw_step keeps them up to date; `state_at_pov` (uint8 [E][A], may be NULL) receives each
 * agent's type at the moment it observed (what TagAgent.pov appends to its observation).
 * sgw_init_agent_state fills `agent_state` with the configured agent types and, for
 * SGW_AGENT_RULE_TAG, draws the initial "it" agent of every env (sorrel/examples/tag/env.py:66-69). */
int sgw_bind_agent_state(sgw_engine* eng, uint8_t* agent_state, uint8_t* state_at_pov);
int sgw_init_agent_state(sgw_engine* eng, uint8_t* agent_state, void* stream);
/* Facing of every agent, uint8 [E][A]: 0 up, 1 right, 2 down, 3 left (MovingAgent.direction; CleanupAgent
 * starts at 2).  Caller-initialised; sgw_step updates it on move actions and reads it to aim beams. */
int sgw_bind_agent_dir(sgw_engine* eng, uint8_t* agent_dir);
/* What every agent stepped on, uint8 [E][A] (GamblingAgent.encounters counts it per kind, sorrel/examples/iowa/agents.py:54-56): once
 * bound, every act of SGW_AGENT_RULE_MOVE -- sgw_step, sgw_rollout, sgw_act / sgw_turn_act*, the commit of sgw_turn_resolve -- writes the
 * type id world.observe(new_location) returned for that agent this turn, 255 for an agent whose action was invalid or whose target lies
 * outside the grid.  Written by the lane that writes the reward; NULL unbinds (nothing is written, nothing is paid).  sgw_rollout has no
 * turn stride for it: the tensor holds the LAST turn of the call. */
int sgw_bind_target_types(sgw_engine* eng, uint8_t* target_types);
/* Encounter counts: what the agents stepped on, summed (GamblingAgent.encounters, sorrel/examples/iowa/agents.py:21-56;
 * CleanupAgent.encounters, sorrel/examples/cleanup/agents.py:161-170).
 * counts: device int64 [E][A][num_slots], caller-owned, 8-byte aligned; NULL unbinds (slot_of_type / num_slots are then ignored).
 * slot_of_type: HOST array [cfg.num_types]; SGW_NO_SLOT = this type is not counted, else < num_slots.  num_slots in 1..32.
 * Once bound, every call that makes an agent act -- sgw_step, every turn of an sgw_rollout launch, sgw_act / sgw_turn_act* -- counts:
 *   SGW_AGENT_RULE_MOVE     an act whose action is valid and whose target lies inside the grid adds 1 to
 *                           counts[env][a][slot_of_type[t]], t = the type on the agent layer of the target cell BEFORE the move (the
 *                           value target_types records: an agent that takes a non-move action finds itself).
 *   SGW_AGENT_RULE_CLEANUP  under the condition the reward has (valid action, target inside the grid): one increment PER LAYER, for
 *                           the type that layer holds at the target cell, read where the reward is read -- after this act's beams are
 *                           placed, before the move.  One act can add two or three to one slot; an agent that stays finds itself.
 *   SGW_AGENT_RULE_TAG      refused (SGW_EINVAL): the reference keeps no such record there.
 * An out-of-range entry of slot_of_type, num_slots outside 1..32 or a misaligned pointer give SGW_EINVAL before anything changes.
 * The library never zeroes the counts: they run on across turns, across the turns of one sgw_rollout launch, across an auto-reset
 * epoch boundary, across sgw_reset and across replays of a recorded graph; when to clear them is the caller's decision.  One writer
 * per (env, agent) row and sequential acts within an env: plain read-modify-writes, no atomics.
 * While counts are bound the engine does not advertise SGW_CAP_RESOLVE (a speculative pass replays acts and would count them more than
 * once; drawn values set the precedent).  Unbinding restores exactly the kernels that ran before, as sgw_bind_target_types(NULL) does. */
#define SGW_NO_SLOT 255
int sgw_bind_encounters(sgw_engine* eng, int64_t* counts, const uint8_t* slot_of_type, int32_t num_slots);

/* Observation element type written by sgw_step / sgw_observe.  SGW_OBS_F32 (default) is the contract
 * format (the reference's replay buffer stores float32, sorrel/buffers.py:31).  SGW_OBS_U8 is a
 * compact extra for one-hot specs: the same [E][A][C][V][V] layout with uint8 counts (exactly the
 * float values, 4x fewer bytes); it is rejected for non one-hot appearance tables. */
#define SGW_OBS_F32 0
#define SGW_OBS_U8 1
int sgw_set_obs_format(sgw_engine* eng, int format);

/* Fill `actions` from STREAM_ACTION without stepping (what a RandomModel would choose). */
int sgw_random_actions(sgw_engine* eng, uint8_t* actions, uint32_t epoch, uint32_t turn, void* stream);

/* Synchronising: copies and clears the device status word (SGW_STATUS_* bits). */
int sgw_get_status(sgw_engine* eng, int32_t* status_out, void* stream);

/* Shape helpers (pure host arithmetic). */
int64_t sgw_obs_elems_per_env(const sgw_config* cfg);
int64_t sgw_grid_bytes_per_env(const sgw_config* cfg);
/* Algorithmic HBM bytes of one env-step (SURVEY.md 8d formula). */
int64_t sgw_algorithmic_bytes_per_env_step(const sgw_config* cfg);

/* Launch timing: with sgw_set_timing(eng, 1) every sgw_step / sgw_observe launch is bracketed by a pair of
 * HIP events on its stream.  sgw_get_step_time_ms returns (and clears) the sum and the number of launches since
 * the last read; sgw_get_step_times_ms copies the per-launch durations since the last read (oldest first, at most
 * `capacity`; *count = how many were written) to the HOST array `out_ms` and clears them; it returns 1 (not an error:
 * the durations written are valid) when launches were left out because `capacity` or the internal cap of 2^20 samples was
 * exceeded.  Both wait for the events they read. */
int sgw_set_timing(sgw_engine* eng, int enable);
int sgw_get_step_time_ms(sgw_engine* eng, double* total_ms, int64_t* launches);
int sgw_get_step_times_ms(sgw_engine* eng, float* out_ms, int64_t capacity, int64_t* count);

/* Auto-reset (Environment.run_experiment's epoch loop, sorrel/environment.py:148-171): once armed with
 * max_turns > 0, the sgw_step call that steps the LAST agent (agent_end == num_agents) of turn == max_turns also,
 * on the same stream and after the step kernel, copies total_reward to `episode_return` (device, double [E]; may be
 * NULL) and runs sgw_reset for epoch + 1 on the grid / agent_pos / total_reward it was given.  The caller goes on
 * with (epoch + 1, turn 1).  max_turns == 0 disarms. */
int sgw_set_auto_reset(sgw_engine* eng, uint32_t max_turns, double* episode_return);

/* Launch tuning of the wave-per-env step kernel.  Large float32 observation bursts of large batches run fastest
 * with fewer waves per CU than the register budget allows (fewer half-written observation streams open in HBM; see
 * DESIGN.md section 6); the only launch-time lever for that is the dynamic-LDS request, which bounds the workgroups
 * a CU admits.  wg_per_cu = 0 selects the documented automatic rule (a cap of 5 for whole-turn float32 observation
 * writes of >= 8 KiB per env when the batch's grids outgrow the caches or the emit is unstaged), 1..8 forces that
 * many workgroups per CU, -1 never caps.  sgw_launch_info writes a one-line description of what a whole-batch, whole-turn
 * sgw_step launches into buf: kernel variant, lanes per env, threads, `lds` = the dynamic-LDS bytes REQUESTED (the cap is
 * part of the request), `wg_per_cu` = the workgroups per CU the runtime admits for that request (occupancy query),
 * `cap` = policy and the cap in force (0 = none), `phase` = the kernel a policy-driven phase (one agent) takes. */
int sgw_set_wg_per_cu(sgw_engine* eng, int wg_per_cu);
int sgw_launch_info(sgw_engine* eng, char* buf, int64_t capacity);

/* ---- Options, the plan, specialised instances (round 4) -----------------------------------------------------------
 * The reference's plugin API takes ANY entity list, channel count and map size (sorrel/observation/observation_spec.py:128-173,
 * sorrel/entities/entity.py:9-68, sorrel/worlds/gridworld.py:36).  The step kernels are templates over exactly those
 * constants; sgw_create instantiates them for the engine's own world in-process (hipRTC; no compiler is spawned) -- EVERY
 * instance its plan counts on (whole turn, direct-store twin, rollout, walking variant, row kernels), so that a refusal of any of
 * them re-plans the whole engine for the prebuilt instances of the library (hipRTC absent, the library built without its embedded
 * sources, a compile error, a code object that does not load) instead of surfacing at a later call.  Code objects are kept on disk
 * (option "jit_cache_dir"; default <directory of libsgw.so>/jit_cache while that is the calling user's own directory, else
 * $XDG_CACHE_HOME/sgw_jit, $HOME/.cache/sgw_jit, /tmp/sgw_jit_cache_<uid>; mode 0700): a file is read only if it belongs to the
 * calling user, nobody else may write it, and its size and checksum are the ones its header states; the key names the compiler
 * (hipRTC version and library file), the architecture, the instance and the embedded source.
 *
 * sgw_set_option: every dispatcher knob is a (key, value) pair of strings; value NULL or "" restores the key's default, key
 * NULL restores all.  eng == NULL addresses the process-wide defaults that the NEXT sgw_create / sgw_plan copies; on a live
 * engine only the keys that do not shape its plan are accepted ("rows_mode", "act_lanes", "jit_verbose").  Keys (sorrel_amd/csrc/
 * options.h holds the table): jit, jit_cache, jit_cache_dir, jit_verbose, jit_own_rtc, jit_refuse (test hook), burst, pack3,
 * force_generic, fast_rules, rules_11k, fast_8k, force_big, group, phase_kernel, phase_rows, stage, stage_agents, fast_wg_per_cu,
 * big_threads, big_stage, big_wg_per_cu, big_walk, big_walk_blocks, big_walk_share, resolve_diag, rows_mode, act_lanes.  (Round 5
 * retired ten A/B hooks of closed experiments: static_radius, static_cleanup, rgb16, rules_8k, big_tag, stage_bytes, big_pad,
 * big_rot, big_walk_static, big_walk_stage -- an unknown key is SGW_EINVAL.)  No dispatcher knob is
 * an environment variable; the library reads SGW_DEBUG=1 (log lines of the specialiser on stderr), ROCM_PATH (which installation's
 * hipRTC: $ROCM_PATH/lib before /opt/rocm/lib) and, only to place the code-object cache, XDG_CACHE_HOME / HOME.
 *
 * sgw_plan: what sgw_create would decide for `cfg` on a device with `num_cus` compute units and `lds_per_workgroup` bytes of
 * LDS per workgroup -- kernel family, lanes per env, LDS layout, staging, the walk window, the instances to launch -- as pure
 * host arithmetic: no HIP call, no device needed (tests/test_plan.py enumerates it on the CPU).  It answers for a machine
 * where specialised instances are available unless option "jit" is 0. */
#define SGW_FAMILY_WAVE 1       /* step_fast: a wave per env (worlds <= 4 KiB; up to 11 KiB in large batches) */
#define SGW_FAMILY_WORKGROUP 2  /* step_big: a workgroup per env */
#define SGW_FAMILY_GENERIC 3    /* step_kernel: 16 / 32 lanes per env (small worlds of large batches), 64, or 256 (ticket-ordered) */
typedef struct sgw_plan_info {
    int32_t family;            /* SGW_FAMILY_* */
    int32_t lanes_per_env;     /* 16 / 32 / 64, or the workgroup size for a workgroup per env */
    int32_t threads;           /* per workgroup */
    int32_t grid_blocks;       /* workgroups of a whole-batch launch */
    int64_t lds_bytes;         /* dynamic LDS of the whole-turn kernel (before any occupancy cap) */
    int32_t env_lds;           /* ... of one env's slice */
    int32_t obs_stage;         /* bytes of window staging per wave (0: direct stores) */
    int32_t stage_agents;      /* agents per staged burst (0: the whole env at once, or no staging) */
    int32_t whole_env_burst;   /* the env's windows leave in ONE burst (compile-time shape) */
    int32_t big_stage;         /* step_big: bytes of window staging per wave */
    int32_t big_pitch;         /* step_big: LDS bytes between grid rows */
    int32_t onehot, rgb16, rules;
    int32_t specialised;       /* the plan counts on instances compiled for this engine */
    int32_t phase_kernel;      /* policy-driven phases of worlds above 4 KiB take the byte-gather phase kernel */
    int32_t rollout_in_one_launch;   /* sgw_rollout runs its turns inside one launch */
    int32_t walk_blocks;       /* step_big<..., WALK>: resident workgroups (0: not used) */
    int64_t walk_min_envs, walk_max_envs;   /* batches in (min, max] take the walking variant */
    int64_t big_stage_min_envs;             /* step_big stages its windows for batches above this */
    char kernel[192];              /* template-id of the whole-turn kernel (the specialised instance when `specialised`) */
    char kernel_prebuilt[192];     /* ... of the prebuilt instance used when the specialised one is unavailable ("-": none fits this plan) */
    char kernel_plain[192];        /* direct-store twin of a STAGE kernel (agent ranges, OBS_NEXT, unaligned tensors) */
    char kernel_rollout[192];      /* the instance with sgw_rollout's turn loop */
    char kernel_walk[192];
    char kernel_phase[96];         /* what a policy-driven phase (one agent) launches */
    char kernel_observe_rows[96];  /* sgw_observe_rows */
} sgw_plan_info;
int sgw_set_option(sgw_engine* eng, const char* key, const char* value);
int sgw_plan(const sgw_config* cfg, int32_t num_cus, int64_t lds_per_workgroup, sgw_plan_info* out);
/* ---- Row tails (round 4): what an agent's pov() appends to its flattened window, in-kernel ---------------------------------
 * TagAgent.pov appends whether the agent is "it" (sorrel/examples/tag/agents.py:57-65), CleanupObservation.observe the
 * positional code of the agent's cell (sorrel/examples/cleanup/agents.py:52-60, sorrel/observation/embedding.py:8-44).  With a
 * tail bound, sgw_observe_rows writes it right behind the window in every row (element C*V*V onwards; env_stride must be
 * >= C*V*V + tail_len) and sgw_act keeps it current (Tag: an agent tagged before its own pov reads 1), so the policy reads
 * the finished row and nothing is concatenated on the host.  SGW_TAIL_AGENT_IS_IT: one element, 1.0 where the agent's current
 * type is tag_it_type (needs sgw_bind_agent_state).  SGW_TAIL_POSITION_TABLE: tail_len elements table[(y*W + x)*tail_len ...]
 * of the agent's cell; `table` is a DEVICE pointer to float [H][W][tail_len] owned by the caller.  float32 rows only. */
#define SGW_TAIL_NONE 0
#define SGW_TAIL_AGENT_IS_IT 1
#define SGW_TAIL_POSITION_TABLE 2
int sgw_bind_row_tail(sgw_engine* eng, int kind, int tail_len, const float* table);

/* ---- A whole policy turn as ONE submission (round 4) ---------------------------------------------------------------
 * Agent.transition is pov -> get_action -> act, agent after agent (sorrel/agents/agent.py:155-173): 1 + A engine launches
 * with the policies' forward passes in between.  Three things change from turn to turn and used to arrive as kernel
 * arguments -- Environment.turn, the epoch, and the rows of the agents' replay rings (sorrel/buffers.py:46-63) -- so a turn
 * could not be recorded once and replayed.  They now live in device memory that the engine advances itself:
 *   sgw_turn_bind(rows)        (blocking, rare) the agents' replay rings: base pointers, capacity, the row the NEXT turn
 *                              fills, rows per turn (agents that share one Buffer advance it together); NULL: no replay rows.
 *                              Waits for everything submitted to the device so far (any stream), then writes the ring fields
 *                              only: epoch, turn and the exploration rates are never touched by it
 *   sgw_turn_set(epoch, turn)  (stream-ordered) the turns of the epoch completed so far: Environment.reset -> (epoch, 0)
 *   sgw_turn_begin(...)        sweep + EVERY agent's window into `obs` [E][A][C][V][V] for turn (completed + 1)
 *                              (= sgw_step(0, A, SGW_STEP_SWEEP | SGW_STEP_NO_MOVE) at the device's turn)
 *   sgw_turn_act(agent, ...)   = sgw_act with the windows in their slots of `obs` (the later agents' windows are repaired
 *                              there); reward and int64 action also go to the agent's ring row of the turn in flight
 *   sgw_turn_end(obs)          the windows of the turn -> each agent's ring row (what Agent.add_memory would copy), then
 *                              every ring advances and the turn counts as completed
 * Every call is asynchronous on `stream` and takes the same arguments every turn, so begin + A x (policy forward,
 * sgw_turn_act) + end can be captured in a hipGraph (torch.cuda.graph) and replayed without the host in the loop;
 * `obs` is the tensor the policies read -- a fixed address, which is what a recorded graph needs -- and the copy into the
 * ring rows is the price (one read + one write of the windows per turn).  sgw_turn_state reads the device's count back
 * (synchronising; tests and resynchronisation of the host's counters). */
typedef struct sgw_turn_rows {
    void* states[SGW_MAX_AGENTS];      /* device [capacity][E][row_elems], element type = sgw_set_obs_format's; NULL: windows not kept */
    float* rewards[SGW_MAX_AGENTS];    /* device [capacity][E]; may be NULL */
    int64_t* actions[SGW_MAX_AGENTS];  /* device [capacity][E]; may be NULL */
    float* dones[SGW_MAX_AGENTS];      /* device [capacity][E], zeroed for the turn's row; NULL when the ring's dones are all zero already */
    int64_t capacity[SGW_MAX_AGENTS];  /* rows of the ring; 0: this agent keeps no replay rows */
    int64_t row[SGW_MAX_AGENTS];       /* the row the next turn fills (Buffer.idx, + k for the k-th agent sharing the Buffer) */
    int64_t step[SGW_MAX_AGENTS];      /* rows the ring advances per turn (how many agents share the Buffer) */
    int64_t row_elems[SGW_MAX_AGENTS]; /* elements per env of a states row, >= C*V*V */
} sgw_turn_rows;
int sgw_turn_bind(sgw_engine* eng, const sgw_turn_rows* rows);
int sgw_turn_set(sgw_engine* eng, uint32_t epoch, uint32_t turn, void* stream);
int sgw_turn_begin(sgw_engine* eng, uint8_t* grid, uint8_t* agent_pos, uint8_t* actions, float* obs, float* rewards,
                   double* total_reward, uint32_t flags, void* stream);
int sgw_turn_act(sgw_engine* eng, uint8_t* grid, uint8_t* agent_pos, uint8_t* actions, void* obs, float* rewards,
                 double* total_reward, int32_t agent, const void* agent_action, int32_t action_kind, void* stream);
int sgw_turn_end(sgw_engine* eng, const void* obs, void* stream);
/* The same protocol with the windows in PER-AGENT rows (`rows[a]` + env * env_stride, as sgw_observe_rows / sgw_act take them; needs
 * SGW_CAP_OBSERVE_ROWS): sgw_turn_begin_rows = the sweep alone + every agent's window into its row AND -- by the device's row count --
 * into its replay row of the turn in flight; sgw_turn_act_rows repairs both copies; sgw_turn_end(eng, NULL, stream) then only
 * advances the rings.  No copy of the windows at the end of the turn (617 MB read + written at config 3's 65 536 envs), and each
 * policy reads a contiguous [E][C*V*V] row at a fixed address. */
int sgw_turn_begin_rows(sgw_engine* eng, uint8_t* grid, uint8_t* agent_pos, uint8_t* actions, float* rewards, double* total_reward,
                        void* const* rows, int64_t env_stride, uint32_t flags, void* stream);
int sgw_turn_act_rows(sgw_engine* eng, uint8_t* grid, uint8_t* agent_pos, uint8_t* actions, void* const* rows, int64_t env_stride,
                      float* rewards, double* total_reward, int32_t agent, const void* agent_action, int32_t action_kind, void* stream);
int sgw_turn_state(sgw_engine* eng, uint32_t* epoch_turn, int64_t* rows, void* stream);
/* ---- Speculative policy turns (round 5): many agents without A dependent (forward, act) pairs -----------------------------
 * Agent.transition runs agent after agent (sorrel/agents/agent.py:155-173): agent j's window shows the moves of the agents before
 * it.  A move changes two cells and a window is small, so for most (env, agent) pairs the action computed from the PRE-move window is
 * already the sequential one.  Protocol (needs SGW_CAP_RESOLVE):
 *   sgw_step(0, 0, SGW_STEP_SWEEP | SGW_STEP_NO_OBS)   the entity sweep alone
 *   sgw_observe_rows(rows, row_elems, 0, A)           every agent's pre-move window into `rows` [A][E][row_elems] float32
 *     (or sgw_turn_resolve(pass = 0))                  (rows[a] = rows + a * E * row_elems: agent-major, so agents that share a
 *                                                      model are ONE contiguous batch for its forward pass; pass 0 renders them for
 *                                                      ANY appearance table and window size, where there is no row kernel)
 *     (or, with SGW_CAP_OBS_AGENT_MAJOR, both in ONE launch: sgw_step(0, A, SGW_STEP_SWEEP | SGW_STEP_NO_MOVE | SGW_STEP_OBS_AGENT_MAJOR))
 *   fresh[A * E] <- policy(rows)                       one batched evaluation, int64 action indices in the rows' order
 *   sgw_turn_resolve(pass = 1, fresh, A * E)          writes the actions into actions[E][A], then resolves every env's moves in agent
 *             order WITHOUT touching the grid; renders, for each agent whose window an earlier mover touches, the window it really
 *             has when its turn comes; where that differs from its row the row is rewritten and the row's index (agent * E + env)
 *             appended to the pass's dirty list.  An env without a dirty agent has reached the fixed point: it is committed (movers'
 *             cells, agent_pos, rewards, the float64 total in agent order -- exactly what sgw_step with these actions would have
 *             written -- and, where given, reward / action once more in agent-major rows of a replay ring); later passes skip it.
 *   n <- counters[pass & 7]                            (the one thing the host reads back per pass)
 *   fresh[n] <- policy(rows[dirty_list[(pass & 1) * E * A + k]]), k < n;  sgw_turn_resolve(pass + 1, fresh, n);  until n == 0.
 * At most A passes (the first dirty agent of an env moves to a higher index every pass); measured three to four for 64 agents, with
 * a fifth of the rows re-evaluated in pass 2 and 0.3 % in pass 3 (profiles/r05_speculation_study.txt, r05_speculative_turn.txt).
 * With a policy that is a function of its window the result equals the sequential turn bit for bit.  Caller-owned scratch:
 * `scratch` 4 * E * A bytes (done flags, row states, the dirty bytes of the last pass at + 2 * E * A, previous moves), `dirty_list`
 * 2 * E * A int64, `counters` 8 uint32; their contents are initialised by pass 0 / 1.  (The list is appended with one atomic per env that has
 * dirty rows; from 8 192 envs on -- where that many atomics on one counter would serialise -- it is laid out by a scan over per-env counts,
 * two more small launches inside the call.)  `dirty_list` / `counters` may be NULL
 * (read the dirty bytes instead), and so may `new_actions` (the caller has written `actions` itself). */
int sgw_turn_resolve(sgw_engine* eng, uint8_t* grid, uint8_t* agent_pos, uint8_t* actions, float* rows, int64_t row_elems,
                     float* rewards, double* total_reward, uint8_t* scratch, int64_t* dirty_list, uint32_t* counters,
                     const int64_t* new_actions, int64_t n_new, float* reward_rows, int64_t* action_rows, int32_t pass, void* stream);
/* The resolve of a speculative turn for ANY agent rule (round 6; Tag, Cleanup, whatever rule comes next): play the current actions as ONE sequential turn on
 * a scratch copy of the state -- sgw_step with given actions, no sweep, observations on: its `obs` [E][A][C][V][V] are the windows the agents really have
 * when their turn comes (Agent.transition, sorrel/agents/agent.py:155-173), its state_at_pov Tag's "it" flags at pov time -- then sgw_verify_rows: row
 * (a, e) of `rows` [A][E][row_elems] (window + the bound row tail) that differs from that is rewritten from it and its index a * E + e appended to `list`
 * (*count = how many; zeroed by the call).  Evaluate the policy on those rows, sgw_apply_actions, play again -- until *count == 0: the scratch state then
 * IS the sequential turn's result (copy it over the state).  A positional tail (SGW_TAIL_POSITION_TABLE) is not compared: an agent's own cell does not
 * change before its own act.  Pays where the sequential loop is host-bound and the agents many (profiles/r06_speculation_study_rules.txt). */
int sgw_verify_rows(sgw_engine* eng, const float* obs, const uint8_t* state_at_pov, float* rows, int64_t row_elems, int64_t* list, uint32_t* count,
                    void* stream);
/* actions[e][a] = new_actions[k] for the k-th entry a * E + e of `list` (NULL: k itself), k < n; values outside [0, 255) become 255 (no ActionSpec has
 * it: SGW_STATUS_BAD_ACTION when played).  The dirty rows' fresh policy outputs into the [E][A] action tensor. */
int sgw_apply_actions(sgw_engine* eng, uint8_t* actions, const int64_t* list, const int64_t* new_actions, int64_t n, void* stream);
/* dst[k][:] = src[idx[k]][:] for k < n: rows of `row_elems` float32 (the dirty rows of a speculative pass as ONE contiguous batch for the
 * policy); src / dst 4-byte aligned device pointers, idx int64 on the device.  Asynchronous on `stream`; needs no engine. */
int sgw_gather_rows(const float* src, int64_t row_elems, const int64_t* idx, int64_t n, float* dst, void* stream);
/* Buffer.current_state (sorrel/buffers.py:143-154) for a recorded turn -- the frames a frame-stacking policy reads in front of its
 * window: the `count` rows of agent `agent`'s replay states BEFORE the row the turn in flight fills, oldest first, wrapping around
 * the ring, by the device's own row count -> out [count][E][row_elems] (device, element type = sgw_set_obs_format's).  Same
 * arguments every turn: recordable.  The ring must be bound with states (sgw_turn_bind); 1 <= count <= capacity. */
int sgw_turn_prev_rows(sgw_engine* eng, int32_t agent, int32_t count, void* out, void* stream);
/* The speculative turn's form of SGW_ACT_QF32 (a policy that returns action VALUES, sorrel/models/pytorch/iqn.py:294-309): for k < n,
 * out[k] = the action sgw_act(SGW_ACT_QF32) would take for agent a = row / E in env = row % E (row = idx[k]; idx NULL: row = k) from
 * values[k][0 .. num_actions): the first index of the maximum (NaN = maximum) or -- with probability epsilon[a] (sgw_turn_epsilon) -- the
 * engine's uniform draw for (env, `turn`, a) of `epoch`.  The draw is keyed, not consumed, so a window's action is a function of the
 * window and the fixed point of sgw_turn_resolve stays the sequential turn with exploration.  values float32 [n][num_actions], idx / out
 * int64 on the device; asynchronous on `stream`. */
int sgw_choose_actions(sgw_engine* eng, const float* values, const int64_t* idx, int64_t n, uint32_t epoch, uint32_t turn, int64_t* out,
                       void* stream);
/* Exploration rate of SGW_ACT_QF32 acts under the turn protocol: `agent` in [0, A) or -1 for every agent; epsilon in [0, 1].
 * Stream-ordered and kept in the device's turn state, so a recorded turn follows a decaying epsilon without being recorded again. */
int sgw_turn_epsilon(sgw_engine* eng, int32_t agent, double epsilon, void* stream);

/* ---- sprite frames (sorrel/utils/visualization.py:27-176: render_sprite + image_from_array, for a batch, on the device) ----
 * Every cell byte of `grid` names a tile of an RGBA atlas (type_tile); a frame is rows x cols tiles.  Composited frames paste the
 * layers bottom-up the way PIL's Image.paste(layer, (0, 0), mask=layer) does on RGBA images, for each of the four bytes:
 *     t = dst * (255 - a) + src * a + 128;   out = ((t >> 8) + t) >> 8        (a = the source pixel's alpha; layer 0 is taken as it is)
 * Needs no engine and knows no type cap: any byte value may be a type.  All pointers are device pointers. */
#define SGW_RENDER_COMPOSITE 0   /* out u8 [n]([k])[rows * th][cols * tw][4] */
#define SGW_RENDER_LAYERS 1      /* out u8 [n]([k])[L][rows * th][cols * tw][4]: what render_sprite returns, one plane per layer */
#define SGW_TILE_OPAQUE 1        /* tile_flags: every pixel of the tile has alpha 255 (what lies under it is not read) */
#define SGW_TILE_CLEAR 2         /* tile_flags: every pixel of the tile has alpha 0 (pasting it changes nothing) */
#define SGW_TILE_KEEP 0xFFFF     /* agent_tile: the agent shows the tile of the cell byte it stands on */
typedef struct sgw_render_desc {
    const uint8_t* grid;         /* [E][L][H][W] cell bytes; env e starts at grid + e * grid_env_stride */
    const uint8_t* atlas;        /* [n_tiles][th][tw][4] RGBA, 4-byte aligned (16-byte aligned for the 16-bytes-per-lane path) */
    const uint8_t* tile_flags;   /* [n_tiles] SGW_TILE_* computed by the caller from the atlas, or NULL (no shortcuts) */
    const uint16_t* type_tile;   /* [256] atlas tile of every cell byte (an entry >= n_tiles shows oob_tile) */
    const uint8_t* agent_pos;    /* [E][A][2] (y, x), or NULL: no agents */
    const uint16_t* agent_tile;  /* [E][A]: replaces the tile of the agent's cell in agent_layer; SGW_TILE_KEEP (or any value >= n_tiles) = keep */
    const int64_t* env_ids;      /* [n] envs to render, any order, repeats allowed; NULL = envs 0 .. E-1 (n is then E).  A frame whose
                                    id is outside [0, E) is left unwritten */
    const int16_t* centres;      /* [n][k][2] (y, x) or NULL: with it a frame is the (2 * vision + 1)^2 tiles around the centre, tiles
                                    outside the map show oob_tile; without it a frame is the whole map and k counts as 1 */
    uint8_t* out;                /* 4-byte aligned (16 for the 16-bytes-per-lane path) */
    int64_t num_envs, n, grid_env_stride;   /* grid_env_stride 0 = L * H * W */
    int32_t layers, height, width;          /* 1..8, 1..4096 each (1..256 with agents); one tile row holds at most 1024 columns
                                               and layers * columns <= 4096 */
    int32_t num_agents, agent_layer;
    int32_t n_tiles, th, tw;                /* 1..65535 tiles of th x tw pixels, 1..64 each */
    int32_t k, vision, oob_tile, mode;      /* mode: SGW_RENDER_COMPOSITE / SGW_RENDER_LAYERS */
} sgw_render_desc;
/* Asynchronous on `stream`.  Bad shapes: SGW_EINVAL with the reason in sgw_last_error(). */
int sgw_render(const sgw_render_desc* desc, void* stream);

/* ---- replay batches (sorrel/buffers.py:98-124: Buffer.sample, for a ring that holds every env, on the device) ----
 * One launch gathers n frame-stacked samples from a replay ring: for sample k with (t, e) = (start, env),
 *     out_states[k]      = rows t .. t + n_frames - 1 of env e, concatenated          (uint8 rows widen exactly: (float)byte)
 *     out_next_states[k] = rows t + 1 .. t + n_frames
 *     out_actions / out_rewards / out_dones [k] = the scalars of row t + n_frames - 1
 *     out_valid[k]       = 1 - (any dones[t .. t + n_frames - 2][e] != 0)
 * Row (t, e) of `states` starts at element t * state_turn_stride + e * state_env_stride; actions, rewards and dones share the two
 * scalar strides in the same way -- so a Buffer ([capacity][E][R]: strides E * R / R and E / 1), one agent of a TurnBuffer
 * ([capacity][E][A][R]: pointers offset by a * R and a, strides E * A * R / A * R and E * A / A) and every agent of one (num_envs =
 * E * A, strides E * A * R / R and E * A / 1) are all read where they lie.  Every source row is read once (n_frames + 1 rows per sample).
 * starts == envs == NULL: the call draws its indices from the engine's counter RNG, stream SGW_STREAM_SAMPLE.  With c = *draw_count
 * (or `draw` when draw_count is NULL), sample k takes u32 number 2k (start) and 2k + 1 (env) of
 *     Philox4x32-10(ctr = {index >> 2, c & 0xffffffff, c >> 32, SGW_STREAM_SAMPLE}, key = {seed lo, seed hi}),
 * start = (u * num_starts) >> 32, env = (u * num_envs) >> 32.  Draws are WITH replacement over (turn, env) pairs; the reference's
 * replace=False holds for its population of one env's turns, which a batch over many envs leaves behind.  A given draw_count is
 * incremented by one after the gather (same stream), so a recorded graph draws a fresh batch at every replay.
 * A GIVEN index outside [0, num_starts) / [0, num_envs) leaves that sample's outputs unwritten.  Needs no engine; all pointers are
 * device pointers. */
#define SGW_SAMPLE_F32 0         /* src_type: the ring's rows are float32 */
#define SGW_SAMPLE_U8 1          /* ... uint8 (the compact observation format) */
#define SGW_SAMPLE_ACT_I64 0     /* act_type: the ring's actions are int64 (Buffer) */
#define SGW_SAMPLE_ACT_U8 1      /* ... uint8 (TurnBuffer) */
typedef struct sgw_sample_desc {
    const void* states;          /* ring of observation rows, element type src_type */
    const void* actions;         /* act_type */
    const float* rewards;
    const float* dones;
    const int64_t* starts;       /* [n] first frame (ring row) of each sample, or NULL: draw */
    const int64_t* envs;         /* [n] env of each sample; NULL exactly when starts is */
    uint64_t* draw_count;        /* device counter [1] read by the draw and incremented after it, or NULL: `draw` is used */
    float* out_states;           /* [n][n_frames * row_elems] */
    float* out_next_states;      /* [n][n_frames * row_elems] */
    int64_t* out_actions;        /* [n] */
    float* out_rewards;          /* [n] */
    float* out_dones;            /* [n] */
    float* out_valid;            /* [n] */
    int64_t* out_index;          /* [n][2] = (start, env) used, or NULL */
    int64_t n, capacity, num_envs, num_starts, row_elems;     /* num_starts + n_frames <= capacity; num_starts, num_envs < 2^31; row_elems < 2^30 */
    int64_t state_turn_stride, state_env_stride;              /* in elements */
    int64_t scalar_turn_stride, scalar_env_stride;            /* in elements: actions, rewards, dones */
    uint64_t seed, draw;
    int32_t n_frames, src_type, act_type, reserved;           /* reserved: 0 */
} sgw_sample_desc;
/* Asynchronous on `stream`.  Bad arguments: SGW_EINVAL with the reason in sgw_last_error(), before anything is launched. */
int sgw_sample(const sgw_sample_desc* desc, void* stream);

/* ---- discounted returns (sorrel/models/pytorch/ppo.py:226-239: the head of PyTorchPPO.train_step, for every column of a ring) ----
 * One launch walks `count` ring rows backwards in time, a lane per column: with row(t) = (first + t) mod capacity, t = count-1 .. 0,
 *     d = 0 where dones[row(t)][c] != 0;   d = fl32(rewards[row(t)][c] + fl32((float)gamma * d));   out_returns[t][c] = d
 * -- float32 with the product and the sum rounded separately (no fused multiply-add): the reference's arithmetic, bit for bit.
 * Element (row, c) of rewards and of dones lies at row * turn_stride + c * col_stride, so a Buffer ([capacity][E]: strides E / 1),
 * every agent of a TurnBuffer ([capacity][E][A]: cols = E * A, strides E * A / 1) and one agent of it (pointers offset by a, cols = E,
 * strides E * A / A) are read where they lie.  out_returns is [count][cols], contiguous; row 0 is ring row `first`.
 * normalize: (x - mean) / (std + 1e-7) in float64 with the unbiased std, written to out_normalized ([count][cols], out_type):
 *   SGW_RETURNS_NORM_COLUMN  mean / std of each column's count values (the reference's normalisation, per world and agent), same launch
 *   SGW_RETURNS_NORM_ALL     one mean / std over all count * cols values: per-workgroup partial moments in `workspace`
 *                            (sgw_returns_workspace_bytes), merged in a fixed order by a second launch; results are reproducible
 * The float32 out_type is the float64 value rounded once.  One value (count == 1, or count * cols == 1) gives NaN, as the reference.
 * out_stats (or NULL) receives (mean, std) pairs: [cols][2] for NORM_COLUMN, [2] for NORM_ALL.  count == 0 launches nothing.
 * Needs no engine; all pointers are device pointers.  Asynchronous on `stream`; bad arguments: SGW_EINVAL with the reason in
 * sgw_last_error(), before anything is launched. */
#define SGW_RETURNS_NORM_NONE 0
#define SGW_RETURNS_NORM_COLUMN 1
#define SGW_RETURNS_NORM_ALL 2
#define SGW_RETURNS_OUT_F64 0    /* out_type: out_normalized is float64 */
#define SGW_RETURNS_OUT_F32 1    /* ... float32 */
typedef struct sgw_returns_desc {
    const float* rewards;
    const float* dones;          /* any non-zero value ends an episode */
    float* out_returns;          /* [count][cols] */
    void* out_normalized;        /* [count][cols] of out_type; NULL with SGW_RETURNS_NORM_NONE */
    double* out_stats;           /* (mean, std) pairs, or NULL */
    void* workspace;             /* SGW_RETURNS_NORM_ALL: sgw_returns_workspace_bytes(count, cols) bytes, 8-byte aligned */
    int64_t workspace_bytes;
    int64_t first, count, capacity, cols;     /* 0 <= first < capacity; 0 <= count <= capacity; 1 <= cols < 2^31 */
    int64_t turn_stride, col_stride;          /* in elements, >= 1: rewards and dones share them */
    double gamma;                /* rounded to float32 by a C cast */
    int32_t normalize, out_type, reserved0, reserved1;        /* reserved: 0 */
} sgw_returns_desc;
int sgw_returns(const sgw_returns_desc* desc, void* stream);
/* Bytes of workspace SGW_RETURNS_NORM_ALL needs for this shape (0 for no turns); a negative code for a shape sgw_returns rejects. */
int64_t sgw_returns_workspace_bytes(int64_t count, int64_t cols);

/* ---- stochastic policies (sorrel/models/pytorch/ppo.py:121-137: ActorCritic.act -- Categorical(probs).sample() and .log_prob() --
 * and :139-152, evaluate's .entropy(); for a batch of distributions, on the device) ----
 * One launch turns n rows of num_actions numbers into an action, its log-probability and the row's entropy.  1 <= num_actions <= 256
 * (beyond SGW_MAX_ACTIONS: the call needs no engine).  The numbers are float32 or float64 (dist_type), probabilities or logits (mode).
 * All arithmetic is float64, sequential in index order: no re-association, and no fused multiply-add where one would change a result.
 *   weights    SGW_POLICY_PROBS:   w_i = (double)x_i -- unnormalised, as Categorical(probs=...) accepts them
 *              SGW_POLICY_LOGITS:  w_i = exp((double)x_i - max_j x_j); -inf gives 0
 *              S = ((w_0 + w_1) + ...)
 *   invalid    a row is invalid if any w_i is negative or NaN, if S is 0 or not finite, or if the maximum logit is NaN or +inf (torch
 *              raises for such a row): it gets action 255, which no ActionSpec has (SGW_STATUS_BAD_ACTION if played), and NaN for its
 *              log-probability and entropy.  So does a row whose `idx` entry names no (env, agent) pair: idx[k] < 0 or
 *              idx[k] / num_envs >= SGW_MAX_AGENTS.  Other rows are untouched by it.
 *   draw       u = Philox4x32-10(ctr = {agent >> 2, turn, first_env + env, epoch << 4 | SGW_STREAM_POLICY}, key = {seed lo, seed hi})[agent & 3]
 *              -- the layout of SGW_STREAM_EXPLORE; `turn` is the turn in flight, as for the exploration draw.  The draw is keyed, not
 *              consumed: a row's action is a function of (its numbers, seed, env, epoch, turn, agent).
 *   action     t = ((double)u + 0.5) * 2^-32 * S; the action is the first i with c_i > t, where c_i = c_(i-1) + w_i is the running sum in
 *              the same order.  A zero-weight action can never be chosen; t < S always holds, so a valid row always finds one.
 *   log-prob,  torch's Categorical, its clamp included: q_i = w_i / S; l_i = log(min(max(q_i, 2^-52), 1 - 2^-52));
 *   entropy    log_prob = (float)l_action; entropy = (float)(-((q_0 * l_0 + q_1 * l_1) + ...)), every product rounded before it is added.
 *              The float32 value is the float64 value rounded once: what the reference's log_probs[idx] = log_prob stores.
 * Row k starts at element k * row_stride of `dist` and is keyed as (env, agent) = (idx[k] % num_envs, idx[k] / num_envs), or with
 * idx == NULL as (k % num_envs, agent0 + k / num_envs): one agent's [E] rows and a shared model's agent-major [A * E] rows alike (the row
 * numbering of sgw_choose_actions); idx may repeat and reorder.  out_log_probs / out_entropy may be NULL (nothing is computed for them).
 * Needs no engine; all pointers are device pointers.  Asynchronous on `stream`; everything the host can see -- NULL dist or out_actions,
 * n < 0, num_actions outside 1..256, num_envs < 1, row_stride < num_actions, an agent key outside [0, SGW_MAX_AGENTS) with idx == NULL,
 * epoch >= 2^28, an unknown dist_type or mode, a misaligned pointer, n * row_stride beyond 64-bit offsets, a non-zero reserved field -- is
 * SGW_EINVAL with the reason in sgw_last_error(), before anything is launched.  n == 0 launches nothing. */
#define SGW_POLICY_F32 0         /* dist_type: the rows are float32 */
#define SGW_POLICY_F64 1         /* ... float64 */
#define SGW_POLICY_PROBS 0       /* mode: unnormalised probabilities */
#define SGW_POLICY_LOGITS 1      /* ... logits */
#define SGW_POLICY_MAX_ACTIONS 256
typedef struct sgw_policy_desc {
    const void* dist;            /* [n] rows of num_actions elements of dist_type, row_stride elements apart */
    const int64_t* idx;          /* [n] row keys agent * num_envs + env, or NULL */
    int64_t* out_actions;        /* [n] */
    float* out_log_probs;        /* [n], or NULL */
    float* out_entropy;          /* [n], or NULL */
    int64_t n, num_envs, row_stride;
    uint64_t seed, first_env;    /* first_env: the global id of env 0 (sgw_config.first_env_id); its low 32 bits enter the counter */
    uint32_t epoch, turn;
    int32_t num_actions, agent0, dist_type, mode;
    int32_t reserved0, reserved1;    /* reserved: 0 */
} sgw_policy_desc;
int sgw_policy_sample(const sgw_policy_desc* desc, void* stream);
/* The same kernel under the turn protocol (sgw_turn_*): agent `agent`'s [E][num_actions] rows (contiguous; num_actions = the engine's) are
 * sampled with the engine's seed and first_env_id, and with epoch and the turn in flight (= completed + 1) read from the device's turn
 * state, as sgw_turn_act reads them.  log_prob_ring is the base of a float32 [capacity][E] ring (capacity = the agent's bound ring's) or
 * NULL: the kernel writes row ts->row[agent] of it -- the row the turn in flight fills.  out_actions int64 [E] (what sgw_turn_act takes as
 * SGW_ACT_I64), out_entropy float32 [E] or NULL.  Same arguments every turn: recordable.  SGW_EINVAL when a ring is given and the agent
 * has no bound replay rows (sgw_turn_bind). */
int sgw_turn_policy_sample(sgw_engine* eng, int32_t agent, const void* dist, int32_t dist_type, int32_t mode, int64_t* out_actions,
                           float* log_prob_ring, float* out_entropy, void* stream);

/* ---- PPO's clipped loss and its gradients (sorrel/models/pytorch/ppo.py:259-285: the body of train_step's k_epochs loop between
 * policy.evaluate's network outputs and optimizer.step -- Categorical(probs), log_prob, entropy, the ratio, the two surrogates, the
 * MSE, loss.mean() and what autograd hands back at the actor's and the critic's outputs; on the device) ----
 * One launch reads each of n rows once and writes the loss terms' partial sums and BOTH gradients; a second, small launch merges the
 * partial sums in a fixed order.  No floating-point atomics: two runs give the same bits.  Row k has num_actions (1..256) numbers x
 * (float32 or float64: dist_type; probabilities or logits: mode), a value v (value_type), an action a (action_type), the stored
 * log-probability `old` (float32, what sgw_policy_sample wrote) and a return R (returns_type).  All arithmetic is float64, sequential in
 * index order, every product rounded before it is added (no fused multiply-add).
 *   distribution  sgw_policy_sample's, in both modes: w_i = x_i, or exp(x_i - max x) for logits; S = ((w_0 + w_1) + ...); q_i = w_i / S;
 *                 l_i = log(min(max(q_i, 2^-52), 1 - 2^-52)); u_i = 1 if 2^-52 <= q_i <= 1 - 2^-52, else 0; lp = l_a;
 *                 H = -((q_0 l_0 + q_1 l_1) + ...).  With unchanged parameters lp reproduces the stored log-probability: the ratio is 1.
 *   invalid       a row that is invalid for sgw_policy_sample (a negative or NaN weight, S zero or not finite, a NaN or +inf maximum
 *                 logit) or whose action is outside [0, num_actions): every per-row output of that row is NaN, and so are the means.
 *                 Other rows are untouched by it.
 *   loss          r = exp(lp - old); A = R - v; lo = 1 - eps_clip, hi = 1 + eps_clip (computed on the host, in double); s1 = r A;
 *                 s2 = min(max(r, lo), hi) A; P = -min(s1, s2); d = v - R.  Pm, M and Hm are the means over n of P, d^2 and H;
 *                 L = Pm + value_coef M - entropy_coef Hm.  The reference's loss.mean() is this with value_coef = 0.5 (its scalar MSE is
 *                 broadcast over the rows).
 *   dL/dr         torch's rule, ties included: s1 < s2: gr = A;  s1 > s2: gr = A if lo <= r <= hi, else 0;
 *                 s1 == s2: gr = A / 2 + (A / 2 if lo <= r <= hi, else 0).  No gradient flows through A (the reference detaches it).
 *   dL/dx         with c = entropy_coef: gl_i = c q_i, at i = a plus -(gr r); gq_i = (u_i ? gl_i / q_i : 0) + c l_i;
 *                 t = ((gq_0 q_0 + gq_1 q_1) + ...);  probabilities: dL/dx_j = ((gq_j - t) / S) / n;  logits: dL/dx_j = (q_j (gq_j - t)) / n.
 *   dL/dv         ((2 value_coef) (v - R)) / n.
 * float32 outputs are the float64 value rounded once.  out_grad_dist has the type and the row stride of dist (what lies between rows is
 * not written), out_grad_values the type of values; both and out_row_terms are optional (NULL).  The gradients depend on n alone, not on
 * the sums: they are final after the first launch.  workspace: sgw_ppo_loss_workspace_bytes(n) bytes, 8-byte aligned, overwritten.
 * Needs no engine; all pointers are device pointers.  Asynchronous on `stream`; everything the host can see -- a NULL required pointer,
 * an unknown dist_type / mode / value_type / action_type / returns_type, n < 0, num_actions outside 1..256, row_stride < num_actions, a
 * negative or non-finite eps_clip, a pointer not aligned to its element type, a workspace that is too small, a non-zero reserved field,
 * n * row_stride beyond 64-bit offsets -- is SGW_EINVAL with the reason in sgw_last_error(), before anything is launched.  n == 0
 * launches nothing and writes nothing. */
#define SGW_PPO_ACT_I64 0        /* action_type: int64 actions (a Buffer's) */
#define SGW_PPO_ACT_U8 1         /* ... uint8 (a TurnBuffer's) */
typedef struct sgw_ppo_loss_desc {
    const void* dist;            /* [n] rows of num_actions elements of dist_type (SGW_POLICY_F32 / _F64), row_stride elements apart */
    const void* values;          /* [n] of value_type (SGW_POLICY_F32 / _F64) */
    const void* actions;         /* [n] of action_type */
    const float* old_log_probs;  /* [n] */
    const void* returns;         /* [n] of returns_type (SGW_POLICY_F32 / _F64) */
    void* out_grad_dist;         /* dL/dx, laid out as dist, or NULL */
    void* out_grad_values;       /* dL/dv [n] of value_type, or NULL */
    double* out_row_terms;       /* [n][3] = (P, d^2, H) of every row, or NULL */
    double* out_terms;           /* [4] = L, Pm, M, Hm */
    void* workspace;
    int64_t workspace_bytes;
    int64_t n, row_stride;
    double eps_clip, entropy_coef, value_coef;
    int32_t num_actions, dist_type, mode, value_type, action_type, returns_type;
    int32_t reserved0, reserved1;    /* reserved: 0 */
} sgw_ppo_loss_desc;
int sgw_ppo_loss(const sgw_ppo_loss_desc* desc, void* stream);
/* Bytes of workspace a call over n rows needs (0 for no rows); a negative code for n < 0. */
int64_t sgw_ppo_loss_workspace_bytes(int64_t n);

/* ---- IQN's quantile Huber loss and its gradient (sorrel/models/pytorch/iqn.py:359-405 and calculate_huber_loss, :451-464: the body of
 * iRainbowModel.train_step between the three network outputs and loss.backward() -- the double-DQN action choice, the two gathers, the
 * n-step target, the [B][N][N] pairwise TD tensor, the Huber `where`, the `valid` mask, the quantile weights, the mean, and what autograd
 * hands back at the local net's output; on the device) ----
 * One launch reads every row once and writes the gradient and per-workgroup sums; a second, small launch merges the sums in a fixed
 * order.  No floating-point atomics: two runs give the same bits.  Batch row b of n has num_quantiles = N (1..64) quantiles of
 * num_actions = A (1..256) actions in each of three contiguous float32 [n][N][A] tensors: q_next_local (the local net on the next
 * states: it only chooses the action), q_next_target (the target net on the next states) and q_expected (the local net on the states:
 * the only tensor with a gradient); taus float32 [n][N] (the taus of the q_expected call); an action (action_type), a reward and a done
 * flag (float32) and a row weight `valid` (valid_type; any weight, not only 0 / 1).  discount = GAMMA ** n_step, computed by the caller.
 * float32 arithmetic is torch's on the CPU, every product rounded before it is added (no fused multiply-add).
 *   action      m_a = (((q_next_local[b][0][a] + q_next_local[b][1][a]) + ...)) / (float)N, summed serially over the quantiles in float32;
 *               a* = the first maximum of m, a NaN counting as a maximum (SGW_ACT_QF32's rule)
 *   target      T_j = rewards_b + (((float)discount * q_next_target[b][j][a*]) * (1.0f - dones_b));  X_i = q_expected[b][i][actions_b];
 *               td_ij = T_j - X_i  (the target's index is the LAST axis; tau_i belongs to X_i)
 *   Huber       kappa = 1:  h_ij = |td_ij| <= 1 ? 0.5f * (td_ij * td_ij) : |td_ij| - 0.5f;  w_ij = |tau_i - (td_ij < 0 ? 1.0f : 0.0f)|
 *   loss        float64 from here on (where the reference's float64 `valid` promotes it): ql_ij = (double)w_ij * ((double)h_ij *
 *               (double)valid_b);  S_b = the serial sum of ql_ij over j for each i, then of those N sums over i, in index order;
 *               L = (the sum of S_b over b) / (n N N).  The S_b are added in an order that depends on indices alone.
 *   gradient    g_ij = (float)(((1.0 / (n N N)) * (double)w_ij) * (double)valid_b);  e_ij = |td_ij| <= 1 ? g_ij * td_ij : g_ij * s_ij
 *               with s_ij = (td_ij > 0) - (td_ij < 0), in float32;  dL/dq_expected[b][i][actions_b] = (float)(-(the serial float64 sum
 *               over j of (double)e_ij)).  Every other element of row b is an exact +0: the WHOLE [n][N][A] gradient is written, no
 *               memset precedes the call.  Nothing flows to q_next_local, q_next_target or taus.
 *   invalid     a row whose action is outside [0, A): X_i is NaN, so its td_error is NaN; S_b and its whole gradient row are NaN, and
 *               so is L.  Its a* and every other row are untouched by it.  Non-finite inputs give what IEEE arithmetic gives.
 * out_grad_expected, out_next_actions, out_row_terms and out_td_error are optional (NULL).  workspace:
 * sgw_iqn_loss_workspace_bytes(n, num_quantiles) bytes, 8-byte aligned, overwritten.  Needs no engine; all pointers are device pointers.
 * Asynchronous on `stream`; everything the host can see -- a NULL required pointer, an unknown action_type / valid_type, n < 0,
 * num_quantiles outside 1..64, num_actions outside 1..256, a discount that is not finite, a pointer not aligned to its element type, a
 * missing or short workspace, a non-zero reserved field, n * N * max(A, N) beyond 64-bit offsets -- is SGW_EINVAL with the reason in
 * sgw_last_error(), before anything is launched.  n == 0 launches nothing and writes nothing. */
#define SGW_IQN_MAX_QUANTILES 64
typedef struct sgw_iqn_loss_desc {
    const float* q_next_local;   /* [n][N][A] */
    const float* q_next_target;  /* [n][N][A] */
    const float* q_expected;     /* [n][N][A] */
    const float* taus;           /* [n][N] */
    const void* actions;         /* [n] of action_type (SGW_PPO_ACT_I64 / _U8) */
    const float* rewards;        /* [n] */
    const float* dones;          /* [n] */
    const void* valid;           /* [n] of valid_type (SGW_POLICY_F32 / _F64) */
    double* out_terms;           /* [1] = L */
    float* out_grad_expected;    /* dL/dq_expected [n][N][A], or NULL */
    int64_t* out_next_actions;   /* [n] = a*, or NULL */
    double* out_row_terms;       /* [n] = S_b, or NULL */
    float* out_td_error;         /* [n][N][N] = td_ij, or NULL */
    void* workspace;
    int64_t workspace_bytes;
    int64_t n;
    double discount;
    int32_t num_quantiles, num_actions, action_type, valid_type;
    int32_t reserved0, reserved1;    /* reserved: 0 */
} sgw_iqn_loss_desc;
int sgw_iqn_loss(const sgw_iqn_loss_desc* desc, void* stream);
/* Bytes of workspace a call over n rows of num_quantiles quantiles needs (0 for no rows); a negative code for n < 0 or num_quantiles
 * outside 1..64. */
int64_t sgw_iqn_loss_workspace_bytes(int64_t n, int32_t num_quantiles);

/* ---- Adam, gradient clipping and the soft update (sorrel/models/pytorch/iqn.py:405-410: clip_grad_norm_(local.parameters(), 1),
 * optimizer.step(), soft_update(); ppo.py:283-285: Adam over two parameter groups in float64 -- what the reference runs after
 * loss.backward(), some eighty small launches on device tensors; on the device in two launches, one when nothing is clipped) ----
 * One call handles num_tensors = T (1..4096) tensors of ONE dtype (SGW_POLICY_F32 / _F64).  Tensor k has a record: param, grad (NULL:
 * the tensor is skipped entirely, as torch skips p.grad is None), exp_avg = m, exp_avg_sq = v, target (NULL: no soft update), numel and
 * a learning rate of its own (so PPO's two groups are one call).  beta1, beta2, eps and tau are call-wide.  No weight decay, amsgrad or
 * maximize.  Arithmetic is done in the tensors' dtype, written F(x) for a double rounded to it; every operation is rounded on its own
 * except the two marked fma, which are single fused multiply-adds -- the order that reproduces torch.optim.Adam(foreach=False) on the CPU.
 *   bias       by value (step >= 1, step_state NULL), in double, torch's _single_tensor_adam for a Python-float step:
 *                  bc1 = 1 - pow(beta1, (double)step);   bc2 = 1 - pow(beta2, (double)step);
 *                  step_size = lr / bc1;                 (per tensor)
 *                  bc2_sqrt = pow(bc2, 0.5);             (torch writes bias_correction2 ** 0.5: libm's pow, not sqrt)
 *              from the device (step_state given, step == 0): the first launch's block 0 advances the state, step += 1,
 *              beta1_pow *= beta1, beta2_pow *= beta2 in double -- RUNNING PRODUCTS, not pow --; the second launch reads it:
 *              bc1 = 1 - beta1_pow; bc2 = 1 - beta2_pow; step_size = lr / bc1; bc2_sqrt = sqrt(bc2).  A fresh state is {0, 1.0, 1.0}.
 *   clip       SGW_ADAM_CLIP_NONE: g = grad.
 *              SGW_ADAM_CLIP_NORM: a chunk is SGW_ADAM_CHUNK = 4096 consecutive elements of one tensor (the last one shorter).  Lane t
 *              of 256 owns the elements 4 (t + 256 r) + e of its chunk, r = 0..3, e = 0..3, and adds (double)grad * (double)grad of
 *              those that exist serially in that order; the 256 sums are merged by the halving tree (slot t += slot t + s,
 *              s = 128 .. 1): S_chunk.  A tensor's chunks are added serially in chunk order: S_k (0 for a skipped or empty tensor).
 *              Lane i adds S_i, S_(i + 256), ... serially and the same tree merges the lanes: S.  norm = sqrt(S) in double;
 *              c = F(max_norm) / (F(norm) + F(1e-6)); c > 1 ? 1 : c (a NaN stays a NaN and propagates, as torch's does).
 *              No atomics: the order depends on indices alone, two runs give the same bits.
 *              SGW_ADAM_CLIP_COEF: c is read from clip_coef, a device scalar of the tensors' dtype (after an all-reduce, say).
 *              In both: g = grad * c, always multiplied, as clip_grad_norm_ does.
 *   moments    m' = fma(F(1 - beta1), g - m, m)                     (fma; torch's lerp_ for a weight below 0.5: 1 - beta1 >= 0.5 is refused)
 *              v' = fma(F(1 - beta2) * g, g, v * F(beta2))          (fma)
 *   param      denom = F(sqrt(v') / F(bc2_sqrt)) + F(eps);   p' = p + (F(-step_size) * m') / denom
 *   target     t' = F(tau) * p' + F(1.0 - tau) * t                  (three roundings; only where a target is given)
 * grad is read only, unless SGW_ADAM_ZERO_GRADS is set: then +0 is stored after the read.  The clipped gradient is NOT written back
 * (after the reference's lines p.grad holds it).  out_norm, if given, receives {norm, c}: norm is NaN unless SGW_ADAM_CLIP_NORM, c is 1
 * for SGW_ADAM_CLIP_NONE.  A tensor of numel 0 is legal and untouched.  Tensors must not overlap.
 * The tensor table lies in device memory so that a call can be recorded; planning and stepping are therefore two calls.
 * sgw_adam_plan validates T records on the host and writes the host image of the table: T device records and the chunk map.  The caller
 * copies info->image_bytes bytes of it to the device (8-byte aligned) and passes that, info->num_chunks and a workspace of
 * info->workspace_bytes bytes (8-byte aligned; read and written by SGW_ADAM_CLIP_NORM only) to sgw_adam_step.  Needs no engine;
 * asynchronous on `stream`; no host synchronisation.  Everything the host can see -- a NULL required pointer (records, host_image, info;
 * param always, exp_avg and exp_avg_sq where grad is given; plan; clip_coef for SGW_ADAM_CLIP_COEF), a pointer not aligned to its element
 * type, numel < 0, T outside 1..4096, 2^31 chunks or more, a beta outside [0, 1), 1 - beta1 >= 0.5, a non-finite lr, max_norm, beta, eps
 * or tau, step < 1 without a step_state or != 0 with one, a short image, plan or workspace, an unknown dtype, clip_mode or flag, a
 * non-zero reserved field -- is SGW_EINVAL with the reason in sgw_last_error(), before anything is launched. */
#define SGW_ADAM_CLIP_NONE 0
#define SGW_ADAM_CLIP_NORM 1
#define SGW_ADAM_CLIP_COEF 2
#define SGW_ADAM_ZERO_GRADS 1    /* flags: store +0 to every gradient after reading it */
#define SGW_ADAM_MAX_TENSORS 4096
#define SGW_ADAM_CHUNK 4096
typedef struct sgw_adam_tensor {
    void* param;
    void* grad;                  /* NULL: skipped entirely */
    void* exp_avg;
    void* exp_avg_sq;
    void* target;                /* NULL: no soft update */
    int64_t numel;
    double lr;
    int64_t reserved;            /* reserved: 0 */
} sgw_adam_tensor;
typedef struct sgw_adam_plan_info {
    int64_t num_chunks, workspace_bytes, image_bytes, total_numel;     /* total_numel: of the tensors that are not skipped */
} sgw_adam_plan_info;
typedef struct sgw_adam_step_state {
    int64_t step;
    double beta1_pow, beta2_pow;
} sgw_adam_step_state;
typedef struct sgw_adam_step_desc {
    const void* plan;            /* the uploaded image of sgw_adam_plan */
    int64_t plan_bytes;
    const void* clip_coef;       /* SGW_ADAM_CLIP_COEF: one element of dtype */
    sgw_adam_step_state* step_state;     /* device; or NULL: `step` counts */
    double* out_norm;            /* [2] = norm, c; or NULL */
    void* workspace;
    int64_t workspace_bytes;
    int64_t num_tensors, num_chunks;
    int64_t step;
    double max_norm, beta1, beta2, eps, tau;
    int32_t dtype, clip_mode, flags;
    int32_t reserved0, reserved1;        /* reserved: 0 */
} sgw_adam_step_desc;
/* Bytes that hold the image of any T tensors of total_numel elements in all (an upper bound); a negative code for T outside 1..4096 or
 * total_numel < 0. */
int64_t sgw_adam_plan_bytes(int64_t num_tensors, int64_t total_numel);
int sgw_adam_plan(const sgw_adam_tensor* records, int64_t num_tensors, int32_t dtype, void* host_image, int64_t image_bytes, sgw_adam_plan_info* info);
int sgw_adam_step(const sgw_adam_step_desc* desc, void* stream);

/* ---- IQN's network forward (sorrel/models/pytorch/iqn.py:110-167: IQN.forward and get_qvalues, with layers.py's NoisyLinear -- the
 * head layer, the cosine embedding of every quantile, their product, the noisy layer, the dueling head and the mean over the
 * quantiles; a dozen torch launches whose [n N][L] intermediates pass through memory; on the device in two launches) ----
 * Row b of n has in_features = D state elements (float32 or uint8: state_type; uint8 is widened exactly), rows state_stride elements
 * apart.  layer_size = L (1..256), num_quantiles = N (1..64), num_actions = A (1..64), n_cos = 64.  The ten weight tensors are
 * contiguous float32 in nn.Linear's [out][in] layout: w_head[L][D], b_head[L], w_cos[L][64], b_cos[L], w_ff[L][L], b_ff[L],
 * w_adv[A][L], b_adv[A], w_val[L], b_val[1].  They are the EFFECTIVE weights: a noisy layer in training mode is weight + sigma * epsilon,
 * formed by the caller; the call knows nothing about noise.  No gradient: this is the forward of acting and of the two next_states calls.
 * All arithmetic is float32.  chain_k(x_k, w_k; b) is ONE fused multiply-add chain over k ascending that starts at the bias,
 * fmaf(x_K-1, w_K-1, ... fmaf(x_1, w_1, fmaf(x_0, w_0, b))) -- no split sums -- so a row's result depends on nothing but the row:
 * not on the batch, on the tile the row lands in, or on the grid.  relu(x) = x > 0 ? x : (x != x ? x : +0): a NaN goes through.
 *   taus       given (taus != NULL: float32 [n][N]), or drawn: row k is keyed as (env, agent) = (idx[k] % num_envs, idx[k] / num_envs), or
 *              with idx == NULL as (k % num_envs, agent0 + k / num_envs) -- sgw_policy_sample's keys --;
 *              u = Philox4x32-10(ctr = {(agent << 4) | (q >> 2), turn, first_env + env, epoch << 4 | SGW_STREAM_TAU},
 *              key = {seed lo, seed hi})[q & 3];  tau_q = (float)(u >> 8) * 2^-24, in [0, 1).  Keyed, not consumed: a function of
 *              (seed, env, epoch, turn, agent, quantile) alone.  A row whose idx entry names no (env, agent) pair gets NaN taus.
 *   head       h_l = relu(chain_k(x_k, w_head[l][k]; b_head[l]))
 *   embedding  arg_qi = tau_q * (float)(M_PI * i), i = 1..64: the constant is the double product rounded once (torch.FloatTensor([np.pi * i])),
 *              the product is float32;  c_qi = cosf(arg_qi), the device library's full-precision cosf;
 *              e_ql = relu(chain_i(c_qi, w_cos[l][i - 1]; b_cos[l]))
 *   product    z_ql = h_l * e_ql, rounded
 *   noisy      y_ql = relu(chain_k(z_qk, w_ff[l][k]; b_ff[l]))
 *   dueling    adv_qa = chain_k(y_qk, w_adv[a][k]; b_adv[a]);  val_q = chain_k(y_qk, w_val[k]; b_val[0]);
 *              mean_q = (((adv_q0 + adv_q1) + ...)) / (float)A, summed serially;  quant_qa = (val_q + adv_qa) - mean_q
 *   qvalues    qvalue_a = (((quant_0a + quant_1a) + ...)) / (float)N, summed serially: sgw_iqn_loss's m_a, and what SGW_ACT_QF32 and
 *              sgw_choose_actions take (argmax and exploration stay theirs)
 * Outputs, all contiguous float32 and each optional (NULL), but one of out_qvalues and out_quantiles must be given: out_qvalues [n][A],
 * out_quantiles [n][N][A], out_taus [n][N], out_cos [n][N][64] (c_qi: everything behind the one library call can be restated from it
 * bit for bit).  workspace: sgw_iqn_forward_workspace_bytes(n, layer_size) bytes, 4-byte aligned, overwritten: h [n][L] between the
 * head launch (rows as the GEMM's M, K = D) and the quantile launch (M = n N).  Nothing of size n N L reaches memory.  No atomics: two
 * runs give the same bits.  Needs no engine; all pointers are device pointers.  Asynchronous on `stream`; everything the host can
 * see -- a NULL required pointer, neither out_qvalues nor out_quantiles, an unknown state_type, n < 0, in_features < 1, layer_size
 * outside 1..256, num_quantiles outside 1..64, num_actions outside 1..64, n_cos != 64, state_stride < in_features, num_envs < 1 or an
 * agent key outside [0, SGW_MAX_AGENTS) (idx == NULL) or epoch >= 2^28 where taus are drawn, a misaligned pointer, a missing or short
 * workspace, a non-zero reserved field, offsets beyond 64 bits -- is SGW_EINVAL with the reason in sgw_last_error(), before anything is
 * launched.  n == 0 launches nothing and writes nothing. */
#define SGW_STREAM_TAU 11u           /* (unsigned) index = (agent << 4) | (quantile >> 2), word quantile & 3, turn = the turn in flight: sgw_iqn_forward's taus */
#define SGW_IQN_STATE_F32 0          /* state_type: the states are float32 */
#define SGW_IQN_STATE_U8 1           /* ... uint8 (a TurnBuffer's) */
#define SGW_IQN_MAX_LAYER 256
#define SGW_IQN_MAX_ACTIONS 64       /* of sgw_iqn_forward (sgw_iqn_loss takes 256) */
#define SGW_IQN_N_COS 64
typedef struct sgw_iqn_forward_desc {
    const void* states;          /* [n] rows of in_features elements of state_type, state_stride elements apart */
    const float* w_head;         /* [L][D] */
    const float* b_head;         /* [L] */
    const float* w_cos;          /* [L][64] */
    const float* b_cos;          /* [L] */
    const float* w_ff;           /* [L][L] */
    const float* b_ff;           /* [L] */
    const float* w_adv;          /* [A][L] */
    const float* b_adv;          /* [A] */
    const float* w_val;          /* [L] */
    const float* b_val;          /* [1] */
    const float* taus;           /* [n][N], or NULL: drawn */
    const int64_t* idx;          /* [n] row keys agent * num_envs + env of the drawn taus, or NULL */
    float* out_qvalues;          /* [n][A], or NULL */
    float* out_quantiles;        /* [n][N][A], or NULL */
    float* out_taus;             /* [n][N], or NULL */
    float* out_cos;              /* [n][N][64], or NULL */
    void* workspace;
    int64_t workspace_bytes;
    int64_t n, state_stride, num_envs;
    uint64_t seed, first_env;    /* as in sgw_policy_desc */
    uint32_t epoch, turn;
    int32_t in_features, layer_size, num_quantiles, num_actions, n_cos, state_type, agent0;
    int32_t reserved0, reserved1;    /* reserved: 0 */
} sgw_iqn_forward_desc;
int sgw_iqn_forward(const sgw_iqn_forward_desc* desc, void* stream);
/* Bytes of workspace a call over n rows needs (0 for no rows); a negative code for n < 0 or layer_size outside 1..256. */
int64_t sgw_iqn_forward_workspace_bytes(int64_t n, int32_t layer_size);
/* The same two launches under the turn protocol (sgw_turn_*): seed and first_env come from the engine, num_envs = the engine's, agent0 =
 * `agent`, idx must be NULL; epoch and the turn in flight (= completed + 1) are read from the device's turn state, as
 * sgw_turn_policy_sample reads them (desc's seed, first_env, num_envs, agent0, epoch and turn are ignored).  Same arguments every turn:
 * recordable. */
int sgw_turn_iqn_forward(sgw_engine* eng, int32_t agent, const sgw_iqn_forward_desc* desc, void* stream);

/* ---- IQN's network backward (what torch's autograd runs behind sorrel/models/pytorch/iqn.py:322-412's loss.backward(): from
 * dL/dquantiles to the gradients of the ten effective weights, in two launches) ----
 * Reads everything sgw_iqn_forward reads, with the same types, strides and limits (states with state_type and state_stride, the ten
 * effective weights, n, in_features = D, layer_size = L 1..256, num_quantiles = N 1..64, num_actions = A 1..64, n_cos = 64), and
 *   taus            float32 [n][N], required: the backward never draws taus;
 *   h               float32 [n][L]: the forward's workspace after the call whose gradient this is;
 *   grad_quantiles  float32 [n][N][A], dense: it need not be one-hot in a.
 * All arithmetic is float32.  Every dot product and every reduction below is ONE fmaf chain in ascending index order that starts at +0
 * (the forward's own chains start at the bias, as before): chain_i(a_i, b_i) = fmaf(a_I-1, b_I-1, ... fmaf(a_0, b_0, +0)).  c, e, z
 * and y are recomputed exactly as sgw_iqn_forward defines them, with the same bits.  mask(x) = !(x <= 0): torch's threshold_backward, 0
 * at 0, and a NaN passes the gradient; it is taken from the stored post-activation value (y <= 0 iff y_pre <= 0, because relu maps those
 * to +0).  With m = a quantile row (m = s N + q), s(m) = its state and g = grad_quantiles[m]:
 *   dueling   G = ((g_0 + g_1) + ...), summed serially;  dval = G;  dadv_a = g_a - G / (float)A;  dO[m] = (dadv_0 .. dadv_(A-1), dval)
 *   dy_j      = mask(y_j) ? chain_o(dO_o, Wo[o][j]), o = 0..A : +0, where Wo = w_adv's rows followed by w_val
 *   dz_k      = chain_j(dy_j, w_ff[j][k])
 *   de_k      = mask(e_k) ? dz_k * h[s][k] : +0
 *   dh[s][k]  = (((dz_k e_k)_q=0 + (dz_k e_k)_q=1) + ...), summed serially over the state's quantiles, every product rounded first
 *   dhp       = mask(h) ? dh : +0
 * Every weight gradient is a chain over the batch rows, ascending (on __builtin_amdgcn_mfma_f32_32x32x2f32 with the batch row as its k:
 * the k-ordered fmaf chain that starts at C, as in the forward):
 *   out_w_adv[o][k] = chain_m(dO[m][o], y[m][k]), o < A;   out_w_val[k] = chain_m(dO[m][A], y[m][k])
 *   out_w_ff[j][k]  = chain_m(dy[m][j], z[m][k])
 *   out_w_cos[j][i] = chain_m(de[m][j], c[m][i])
 *   out_w_head[j][d] = chain_s(dhp[s][j], (float)state[s][d])
 * and every bias gradient the same chain with the activation replaced by 1.  Nothing flows to the states or to the taus.
 * Outputs: ten pointers, one per effective weight and in its shape, each optional (NULL); out_grad_h [n][L] = dh, optional.
 * workspace: sgw_iqn_backward_workspace_bytes(...) bytes, 4-byte aligned, overwritten: z, y, dy, de [n N][L], c [n N][64],
 * dO [n N][A + 1] and dhp [n][L] pass through memory between the two launches ON PURPOSE: a learner's batch is a sampled batch (64
 * states in the reference), and the forward's rule that nothing of size n N L reaches memory was written for acting.  The weight
 * gradients are serial in the batch rows: one wave owns each 32 x 32 tile of a gradient for all rows.  No float atomics: two calls give
 * the same bits.  Non-finite inputs give what IEEE arithmetic gives.  Needs no engine; all pointers are device pointers.  Asynchronous
 * on `stream`; a NULL required pointer (states, a weight, taus, h, grad_quantiles), a misaligned pointer, sizes out of range (as
 * sgw_iqn_forward's), a missing or short workspace, a non-zero reserved field and offsets beyond 64 bits are SGW_EINVAL with the reason
 * in sgw_last_error(), before anything is launched.  n == 0 launches nothing and writes nothing. */
typedef struct sgw_iqn_backward_desc {
    const void* states;          /* [n] rows of in_features elements of state_type, state_stride elements apart */
    const float* w_head;         /* the ten effective weights, as in sgw_iqn_forward_desc */
    const float* b_head;
    const float* w_cos;
    const float* b_cos;
    const float* w_ff;
    const float* b_ff;
    const float* w_adv;
    const float* b_adv;
    const float* w_val;
    const float* b_val;
    const float* taus;           /* [n][N] */
    const float* h;              /* [n][L] */
    const float* grad_quantiles; /* [n][N][A] */
    float* out_w_head;           /* [L][D], or NULL; and so on: each in its weight's shape */
    float* out_b_head;
    float* out_w_cos;
    float* out_b_cos;
    float* out_w_ff;
    float* out_b_ff;
    float* out_w_adv;
    float* out_b_adv;
    float* out_w_val;
    float* out_b_val;
    float* out_grad_h;           /* [n][L], or NULL */
    void* workspace;
    int64_t workspace_bytes;
    int64_t n, state_stride;
    int32_t in_features, layer_size, num_quantiles, num_actions, n_cos, state_type;
    int32_t reserved0, reserved1;    /* reserved: 0 */
} sgw_iqn_backward_desc;
int sgw_iqn_backward(const sgw_iqn_backward_desc* desc, void* stream);
/* Bytes of workspace a call needs (0 for no rows); a negative code for n outside [0, 2^40) or a size outside sgw_iqn_backward's ranges. */
int64_t sgw_iqn_backward_workspace_bytes(int64_t n, int32_t in_features, int32_t layer_size, int32_t num_quantiles, int32_t num_actions);

/* ---- The noisy layers' weights (sorrel/models/pytorch/layers.py:9-65: NoisyLinear.forward's epsilon.normal_() and
 * weight + sigma * epsilon for the weight and the bias of IQN's three noisy layers in each of the three network calls of
 * iRainbowModel.train_step -- 18 normal_, 18 mul and 18 add launches a step -- and autograd's grad * epsilon for the six sigma tensors
 * behind loss.backward(); one launch over a table of tensors each way) ----
 * A call serves num_jobs <= SGW_NOISY_MAX_JOBS jobs; job k is one tensor of count float32 elements.  All tensors are contiguous float32,
 * aligned to 4 bytes (no more is asked: a bias of one element lies anywhere).
 *   mode = SGW_NOISY_FORWARD, per element i of a job:
 *     eps_i      = eps_in[i] where eps_in is given; otherwise drawn KEYED, a pure function of (seed, draw, tensor_id, i):
 *                  w = Philox4x32-10(ctr = {i >> 2, draw & 0xffffffff, draw >> 32, tensor_id << 4 | SGW_STREAM_NOISE}, key = {seed lo, seed hi});
 *                  one block gives four consecutive elements by Box-Muller over its word pairs (w_a, w_b) = (w0, w1) for i & 3 = 0, 1 and
 *                  (w2, w3) for i & 3 = 2, 3:  u1 = (float)((w_a >> 8) + 1) * 2^-24 in (0, 1],  u2 = (float)(w_b >> 8) * 2^-24 in [0, 1),
 *                  r = sqrtf(-2 * logf(u1)),  arg = (float)(2 pi) * u2 (a float32 product),  eps = r * cosf(arg) for even i and r * sinf(arg) for
 *                  odd i; logf, cosf and sinf are the device library's full-precision ones.  |eps| <= sqrt(48 ln 2) = 5.77.  Not consumed:
 *                  the same key gives the same normals whichever jobs share the call and wherever the job stands in the table.
 *     out_eff[i] = weight[i] + (sigma[i] * eps_i): the product is rounded, then the sum (no fused multiply-add), which is torch's
 *                  self.weight + self.sigma_weight * self.epsilon_weight bit for bit.
 *     out_eps[i] = eps_i, where out_eps is given (what the backward needs of a drawn job).
 *     weight, sigma and out_eff are required; grad_eff and out_grad_sigma must be NULL.
 *   mode = SGW_NOISY_BACKWARD, per element:  out_grad_sigma[i] = grad_eff[i] * eps_in[i], one rounding; eps_in (the forward's eps), grad_eff
 *     and out_grad_sigma are required, the forward's pointers must be NULL, tensor_id is ignored.  (The gradient of weight IS grad_eff.)
 * Non-finite inputs give what IEEE arithmetic gives, in that element only.  A job of count 0 and a call of num_jobs 0 write nothing.
 * Jobs past num_jobs are ignored.  No atomics.  Needs no engine; all pointers are device pointers; outputs must not overlap anything.
 * Asynchronous on `stream`; a NULL required pointer, a pointer the mode does not take, a misaligned pointer, count outside [0, 2^32],
 * tensor_id outside [0, 2^28), num_jobs outside [0, SGW_NOISY_MAX_JOBS], an unknown mode and a non-zero reserved field are SGW_EINVAL
 * with the reason in sgw_last_error(), before anything is launched. */
enum { SGW_STREAM_NOISE = 12 };      /* index = element of the tensor, turn / env slots = low / high word of `draw`, epoch slot = tensor_id: sgw_noisy_weights' normals (the thirteenth stream; an enumerator) */
#define SGW_NOISY_MAX_JOBS 24        /* a learner's step: 18 forward (3 network calls x 6 tensors), 6 backward */
#define SGW_NOISY_FORWARD 0
#define SGW_NOISY_BACKWARD 1
typedef struct sgw_noisy_job {
    const float* weight;         /* forward: [count] */
    const float* sigma;          /* forward: [count] */
    const float* eps_in;         /* forward: [count], or NULL: drawn; backward: [count], the forward's eps */
    const float* grad_eff;       /* backward: [count] */
    float* out_eff;              /* forward: [count] */
    float* out_eps;              /* forward: [count], or NULL */
    float* out_grad_sigma;       /* backward: [count] */
    int64_t count;
    int32_t tensor_id;
    int32_t reserved;            /* reserved: 0 */
} sgw_noisy_job;
typedef struct sgw_noisy_weights_desc {
    sgw_noisy_job jobs[SGW_NOISY_MAX_JOBS];
    uint64_t seed, draw;         /* the drawn normals' key, with each job's tensor_id */
    int32_t num_jobs, mode;
    int32_t reserved0, reserved1;    /* reserved: 0 */
} sgw_noisy_weights_desc;
int sgw_noisy_weights(const sgw_noisy_weights_desc* desc, void* stream);

/* ---- The learner clock: a learner's step recorded once and replayed (a graph's argument blocks are frozen, so what changes from one
 * step to the next must be read from device memory) ----
 * A learner's step takes three scalars that change with every step: `draw` of sgw_noisy_weights and `turn` of sgw_iqn_forward, which are
 * both the count of steps done, and `num_starts` of sgw_sample, which grows while the replay ring fills.  The clock holds them in DEVICE
 * memory, 8-byte aligned, filled by the caller; the *_clocked calls read them there, once, with a uniform load at the top of the kernel
 * that needs them, and are otherwise the unclocked calls: every key formula, rule, limit and refusal above holds unchanged, and the
 * results are bit for bit those of the unclocked call given the same scalar.
 *   sgw_noisy_weights_clocked:  draw = clock->count (both words).  desc->draw must be 0.
 *   sgw_iqn_forward_clocked:    the drawn taus' turn = (uint32_t)clock->count; epoch, seed, first_env, num_envs, agent0 and idx come from
 *                               the descriptor.  desc->turn must be 0 and desc->taus NULL (given taus need no clock).
 *   sgw_sample_clocked:         drawn indices only: desc->starts and desc->envs must be NULL; draw_count / draw as in sgw_sample.  The draws
 *                               use num_starts = min(max(clock->num_starts, 1), desc->num_starts): desc->num_starts is the UPPER BOUND,
 *                               checked against capacity and n_frames as sgw_sample checks it, and the clamp runs in the kernel, so no
 *                               value in the clock makes a read leave the ring.
 *   sgw_learn_clock_advance:    count += 1 (one thread), after the step's kernels on `stream`: a recorded chain's last node.
 * All four refuse a NULL clock, a clock whose address is not a multiple of 8 and a non-zero scalar the clock replaces with SGW_EINVAL
 * and the reason in sgw_last_error(), before anything is launched.  reserved is not read. */
typedef struct sgw_learn_clock {
    uint64_t count;              /* learner steps completed = the key of the step in flight */
    int64_t num_starts;          /* ring rows a drawn sample may start from, now */
    uint64_t reserved[2];        /* reserved: 0 */
} sgw_learn_clock;
int sgw_noisy_weights_clocked(const sgw_noisy_weights_desc* desc, const sgw_learn_clock* clock, void* stream);
int sgw_iqn_forward_clocked(const sgw_iqn_forward_desc* desc, const sgw_learn_clock* clock, void* stream);
int sgw_sample_clocked(const sgw_sample_desc* desc, const sgw_learn_clock* clock, void* stream);
int sgw_learn_clock_advance(sgw_learn_clock* clock, void* stream);

/* out6 = { instances compiled, loaded from the disk cache, reused in memory, refused, ms spent compiling, ms spent loading }
 * of this process so far. */
int sgw_jit_stats(double* out6);
/* Compile (or find in the disk cache) the code object of one template instance -- e.g. "step_fast<true, 2, 5, 3, 32, 32>", the
 * `kernel` of an sgw_plan -- for `arch` ("gfx950") WITHOUT loading it: needs no device.  Fills a cache ahead of time (a build
 * machine, a container without a GPU) and lets tools look at the code (registers, scratch).  path_out receives the cache file:
 * "SGWJIT1\n", u32 name length, the lowered kernel name, the code object. */
int sgw_jit_compile(const char* instance, const char* arch, char* path_out, int64_t capacity);

const char* sgw_last_error(void);
const char* sgw_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SGW_H */
