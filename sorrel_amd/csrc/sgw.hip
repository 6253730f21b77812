// sgw.hip -- MI355X (gfx950 / CDNA4) batched gridworld step + observation engine.
//
// Hand-written HIP behind the C ABI of include/sgw.h.  One thread GROUP owns one environment for a whole take_turn
// (or, through sgw_rollout, for T turns): the env's grid (uint8 type ids, [L][H][W]) is staged once into LDS with 16-byte
// loads, the entity sweep and all sequential agent phases run against LDS, observation windows are gathered from LDS
// (lane = window cell) and the grid is written back once.  Integer / indexing work only: no MFMA; the bound is HBM
// bandwidth for the big shapes (observation stores dominate) and instruction issue for the small ones.
//
// Kernels, in file order:
//   step_kernel<G, ONEHOT, L, C, RULE, r, H, W>
//                                        every shape and rule; G = lanes per env: 256 (a workgroup per env, worlds above
//                                        4 KiB: the four waves take the agents in turn behind an LDS ticket, window bytes
//                                        captured before the act and stored after it), 64 (a wave per env), or 32 / 16 --
//                                        two / four SMALL envs share a wave and its instruction stream (what 10x10 ...
//                                        24x24 worlds of large batches run on; compile-time window for the examples as
//                                        shipped); all per-env state in the group's LDS slice; turn loop for sgw_rollout
//                                        built in
//   step_fast<ONEHOT, L, C, r, H, W, TAG, RULES, STAGE, MULTI>
//                                        a wave per env, worlds <= 4 KiB: register sweep, per-lane move inputs + scalar
//                                        move resolution, compile-time window geometry for the BASELINE shapes; one-hot
//                                        observations staged as bytes in LDS and emitted as one burst of streaming
//                                        16-byte stores (fixed shapes: whole env; STAGE: chunks of agents, any alignment);
//                                        MULTI = the turn loop of sgw_rollout
//   step_big<ONEHOT, L, C, r, MULTI, WALK>
//                                        a 512-thread workgroup per env, worlds above 4 KiB (config 5): padded LDS row
//                                        pitch, moves resolved in registers by wave 0 (only interfering agents are walked),
//                                        observations rendered by all waves from the post-move grid with later moves
//                                        undone in registers; WALK = resident workgroups walking the batch, the next
//                                        env's loads issued ahead of this env's observation stores
//   phase_kernel<ONEHOT>                 one policy-driven phase of a world above 4 KiB without staging the env
//   reset_kernel, random_actions_kernel, init_agent_state_kernel, reduce_stage1/2
//   render_kernel<TW, VEC, LDS_ATLAS>    sprite frames of the world tensor (render.h): engine-free, write-bound
// then the host side: options.h, jit.h (the in-process specialiser), plan.h (validation, table building, kernel selection: the planner), and below
// the engine, the launchers and the C entry points.
//
// Semantics follow the reference Python step loop bit for bit; see include/sgw.h for the reference file:line each entry
// point replaces and oracle/gridstep_oracle.py for the line-by-line CPU restatement the kernels are tested against
// (the product never calls it).
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <dlfcn.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/sgw.h"

namespace {

#include "common.h"
#include "step_generic.h"
#include "step_fast.h"
#include "step_big.h"
#include "phase.h"
#include "block_reduce.h"
#include "small_kernels.h"
#include "resolve.h"
#include "render.h"
#include "sample.h"
#include "returns.h"
#include "categorical.h"
#include "policy.h"
#include "ppo_loss.h"
#include "iqn_loss.h"
#include "adam_step.h"
#include "iqn_forward.h"
#include "iqn_backward.h"
#include "noisy.h"

// ---------------------------------------------------------------- host side
#include "options.h"
#include "jit.h"

thread_local char g_err[768] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) return fail(SGW_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// what the engine-free entry points (sgw_sample, sgw_returns, sgw_policy_sample, sgw_ppo_loss, sgw_iqn_loss, sgw_adam_step, sgw_iqn_forward, sgw_noisy_weights) ask of their arguments
inline uintptr_t at(const void* q) { return reinterpret_cast<uintptr_t>(q); }
// is any of these pointers off the alignment `mask` + 1?  (NULL, an optional argument or one of another type, is aligned to everything)
inline bool misaligned(const uintptr_t mask, std::initializer_list<const void*> ptrs) {
    uintptr_t bits = 0;
    for (const void* q : ptrs) bits |= at(q);
    return (bits & mask) != 0;
}
inline bool is_float_type(const int32_t t) { return t == SGW_POLICY_F32 || t == SGW_POLICY_F64; }
inline uintptr_t float_mask(const int32_t t) { return t == SGW_POLICY_F64 ? 7 : 3; }
// SGW_OK, or the refusal of a workspace that is missing or smaller than `need` bytes (`when`: the case that needs one, if not every call does)
int workspace_short(const char* who, const void* ptr, const int64_t have, const int64_t need, const char* when = "") {
    if (need <= 0 || (ptr && have >= need)) return SGW_OK;
    return fail(SGW_EINVAL, "%s:%s needs a workspace of %lld bytes (%s_workspace_bytes); got %lld", who, when, (long long)need, who, ptr ? (long long)have : 0ll);
}

// one launch of kBlock-thread workgroups and the check behind it (a failure reads "hipGetLastError(): ...", as it always has)
#define LAUNCH_TRY(kernel, blocks, s, p) do { hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, s, p); HIP_TRY(hipGetLastError()); } while (0)
// ... of a clocked twin: the same argument block with the learner clock's device address behind it
#define LAUNCH_CLOCKED_TRY(kernel, blocks, s, p, clock) do { hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, s, p, clock); HIP_TRY(hipGetLastError()); } while (0)

constexpr int kEventPool = 4096;

#include "plan.h"

// the agent keys the host can see (rows without idx): agent0 .. agent0 + (n - 1) / num_envs
int keyed_agents_check(const char* who, int32_t agent0, int64_t n, int64_t num_envs) {
    const int64_t last = (int64_t)agent0 + (n > 0 ? (n - 1) / num_envs : 0);
    if (agent0 < 0 || last >= SGW_MAX_AGENTS)
        return fail(SGW_EINVAL, "%s: rows are keyed by agents %d .. %lld, outside [0, %d)", who, agent0, (long long)last, SGW_MAX_AGENTS);
    return SGW_OK;
}

// the network of a descriptor: sgw_iqn_forward_desc and sgw_iqn_backward_desc name its fields alike, so one check and one fill serve both
int iqn_sizes(const char* who, int64_t n, int n_bits, int32_t D, int32_t L, int32_t N, int32_t A) {
    if (n < 0 || (n >> n_bits)) return fail(SGW_EINVAL, "%s: n = %lld outside [0, 2^%d)", who, (long long)n, n_bits);
    if (D < 1) return fail(SGW_EINVAL, "%s: in_features = %d", who, D);
    if (L < 1 || L > kFwdMaxL) return fail(SGW_EINVAL, "%s: layer_size = %d outside [1, %d]", who, L, kFwdMaxL);
    if (N < 1 || N > kFwdM) return fail(SGW_EINVAL, "%s: num_quantiles = %d outside [1, %d]", who, N, kFwdM);
    if (A < 1 || A > SGW_IQN_MAX_ACTIONS) return fail(SGW_EINVAL, "%s: num_actions = %d outside [1, %d]", who, A, SGW_IQN_MAX_ACTIONS);
    return SGW_OK;
}

// states, the ten weights, the sizes (n below 2^n_bits) and the largest byte offset into the states: 4 n state_stride
template <class Desc>
int iqn_network_check(const Desc* d, const char* who, int n_bits) {
    if (!d->states || !d->w_head || !d->b_head || !d->w_cos || !d->b_cos || !d->w_ff || !d->b_ff || !d->w_adv || !d->b_adv || !d->w_val || !d->b_val)
        return fail(SGW_EINVAL, "%s: states and the ten weight pointers must not be NULL", who);
    if (int rc = iqn_sizes(who, d->n, n_bits, d->in_features, d->layer_size, d->num_quantiles, d->num_actions)) return rc;
    if (d->n_cos != SGW_IQN_N_COS) return fail(SGW_EINVAL, "%s: n_cos = %d: only %d is built", who, d->n_cos, SGW_IQN_N_COS);
    if (d->state_type != SGW_IQN_STATE_F32 && d->state_type != SGW_IQN_STATE_U8) return fail(SGW_EINVAL, "%s: unknown state_type %d", who, d->state_type);
    if (d->state_stride < d->in_features) return fail(SGW_EINVAL, "%s: state_stride = %lld is smaller than in_features = %d", who, (long long)d->state_stride, d->in_features);
    if (d->reserved0 || d->reserved1) return fail(SGW_EINVAL, "%s: reserved fields must be 0", who);
    if (d->state_type == SGW_IQN_STATE_F32 && misaligned(3, {d->states})) return fail(SGW_EINVAL, "%s: states is not aligned to its element type", who);
    if (misaligned(3, {d->w_head, d->b_head, d->w_cos, d->b_cos, d->w_ff, d->b_ff, d->w_adv, d->b_adv, d->w_val, d->b_val}))
        return fail(SGW_EINVAL, "%s: misaligned float32 pointer (a weight)", who);
    if (d->n > INT64_MAX / 8 / d->state_stride)
        return fail(SGW_EINVAL, "%s: n = %lld rows of stride %lld do not fit 64-bit offsets", who, (long long)d->n, (long long)d->state_stride);
    return SGW_OK;
}

// what both directions' kernels read of IqnFwdParams (the caller adds h, and the forward its key and its outputs)
template <class Desc>
void iqn_network_fill(IqnFwdParams& p, const Desc* d) {
    p.states = d->states;
    p.w_head = d->w_head; p.b_head = d->b_head; p.w_cos = d->w_cos; p.b_cos = d->b_cos; p.w_ff = d->w_ff; p.b_ff = d->b_ff;
    p.w_adv = d->w_adv; p.b_adv = d->b_adv; p.w_val = d->w_val; p.b_val = d->b_val; p.taus = d->taus;
    p.n = d->n; p.stride = d->state_stride; p.num_envs = 1;
    p.D = d->in_features; p.L = d->layer_size; p.N = d->num_quantiles; p.A = d->num_actions; p.u8 = d->state_type == SGW_IQN_STATE_U8;
    p.R = kFwdM / d->num_quantiles;
    p.q_tiles = ceil_div(d->n, p.R);
}

}  // namespace

struct sgw_engine : Plan {   // the plan (plan.h: what make_plan decided) + the run-time state below, which the planner never writes
    sgw_config cfg;
    Options opt;          // the process-wide options as they were at sgw_create (live keys: sgw_set_option on the engine)
    DevTables* d_tab = nullptr;
    uint8_t* d_tmpl = nullptr;   // fill + border image of one env (reset)
    int* d_status = nullptr;
    double* d_part = nullptr;
    uint8_t* d_dcount = nullptr;     // sgw_turn_resolve, large batches: dirty rows per env of the pass, and where each env's part of the list begins
    uint32_t* d_doffsets = nullptr;
    TurnState* d_turn = nullptr;   // device-side turn state (sgw_turn_*): a whole policy turn as one capturable submission
    bool turn_rows = false;        // sgw_turn_bind gave replay rows
    int64_t turn_ring_cap[SGW_MAX_AGENTS] = {};   // ... host mirror: rows of agent a's ring, whatever columns it binds (sgw_turn_policy_sample)
    int64_t turn_cap[SGW_MAX_AGENTS] = {};        // ... host mirror: rows of agent a's ring (0: none, or no states)
    int64_t turn_row_bytes[SGW_MAX_AGENTS] = {};  // ... bytes of one of its rows (E * row_elems * element size)
    const void* turn_states[SGW_MAX_AGENTS] = {};
    bool turn_rows_even = false;   // ... all of them 8-byte aligned with an even row stride (float2 copies)
    bool turn_rows_flat = false;   // ... all of them 16-byte aligned rows of exactly one window per env, E * N * 4 a multiple of 16 (flat second copies)
    int obs_format = SGW_OBS_F32;
    uint8_t* agent_state = nullptr;    // caller-owned, bound with sgw_bind_agent_state
    uint8_t* state_at_pov = nullptr;
    uint8_t* agent_dir = nullptr;      // caller-owned, bound with sgw_bind_agent_dir
    int tail_kind = SGW_TAIL_NONE, tail_len = 0;   // sgw_bind_row_tail
    const float* tail_table = nullptr;
    int wg_per_cu = 0;     // sgw_set_wg_per_cu: 0 = the automatic rule (Plan::fast_wg_cap), 1..8 = forced, -1 = never capped
    uint32_t auto_max_turns = 0;       // sgw_set_auto_reset
    double* episode_return = nullptr;  // caller-owned
    int num_cus = 256;
    size_t lds_cap = 65536;  // sharedMemPerBlock of the device
    int dev = 0;
    std::string arch = "gfx950";
    // timing
    bool timing = false;
    std::vector<hipEvent_t> ev0, ev1;
    int ev_used = 0;
    double ms_acc = 0.0;
    int64_t launches = 0;
    std::vector<float> series;   // per-launch durations since the last sgw_get_step_times_ms
    int64_t series_dropped = 0;  // launches beyond kSeriesCap since the last read: in the sum, not in the series
};

namespace {

constexpr size_t kSeriesCap = (size_t)1 << 20;

// Compiles / loads one specialised instance (hipRTC: jit.h) and raises its dynamic-LDS limit to `lds` + 16 where that is above the 64 KiB every
// kernel may ask for -- what hipFuncSetAttribute does for the prebuilt instances (0: not here).  nullptr: refused, *err says why.
// The ONE place an instance comes from.
hipFunction_t load_instance(sgw_engine* e, const std::string& name, size_t lds, std::string* err) {
    hipFunction_t f = jit_get(name, e->opt, e->arch.c_str(), e->dev, err);
    if (f && lds > 65536) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(f), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds + 16);
    return f;
}
// The specialised instance of `k`, asked for once.  false: there is none (refused now: *err says why; refused before; or none wanted).
bool resolve_instance(sgw_engine* e, Kernel& k, size_t lds, std::string* err) {
    if (!k.jit && !k.want.empty() && !k.tried) {
        k.tried = true;
        k.jit = load_instance(e, k.want, lds, err);
    }
    return k.jit != nullptr;
}
// ... at first use.  A refusal leaves the prebuilt twin in charge (or, if the plan has none, is an error the caller reports).
int resolve_kernel(sgw_engine* e, Kernel& k) {
    const bool asks = !k.jit && !k.want.empty() && !k.tried;
    std::string err;
    if (resolve_instance(e, k, e->step_lds_bytes > 65536 ? std::max(e->lds_bytes, e->step_lds_bytes) : 0, &err) || k.host) return SGW_OK;
    if (!asks) return fail(SGW_EHIP, "no instance of %s is available", k.want.c_str());
    return fail(SGW_EHIP, "specialising %s failed and the library holds no prebuilt twin: %s", k.want.c_str(), err.c_str());
}

// Specialised instances carry no code for drawn values / target_types (common.h: kExtrasDefault), nor do the prebuilt step_fast instances with
// compile-time tables; the kernels that act have a twin that does, compiled by the specialiser.  "" : `k` serves the extras itself (a prebuilt
// instance with the wave-uniform test) or nobody acts in it.
std::string extras_twin_name(const Kernel& k) {
    if (!k.x_twin) return std::string();
    const std::string src = k.jit ? k.want : ((k.host && k.compile_time_tables) ? std::string(k.host_name) : std::string());
    const size_t lt = src.find('<');
    return lt == std::string::npos ? std::string() : src.substr(0, lt) + "_x" + src.substr(lt);
}
int resolve_twin(sgw_engine* e, Kernel& k) {
    if (k.jit_x) return SGW_OK;
    const std::string name = extras_twin_name(k);
    if (name.empty()) return SGW_OK;
    if (k.tried_x) return fail(SGW_EHIP, "no instance of %s is available", name.c_str());
    k.tried_x = true;
    std::string err;
    k.jit_x = load_instance(e, name, std::max(e->lds_bytes, e->step_lds_bytes), &err);
    if (!k.jit_x) return fail(SGW_EHIP, "specialising %s failed: %s", name.c_str(), err.c_str());   // (a missing kernel is an error, not a silent constant reward)
    return SGW_OK;
}
// ... for every instance in which agents act: at sgw_create / sgw_bind_target_types, so that no stream-ordered call compiles
int resolve_twins(sgw_engine* e) {
    return for_each_kernel(*e, kTwinAtBind, [e](Kernel& k) { return resolve_twin(e, k); });
}

int launch_kernel(sgw_engine* e, Kernel& k, unsigned blocks, unsigned threads, size_t lds, hipStream_t s, Params& p, RowPtrs* rp) {
    if (!k.jit && !k.want.empty() && !k.tried)
        if (int rc = resolve_kernel(e, k)) return rc;
    static RowPtrs no_rows{};                 // (kernels that take the row pointers read them only when Params says so: rows_on, ...)
    void* args[2] = {&p, rp ? rp : &no_rows};
    if (p.extras && p.do_move && !extras_twin_name(k).empty()) {
        if (int rc = resolve_twin(e, k)) return rc;       // (an instance resolved late, e.g. the turn loop of sgw_rollout: its twin follows now)
        HIP_TRY(hipModuleLaunchKernel(k.jit_x, blocks, 1, 1, threads, 1, 1, (unsigned)lds, s, args, nullptr));
        return SGW_OK;
    }
    if (k.jit) HIP_TRY(hipModuleLaunchKernel(k.jit, blocks, 1, 1, threads, 1, 1, (unsigned)lds, s, args, nullptr));
    else if (k.host) HIP_TRY(hipLaunchKernel(k.host, dim3(blocks), dim3(threads), args, lds, s));
    else return fail(SGW_EHIP, "no kernel to launch");
    return SGW_OK;
}

// Waits for the recorded event pairs and folds them into the running sum and the per-launch series.
int time_drain(sgw_engine* e) {
    if (e->ev_used == 0) return SGW_OK;
    for (int i = 0; i < e->ev_used; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventSynchronize(e->ev1[i]));   // each pair on its own: timed launches may have gone to different streams
        HIP_TRY(hipEventElapsedTime(&ms, e->ev0[i], e->ev1[i]));
        e->ms_acc += ms;
        if (e->series.size() < kSeriesCap) e->series.push_back(ms);
        else e->series_dropped++;
    }
    e->ev_used = 0;
    return SGW_OK;
}

int time_begin(sgw_engine* e, hipStream_t s) {
    if (!e->timing) return SGW_OK;
    if (e->ev_used == kEventPool)   // the pool wraps: the one place a launch call waits (include/sgw.h, Conventions)
        if (int rc = time_drain(e)) return rc;
    HIP_TRY(hipEventRecord(e->ev0[e->ev_used], s));
    return SGW_OK;
}

int time_end(sgw_engine* e, hipStream_t s) {
    if (!e->timing) return SGW_OK;
    HIP_TRY(hipEventRecord(e->ev1[e->ev_used], s));
    e->ev_used++;
    e->launches++;
    return SGW_OK;
}

}  // namespace

extern "C" {

const char* sgw_last_error(void) { return g_err; }
#ifdef SGW_STAMPS
int sgw_debug_stamps(unsigned long long* out) {   // diagnostic builds only; not part of the ABI: [kStampEnvs][8] of the last launch
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 8 * kStampEnvs) == hipSuccess ? 0 : -1;
}
#endif

const char* sgw_version(void) { return "sgw 0.3 (gfx950)"; }

int64_t sgw_obs_elems_per_env(const sgw_config* c) {
    const int64_t V = 2 * c->vision_radius + 1;
    return (int64_t)c->num_agents * c->num_channels * V * V;
}
int64_t sgw_grid_bytes_per_env(const sgw_config* c) { return (int64_t)c->layers * c->height * c->width; }
int64_t sgw_algorithmic_bytes_per_env_step(const sgw_config* c) {
    const int64_t V = 2 * c->vision_radius + 1;
    // grid read+write, per agent obs f32 store + action + reward + pos load/store, total f64 rw
    return 2 * sgw_grid_bytes_per_env(c) + (int64_t)c->num_agents * (c->num_channels * V * V * 4 + 1 + 4 + 4) + 16;
}

int sgw_set_option(sgw_engine* e, const char* key, const char* value) {
    int rc;
    if (e) {
        rc = option_set(e->opt, key, value, true);
    } else {
        std::lock_guard<std::mutex> lock(g_opt_mu);
        rc = option_set(g_opts, key, value, false);
    }
    if (rc == 1) return fail(SGW_EINVAL, "sgw_set_option: unknown key '%s'", key ? key : "(null)");
    if (rc == 2) return fail(SGW_EINVAL, "sgw_set_option: value '%s' is out of range for '%s'", value ? value : "(null)", key);
    if (rc == 3) return fail(SGW_EINVAL, "sgw_set_option: '%s' shapes the plan of an engine: set it (with a NULL engine) before sgw_create", key ? key : "(all keys)");
    return SGW_OK;
}

static int sgw_debug(void) {   // the ONE environment variable the shipped library reads: SGW_DEBUG=1 turns on the specialiser's log lines
    static const int v = [] { const char* f = getenv("SGW_DEBUG"); return (f && f[0] == '1') ? 1 : 0; }();
    return v;
}

// what make_plan decided, in the ABI's words
static void describe_plan(const Plan* e, sgw_plan_info* out) {
    memset(out, 0, sizeof(*out));
    out->family = e->fast ? SGW_FAMILY_WAVE : (e->big ? SGW_FAMILY_WORKGROUP : SGW_FAMILY_GENERIC);
    out->lanes_per_env = (e->fast || e->big) ? (e->big ? e->big_threads : kWave) : e->group;
    out->threads = e->big ? e->big_threads : kBlock;
    out->grid_blocks = e->grid_blocks;
    out->lds_bytes = (int64_t)e->step_lds_bytes;
    out->env_lds = e->step_env_lds;
    out->obs_stage = e->obs_stage;
    out->stage_agents = e->stage_agents;
    out->whole_env_burst = e->whole_env_burst ? 1 : 0;
    out->big_stage = e->big_stage;
    out->big_pitch = e->base.big_pitch;
    out->onehot = e->onehot ? 1 : 0;
    out->rgb16 = e->rgb16 ? 1 : 0;
    out->rules = e->fast_rules ? 1 : 0;
    out->specialised = e->jit ? 1 : 0;
    out->phase_kernel = e->phase_ok ? 1 : 0;
    out->rollout_in_one_launch = e->multi_turn ? 1 : 0;
    out->walk_blocks = e->walk_blocks;
    out->walk_min_envs = e->walk_min_envs;
    out->walk_max_envs = e->walk_max_envs;
    out->big_stage_min_envs = e->big_stage_min_envs;
    auto put = [](char* dst, size_t cap, const Kernel& k, bool prebuilt) {
        const char* s = prebuilt ? (k.host ? k.host_name : "-") : (k.want.empty() ? (k.host ? k.host_name : "-") : k.want.c_str());
        snprintf(dst, cap, "%s", s);
    };
    put(out->kernel, sizeof(out->kernel), e->k_step, false);
    put(out->kernel_prebuilt, sizeof(out->kernel_prebuilt), e->k_step, true);
    put(out->kernel_plain, sizeof(out->kernel_plain), e->k_plain, false);
    put(out->kernel_rollout, sizeof(out->kernel_rollout), e->k_multi, false);
    put(out->kernel_walk, sizeof(out->kernel_walk), e->k_walk, false);
    put(out->kernel_phase, sizeof(out->kernel_phase), e->k_rows, false);
    if (!e->k_rows.usable()) snprintf(out->kernel_phase, sizeof(out->kernel_phase), "%s", e->phase_ok ? (e->onehot ? "phase_kernel<true>" : "phase_kernel<false>") : "the step kernel");
    put(out->kernel_observe_rows, sizeof(out->kernel_observe_rows), e->k_obs_rows, false);
}

int sgw_plan(const sgw_config* cfg, int32_t num_cus, int64_t lds_per_workgroup, sgw_plan_info* out) {
    if (!out) return fail(SGW_EINVAL, "sgw_plan: out is NULL");
    if (int rc = validate(cfg)) return rc;
    Options o;
    {
        std::lock_guard<std::mutex> lock(g_opt_mu);
        o = g_opts;
    }
    Plan* plan = new (std::nothrow) Plan();
    if (!plan) return fail(SGW_ENOMEM, "out of host memory");
    // (whether hipRTC can be loaded is a property of the machine, not of the plan: sgw_plan answers for a machine that has it
    // unless the option says otherwise; sgw_create re-plans with jit = false when a compile is refused)
    const int rc = make_plan(*cfg, o, num_cus > 0 ? num_cus : 256, lds_per_workgroup > 0 ? (size_t)lds_per_workgroup : 65536, o.jit != 0 && SGW_JIT_SOURCES, plan);
    if (rc == SGW_OK) describe_plan(plan, out);
    delete plan;
    return rc;
}

int sgw_jit_compile(const char* instance, const char* arch, char* path_out, int64_t capacity) {
    if (!instance || !arch) return fail(SGW_EINVAL, "sgw_jit_compile: NULL argument");
    Options o;
    {
        std::lock_guard<std::mutex> lock(g_opt_mu);
        o = g_opts;
    }
    std::lock_guard<std::mutex> lock(g_jit_mu);
    std::string lowered, code, path, err;
    bool from_disk = false;
    const auto t0 = std::chrono::steady_clock::now();
    if (!jit_build(instance, o, arch, &lowered, &code, &path, &from_disk, &err)) return fail(SGW_EHIP, "sgw_jit_compile: %s", err.c_str());
    if (!from_disk) {
        g_jit_stats.compiled++;
        g_jit_stats.compile_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    } else {
        g_jit_stats.disk_hits++;
    }
    if (path_out && capacity > 0) snprintf(path_out, (size_t)capacity, "%s", path.c_str());
    return SGW_OK;
}

int sgw_jit_stats(double* out6) {
    if (!out6) return fail(SGW_EINVAL, "sgw_jit_stats: NULL argument");
    std::lock_guard<std::mutex> lock(g_jit_mu);
    out6[0] = (double)g_jit_stats.compiled; out6[1] = (double)g_jit_stats.disk_hits; out6[2] = (double)g_jit_stats.mem_hits;
    out6[3] = (double)g_jit_stats.failed; out6[4] = g_jit_stats.compile_ms; out6[5] = g_jit_stats.load_ms;
    return SGW_OK;
}

int sgw_create(const sgw_config* cfg, sgw_engine** out) {
    if (!out) return fail(SGW_EINVAL, "out is NULL");
    *out = nullptr;
    if (int rc = validate(cfg)) return rc;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));

    sgw_engine* e = new (std::nothrow) sgw_engine();
    if (!e) return fail(SGW_ENOMEM, "out of host memory");
    e->cfg = *cfg;
    {
        std::lock_guard<std::mutex> lock(g_opt_mu);
        e->opt = g_opts;
    }
    if (sgw_debug()) e->opt.jit_verbose = 1;
    e->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    e->lds_cap = prop.sharedMemPerBlock > 0 ? prop.sharedMemPerBlock : 65536;
    e->dev = dev;
    e->arch = prop.gcnArchName[0] ? prop.gcnArchName : "gfx950";

    // the plan; EVERY specialised instance it counts on is compiled / loaded now, and a refusal of any of them (no hipRTC, no embedded
    // sources, a compile error, a code object that does not load) re-plans for the prebuilt instances.  (Until round 5 only the whole-turn
    // kernel was resolved here and the others at first use: a late refusal then left a prebuilt run-time-shape twin running under a plan
    // laid out for compile-time shapes -- no slack behind the staged chunk for the planes a run-time channel count writes in groups of
    // four -- and sgw_capabilities promised row kernels that existed only specialised.)
    bool jit = e->opt.jit != 0 && SGW_JIT_SOURCES;
    for (;;) {
        if (int rc = make_plan(e->cfg, e->opt, e->num_cus, e->lds_cap, jit, e)) { delete e; return rc; }
        if (!jit) break;
        {   // (the ones that have to be compiled: in one program, jit.h)
            std::vector<std::string> names;
            for_each_kernel(*e, kResolvedAtCreate, [&](Kernel& k) { if (!k.want.empty()) names.push_back(k.want); return 0; });
            jit_prefetch(names, e->opt, e->arch.c_str(), e->dev);
        }
        std::string err;   // (their LDS limit: with the prebuilt instances' below)
        if (!for_each_kernel(*e, kResolvedAtCreate, [&](Kernel& k) { return (k.want.empty() || resolve_instance(e, k, 0, &err)) ? 0 : 1; })) break;
        jit = false;
    }

    hipError_t err = hipMalloc(&e->d_tab, sizeof(DevTables));
    if (err == hipSuccess) err = hipMemcpy(e->d_tab, &e->h_tab, sizeof(DevTables), hipMemcpyHostToDevice);
    {   // the reset image: per layer the fill type, the border type around it; bytes past the last cell are not cells
        const sgw_config& c = e->cfg;
        std::vector<uint8_t> img((size_t)e->base.cells_pad, (uint8_t)0xFF);
        for (int z = 0; z < c.layers; ++z)
            for (int y = 0; y < c.height; ++y)
                for (int x = 0; x < c.width; ++x) {
                    const bool edge = y == 0 || y == c.height - 1 || x == 0 || x == c.width - 1;
                    const uint8_t b = c.layer_border_type[z];
                    img[((size_t)z * c.height + y) * c.width + x] = (b != SGW_NO_BORDER && edge) ? b : c.layer_fill_type[z];
                }
        if (err == hipSuccess) err = hipMalloc(&e->d_tmpl, img.size());
        if (err == hipSuccess) err = hipMemcpy(e->d_tmpl, img.data(), img.size(), hipMemcpyHostToDevice);
    }
    if (err == hipSuccess) err = hipMalloc(&e->d_status, 4 * sizeof(int));
    if (err == hipSuccess) err = hipMemset(e->d_status, 0, 4 * sizeof(int));
    if (err == hipSuccess) err = hipMalloc(&e->d_part, 2 * kRedBlocks * sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&e->d_turn, sizeof(TurnState));
    if (err == hipSuccess) err = hipMemset(e->d_turn, 0, sizeof(TurnState));
    if (e->cfg.num_envs >= 8192) {     // sgw_turn_resolve's scan-built dirty list (large batches): allocated HERE, not inside a stream-ordered (capturable) call
        const size_t nb = (size_t)ceil_div(e->cfg.num_envs, 256);
        if (err == hipSuccess) err = hipMalloc(&e->d_dcount, (size_t)e->cfg.num_envs);
        if (err == hipSuccess) err = hipMalloc(&e->d_doffsets, 2 * nb * sizeof(uint32_t));      // block sums | block offsets
        if (err == hipSuccess) err = hipMemset(e->d_doffsets, 0, 2 * nb * sizeof(uint32_t));
    }
    if (err != hipSuccess) {
        sgw_destroy(e);
        return fail(SGW_EHIP, "device allocation failed: %s", hipGetErrorString(err));
    }
    e->base.tab = e->d_tab;
    e->base.tmpl = e->d_tmpl;
    e->base.status = e->d_status;

    if (std::max(e->lds_bytes, e->step_lds_bytes) > std::min<size_t>(e->lds_cap, 65536)) {
        err = hipSuccess;
        for_each_kernel(*e, kWholeStep, [&](Kernel& k) {
            if (err == hipSuccess && k.host) err = hipFuncSetAttribute(k.host, hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->step_lds_bytes + 16);   // (+ the walking variant's hand-over word)
            return 0;
        });
        for_each_kernel(*e, kWholeStep, [&](Kernel& k) {
            if (err == hipSuccess && k.jit) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k.jit), hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->step_lds_bytes + 16);
            return 0;
        });
        if (err == hipSuccess)
            err = hipFuncSetAttribute(reinterpret_cast<const void*>(e->reset_fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->lds_bytes);
        if (err != hipSuccess) {
            sgw_destroy(e);
            return fail(SGW_EHIP, "cannot reserve %zu bytes of LDS: %s", e->lds_bytes, hipGetErrorString(err));
        }
    }
    if (e->base.extras)
        if (int rc = resolve_twins(e)) { sgw_destroy(e); return rc; }
    *out = e;
    return SGW_OK;
}

void sgw_destroy(sgw_engine* e) {
    if (!e) return;
    for (hipEvent_t ev : e->ev0) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : e->ev1) (void)hipEventDestroy(ev);
    if (e->d_tab) (void)hipFree(e->d_tab);
    if (e->d_tmpl) (void)hipFree(e->d_tmpl);
    if (e->d_status) (void)hipFree(e->d_status);
    if (e->d_part) (void)hipFree(e->d_part);
    if (e->d_dcount) (void)hipFree(e->d_dcount);
    if (e->d_doffsets) (void)hipFree(e->d_doffsets);
    if (e->d_turn) (void)hipFree(e->d_turn);
    delete e;
}

static int launch_reset(sgw_engine* e, uint8_t* grid, uint8_t* agent_pos, double* total_reward, uint32_t epoch, void* stream) {
    const sgw_config& c = e->cfg;
    const int b = c.layer_border_type[c.agent_layer];
    if (b == SGW_NO_BORDER || c.type_passable[b])
        return fail(SGW_EINVAL, "sgw_reset: the agent layer needs an impassable border type (the reference has no bounds check in move)");
    if (epoch >= (1u << 28)) return fail(SGW_EINVAL, "epoch must be < 2^28");
    Params p = e->base;
    p.grid = grid; p.pos = agent_pos; p.total = total_reward; p.epoch = epoch;
    p.agent_state = e->agent_state;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(e->reset_fn, dim3(e->reset_blocks), dim3(kBlock), e->lds_bytes, s, p);
    HIP_TRY(hipGetLastError());
    return SGW_OK;
}

int sgw_reset(sgw_engine* e, uint8_t* grid, uint8_t* agent_pos, double* total_reward, uint32_t epoch, void* stream) {
    if (!e || !grid || !agent_pos || !total_reward) return fail(SGW_EINVAL, "sgw_reset: NULL argument");
    return launch_reset(e, grid, agent_pos, total_reward, epoch, stream);
}

// The dynamic-LDS request of a step launch, and the workgroup-per-CU cap it encodes (0 = none).  The cap is the one
// launch-time lever on occupancy; the policy (sgw_set_wg_per_cu: 0 = the automatic rule, 1..8 forced, -1 never):
// five workgroups per CU for whole-turn float32 observation writes of 8 KiB or more per env in large batches, where fewer
// concurrent waves mean fewer half-written lines open in HBM --
//  - the unstaged path (Cleanup, 21x31x3 at 65 536 envs: 893 -> 801 us);
//  - the staged path only when the grids of the batch no longer fit the caches, and SIX per CU there since its bursts sit on
//    128-byte lines (round 3, config 3's shape, us per launch at 8 / 7 / 6 / 5 / 4 per CU: 524 288 envs 1 321 / 1 061 / 1 082 / 1 167 / 1 347,
//    262 144 envs 640 / 598 / 566 / 595 / 679; before the aligned bursts five was best: 262 144 envs 662 -> 578 us, 524 288: 1375 -> 1146 us).  While they do fit (configs 3/4: 65 536 envs, 134 MB) the staged emit with its streaming
//    full-line stores is fastest at full occupancy (124 us at 8 and 7 per CU, 126 at 6, 131 at 5; 131 072 envs: 248 vs 281).
// The uint8 format, small batches and the shapes with small windows, which are latency-bound (Tag 11x11, 6.5 KB per env:
// 164 us at full occupancy, 192 us capped), are not capped.
static size_t step_lds_request(const sgw_engine* e, const Params& p, int* cap_out) {
    size_t lds = e->step_lds_bytes;
    int cap = 0;
    if (e->fast && e->wg_per_cu > 0) cap = e->wg_per_cu;
    else if (e->fast && e->wg_per_cu == 0 && e->fast_wg_cap > 0 && p.obs && !(p.flags & SGW_STEP_NO_OBS) && !p.obs_u8 &&
             (!p.obs_stage || (size_t)p.E * (size_t)p.env_stride > kCacheResidentGrid) && p.a1 == p.A && p.a0 == 0 &&
             (size_t)p.A * p.C * p.VV * 4 >= 8192 && p.E >= (int64_t)e->num_cus * 32 * 2)
        cap = (p.obs_stage && !e->fast_wg_cap_forced) ? 6 : e->fast_wg_cap;   // (staged, line-aligned bursts: six -- see above)
    if (cap > 0) lds = std::max(lds, (size_t)(kLdsPerCu / cap - 1024) & ~(size_t)511);   // 1 KiB below the share: LDS is handed out in 1 KiB granules
    if (cap_out) *cap_out = cap;
    return lds;
}

// A/B hook (option big_wg_per_cu): fewer step_big workgroups per CU than the code object admits, through the LDS request
static size_t big_cap_lds(const sgw_engine* e, size_t lds) {
    if (!e->big || e->opt.big_wg_per_cu <= 0) return lds;
    const size_t want = (size_t)(kLdsPerCu / e->opt.big_wg_per_cu - 1024) & ~(size_t)511;
    return (want > lds && want <= 65536) ? want : lds;
}

// What a step call launches: decided HERE for launch_step, which launches it, and for sgw_launch_info, which prints it.
struct StepLaunch {
    Kernel* k = nullptr;      // nullptr: phase_kernel<ONEHOT>, the byte-gather phase kernel (no instance of the plan)
    unsigned blocks = 0, threads = kBlock;
    size_t lds = 0;           // the dynamic-LDS request (a workgroup-per-CU cap is part of it)
    size_t lds_info = 0;      // ... of the step kernels, as sgw_launch_info has always shown it: without the walking variant's hand-over word
    int cap = 0;              // workgroups per CU that request encodes (0: none)
    bool walk = false;        // step_big<..., WALK>: resident workgroups walking the batch
    int big_stage = 0;        // step_big: staging bytes per wave of THIS launch (0: direct stores)
    RowPtrs* rows = nullptr;  // the kernel's second argument
};

// Completes the per-call fields of `p` and says what runs.  The order of the tests below is behaviour.
static int step_launch(sgw_engine* e, Params& p, RowPtrs* sweep_rows, StepLaunch* d) {
    p.env_lds = e->step_env_lds;
    if (e->fast || e->big) p.tab_bytes = e->big ? e->big_tab_bytes : e->fast_tab_bytes;
    p.obs_stage = (e->fast && p.obs && (reinterpret_cast<uintptr_t>(p.obs) & 15) == 0) ? e->obs_stage : 0;
    if (sweep_rows) p.obs_stage = e->obs_stage;   // (step_fast_rows: the staged windows leave per agent, whatever `obs` is)
    if (p.spawn_mask == 0 && !p.has_become) p.flags &= ~SGW_STEP_SWEEP;   // nothing transitions
    size_t lds = step_lds_request(e, p, &d->cap);
    // step_big: the walking variant keeps the direct stores (measured faster there), and so does a launch whose observation
    // pointer is not 16-byte aligned; such a launch does not ask for the staging area either
    const bool walk = e->big && p.nturns == 1 && !sweep_rows && e->k_walk.usable() && p.E > e->walk_min_envs && p.E <= e->walk_max_envs;
    p.big_stage = (e->big && ((p.obs && (reinterpret_cast<uintptr_t>(p.obs) & 15) == 0) || (sweep_rows && !p.obs_u8)) && !walk && p.E > e->big_stage_min_envs) ? e->big_stage : 0;
    if (walk) {     // the walking workgroups: a static share each, the rest off a counter (step_big.h)
        p.walk_ctr = reinterpret_cast<uint32_t*>(e->d_status) + 1;
        p.walk_static = e->opt.big_walk_share > 0 ? e->opt.big_walk_share : (int)std::max<int64_t>(1, p.E / e->walk_blocks);
    }
    if (e->big && p.nturns > 1 && e->big_threads != kBigThreads) p.big_stage = 0;   // (the rollout instance runs kBigThreads: the staging area is sized for this engine's waves)
    if (e->big && e->big_stage && !p.big_stage) lds -= (size_t)(e->big_threads / 64) * e->big_stage;
    d->walk = walk;
    d->big_stage = p.big_stage;
    d->lds_info = big_cap_lds(e, lds);
    if (walk) { p.walk_word = (int)lds; lds += 16; }   // (behind the grid image: the walking variant has no staging area there)
    lds = big_cap_lds(e, lds);
    d->lds = lds;
    if (sweep_rows && e->fast) {
        if (p.obs_stage <= 0 || p.a0 != 0 || p.a1 != p.A || (p.flags & SGW_STEP_NO_OBS))      // (step_fast_rows has no other way to emit than its staged burst)
            return fail(SGW_EINVAL, "sgw_sweep_observe_rows: this engine does not stage its windows");
        if (e->sweep_rows_chunked) p.stage_agents = 1;                                           // (ROWX: a chunk = one agent = one row)
        d->k = (p.tail_kind != SGW_TAIL_NONE && !e->sweep_rows_chunked) ? &e->k_sweep_rows_tail : &e->k_sweep_rows;
        d->blocks = (unsigned)e->grid_blocks;
        d->rows = sweep_rows;
        return SGW_OK;
    }
    // A policy-driven phase (at most one agent moves, at most one window is rendered, no sweep, plain moves) of a one-hot
    // world whose (layers, channels, radius) has a phase_rows instance: a lane per window row, no staging, any world size.
    // (the phase kernels take the acting agent's action from the tensor: a phase whose action is drawn on the device -- SGW_STEP_RANDOM_ACTIONS,
    // an agent with a RandomModel among agents that step one by one -- stays on the step kernel, which draws it)
    // (known defect, left alone: one_phase does not exclude sweep_rows -- a single-agent world on a workgroup-per-env or generic engine reaches it from sgw_sweep_observe_rows)
    const bool one_phase = p.nturns == 1 && !(p.flags & (SGW_STEP_SWEEP | SGW_STEP_RANDOM_ACTIONS)) && p.a1 - p.a0 <= 1 && (p.do_move || p.a1 - p.a0 == 1);
    if (e->k_rows.usable() && one_phase && !p.obs_u8) {
        // one window per env: contiguous for all envs only in the packed destination ([E][C][V][V])
        const uintptr_t dst = reinterpret_cast<uintptr_t>(p.obs);
        p.rows_mode = (p.obs_A == 1 && (dst & 15) == 0) ? kRowsFlat : kRowsRun;
        d->k = &e->k_rows;
        d->blocks = (unsigned)ceil_div(p.E, e->rows_epb);
        d->lds = e->rows_lds;
        return SGW_OK;
    }
    // ... otherwise, for worlds above 4 KiB: the byte-gather phase kernel (option phase_kernel)
    if (e->phase_ok && one_phase) {
        const int env_lds = (e->onehot ? 4 * SGW_MAX_TYPES * 4 : SGW_MAX_TYPES * SGW_MAX_CHANNELS * 8) + SGW_MAX_TYPES * 8;   // + the value table
        d->k = nullptr;
        d->blocks = (unsigned)ceil_div(p.E, 4);
        d->lds = (size_t)4 * env_lds;
        return SGW_OK;
    }
    // a STAGE kernel has no direct-store path: calls it cannot serve take the plain variant
    Kernel* k = &e->k_step;
    if (e->fast && e->stage_agents > 0 && e->k_plain.usable() &&
        (p.obs_stage == 0 || p.a0 != 0 || p.a1 != p.A || p.obs_next || (p.flags & SGW_STEP_NO_OBS))) {
        k = &e->k_plain;
        p.obs_stage = 0;   // (a compile-time-shape plain instance would otherwise stage a whole env into a chunk-sized area)
        if (e->rgb16) {    // the float64 kernel: its own table area, no staging, no result table
            p.tab_bytes = e->plain_tab_bytes;
            p.env_lds = e->plain_tab_bytes + p.cells_pad;
            lds = (size_t)(kBlock / kWave) * p.env_lds;
        }
    }
    d->lds = lds;
    if (p.nturns > 1) k = &e->k_multi;   // sgw_rollout made sure it exists and the call qualifies
    int blocks = e->grid_blocks;
    if (walk) {   // two to three rounds of the plain kernel
        k = &e->k_walk;
        blocks = e->walk_blocks;
    }
    if (sweep_rows) k = &e->k_sweep_rows;     // (step_big<..., ROWS> / step_kernel<..., ROWS>: the plain single-turn variant with the row pointers as its second argument; `walk` is off above)
    d->k = k;
    d->blocks = (unsigned)blocks;
    d->threads = e->big ? (p.nturns > 1 ? kBigThreads : e->big_threads) : kBlock;
    d->rows = sweep_rows;
    return SGW_OK;
}

static int launch_step(sgw_engine* e, Params& p, hipStream_t s, RowPtrs* sweep_rows = nullptr) {
    p.agent_state = e->agent_state;
    p.state_at_pov = e->state_at_pov;
    p.agent_dir = e->agent_dir;
    if (p.agent_rule == SGW_AGENT_RULE_CLEANUP && p.do_move && !p.agent_dir)
        return fail(SGW_EINVAL, "SGW_AGENT_RULE_CLEANUP needs sgw_bind_agent_dir");
    p.obs_u8 = e->obs_format == SGW_OBS_U8 ? 1 : 0;
    if (p.agent_rule == SGW_AGENT_RULE_TAG && p.do_move && !p.agent_state)
        return fail(SGW_EINVAL, "SGW_AGENT_RULE_TAG needs sgw_bind_agent_state");
    if (int rc = time_begin(e, s)) return rc;
    StepLaunch d;
    if (int rc = step_launch(e, p, sweep_rows, &d)) return rc;
    if (!d.k) {
        Params q = p;
        q.env_lds = (int)(d.lds / 4);
        hipLaunchKernelGGL(e->onehot ? phase_kernel<true> : phase_kernel<false>, dim3(d.blocks), dim3(d.threads), d.lds, s, q);
        HIP_TRY(hipGetLastError());
    } else if (int rc = launch_kernel(e, *d.k, d.blocks, d.threads, d.lds, s, p, d.rows)) {
        return rc;
    }
    return time_end(e, s);
}

int sgw_observe(sgw_engine* e, const uint8_t* grid, const uint8_t* agent_pos, float* obs, int32_t agent_begin,
                int32_t agent_end, void* stream) {
    if (!e || !grid || !agent_pos || !obs) return fail(SGW_EINVAL, "sgw_observe: NULL argument");
    if (agent_begin < 0 || agent_end > e->cfg.num_agents || agent_begin > agent_end)
        return fail(SGW_EINVAL, "sgw_observe: agent range [%d, %d) invalid", agent_begin, agent_end);
    Params p = e->base;
    p.grid = const_cast<uint8_t*>(grid); p.pos = const_cast<uint8_t*>(agent_pos); p.obs = obs;
    p.a0 = agent_begin; p.a1 = agent_end; p.flags = 0; p.do_move = 0;
    return launch_step(e, p, static_cast<hipStream_t>(stream));
}

int sgw_observe_full(sgw_engine* e, const uint8_t* grid, void* out, void* stream) {
    if (!e || !grid || !out) return fail(SGW_EINVAL, "sgw_observe_full: NULL argument");
    Params p = e->base;
    p.grid = const_cast<uint8_t*>(grid);
    p.obs_u8 = e->obs_format == SGW_OBS_U8 ? 1 : 0;
    const int64_t n = p.E * (int64_t)p.H * p.W;
    const int blocks = (int)std::min<int64_t>(ceil_div(n, kBlock), (int64_t)e->num_cus * 16);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = time_begin(e, s)) return rc;
    hipLaunchKernelGGL(observe_full_kernel, dim3(blocks), dim3(kBlock), 0, s, p, out);
    HIP_TRY(hipGetLastError());
    return time_end(e, s);
}

int sgw_step(sgw_engine* e, uint8_t* grid, uint8_t* agent_pos, uint8_t* actions, float* obs, float* rewards,
             double* total_reward, uint32_t epoch, uint32_t turn, int32_t agent_begin, int32_t agent_end,
             uint32_t flags, void* stream) {
    if (!e || !grid || !agent_pos || !actions || !rewards || !total_reward)
        return fail(SGW_EINVAL, "sgw_step: NULL argument");
    if (!obs && (flags & SGW_STEP_OBS_NEXT)) return fail(SGW_EINVAL, "sgw_step: SGW_STEP_OBS_NEXT needs obs");
    if (!obs && !(flags & SGW_STEP_NO_OBS)) return fail(SGW_EINVAL, "sgw_step: obs is NULL without SGW_STEP_NO_OBS");
    if (agent_begin < 0 || agent_end > e->cfg.num_agents || agent_begin > agent_end)
        return fail(SGW_EINVAL, "sgw_step: agent range [%d, %d) invalid", agent_begin, agent_end);
    if (epoch >= (1u << 28)) return fail(SGW_EINVAL, "epoch must be < 2^28");
    Params p = e->base;
    p.grid = grid; p.pos = agent_pos; p.actions = actions; p.obs = obs; p.rewards = rewards; p.total = total_reward;
    p.epoch = epoch; p.turn = turn; p.a0 = agent_begin; p.a1 = agent_end; p.flags = flags; p.do_move = 1;
    if (flags & SGW_STEP_OBS_AGENT_MAJOR) {
        if (!e->big || agent_begin != 0 || agent_end != e->cfg.num_agents || (flags & (SGW_STEP_OBS_NEXT | SGW_STEP_NO_OBS)) || !obs)
            return fail(SGW_EINVAL, "sgw_step: SGW_STEP_OBS_AGENT_MAJOR is for whole-turn calls with observations on engines with SGW_CAP_OBS_AGENT_MAJOR");
        p.obs_ag = (int64_t)e->cfg.num_envs * e->base.C * e->base.VV;
        p.flags &= ~SGW_STEP_OBS_AGENT_MAJOR;
    }
    if (flags & SGW_STEP_NO_MOVE) {    // sweep + windows, nobody acts
        if (flags & (SGW_STEP_RANDOM_ACTIONS | SGW_STEP_OBS_NEXT | SGW_STEP_OBS_NEXT_PACKED))
            return fail(SGW_EINVAL, "sgw_step: SGW_STEP_NO_MOVE does not combine with RANDOM_ACTIONS / OBS_NEXT");
        p.do_move = 0;
        p.flags &= ~SGW_STEP_NO_MOVE;
        return launch_step(e, p, static_cast<hipStream_t>(stream));
    }
    if (flags & SGW_STEP_OBS_NEXT) {   // the stepped agents' own observations are not written
        p.obs_next = 1;
        p.flags |= SGW_STEP_NO_OBS;
        if (flags & SGW_STEP_OBS_NEXT_PACKED) {   // `obs` holds one window per env: agent_end's
            p.obs_A = 1;
            p.obs_a0 = agent_end;
        }
    } else if (flags & SGW_STEP_OBS_NEXT_PACKED) {
        return fail(SGW_EINVAL, "sgw_step: SGW_STEP_OBS_NEXT_PACKED qualifies SGW_STEP_OBS_NEXT");
    }
    if (int rc = launch_step(e, p, static_cast<hipStream_t>(stream))) return rc;
    if (e->auto_max_turns && turn == e->auto_max_turns && agent_end == e->cfg.num_agents) {
        // end of the epoch: keep the returns, then create_world + populate_environment for the next one
        if (epoch + 1 >= (1u << 28)) return fail(SGW_EINVAL, "epoch must be < 2^28");
        if (e->episode_return)
            HIP_TRY(hipMemcpyAsync(e->episode_return, total_reward, sizeof(double) * (size_t)e->cfg.num_envs,
                                   hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
        return launch_reset(e, grid, agent_pos, total_reward, epoch + 1, stream);
    }
    return SGW_OK;
}

int sgw_rollout(sgw_engine* e, uint8_t* grid, uint8_t* agent_pos, uint8_t* actions, float* obs, float* rewards,
                double* total_reward, uint32_t epoch, uint32_t first_turn, uint32_t num_turns, int64_t obs_turn_stride,
                int64_t actions_turn_stride, int64_t rewards_turn_stride, uint32_t flags, void* stream) {
    if (!e || !grid || !agent_pos || !actions || !rewards || !total_reward)
        return fail(SGW_EINVAL, "sgw_rollout: NULL argument");
    if (!obs && !(flags & SGW_STEP_NO_OBS)) return fail(SGW_EINVAL, "sgw_rollout: obs is NULL without SGW_STEP_NO_OBS");
    if (flags & SGW_STEP_OBS_NEXT) return fail(SGW_EINVAL, "sgw_rollout: SGW_STEP_OBS_NEXT is a per-agent flag of sgw_step");
    if (obs_turn_stride < 0 || actions_turn_stride < 0 || rewards_turn_stride < 0)
        return fail(SGW_EINVAL, "sgw_rollout: negative turn stride");
    const int A = e->cfg.num_agents;
    if (e->multi_turn && !e->k_multi.jit && !e->k_multi.host) {   // the turn-loop instance exists only specialised: get it now, or loop over single turns
        if (resolve_kernel(e, e->k_multi) != SGW_OK) e->multi_turn = false;
    }
    uint32_t done = 0;
    while (done < num_turns) {
        const uint32_t turn = first_turn + done;
        // turns of one launch: up to the end of the epoch if auto-reset is armed; one per launch on kernels without a turn loop
        uint32_t n = num_turns - done;
        if (e->auto_max_turns && turn <= e->auto_max_turns) n = std::min(n, e->auto_max_turns - turn + 1);
        if (!e->multi_turn) n = 1;
        // the wave-per-env MULTI kernels stage their observations: every turn's slot must keep the 16-byte alignment
        if (e->fast && (!obs || (flags & SGW_STEP_NO_OBS) || (reinterpret_cast<uintptr_t>(obs) & 15) || (obs_turn_stride & 3) || e->obs_stage == 0)) n = 1;
        if (epoch >= (1u << 28)) return fail(SGW_EINVAL, "epoch must be < 2^28");
        Params p = e->base;
        p.grid = grid; p.pos = agent_pos; p.total = total_reward;
        p.actions = actions + (int64_t)done * actions_turn_stride;
        p.obs = obs ? reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(obs) + (int64_t)done * obs_turn_stride * (e->obs_format == SGW_OBS_U8 ? 1 : 4)) : nullptr;
        p.rewards = rewards + (int64_t)done * rewards_turn_stride;
        p.epoch = epoch; p.turn = turn; p.a0 = 0; p.a1 = A; p.flags = flags; p.do_move = 1;
        p.nturns = n; p.ts_obs = obs_turn_stride; p.ts_act = actions_turn_stride; p.ts_rew = rewards_turn_stride;
        if (int rc = launch_step(e, p, static_cast<hipStream_t>(stream))) return rc;
        done += n;
        if (e->auto_max_turns && first_turn + done - 1 == e->auto_max_turns) {
            // end of the epoch: keep the returns, reset for the next one; the caller's turn counter restarts at 1
            if (epoch + 1 >= (1u << 28)) return fail(SGW_EINVAL, "epoch must be < 2^28");
            if (e->episode_return)
                HIP_TRY(hipMemcpyAsync(e->episode_return, total_reward, sizeof(double) * (size_t)e->cfg.num_envs,
                                       hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
            if (int rc = launch_reset(e, grid, agent_pos, total_reward, epoch + 1, stream)) return rc;
            epoch += 1;
            first_turn = 1 - done;     // turn = first_turn + done continues at 1 (unsigned wrap-around is intended)
        }
    }
    return SGW_OK;
}

int sgw_capabilities(sgw_engine* e) {
    if (!e) return 0;
    int caps = 0;
    if (e->k_obs_rows.usable() && e->obs_format == SGW_OBS_F32) caps |= SGW_CAP_OBSERVE_ROWS;
    caps |= SGW_CAP_ACT;      // MovingAgent.act, TagAgent.act and CleanupAgent.act all have an sgw_act instance
    {   // sgw_turn_resolve: plain movers with impassable agent types, float32 windows
        bool ok = e->cfg.agent_rule == SGW_AGENT_RULE_MOVE && e->obs_format == SGW_OBS_F32 && e->cfg.num_agents <= 64;   // (the resolve kernel keeps an agent per lane)
        for (int a = 0; a < e->cfg.num_agents; ++a) ok = ok && !e->cfg.type_passable[e->cfg.agent_type[a]];
        ok = ok && !e->base.drawn_mask;   // (a drawn value: the commit of sgw_turn_resolve knows no turn -- such worlds take the sequential turn)
        ok = ok && !e->base.enc_counts;   // (bound encounter counts: a speculative pass replays acts and would count them more than once)
        if (ok) caps |= SGW_CAP_RESOLVE;
    }
    if (e->big) caps |= SGW_CAP_OBS_AGENT_MAJOR;
    // (round 6: also step_big<..., ROWS> and the chunk-staging twins, which write the bound row tail themselves; the whole-env instance has a TAIL twin)
    if (e->k_sweep_rows.usable() && e->obs_format == SGW_OBS_F32 &&
        (e->tail_kind == SGW_TAIL_NONE || !e->fast || e->sweep_rows_chunked || e->k_sweep_rows_tail.jit)) caps |= SGW_CAP_SWEEP_ROWS;
    return caps;
}

static int fill_rows(const sgw_engine* e, void* const* rows, int64_t env_stride, int a0, int a1, bool need_all, RowPtrs* rp, const char* who) {
    const sgw_config& c = e->cfg;
    const int64_t V = 2 * c.vision_radius + 1;
    if (!rows) return fail(SGW_EINVAL, "%s: rows is NULL", who);
    if (env_stride < (int64_t)c.num_channels * V * V) return fail(SGW_EINVAL, "%s: env_stride is smaller than one window", who);
    if (e->tail_kind != SGW_TAIL_NONE && env_stride < (int64_t)c.num_channels * V * V + e->tail_len)
        return fail(SGW_EINVAL, "%s: env_stride is smaller than one window + the bound row tail (%d elements)", who, e->tail_len);
    memset(rp, 0, sizeof(*rp));
    for (int a = a0; a < a1; ++a) {
        if (!rows[a] && need_all) return fail(SGW_EINVAL, "%s: rows[%d] is NULL", who, a);
        if (e->obs_format == SGW_OBS_F32 && (reinterpret_cast<uintptr_t>(rows[a]) & 3u))
            return fail(SGW_EINVAL, "%s: rows[%d] is not 4-byte aligned", who, a);
        rp->p[a] = rows[a];
    }
    rp->stride = env_stride;
    return SGW_OK;
}

static int observe_rows_impl(sgw_engine* e, const uint8_t* grid, const uint8_t* agent_pos, void* const* rows, int64_t env_stride,
                             int32_t agent_begin, int32_t agent_end, const TurnState* ts, void* stream) {
    if (!e || !grid || !agent_pos) return fail(SGW_EINVAL, "sgw_observe_rows: NULL argument");
    if (agent_begin < 0 || agent_end > e->cfg.num_agents || agent_begin >= agent_end)
        return fail(SGW_EINVAL, "sgw_observe_rows: agent range [%d, %d) invalid", agent_begin, agent_end);
    if (!(sgw_capabilities(e) & SGW_CAP_OBSERVE_ROWS))
        return fail(SGW_EINVAL, "sgw_observe_rows: no row-load instance for this world (one-hot float32 windows of plain movers only; "
                                "see sgw_capabilities) -- use sgw_observe");
    RowPtrs rp;
    if (int rc = fill_rows(e, rows, env_stride, agent_begin, agent_end, true, &rp, "sgw_observe_rows")) return rc;
    if (ts && e->turn_rows) {   // a recorded turn: the windows also go to the replay rows of the turn in flight
        rp.ts = ts;
        rp.dual = 1;
        rp.rows_mode2 = e->turn_rows_flat ? kRowsFlat : kRowsRun;
    }
    Params p = e->base;
    p.grid = const_cast<uint8_t*>(grid); p.pos = const_cast<uint8_t*>(agent_pos);
    p.a0 = agent_begin; p.a1 = agent_end; p.flags = 0; p.do_move = 0;
    p.agent_state = e->agent_state;
    p.tail_kind = e->tail_kind; p.tail_len = e->tail_len; p.tail_table = e->tail_table;
    if (p.tail_kind == SGW_TAIL_AGENT_IS_IT && !p.agent_state) return fail(SGW_EINVAL, "SGW_TAIL_AGENT_IS_IT needs sgw_bind_agent_state");
    {   // how the windows leave (phase.h, rows_emit)
        const int64_t N = (int64_t)p.C * p.VV;
        const int nA = agent_end - agent_begin;
        bool al16 = true, al8 = true, slots = env_stride == (int64_t)nA * N;     // slots: rows[a] = rows[a0] + (a - a0) * N, i.e. one [E][nA][N] tensor
        for (int a = agent_begin; a < agent_end; ++a) {
            const uintptr_t q = reinterpret_cast<uintptr_t>(rows[a]);
            al16 = al16 && (q & 15) == 0;
            al8 = al8 && (q & 7) == 0;
            slots = slots && q == reinterpret_cast<uintptr_t>(rows[agent_begin]) + (uintptr_t)(a - agent_begin) * N * 4;
        }
        p.rows_by_agent = 0;
        const bool pair_ok = al8 && (N & 1) == 0 && (env_stride & 1) == 0;
        if (slots && (reinterpret_cast<uintptr_t>(rows[agent_begin]) & 15) == 0) p.rows_mode = kRowsFlat;
        else if (env_stride == N && al16) { p.rows_mode = kRowsFlat; p.rows_by_agent = 1; }
        else p.rows_mode = kRowsRun;      // per window: aligned float4 runs, the ends element by element
        const int m = e->opt.rows_mode;   // test hook: force another emit (1 = single floats, 2 = float2 runs where legal, 3 = aligned runs)
        if (m == kRowsSingle || m == kRowsRun || (m == kRowsPair && pair_ok)) { p.rows_mode = m; p.rows_by_agent = 0; }
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = time_begin(e, s)) return rc;
    const int wpw = e->rows_wpb / 4;                                   // windows per wave
    const int64_t waves = p.rows_by_agent ? ceil_div(p.E, wpw) * (agent_end - agent_begin) : ceil_div(p.E * (agent_end - agent_begin), wpw);
    if (rp.dual && rp.rows_mode2 == kRowsFlat && !p.rows_by_agent) rp.rows_mode2 = kRowsRun;   // (flat second copies need a wave = consecutive envs of ONE agent)
    if (int rc = launch_kernel(e, e->k_obs_rows, (unsigned)ceil_div(waves, 4), kBlock, e->rows_lds, s, p, &rp)) return rc;
    return time_end(e, s);
}

int sgw_observe_rows(sgw_engine* e, const uint8_t* grid, const uint8_t* agent_pos, void* const* rows, int64_t env_stride,
                     int32_t agent_begin, int32_t agent_end, void* stream) {
    return observe_rows_impl(e, grid, agent_pos, rows, env_stride, agent_begin, agent_end, nullptr, stream);
}

int sgw_sweep_observe_rows(sgw_engine* e, uint8_t* grid, const uint8_t* agent_pos, void* const* rows, int64_t env_stride, uint32_t epoch,
                           uint32_t turn, uint32_t flags, void* stream) {
    if (!e || !grid || !agent_pos) return fail(SGW_EINVAL, "sgw_sweep_observe_rows: NULL argument");
    if (!(sgw_capabilities(e) & SGW_CAP_SWEEP_ROWS))
        return fail(SGW_EINVAL, "sgw_sweep_observe_rows: no fused instance for this world (see sgw_capabilities: SGW_CAP_SWEEP_ROWS) -- "
                                "sgw_step(sweep only) + sgw_observe_rows do the same in two launches");
    if (flags & ~(uint32_t)SGW_STEP_SWEEP) return fail(SGW_EINVAL, "sgw_sweep_observe_rows: flags may hold SGW_STEP_SWEEP only");
    if (epoch >= (1u << 28)) return fail(SGW_EINVAL, "epoch must be < 2^28");
    const int A = e->cfg.num_agents;
    if (env_stride != (int64_t)e->base.C * e->base.VV + e->tail_len)
        return fail(SGW_EINVAL, "sgw_sweep_observe_rows: env_stride must be exactly one window (C * V * V elements) + the bound row tail (%d)", e->tail_len);
    RowPtrs rp;
    if (int rc = fill_rows(e, rows, env_stride, 0, A, true, &rp, "sgw_sweep_observe_rows")) return rc;
    Params p = e->base;
    p.grid = grid; p.pos = const_cast<uint8_t*>(agent_pos);
    p.actions = nullptr; p.obs = nullptr; p.rewards = nullptr; p.total = nullptr;
    p.epoch = epoch; p.turn = turn; p.a0 = 0; p.a1 = A; p.flags = flags & SGW_STEP_SWEEP; p.do_move = 0;
    p.tail_kind = e->tail_kind; p.tail_len = e->tail_len; p.tail_table = e->tail_table;
    if (p.tail_kind == SGW_TAIL_AGENT_IS_IT && !e->agent_state) return fail(SGW_EINVAL, "SGW_TAIL_AGENT_IS_IT needs sgw_bind_agent_state");
    return launch_step(e, p, static_cast<hipStream_t>(stream), &rp);
}

static int act_impl(sgw_engine* e, uint8_t* grid, uint8_t* agent_pos, uint8_t* actions, void* const* rows, int64_t env_stride,
                    float* rewards, double* total_reward, int32_t agent, const void* agent_action, int32_t action_kind,
                    float* reward_row, int64_t* action_row, const TurnState* ts, void* stream, int dual = 0) {
    if (!e || !grid || !agent_pos || !actions || !rewards || !total_reward) return fail(SGW_EINVAL, "sgw_act: NULL argument");
    if (agent < 0 || agent >= e->cfg.num_agents) return fail(SGW_EINVAL, "sgw_act: agent %d out of range", agent);
    if (e->cfg.agent_rule == SGW_AGENT_RULE_TAG && !e->agent_state) return fail(SGW_EINVAL, "SGW_AGENT_RULE_TAG needs sgw_bind_agent_state");
    if (e->cfg.agent_rule == SGW_AGENT_RULE_CLEANUP && !e->agent_dir) return fail(SGW_EINVAL, "SGW_AGENT_RULE_CLEANUP needs sgw_bind_agent_dir");
    RowPtrs rp;
    memset(&rp, 0, sizeof(rp));
    if (rows)
        if (int rc = fill_rows(e, rows, env_stride, agent + 1, e->cfg.num_agents, false, &rp, "sgw_act")) return rc;
    if (agent_action && action_kind != SGW_ACT_U8 && action_kind != SGW_ACT_I32 && action_kind != SGW_ACT_I64 && action_kind != SGW_ACT_QF32)
        return fail(SGW_EINVAL, "sgw_act: unknown action_kind %d", action_kind);
    if (agent_action && action_kind == SGW_ACT_QF32 && (reinterpret_cast<uintptr_t>(agent_action) & 3))
        return fail(SGW_EINVAL, "sgw_act: SGW_ACT_QF32 action values must be 4-byte aligned");
    rp.agent_action = agent_action; rp.action_kind = action_kind; rp.reward_row = reward_row; rp.action_row = action_row;
    rp.ts = ts;
    rp.ets = ((agent_action && action_kind == SGW_ACT_QF32) || e->base.drawn_mask) ? e->d_turn : nullptr;   // (a drawn value is keyed by the turn in flight, too)
    rp.dual = (dual && ts && e->turn_rows) ? 1 : 0;
    Params p = e->base;
    p.grid = grid; p.pos = agent_pos; p.actions = actions; p.rewards = rewards; p.total = total_reward;
    p.a0 = agent; p.a1 = agent + 1; p.flags = SGW_STEP_NO_OBS; p.do_move = 1;
    p.agent_state = e->agent_state;
    p.state_at_pov = e->state_at_pov;
    p.agent_dir = e->agent_dir;
    p.obs_u8 = e->obs_format == SGW_OBS_U8 ? 1 : 0;
    p.tail_kind = rows ? e->tail_kind : SGW_TAIL_NONE; p.tail_len = e->tail_len; p.tail_table = e->tail_table;
    if (p.tail_kind != SGW_TAIL_NONE && env_stride < (int64_t)e->base.C * e->base.VV + e->tail_len) p.tail_kind = SGW_TAIL_NONE;   // (windows in the observation tensor: no room for tails)
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = time_begin(e, s)) return rc;
    const int A = e->cfg.num_agents;
    const bool wide = A > 8 && A <= 16 && (e->opt.act_lanes == 16 || (e->opt.act_lanes == 0 && p.E <= 32768));   // (two agents per lane pay off once the waves outnumber the SIMDs' slots: profiles/r04_act_probe.txt)
    const int G = A <= 16 ? (wide ? 16 : 8) : (A <= 32 ? 32 : 64);      // lanes per env; 9..16 agents: two per lane
    const unsigned blocks = (unsigned)ceil_div(p.E, 4 * (64 / G));
#define ACT_PICK(R, OH) (A <= 8 ? act_patch<8, 1, R, OH> : (A <= 16 ? (wide ? act_patch<16, 1, R, OH> : act_patch<8, 2, R, OH>) : (A <= 32 ? act_patch<32, 1, R, OH> : (A <= 64 ? act_patch<64, 1, R, OH> : act_patch<64, 2, R, OH>))))
#define ACT_RULE(OH) (e->cfg.agent_rule == SGW_AGENT_RULE_TAG ? ACT_PICK(SGW_AGENT_RULE_TAG, OH) \
                      : e->cfg.agent_rule == SGW_AGENT_RULE_CLEANUP ? ACT_PICK(SGW_AGENT_RULE_CLEANUP, OH) : ACT_PICK(SGW_AGENT_RULE_MOVE, OH))
    RowsFn fn = e->onehot ? ACT_RULE(true) : ACT_RULE(false);
#undef ACT_RULE
#undef ACT_PICK
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(kBlock), 0, s, p, rp);
    HIP_TRY(hipGetLastError());
    return time_end(e, s);
}

int sgw_act(sgw_engine* e, uint8_t* grid, uint8_t* agent_pos, uint8_t* actions, void* const* rows, int64_t env_stride,
            float* rewards, double* total_reward, int32_t agent, const void* agent_action, int32_t action_kind,
            float* reward_row, int64_t* action_row, void* stream) {
    return act_impl(e, grid, agent_pos, actions, rows, env_stride, rewards, total_reward, agent, agent_action, action_kind, reward_row,
                    action_row, nullptr, stream);
}

// ---- a whole policy turn as ONE submission (include/sgw.h: sgw_turn_*)
int sgw_turn_bind(sgw_engine* e, const sgw_turn_rows* rows) {
    if (!e) return fail(SGW_EINVAL, "sgw_turn_bind: NULL engine");
    // Only the ring fields (row ... row_elems: one contiguous range of TurnState) are written; epoch, turn and the exploration
    // thresholds are the stream-ordered kernels' (sgw_turn_set / sgw_turn_epsilon / sgw_turn_end) and are never read back or rewritten
    // here.  The call blocks: everything submitted before it -- on ANY stream, a recorded turn's side stream included -- has finished
    // when the rings change (until round 5 a read-modify-write of the whole struct on the null stream could overtake kernels in
    // flight on a non-blocking stream and write stale counters back).
    TurnState h;
    memset(&h, 0, sizeof(h));
    HIP_TRY(hipDeviceSynchronize());
    const int A = e->cfg.num_agents;
    const int64_t N = (int64_t)e->base.C * e->base.VV;
    for (int a = 0; a < SGW_MAX_AGENTS; ++a) {
        h.row[a] = h.cap[a] = h.step[a] = h.row_elems[a] = 0;
        h.states[a] = nullptr; h.rewards[a] = nullptr; h.actions[a] = nullptr; h.dones[a] = nullptr;
    }
    e->turn_rows = false;
    for (int a = 0; a < SGW_MAX_AGENTS; ++a) { e->turn_cap[a] = 0; e->turn_ring_cap[a] = 0; e->turn_row_bytes[a] = 0; e->turn_states[a] = nullptr; }
    if (rows) {
        for (int a = 0; a < A; ++a) {
            if (rows->capacity[a] <= 0) continue;
            if (rows->row[a] < 0 || rows->row[a] >= rows->capacity[a] || rows->step[a] < 1)
                return fail(SGW_EINVAL, "sgw_turn_bind: agent %d: row must be in [0, capacity) and step >= 1", a);
            if (rows->states[a] && rows->row_elems[a] < N) return fail(SGW_EINVAL, "sgw_turn_bind: agent %d: row_elems is smaller than one window", a);
            const int esz = e->obs_format == SGW_OBS_U8 ? 1 : 4;
            if (rows->states[a] && (reinterpret_cast<uintptr_t>(rows->states[a]) % esz)) return fail(SGW_EINVAL, "sgw_turn_bind: agent %d: states is misaligned", a);
            h.row[a] = rows->row[a]; h.cap[a] = rows->capacity[a]; h.step[a] = rows->step[a]; h.row_elems[a] = rows->row_elems[a];
            h.states[a] = rows->states[a]; h.rewards[a] = rows->rewards[a]; h.actions[a] = rows->actions[a];
            h.dones[a] = rows->states[a] ? rows->dones[a] : nullptr;   // (zeroed by the window copy)
            e->turn_ring_cap[a] = rows->capacity[a];
            if (rows->states[a]) {
                e->turn_cap[a] = rows->capacity[a];
                e->turn_row_bytes[a] = (int64_t)e->cfg.num_envs * rows->row_elems[a] * esz;
                e->turn_states[a] = rows->states[a];
            }
            if (!e->turn_rows) e->turn_rows_even = e->turn_rows_flat = true;
            e->turn_rows = true;
            if (rows->states[a] && ((reinterpret_cast<uintptr_t>(rows->states[a]) & 15) || rows->row_elems[a] != N || (((int64_t)e->cfg.num_envs * N * 4) & 15)))
                e->turn_rows_flat = false;
            if (rows->states[a] && ((reinterpret_cast<uintptr_t>(rows->states[a]) & 7) || (rows->row_elems[a] & 1))) e->turn_rows_even = false;
        }
    }
    constexpr size_t r0 = offsetof(TurnState, row), r1 = offsetof(TurnState, eps_thr);
    HIP_TRY(hipMemcpy(reinterpret_cast<char*>(e->d_turn) + r0, reinterpret_cast<const char*>(&h) + r0, r1 - r0, hipMemcpyHostToDevice));
    return SGW_OK;
}

int sgw_turn_set(sgw_engine* e, uint32_t epoch, uint32_t turn, void* stream) {
    if (!e) return fail(SGW_EINVAL, "sgw_turn_set: NULL engine");
    if (epoch >= (1u << 28)) return fail(SGW_EINVAL, "epoch must be < 2^28");
    hipLaunchKernelGGL(turn_set_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), e->d_turn, epoch, turn);
    HIP_TRY(hipGetLastError());
    return SGW_OK;
}

int sgw_turn_epsilon(sgw_engine* e, int32_t agent, double epsilon, void* stream) {
    if (!e) return fail(SGW_EINVAL, "sgw_turn_epsilon: NULL engine");
    if (agent < -1 || agent >= e->cfg.num_agents) return fail(SGW_EINVAL, "sgw_turn_epsilon: agent %d out of range", agent);
    if (!(epsilon >= 0.0 && epsilon <= 1.0)) return fail(SGW_EINVAL, "sgw_turn_epsilon: epsilon must be in [0, 1]");
    const double t = std::floor(epsilon * 4294967296.0);
    const uint64_t thr = t >= 4294967296.0 ? 4294967296ull : (uint64_t)t;
    hipLaunchKernelGGL(turn_epsilon_kernel, dim3(1), dim3(SGW_MAX_AGENTS), 0, static_cast<hipStream_t>(stream), e->d_turn, agent, e->cfg.num_agents, thr);
    HIP_TRY(hipGetLastError());
    return SGW_OK;
}

int sgw_turn_begin(sgw_engine* e, uint8_t* grid, uint8_t* agent_pos, uint8_t* actions, float* obs, float* rewards, double* total_reward,
                   uint32_t flags, void* stream) {
    if (!e || !grid || !agent_pos || !actions || !obs || !rewards || !total_reward) return fail(SGW_EINVAL, "sgw_turn_begin: NULL argument");
    if (flags & ~(SGW_STEP_SWEEP)) return fail(SGW_EINVAL, "sgw_turn_begin: only SGW_STEP_SWEEP may be set");
    hipStream_t s = static_cast<hipStream_t>(stream);
    Params p = e->base;
    p.grid = grid; p.pos = agent_pos; p.actions = actions; p.obs = obs; p.rewards = rewards; p.total = total_reward;
    p.ts = e->d_turn;      // the turn in flight = the device's count of completed turns + 1 (Environment.take_turn: self.turn += 1)
    p.a0 = 0; p.a1 = e->cfg.num_agents; p.flags = flags; p.do_move = 0;
    return launch_step(e, p, s);
}

int sgw_turn_act(sgw_engine* e, uint8_t* grid, uint8_t* agent_pos, uint8_t* actions, void* obs, float* rewards, double* total_reward,
                 int32_t agent, const void* agent_action, int32_t action_kind, void* stream) {
    if (!e || !obs) return fail(SGW_EINVAL, "sgw_turn_act: NULL argument");
    const int A = e->cfg.num_agents;
    const int64_t N = (int64_t)e->base.C * e->base.VV;
    const int esz = e->obs_format == SGW_OBS_U8 ? 1 : 4;
    void* rows[SGW_MAX_AGENTS];
    for (int a = 0; a < A; ++a) rows[a] = static_cast<uint8_t*>(obs) + (int64_t)a * N * esz;   // slot a of the [E][A][C][V][V] tensor
    return act_impl(e, grid, agent_pos, actions, rows, (int64_t)A * N, rewards, total_reward, agent, agent_action, action_kind, nullptr, nullptr,
                    e->d_turn, stream);
}

int sgw_turn_begin_rows(sgw_engine* e, uint8_t* grid, uint8_t* agent_pos, uint8_t* actions, float* rewards, double* total_reward,
                        void* const* rows, int64_t env_stride, uint32_t flags, void* stream) {
    if (!e || !grid || !agent_pos || !actions || !rewards || !total_reward || !rows) return fail(SGW_EINVAL, "sgw_turn_begin_rows: NULL argument");
    if (flags & ~(SGW_STEP_SWEEP)) return fail(SGW_EINVAL, "sgw_turn_begin_rows: only SGW_STEP_SWEEP may be set");
    if (!(sgw_capabilities(e) & SGW_CAP_OBSERVE_ROWS)) return fail(SGW_EINVAL, "sgw_turn_begin_rows needs SGW_CAP_OBSERVE_ROWS (one-hot float32 windows); use sgw_turn_begin");
    hipStream_t s = static_cast<hipStream_t>(stream);
    // both steps in one launch -- on the whole-env instance, whose emit also writes the recorded turn's second copy (the ring rows by the device's
    // row count); step_big, the chunk-staging and the generic instances (round 6) render into the rows alone, so a recorded turn keeps the two launches there
    if ((sgw_capabilities(e) & SGW_CAP_SWEEP_ROWS) && e->fast && !e->sweep_rows_chunked && e->tail_kind == SGW_TAIL_NONE &&
        env_stride == (int64_t)e->base.C * e->base.VV) {
        RowPtrs rp;
        if (int rc = fill_rows(e, rows, env_stride, 0, e->cfg.num_agents, true, &rp, "sgw_turn_begin_rows")) return rc;
        rp.ts = e->d_turn;
        rp.dual = e->turn_rows ? 1 : 0;
        Params p = e->base;
        p.grid = grid; p.pos = agent_pos; p.actions = nullptr; p.obs = nullptr; p.rewards = nullptr; p.total = nullptr;
        p.ts = e->d_turn;
        p.a0 = 0; p.a1 = e->cfg.num_agents; p.flags = flags & SGW_STEP_SWEEP; p.do_move = 0;
        return launch_step(e, p, s, &rp);
    }
    if (flags & SGW_STEP_SWEEP) {     // the entity sweep alone, at the device's turn
        Params p = e->base;
        p.grid = grid; p.pos = agent_pos; p.actions = actions; p.obs = nullptr; p.rewards = rewards; p.total = total_reward;
        p.ts = e->d_turn;
        p.a0 = 0; p.a1 = 0; p.flags = SGW_STEP_SWEEP | SGW_STEP_NO_OBS; p.do_move = 1;
        if (int rc = launch_step(e, p, s)) return rc;
    }
    return observe_rows_impl(e, grid, agent_pos, rows, env_stride, 0, e->cfg.num_agents, e->d_turn, stream);
}

int sgw_turn_act_rows(sgw_engine* e, uint8_t* grid, uint8_t* agent_pos, uint8_t* actions, void* const* rows, int64_t env_stride, float* rewards,
                      double* total_reward, int32_t agent, const void* agent_action, int32_t action_kind, void* stream) {
    if (!e || !rows) return fail(SGW_EINVAL, "sgw_turn_act_rows: NULL argument");
    return act_impl(e, grid, agent_pos, actions, rows, env_stride, rewards, total_reward, agent, agent_action, action_kind, nullptr, nullptr,
                    e->d_turn, stream, 1);
}

int sgw_turn_resolve(sgw_engine* e, uint8_t* grid, uint8_t* agent_pos, uint8_t* actions, float* rows, int64_t row_elems, float* rewards,
                     double* total_reward, uint8_t* scratch, int64_t* dirty_list, uint32_t* counters, const int64_t* new_actions,
                     int64_t n_new, float* reward_rows, int64_t* action_rows, int32_t pass, void* stream) {
    if (!e || !grid || !agent_pos || !actions || !rows || !rewards || !total_reward || !scratch)
        return fail(SGW_EINVAL, "sgw_turn_resolve: NULL argument");
    const sgw_config& c = e->cfg;
    if (c.agent_rule != SGW_AGENT_RULE_MOVE) return fail(SGW_EINVAL, "sgw_turn_resolve: plain movers only (SGW_AGENT_RULE_MOVE)");
    if (c.num_agents > 64) return fail(SGW_EINVAL, "sgw_turn_resolve: at most 64 agents (an agent per lane)");
    if (e->obs_format != SGW_OBS_F32) return fail(SGW_EINVAL, "sgw_turn_resolve: float32 windows only");
    for (int a = 0; a < c.num_agents; ++a)
        if (c.type_passable[c.agent_type[a]]) return fail(SGW_EINVAL, "sgw_turn_resolve: agent types must be impassable");
    if (row_elems < (int64_t)e->base.C * e->base.VV) return fail(SGW_EINVAL, "sgw_turn_resolve: row_elems is smaller than one window");
    if (reinterpret_cast<uintptr_t>(rows) & 3u) return fail(SGW_EINVAL, "sgw_turn_resolve: rows is not 4-byte aligned");
    if (pass < 0) return fail(SGW_EINVAL, "sgw_turn_resolve: pass must be 0 (render the pre-move windows) or the number of the pass, 1 ...");
    const int64_t EA = (int64_t)c.num_envs * c.num_agents;
    if ((dirty_list == nullptr) != (counters == nullptr)) return fail(SGW_EINVAL, "sgw_turn_resolve: dirty_list and counters come together");
    if (new_actions && (n_new < 0 || n_new > EA || (pass == 1 && n_new != EA) || pass == 0))
        return fail(SGW_EINVAL, "sgw_turn_resolve: new_actions holds every row's action in pass 1 (n_new = E * A), the previous pass's dirty rows' afterwards");
    if (new_actions && pass > 1 && !dirty_list) return fail(SGW_EINVAL, "sgw_turn_resolve: new_actions of a later pass follow the dirty list");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = time_begin(e, s)) return rc;
    if (pass == 1 && counters) HIP_TRY(hipMemsetAsync(counters, 0, 8 * sizeof(uint32_t), s));
    if (new_actions && n_new > 0) {      // the policy's output -> actions[env][agent]
        const int64_t* lst = pass == 1 ? nullptr : dirty_list + ((pass - 1) & 1) * EA;
        const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(n_new, kBlock), (int64_t)e->num_cus * 8);
        hipLaunchKernelGGL(resolve_apply_actions, dim3(blocks), dim3(kBlock), 0, s, actions, lst, new_actions, n_new, (int64_t)c.num_envs, c.num_agents);
    }
    Params p = e->base;
    p.grid = grid; p.pos = agent_pos; p.actions = actions; p.rewards = rewards; p.total = total_reward;
    p.a0 = 0; p.a1 = c.num_agents; p.do_move = 1; p.flags = 0;
    ResolveArgs ra;
    ra.rows = rows; ra.row_elems = row_elems;
    ra.env_done = scratch; ra.pristine = scratch + EA; ra.dirty = scratch + 2 * EA; ra.prev = scratch + 3 * EA;
    // the dirty list: appended with one atomic per env -- or, from 8 192 envs on (where those atomics on one counter would serialise for
    // hundreds of microseconds), laid out afterwards by a scan over per-env counts
    const bool scan = dirty_list && pass >= 1 && c.num_envs >= 8192;
    const int nb = (int)ceil_div(c.num_envs, 256);
    if (scan && (!e->d_dcount || !e->d_doffsets)) return fail(SGW_EINVAL, "sgw_turn_resolve: the scan buffers of this engine are missing");   // (sgw_create allocates both from 8 192 envs on)
    ra.list = (dirty_list && !scan) ? dirty_list + (pass & 1) * EA : nullptr;
    ra.count = (counters && !scan) ? counters + (pass & 7) : nullptr;
    ra.count_next = counters ? counters + ((pass + 1) & 7) : nullptr;
    ra.dcount = scan ? e->d_dcount : nullptr;
    ra.bsum = scan ? e->d_doffsets : nullptr;
    ra.reward_rows = reward_rows; ra.action_rows = action_rows;
    ra.first = pass == 0 ? 2 : (pass == 1 ? 1 : 0);
    ra.diag = e->opt.resolve_diag;
    // a workgroup per env (four waves share the windows to verify) from 16 agents on, a wave per env below
    const bool wide = c.num_agents >= 16;
    const unsigned blocks = (unsigned)(wide ? p.E : ceil_div(p.E, 4));
    const size_t tab = e->onehot ? (size_t)4 * SGW_MAX_TYPES * 4 : (size_t)SGW_MAX_TYPES * SGW_MAX_CHANNELS * 8;
    const size_t lds = 4 * tab + 64;
    if (e->onehot) {
        if (wide) hipLaunchKernelGGL((turn_resolve<true, 4>), dim3(blocks), dim3(kBlock), lds, s, p, ra);
        else hipLaunchKernelGGL((turn_resolve<true, 1>), dim3(blocks), dim3(kBlock), lds, s, p, ra);
    } else {
        if (wide) hipLaunchKernelGGL((turn_resolve<false, 4>), dim3(blocks), dim3(kBlock), lds, s, p, ra);
        else hipLaunchKernelGGL((turn_resolve<false, 1>), dim3(blocks), dim3(kBlock), lds, s, p, ra);
    }
    if (scan) {
        hipLaunchKernelGGL(resolve_scan_blocks, dim3(1), dim3(256), 0, s, e->d_doffsets, nb, e->d_doffsets + nb, counters + (pass & 7));
        hipLaunchKernelGGL(resolve_fill_list, dim3((unsigned)nb), dim3(256), 0, s, ra.dirty, e->d_dcount, ra.env_done, e->d_doffsets + nb,
                           (int64_t)c.num_envs, c.num_agents, dirty_list + (pass & 1) * EA);
    }
    HIP_TRY(hipGetLastError());
    return time_end(e, s);
}

int sgw_verify_rows(sgw_engine* e, const float* obs, const uint8_t* state_at_pov, float* rows, int64_t row_elems, int64_t* list, uint32_t* count, void* stream) {
    if (!e || !obs || !rows || !list || !count) return fail(SGW_EINVAL, "sgw_verify_rows: NULL argument");
    if (e->obs_format != SGW_OBS_F32) return fail(SGW_EINVAL, "sgw_verify_rows: float32 windows only");
    const int N = e->base.C * e->base.VV;
    const bool tail_it = e->tail_kind == SGW_TAIL_AGENT_IS_IT;
    if (row_elems < N + e->tail_len) return fail(SGW_EINVAL, "sgw_verify_rows: row_elems is smaller than one window + the bound row tail");
    if (tail_it && !state_at_pov) return fail(SGW_EINVAL, "sgw_verify_rows: SGW_TAIL_AGENT_IS_IT needs the scratch turn's state_at_pov");
    if ((reinterpret_cast<uintptr_t>(obs) | reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(count)) & 3u) return fail(SGW_EINVAL, "sgw_verify_rows: misaligned pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(count, 0, sizeof(uint32_t), s));
    const int64_t waves = (int64_t)e->cfg.num_envs * e->cfg.num_agents;
    hipLaunchKernelGGL(verify_rows_kernel, dim3((unsigned)ceil_div(waves, kBlock / 64)), dim3(kBlock), 0, s, obs, state_at_pov, rows, row_elems, N, (int64_t)e->cfg.num_envs,
                       e->cfg.num_agents, tail_it ? 1 : 0, (uint32_t)e->cfg.tag_it_type, list, count);
    HIP_TRY(hipGetLastError());
    return SGW_OK;
}

int sgw_apply_actions(sgw_engine* e, uint8_t* actions, const int64_t* list, const int64_t* new_actions, int64_t n, void* stream) {
    if (!e || !actions || !new_actions) return fail(SGW_EINVAL, "sgw_apply_actions: NULL argument");
    if (n < 0 || n > (int64_t)e->cfg.num_envs * e->cfg.num_agents) return fail(SGW_EINVAL, "sgw_apply_actions: n = %lld outside [0, E * A]", (long long)n);
    if (n == 0) return SGW_OK;
    const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(n, kBlock), (int64_t)e->num_cus * 8);
    hipLaunchKernelGGL(resolve_apply_actions, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), actions, list, new_actions, n, (int64_t)e->cfg.num_envs, e->cfg.num_agents);
    HIP_TRY(hipGetLastError());
    return SGW_OK;
}

int sgw_gather_rows(const float* src, int64_t row_elems, const int64_t* idx, int64_t n, float* dst, void* stream) {
    if (!src || !idx || !dst || row_elems < 1 || n < 0) return fail(SGW_EINVAL, "sgw_gather_rows: bad argument");
    if (n == 0) return SGW_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(n, kBlock / 64), 256 * 32);
    const bool v2 = (row_elems & 1) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 7) == 0;
    if (v2) hipLaunchKernelGGL(gather_rows_kernel<2>, dim3(blocks), dim3(kBlock), 0, s, src, row_elems, idx, n, dst);
    else hipLaunchKernelGGL(gather_rows_kernel<1>, dim3(blocks), dim3(kBlock), 0, s, src, row_elems, idx, n, dst);
    HIP_TRY(hipGetLastError());
    return SGW_OK;
}

// ---------------------------------------------------------------- sprite frames (render.h)
int sgw_render(const sgw_render_desc* d, void* stream) {
    if (!d) return fail(SGW_EINVAL, "sgw_render: desc is NULL");
    if (!d->grid || !d->atlas || !d->type_tile || !d->out) return fail(SGW_EINVAL, "sgw_render: grid, atlas, type_tile and out must not be NULL");
    if (d->num_envs < 1) return fail(SGW_EINVAL, "sgw_render: num_envs = %lld", (long long)d->num_envs);
    if (d->layers < 1 || d->layers > 8) return fail(SGW_EINVAL, "sgw_render: layers = %d outside 1..8", d->layers);
    if (d->height < 1 || d->height > 4096 || d->width < 1 || d->width > 4096)
        return fail(SGW_EINVAL, "sgw_render: map %d x %d outside 1..4096", d->height, d->width);
    if (d->th < 1 || d->th > 64 || d->tw < 1 || d->tw > 64) return fail(SGW_EINVAL, "sgw_render: tile %d x %d outside 1..64", d->th, d->tw);
    if (d->n_tiles < 1 || d->n_tiles > 65535) return fail(SGW_EINVAL, "sgw_render: n_tiles = %d outside 1..65535", d->n_tiles);
    if (d->oob_tile < 0 || d->oob_tile >= d->n_tiles) return fail(SGW_EINVAL, "sgw_render: oob_tile = %d is not a tile of the atlas", d->oob_tile);
    if (d->mode != SGW_RENDER_COMPOSITE && d->mode != SGW_RENDER_LAYERS) return fail(SGW_EINVAL, "sgw_render: unknown mode %d", d->mode);
    const int64_t cells = (int64_t)d->layers * d->height * d->width;
    const int64_t env_stride = d->grid_env_stride ? d->grid_env_stride : cells;
    if (env_stride < cells) return fail(SGW_EINVAL, "sgw_render: grid_env_stride is smaller than one env");
    if (d->agent_pos) {
        if (!d->agent_tile) return fail(SGW_EINVAL, "sgw_render: agent_pos without agent_tile");
        if (d->num_agents < 1) return fail(SGW_EINVAL, "sgw_render: num_agents = %d", d->num_agents);
        if (d->agent_layer < 0 || d->agent_layer >= d->layers) return fail(SGW_EINVAL, "sgw_render: agent_layer = %d outside the world's layers", d->agent_layer);
        if (d->height > 256 || d->width > 256) return fail(SGW_EINVAL, "sgw_render: agent positions are bytes: the map must be at most 256 x 256");
        if (reinterpret_cast<uintptr_t>(d->agent_tile) & 1) return fail(SGW_EINVAL, "sgw_render: agent_tile is not 2-byte aligned");
    }
    int64_t n = d->env_ids ? d->n : d->num_envs;
    if (n < 0) return fail(SGW_EINVAL, "sgw_render: n = %lld", (long long)n);
    int k = 1, rows = d->height, cols = d->width;
    if (d->centres) {
        if (d->k < 1) return fail(SGW_EINVAL, "sgw_render: k = %d windows per env", d->k);
        if (d->vision < 0 || d->vision > 511) return fail(SGW_EINVAL, "sgw_render: vision = %d outside 0..511", d->vision);
        k = d->k;
        rows = cols = 2 * d->vision + 1;
    }
    if (cols > kRenderMaxCols || (int64_t)d->layers * cols > kRenderMaxCells)
        return fail(SGW_EINVAL, "sgw_render: %d layers x %d columns: a tile row holds at most %d columns and layers * columns <= %d", d->layers, cols, kRenderMaxCols, kRenderMaxCells);
    const uintptr_t a_out = reinterpret_cast<uintptr_t>(d->out), a_atlas = reinterpret_cast<uintptr_t>(d->atlas);
    if ((a_out & 3) || (a_atlas & 3)) return fail(SGW_EINVAL, "sgw_render: out and atlas must be 4-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d->type_tile) & 1) || (reinterpret_cast<uintptr_t>(d->centres) & 1) || (reinterpret_cast<uintptr_t>(d->env_ids) & 7))
        return fail(SGW_EINVAL, "sgw_render: misaligned type_tile / centres / env_ids");
    if (n == 0) return SGW_OK;
    RenderParams p{};
    p.grid = d->grid; p.atlas = d->atlas; p.tile_flags = d->tile_flags; p.type_tile = d->type_tile;
    p.agent_pos = d->agent_pos; p.agent_tile = d->agent_tile; p.env_ids = d->env_ids; p.centres = d->centres; p.out = d->out;
    p.E = d->num_envs; p.n = n; p.env_stride = env_stride;
    p.L = d->layers; p.H = d->height; p.W = d->width; p.A = d->agent_pos ? d->num_agents : 0; p.agent_layer = d->agent_layer;
    p.n_tiles = d->n_tiles; p.th = d->th; p.tw = d->tw; p.k = k; p.vision = d->vision; p.oob_tile = d->oob_tile;
    p.per_layer = d->mode == SGW_RENDER_LAYERS;
    p.rows = rows; p.cols = cols;
    p.span_bytes = (int64_t)d->th * cols * d->tw * 4;
    p.tile_bytes = d->th * d->tw * 4;
    p.tile_pitch = p.tile_bytes + kRenderAtlasPad;
    const bool vec4 = (d->tw % 4) == 0 && !(a_out & 15) && !(a_atlas & 15);
    p.units_per_row = cols * d->tw / (vec4 ? 4 : 1);
    const bool lds_atlas = (int64_t)d->n_tiles * p.tile_pitch <= kRenderAtlasLds;
    const size_t lds = lds_atlas ? (size_t)d->n_tiles * p.tile_pitch : 0;
    static int cus[64] = {};
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || cus[dev] == 0) {
        int c = 0;
        HIP_TRY(hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev));
        if (c < 1) c = 256;
        if (dev >= 0 && dev < 64) cus[dev] = c;
        else cus[0] = cus[0] ? cus[0] : c, dev = 0;
    }
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (size_t)(160 * 1024) / (kRenderStaticLds + lds)));
    const int64_t resident = (int64_t)cus[dev] * per_cu;
    // tile rows per work item: as many as the cell table holds, halved while the launch has fewer than two items per resident workgroup
    int rpi = std::max(1, std::min(rows, kRenderMaxCells / (d->layers * cols)));
    while (rpi > 1 && n * k * ceil_div(rows, rpi) < 2 * resident) rpi = (rpi + 1) / 2;
    p.rpi = rpi;
    p.items_per_frame = (int)ceil_div(rows, rpi);
    p.items = n * k * p.items_per_frame;
    const unsigned blocks = (unsigned)std::min<int64_t>(p.items, resident);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec4) { if (lds_atlas) launch_render<4, true>(p, blocks, lds, s); else launch_render<4, false>(p, blocks, lds, s); }
    else { if (lds_atlas) launch_render<1, true>(p, blocks, lds, s); else launch_render<1, false>(p, blocks, lds, s); }
    HIP_TRY(hipGetLastError());
    return SGW_OK;
}

// ---------------------------------------------------------------- replay batches (sample.h)
static int sample_launch(const sgw_sample_desc* d, const sgw_learn_clock* clock, const char* who, void* stream) {
    if (!d->states || !d->actions || !d->rewards || !d->dones) return fail(SGW_EINVAL, "%s: states, actions, rewards and dones must not be NULL", who);
    if (!d->out_states || !d->out_next_states || !d->out_actions || !d->out_rewards || !d->out_dones || !d->out_valid)
        return fail(SGW_EINVAL, "%s: every output except out_index must not be NULL", who);
    if (d->n < 0) return fail(SGW_EINVAL, "%s: n = %lld", who, (long long)d->n);
    if (d->n_frames < 1) return fail(SGW_EINVAL, "%s: n_frames = %d", who, d->n_frames);
    if (d->row_elems < 1 || d->row_elems >= (1ll << 30)) return fail(SGW_EINVAL, "%s: row_elems = %lld outside [1, 2^30)", who, (long long)d->row_elems);   // (the kernels index a row's units in 32 bits, a piece past its end included)
    if (d->num_envs < 1 || d->num_envs >= (1ll << 31)) return fail(SGW_EINVAL, "%s: num_envs = %lld outside [1, 2^31)", who, (long long)d->num_envs);
    if (d->num_starts < 1 || d->num_starts >= (1ll << 31)) return fail(SGW_EINVAL, "%s: num_starts = %lld outside [1, 2^31)", who, (long long)d->num_starts);
    if (d->num_starts + d->n_frames > d->capacity)
        return fail(SGW_EINVAL, "%s: num_starts + n_frames = %lld exceeds the capacity %lld: the last row read must lie inside the ring", who, (long long)(d->num_starts + d->n_frames), (long long)d->capacity);
    if (!d->starts != !d->envs) return fail(SGW_EINVAL, "%s: starts and envs are both given or both NULL", who);
    if (d->src_type != SGW_SAMPLE_F32 && d->src_type != SGW_SAMPLE_U8) return fail(SGW_EINVAL, "%s: unknown src_type %d", who, d->src_type);
    if (d->act_type != SGW_SAMPLE_ACT_I64 && d->act_type != SGW_SAMPLE_ACT_U8) return fail(SGW_EINVAL, "%s: unknown act_type %d", who, d->act_type);
    const bool u8 = d->src_type == SGW_SAMPLE_U8;
    if (misaligned(3, {u8 ? nullptr : d->states, d->rewards, d->dones, d->out_states, d->out_next_states, d->out_rewards, d->out_dones, d->out_valid}))
        return fail(SGW_EINVAL, "%s: misaligned float32 pointer", who);
    if (misaligned(7, {d->act_type == SGW_SAMPLE_ACT_I64 ? d->actions : nullptr, d->starts, d->envs, d->draw_count, d->out_actions, d->out_index}))
        return fail(SGW_EINVAL, "%s: misaligned int64 pointer", who);
    if (d->n > INT64_MAX / ((int64_t)d->n_frames + 1) / d->row_elems) return fail(SGW_EINVAL, "%s: n = %lld: the batch does not fit 64-bit offsets", who, (long long)d->n);
    if (d->n == 0) return SGW_OK;
    SampleParams p{};
    p.states = d->states; p.actions = d->actions; p.rewards = d->rewards; p.dones = d->dones;
    p.starts = d->starts; p.envs = d->envs; p.draw_count = d->draw_count;
    p.out_states = d->out_states; p.out_next = d->out_next_states; p.out_actions = d->out_actions;
    p.out_rewards = d->out_rewards; p.out_dones = d->out_dones; p.out_valid = d->out_valid; p.out_index = d->out_index;
    p.n = d->n; p.num_envs = d->num_envs; p.num_starts = d->num_starts; p.R = d->row_elems;
    p.sts = d->state_turn_stride; p.ses = d->state_env_stride; p.scs = d->scalar_turn_stride; p.sce = d->scalar_env_stride;
    p.draw = d->draw; p.seed_lo = (uint32_t)d->seed; p.seed_hi = (uint32_t)(d->seed >> 32);
    p.F = d->n_frames; p.act_u8 = d->act_type == SGW_SAMPLE_ACT_U8;
    // 16 bytes per lane on the float32 side when every row -- source and destination -- starts on a 16-byte (uint8 source: 4-byte) boundary
    const uintptr_t src_mask = u8 ? 3 : 15;
    const int64_t src_elem = u8 ? 1 : 4;
    const bool vec4 = (d->row_elems % 4) == 0 && !(at(d->states) & src_mask) && ((d->state_turn_stride * src_elem) & (int64_t)src_mask) == 0 &&
                      ((d->state_env_stride * src_elem) & (int64_t)src_mask) == 0 && !((at(d->out_states) | at(d->out_next_states)) & 15);
    const int per_piece = 64 * (vec4 ? 4 * (kSamplePieces / 2) : kSamplePieces);
    p.pieces = (int)ceil_div(d->row_elems, (int64_t)per_piece);
    const int64_t items = d->n * ((int64_t)d->n_frames + 1);
    const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(items, kBlock / 64), kSampleMaxBlocks);
    const int64_t waves = (int64_t)blocks * (kBlock / 64);
    p.step_k = waves / (d->n_frames + 1);
    p.step_j = (int32_t)(waves % (d->n_frames + 1));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (clock) {
        if (vec4 && u8) LAUNCH_CLOCKED_TRY((sample_rows_clocked_kernel<4, true>), blocks, s, p, clock);
        else if (vec4) LAUNCH_CLOCKED_TRY((sample_rows_clocked_kernel<4, false>), blocks, s, p, clock);
        else if (u8) LAUNCH_CLOCKED_TRY((sample_rows_clocked_kernel<1, true>), blocks, s, p, clock);
        else LAUNCH_CLOCKED_TRY((sample_rows_clocked_kernel<1, false>), blocks, s, p, clock);
    }
    else if (vec4 && u8) LAUNCH_TRY((sample_rows_kernel<4, true>), blocks, s, p);
    else if (vec4) LAUNCH_TRY((sample_rows_kernel<4, false>), blocks, s, p);
    else if (u8) LAUNCH_TRY((sample_rows_kernel<1, true>), blocks, s, p);
    else LAUNCH_TRY((sample_rows_kernel<1, false>), blocks, s, p);
    if (!d->starts && d->draw_count) {
        hipLaunchKernelGGL(sample_count_kernel, dim3(1), dim3(64), 0, s, d->draw_count);
        HIP_TRY(hipGetLastError());
    }
    return SGW_OK;
}

int sgw_sample(const sgw_sample_desc* d, void* stream) {
    if (!d) return fail(SGW_EINVAL, "sgw_sample: desc is NULL");
    return sample_launch(d, nullptr, "sgw_sample", stream);
}

// ---------------------------------------------------------------- the learner clock (learn_clock.h)
// SGW_OK, or the refusal of a clock that is missing or not 8-byte aligned
static int clock_refused(const char* who, const sgw_learn_clock* clock) {
    if (!clock) return fail(SGW_EINVAL, "%s: clock is NULL", who);
    if (misaligned(7, {clock})) return fail(SGW_EINVAL, "%s: misaligned clock (a device address that is a multiple of 8)", who);
    return SGW_OK;
}

int sgw_sample_clocked(const sgw_sample_desc* d, const sgw_learn_clock* clock, void* stream) {
    const char* who = "sgw_sample_clocked";
    if (!d) return fail(SGW_EINVAL, "%s: desc is NULL", who);
    if (int rc = clock_refused(who, clock)) return rc;
    if (d->starts || d->envs) return fail(SGW_EINVAL, "%s: starts and envs must be NULL (the clock bounds drawn indices; given ones take sgw_sample)", who);
    return sample_launch(d, clock, who, stream);
}

int sgw_learn_clock_advance(sgw_learn_clock* clock, void* stream) {
    if (int rc = clock_refused("sgw_learn_clock_advance", clock)) return rc;
    hipLaunchKernelGGL(learn_clock_advance_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), clock);
    HIP_TRY(hipGetLastError());
    return SGW_OK;
}

// ---------------------------------------------------------------- discounted returns (returns.h)
int64_t sgw_returns_workspace_bytes(int64_t count, int64_t cols) {
    if (count < 0) return fail(SGW_EINVAL, "sgw_returns_workspace_bytes: count = %lld", (long long)count);
    if (cols < 1 || cols >= (1ll << 31)) return fail(SGW_EINVAL, "sgw_returns_workspace_bytes: cols = %lld outside [1, 2^31)", (long long)cols);
    return count == 0 ? 0 : returns_blocks(cols) * 3 * (int64_t)sizeof(double);
}

int sgw_returns(const sgw_returns_desc* d, void* stream) {
    if (!d) return fail(SGW_EINVAL, "sgw_returns: desc is NULL");
    if (!d->rewards || !d->dones || !d->out_returns) return fail(SGW_EINVAL, "sgw_returns: rewards, dones and out_returns must not be NULL");
    if (d->normalize != SGW_RETURNS_NORM_NONE && d->normalize != SGW_RETURNS_NORM_COLUMN && d->normalize != SGW_RETURNS_NORM_ALL)
        return fail(SGW_EINVAL, "sgw_returns: unknown normalize %d", d->normalize);
    if (d->out_type != SGW_RETURNS_OUT_F64 && d->out_type != SGW_RETURNS_OUT_F32) return fail(SGW_EINVAL, "sgw_returns: unknown out_type %d", d->out_type);
    if (d->reserved0 || d->reserved1) return fail(SGW_EINVAL, "sgw_returns: reserved fields must be 0");
    const bool norm = d->normalize != SGW_RETURNS_NORM_NONE, out32 = d->out_type == SGW_RETURNS_OUT_F32;
    if (norm && !d->out_normalized) return fail(SGW_EINVAL, "sgw_returns: normalize = %d needs out_normalized", d->normalize);
    if (d->capacity < 1) return fail(SGW_EINVAL, "sgw_returns: capacity = %lld", (long long)d->capacity);
    if (d->count < 0 || d->count > d->capacity) return fail(SGW_EINVAL, "sgw_returns: count = %lld outside [0, capacity = %lld]", (long long)d->count, (long long)d->capacity);
    if (d->first < 0 || d->first >= d->capacity) return fail(SGW_EINVAL, "sgw_returns: first = %lld outside [0, capacity = %lld)", (long long)d->first, (long long)d->capacity);
    if (d->cols < 1 || d->cols >= (1ll << 31)) return fail(SGW_EINVAL, "sgw_returns: cols = %lld outside [1, 2^31)", (long long)d->cols);
    if (d->turn_stride < 1 || d->col_stride < 1) return fail(SGW_EINVAL, "sgw_returns: turn_stride = %lld, col_stride = %lld: strides must be at least 1", (long long)d->turn_stride, (long long)d->col_stride);
    if (misaligned(3, {d->rewards, d->dones, d->out_returns, out32 ? d->out_normalized : nullptr})) return fail(SGW_EINVAL, "sgw_returns: misaligned float32 pointer");
    if (misaligned(7, {out32 ? nullptr : d->out_normalized, d->out_stats, d->workspace})) return fail(SGW_EINVAL, "sgw_returns: misaligned float64 pointer");
    // the largest element offset read, capacity * turn_stride + cols * col_stride, and the largest byte offset written, 8 * count * cols
    if (d->capacity > INT64_MAX / 2 / d->turn_stride || d->cols > INT64_MAX / 2 / d->col_stride || d->count > INT64_MAX / 16 / d->cols)
        return fail(SGW_EINVAL, "sgw_returns: capacity = %lld, cols = %lld with strides %lld / %lld do not fit 64-bit offsets", (long long)d->capacity, (long long)d->cols, (long long)d->turn_stride, (long long)d->col_stride);
    const unsigned blocks = (unsigned)returns_blocks(d->cols);
    if (d->normalize == SGW_RETURNS_NORM_ALL)
        if (int rc = workspace_short("sgw_returns", d->workspace, d->workspace_bytes, (int64_t)blocks * 3 * (int64_t)sizeof(double), " SGW_RETURNS_NORM_ALL")) return rc;
    if (d->count == 0) return SGW_OK;
    ReturnsParams p{};
    p.rewards = d->rewards; p.dones = d->dones; p.out_returns = d->out_returns; p.out_norm = d->out_normalized; p.out_stats = d->out_stats;
    p.partials = static_cast<double*>(d->workspace);
    p.first = d->first; p.count = d->count; p.capacity = d->capacity; p.cols = d->cols; p.ts = d->turn_stride; p.cs = d->col_stride;
    p.tiles = ceil_div(d->cols, kBlock);
    p.gamma = (float)d->gamma;                  // round to nearest even: what NumPy does with a Python float next to float32 data
    p.nparts = (int32_t)blocks;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (d->normalize == SGW_RETURNS_NORM_NONE) launch_returns<SGW_RETURNS_NORM_NONE>(p, false, blocks, s);
    else if (d->normalize == SGW_RETURNS_NORM_COLUMN) launch_returns<SGW_RETURNS_NORM_COLUMN>(p, out32, blocks, s);
    else launch_returns<SGW_RETURNS_NORM_ALL>(p, false, blocks, s);
    HIP_TRY(hipGetLastError());
    if (d->normalize == SGW_RETURNS_NORM_ALL) {
        const unsigned nblocks = (unsigned)std::min<int64_t>(ceil_div(d->count * d->cols, kBlock * 4), kReturnsMaxBlocks);
        if (out32) LAUNCH_TRY(returns_normalize_all_kernel<true>, nblocks, s, p);
        else LAUNCH_TRY(returns_normalize_all_kernel<false>, nblocks, s, p);
    }
    return SGW_OK;
}

// ---------------------------------------------------------------- stochastic policies (policy.h)
static int policy_launch(const sgw_policy_desc* d, const TurnState* ts, const char* who, void* stream) {
    if (!d->dist || !d->out_actions) return fail(SGW_EINVAL, "%s: dist and out_actions must not be NULL", who);
    if (d->n < 0) return fail(SGW_EINVAL, "%s: n = %lld", who, (long long)d->n);
    if (d->num_actions < 1 || d->num_actions > kPolicyMaxActions) return fail(SGW_EINVAL, "%s: num_actions = %d outside [1, %d]", who, d->num_actions, kPolicyMaxActions);
    if (d->num_envs < 1) return fail(SGW_EINVAL, "%s: num_envs = %lld", who, (long long)d->num_envs);
    if (d->row_stride < d->num_actions) return fail(SGW_EINVAL, "%s: row_stride = %lld is smaller than num_actions = %d", who, (long long)d->row_stride, d->num_actions);
    if (!is_float_type(d->dist_type)) return fail(SGW_EINVAL, "%s: unknown dist_type %d", who, d->dist_type);
    if (d->mode != SGW_POLICY_PROBS && d->mode != SGW_POLICY_LOGITS) return fail(SGW_EINVAL, "%s: unknown mode %d", who, d->mode);
    if (d->reserved0 || d->reserved1) return fail(SGW_EINVAL, "%s: reserved fields must be 0", who);
    if (d->epoch >= (1u << 28)) return fail(SGW_EINVAL, "%s: epoch must be < 2^28", who);
    if (!d->idx)
        if (int rc = keyed_agents_check(who, d->agent0, d->n, d->num_envs)) return rc;
    const bool f64 = d->dist_type == SGW_POLICY_F64;
    const int64_t esz = f64 ? 8 : 4;
    if (misaligned(float_mask(d->dist_type), {d->dist})) return fail(SGW_EINVAL, "%s: dist is not aligned to its element type", who);
    if (misaligned(3, {d->out_log_probs, d->out_entropy})) return fail(SGW_EINVAL, "%s: misaligned float32 pointer", who);
    if (misaligned(7, {d->out_actions, d->idx})) return fail(SGW_EINVAL, "%s: misaligned int64 pointer", who);
    if (d->n > INT64_MAX / 8 / d->row_stride) return fail(SGW_EINVAL, "%s: n = %lld rows of stride %lld do not fit 64-bit offsets", who, (long long)d->n, (long long)d->row_stride);
    if (d->n == 0) return SGW_OK;
    PolicyParams p{};
    p.dist = d->dist; p.idx = d->idx; p.out_actions = d->out_actions; p.out_log_probs = d->out_log_probs; p.out_entropy = d->out_entropy;
    p.ts = ts;
    p.n = d->n; p.num_envs = d->num_envs; p.stride = d->row_stride; p.tiles = ceil_div(d->n, kBlock);
    p.nact = d->num_actions; p.agent0 = d->agent0; p.mode = d->mode;
    p.seed_lo = (uint32_t)d->seed; p.seed_hi = (uint32_t)(d->seed >> 32); p.first_env = (uint32_t)d->first_env;
    p.epoch = d->epoch; p.turn = d->turn;
    // 16 bytes per load where every row starts on a 16-byte boundary and is whole 16-byte pieces (nothing behind a row is read)
    const bool vec = d->num_actions <= 16 && !(at(d->dist) & 15) && ((d->row_stride * esz) & 15) == 0 && ((d->num_actions * esz) & 15) == 0;
    const unsigned blocks = (unsigned)std::min<int64_t>(p.tiles, kPolicyMaxBlocks);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (f64) launch_policy<true>(p, vec, blocks, s);
    else launch_policy<false>(p, vec, blocks, s);
    HIP_TRY(hipGetLastError());
    return SGW_OK;
}

int sgw_policy_sample(const sgw_policy_desc* d, void* stream) {
    if (!d) return fail(SGW_EINVAL, "sgw_policy_sample: desc is NULL");
    return policy_launch(d, nullptr, "sgw_policy_sample", stream);
}

int sgw_turn_policy_sample(sgw_engine* e, int32_t agent, const void* dist, int32_t dist_type, int32_t mode, int64_t* out_actions,
                           float* log_prob_ring, float* out_entropy, void* stream) {
    if (!e) return fail(SGW_EINVAL, "sgw_turn_policy_sample: NULL engine");
    if (agent < 0 || agent >= e->cfg.num_agents) return fail(SGW_EINVAL, "sgw_turn_policy_sample: agent %d out of range", agent);
    if (log_prob_ring && e->turn_ring_cap[agent] <= 0)
        return fail(SGW_EINVAL, "sgw_turn_policy_sample: agent %d has no replay rows bound (sgw_turn_bind): which row of the ring the turn fills is unknown", agent);
    sgw_policy_desc d;
    memset(&d, 0, sizeof(d));
    d.dist = dist; d.out_actions = out_actions; d.out_log_probs = log_prob_ring; d.out_entropy = out_entropy;
    d.n = d.num_envs = e->cfg.num_envs; d.row_stride = d.num_actions = e->cfg.num_actions;
    d.seed = e->cfg.seed; d.first_env = e->cfg.first_env_id;
    d.agent0 = agent; d.dist_type = dist_type; d.mode = mode;
    return policy_launch(&d, e->d_turn, "sgw_turn_policy_sample", stream);
}

// ---------------------------------------------------------------- PPO's clipped loss (ppo_loss.h)
int64_t sgw_ppo_loss_workspace_bytes(int64_t n) {
    if (n < 0 || n > INT64_MAX / 32) return fail(SGW_EINVAL, "sgw_ppo_loss_workspace_bytes: n = %lld outside [0, 2^58)", (long long)n);
    return ppo_loss_blocks(n) * 3 * (int64_t)sizeof(double);
}

int sgw_ppo_loss(const sgw_ppo_loss_desc* d, void* stream) {
    if (!d) return fail(SGW_EINVAL, "sgw_ppo_loss: desc is NULL");
    if (!d->dist || !d->values || !d->actions || !d->old_log_probs || !d->returns || !d->out_terms)
        return fail(SGW_EINVAL, "sgw_ppo_loss: dist, values, actions, old_log_probs, returns and out_terms must not be NULL");
    if (d->n < 0) return fail(SGW_EINVAL, "sgw_ppo_loss: n = %lld", (long long)d->n);
    if (d->num_actions < 1 || d->num_actions > kPpoMaxActions) return fail(SGW_EINVAL, "sgw_ppo_loss: num_actions = %d outside [1, %d]", d->num_actions, kPpoMaxActions);
    if (d->row_stride < d->num_actions) return fail(SGW_EINVAL, "sgw_ppo_loss: row_stride = %lld is smaller than num_actions = %d", (long long)d->row_stride, d->num_actions);
    if (!is_float_type(d->dist_type)) return fail(SGW_EINVAL, "sgw_ppo_loss: unknown dist_type %d", d->dist_type);
    if (d->mode != SGW_POLICY_PROBS && d->mode != SGW_POLICY_LOGITS) return fail(SGW_EINVAL, "sgw_ppo_loss: unknown mode %d", d->mode);
    if (!is_float_type(d->value_type)) return fail(SGW_EINVAL, "sgw_ppo_loss: unknown value_type %d", d->value_type);
    if (d->action_type != SGW_PPO_ACT_I64 && d->action_type != SGW_PPO_ACT_U8) return fail(SGW_EINVAL, "sgw_ppo_loss: unknown action_type %d", d->action_type);
    if (!is_float_type(d->returns_type)) return fail(SGW_EINVAL, "sgw_ppo_loss: unknown returns_type %d", d->returns_type);
    if (d->reserved0 || d->reserved1) return fail(SGW_EINVAL, "sgw_ppo_loss: reserved fields must be 0");
    if (!(d->eps_clip >= 0.0) || !std::isfinite(d->eps_clip)) return fail(SGW_EINVAL, "sgw_ppo_loss: eps_clip = %g must be finite and not negative", d->eps_clip);
    if (misaligned(float_mask(d->dist_type), {d->dist, d->out_grad_dist})) return fail(SGW_EINVAL, "sgw_ppo_loss: dist / out_grad_dist is not aligned to its element type");
    if (misaligned(float_mask(d->value_type), {d->values, d->out_grad_values})) return fail(SGW_EINVAL, "sgw_ppo_loss: values / out_grad_values is not aligned to its element type");
    if (misaligned(float_mask(d->returns_type), {d->returns})) return fail(SGW_EINVAL, "sgw_ppo_loss: returns is not aligned to its element type");
    if (misaligned(3, {d->old_log_probs})) return fail(SGW_EINVAL, "sgw_ppo_loss: misaligned float32 pointer (old_log_probs)");
    if (d->action_type == SGW_PPO_ACT_I64 && misaligned(7, {d->actions})) return fail(SGW_EINVAL, "sgw_ppo_loss: misaligned int64 pointer (actions)");
    if (misaligned(7, {d->out_row_terms, d->out_terms, d->workspace})) return fail(SGW_EINVAL, "sgw_ppo_loss: misaligned float64 pointer (out_row_terms, out_terms or workspace)");
    if (d->n > INT64_MAX / 8 / d->row_stride || d->n > INT64_MAX / 32) return fail(SGW_EINVAL, "sgw_ppo_loss: n = %lld rows of stride %lld do not fit 64-bit offsets", (long long)d->n, (long long)d->row_stride);
    const unsigned blocks = (unsigned)ppo_loss_blocks(d->n);
    if (int rc = workspace_short("sgw_ppo_loss", d->workspace, d->workspace_bytes, (int64_t)blocks * 3 * (int64_t)sizeof(double))) return rc;
    if (d->n == 0) return SGW_OK;
    PpoLossParams p{};
    p.dist = d->dist; p.values = d->values; p.actions = d->actions; p.old_lp = d->old_log_probs; p.returns = d->returns;
    p.g_dist = d->out_grad_dist; p.g_values = d->out_grad_values; p.row_terms = d->out_row_terms; p.out_terms = d->out_terms;
    p.partials = static_cast<double*>(d->workspace);
    p.n = d->n; p.stride = d->row_stride; p.tiles = ceil_div(d->n, kBlock);
    p.lo = 1.0 - d->eps_clip; p.hi = 1.0 + d->eps_clip; p.c = d->entropy_coef; p.vc = d->value_coef;
    p.nact = d->num_actions; p.mode = d->mode; p.vtype = d->value_type; p.atype = d->action_type; p.rtype = d->returns_type;
    p.nparts = (int32_t)blocks;
    const bool f64 = d->dist_type == SGW_POLICY_F64;
    const int64_t esz = f64 ? 8 : 4;
    // 16 bytes per access where every row of dist AND of its gradient starts on a 16-byte boundary and is whole 16-byte pieces
    const bool vec = d->num_actions <= 16 && !((at(d->dist) | at(d->out_grad_dist)) & 15) && ((d->row_stride * esz) & 15) == 0 && ((d->num_actions * esz) & 15) == 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (f64) launch_ppo_loss<true>(p, vec, blocks, s);
    else launch_ppo_loss<false>(p, vec, blocks, s);
    HIP_TRY(hipGetLastError());
    LAUNCH_TRY(ppo_loss_merge_kernel, 1, s, p);
    return SGW_OK;
}

// ---------------------------------------------------------------- IQN's quantile Huber loss (iqn_loss.h)
int64_t sgw_iqn_loss_workspace_bytes(int64_t n, int32_t num_quantiles) {
    if (n < 0 || n > INT64_MAX / 32) return fail(SGW_EINVAL, "sgw_iqn_loss_workspace_bytes: n = %lld outside [0, 2^58)", (long long)n);
    if (num_quantiles < 1 || num_quantiles > kIqnMaxQuantiles) return fail(SGW_EINVAL, "sgw_iqn_loss_workspace_bytes: num_quantiles = %d outside [1, %d]", num_quantiles, kIqnMaxQuantiles);
    return iqn_loss_blocks(n, num_quantiles) * (int64_t)sizeof(double);
}

int sgw_iqn_loss(const sgw_iqn_loss_desc* d, void* stream) {
    if (!d) return fail(SGW_EINVAL, "sgw_iqn_loss: desc is NULL");
    if (!d->q_next_local || !d->q_next_target || !d->q_expected || !d->taus || !d->actions || !d->rewards || !d->dones || !d->valid || !d->out_terms)
        return fail(SGW_EINVAL, "sgw_iqn_loss: q_next_local, q_next_target, q_expected, taus, actions, rewards, dones, valid and out_terms must not be NULL");
    if (d->n < 0) return fail(SGW_EINVAL, "sgw_iqn_loss: n = %lld", (long long)d->n);
    if (d->num_quantiles < 1 || d->num_quantiles > kIqnMaxQuantiles) return fail(SGW_EINVAL, "sgw_iqn_loss: num_quantiles = %d outside [1, %d]", d->num_quantiles, kIqnMaxQuantiles);
    if (d->num_actions < 1 || d->num_actions > kIqnMaxActions) return fail(SGW_EINVAL, "sgw_iqn_loss: num_actions = %d outside [1, %d]", d->num_actions, kIqnMaxActions);
    if (d->action_type != SGW_PPO_ACT_I64 && d->action_type != SGW_PPO_ACT_U8) return fail(SGW_EINVAL, "sgw_iqn_loss: unknown action_type %d", d->action_type);
    if (!is_float_type(d->valid_type)) return fail(SGW_EINVAL, "sgw_iqn_loss: unknown valid_type %d", d->valid_type);
    if (d->reserved0 || d->reserved1) return fail(SGW_EINVAL, "sgw_iqn_loss: reserved fields must be 0");
    if (!std::isfinite(d->discount)) return fail(SGW_EINVAL, "sgw_iqn_loss: discount = %g must be finite", d->discount);
    if (misaligned(3, {d->q_next_local, d->q_next_target, d->q_expected, d->taus, d->rewards, d->dones, d->out_grad_expected, d->out_td_error}))
        return fail(SGW_EINVAL, "sgw_iqn_loss: misaligned float32 pointer (q_next_local, q_next_target, q_expected, taus, rewards, dones, out_grad_expected or out_td_error)");
    if (d->action_type == SGW_PPO_ACT_I64 && misaligned(7, {d->actions})) return fail(SGW_EINVAL, "sgw_iqn_loss: misaligned int64 pointer (actions)");
    if (misaligned(float_mask(d->valid_type), {d->valid})) return fail(SGW_EINVAL, "sgw_iqn_loss: valid is not aligned to its element type");
    if (misaligned(7, {d->out_terms, d->out_next_actions, d->out_row_terms, d->workspace}))
        return fail(SGW_EINVAL, "sgw_iqn_loss: misaligned 8-byte pointer (out_terms, out_next_actions, out_row_terms or workspace)");
    const int64_t widest = (int64_t)d->num_quantiles * std::max(d->num_actions, d->num_quantiles);
    if (d->n > INT64_MAX / 8 / widest || d->n > INT64_MAX / 32)
        return fail(SGW_EINVAL, "sgw_iqn_loss: n = %lld rows of %d x %d do not fit 64-bit offsets", (long long)d->n, d->num_quantiles, d->num_actions);
    const unsigned blocks = (unsigned)iqn_loss_blocks(d->n, d->num_quantiles);
    if (int rc = workspace_short("sgw_iqn_loss", d->workspace, d->workspace_bytes, (int64_t)blocks * (int64_t)sizeof(double))) return rc;
    if (d->n == 0) return SGW_OK;
    IqnLossParams p{};
    p.q_next_local = d->q_next_local; p.q_next_target = d->q_next_target; p.q_expected = d->q_expected; p.taus = d->taus;
    p.actions = d->actions; p.rewards = d->rewards; p.dones = d->dones; p.valid = d->valid;
    p.grad = d->out_grad_expected; p.next_actions = d->out_next_actions; p.row_terms = d->out_row_terms; p.td_error = d->out_td_error;
    p.out_terms = d->out_terms; p.partials = static_cast<double*>(d->workspace);
    p.n = d->n; p.tiles = iqn_loss_tiles(d->n, d->num_quantiles);
    p.count = (double)(d->n * d->num_quantiles * d->num_quantiles);
    p.inv = 1.0 / p.count;
    p.discount = (float)d->discount;
    p.N = d->num_quantiles; p.A = d->num_actions; p.atype = d->action_type; p.vtype = d->valid_type; p.nparts = (int32_t)blocks;
    // 16 bytes per gradient store where a quad of actions lies inside one quantile's and every row starts on a 16-byte boundary
    const bool vec = d->out_grad_expected && (d->num_actions & 3) == 0 && !(at(d->out_grad_expected) & 15);
    hipStream_t s = static_cast<hipStream_t>(stream);
    launch_iqn_loss(p, vec, blocks, s);
    HIP_TRY(hipGetLastError());
    LAUNCH_TRY(iqn_loss_merge_kernel, 1, s, p);
    return SGW_OK;
}

// ---------------------------------------------------------------- IQN's network forward (iqn_forward.h)
int64_t sgw_iqn_forward_workspace_bytes(int64_t n, int32_t layer_size) {
    if (n < 0 || n > INT64_MAX / 4096) return fail(SGW_EINVAL, "sgw_iqn_forward_workspace_bytes: n = %lld outside [0, 2^51)", (long long)n);
    if (layer_size < 1 || layer_size > kFwdMaxL) return fail(SGW_EINVAL, "sgw_iqn_forward_workspace_bytes: layer_size = %d outside [1, %d]", layer_size, kFwdMaxL);
    return n * layer_size * (int64_t)sizeof(float);
}

static int iqn_forward_launch(const sgw_iqn_forward_desc* d, const TurnState* ts, const char* who, void* stream, const sgw_learn_clock* clock = nullptr) {
    if (int rc = iqn_network_check(d, who, 63)) return rc;
    if (!d->out_qvalues && !d->out_quantiles) return fail(SGW_EINVAL, "%s: one of out_qvalues and out_quantiles must be given", who);
    if (!d->taus) {                           // the draw's key
        if (d->num_envs < 1) return fail(SGW_EINVAL, "%s: num_envs = %lld", who, (long long)d->num_envs);
        if (d->epoch >= (1u << 28)) return fail(SGW_EINVAL, "%s: epoch must be < 2^28", who);
        if (!d->idx)
            if (int rc = keyed_agents_check(who, d->agent0, d->n, d->num_envs)) return rc;
    }
    if (misaligned(3, {d->taus, d->out_qvalues, d->out_quantiles, d->out_taus, d->out_cos, d->workspace}))
        return fail(SGW_EINVAL, "%s: misaligned float32 pointer (taus, an output or the workspace)", who);
    if (misaligned(7, {d->idx})) return fail(SGW_EINVAL, "%s: misaligned int64 pointer (idx)", who);
    // the other large byte offsets: 4 n N max(64, A) (out_cos, out_quantiles), 4 n L (the workspace)
    if (d->n > INT64_MAX / 8 / ((int64_t)kFwdM * kFwdMaxL))
        return fail(SGW_EINVAL, "%s: n = %lld rows do not fit 64-bit offsets", who, (long long)d->n);
    if (int rc = workspace_short(who, d->workspace, d->workspace_bytes, d->n * d->layer_size * (int64_t)sizeof(float))) return rc;
    if (d->n == 0) return SGW_OK;
    IqnFwdParams p{};
    iqn_network_fill(p, d);
    p.idx = d->idx;
    p.out_q = d->out_qvalues; p.out_quant = d->out_quantiles; p.out_taus = d->out_taus; p.out_cos = d->out_cos;
    p.h = static_cast<float*>(d->workspace);
    p.ts = ts;
    if (!d->taus) p.num_envs = d->num_envs;
    p.agent0 = d->agent0;
    p.head_tiles = ceil_div(d->n, kFwdM);
    p.seed_lo = (uint32_t)d->seed; p.seed_hi = (uint32_t)(d->seed >> 32); p.first_env = (uint32_t)d->first_env;
    p.epoch = d->epoch; p.turn = d->turn;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 head_grid((unsigned)std::min<int64_t>(p.head_tiles, kFwdMaxBlocks));
    if (p.u8) hipLaunchKernelGGL(iqn_head_kernel<true>, head_grid, dim3(kFwdThreads), 0, s, p);
    else hipLaunchKernelGGL(iqn_head_kernel<false>, head_grid, dim3(kFwdThreads), 0, s, p);
    HIP_TRY(hipGetLastError());
    const dim3 q_grid((unsigned)std::min<int64_t>(p.q_tiles, kFwdMaxBlocks));
    if (clock) hipLaunchKernelGGL(iqn_quantile_clocked_kernel, q_grid, dim3(kFwdThreads), 0, s, p, clock);
    else hipLaunchKernelGGL(iqn_quantile_kernel, q_grid, dim3(kFwdThreads), 0, s, p);
    HIP_TRY(hipGetLastError());
    return SGW_OK;
}

int sgw_iqn_forward(const sgw_iqn_forward_desc* d, void* stream) {
    if (!d) return fail(SGW_EINVAL, "sgw_iqn_forward: desc is NULL");
    return iqn_forward_launch(d, nullptr, "sgw_iqn_forward", stream);
}

int sgw_iqn_forward_clocked(const sgw_iqn_forward_desc* d, const sgw_learn_clock* clock, void* stream) {
    const char* who = "sgw_iqn_forward_clocked";
    if (!d) return fail(SGW_EINVAL, "%s: desc is NULL", who);
    if (int rc = clock_refused(who, clock)) return rc;
    if (d->turn) return fail(SGW_EINVAL, "%s: turn = %u must be 0 (the drawn taus' turn is the clock's count)", who, d->turn);
    if (d->taus) return fail(SGW_EINVAL, "%s: taus must be NULL (given taus need no clock: sgw_iqn_forward)", who);
    return iqn_forward_launch(d, nullptr, who, stream, clock);
}

int sgw_turn_iqn_forward(sgw_engine* e, int32_t agent, const sgw_iqn_forward_desc* desc, void* stream) {
    if (!e) return fail(SGW_EINVAL, "sgw_turn_iqn_forward: NULL engine");
    if (!desc) return fail(SGW_EINVAL, "sgw_turn_iqn_forward: desc is NULL");
    if (agent < 0 || agent >= e->cfg.num_agents) return fail(SGW_EINVAL, "sgw_turn_iqn_forward: agent %d out of range", agent);
    if (desc->idx) return fail(SGW_EINVAL, "sgw_turn_iqn_forward: idx must be NULL (the rows are the agent's envs in order)");
    sgw_iqn_forward_desc d = *desc;
    d.num_envs = e->cfg.num_envs; d.seed = e->cfg.seed; d.first_env = e->cfg.first_env_id; d.agent0 = agent; d.epoch = 0; d.turn = 0;
    return iqn_forward_launch(&d, e->d_turn, "sgw_turn_iqn_forward", stream);
}

// ---------------------------------------------------------------- IQN's network backward (iqn_backward.h)
// floats of workspace per quantile row (z, y, dy, de, c, dO) and per state (dhp)
static int64_t iqn_backward_floats(int64_t n, int64_t L, int64_t N, int64_t A) { return n * N * (4 * L + SGW_IQN_N_COS + A + 1) + n * L; }

int64_t sgw_iqn_backward_workspace_bytes(int64_t n, int32_t in_features, int32_t layer_size, int32_t num_quantiles, int32_t num_actions) {
    if (int rc = iqn_sizes("sgw_iqn_backward_workspace_bytes", n, 40, in_features, layer_size, num_quantiles, num_actions)) return rc;
    return iqn_backward_floats(n, layer_size, num_quantiles, num_actions) * (int64_t)sizeof(float);     // (< 2^40 * 2^17 * 4)
}

int sgw_iqn_backward(const sgw_iqn_backward_desc* d, void* stream) {
    const char* who = "sgw_iqn_backward";
    if (!d) return fail(SGW_EINVAL, "%s: desc is NULL", who);
    if (int rc = iqn_network_check(d, who, 40)) return rc;        // (n < 2^40: the workspace's byte offsets stay below 2^59)
    if (!d->taus || !d->h || !d->grad_quantiles) return fail(SGW_EINVAL, "%s: taus, h and grad_quantiles must not be NULL", who);
    if (misaligned(3, {d->taus, d->h, d->grad_quantiles, d->out_w_head, d->out_b_head, d->out_w_cos, d->out_b_cos, d->out_w_ff, d->out_b_ff, d->out_w_adv,
                       d->out_b_adv, d->out_w_val, d->out_b_val, d->out_grad_h, d->workspace}))
        return fail(SGW_EINVAL, "%s: misaligned float32 pointer (taus, h, grad_quantiles, an output or the workspace)", who);
    const int64_t n = d->n, L = d->layer_size, N = d->num_quantiles, A = d->num_actions, D = d->in_features, M = n * N;
    if (int rc = workspace_short(who, d->workspace, d->workspace_bytes, iqn_backward_floats(n, L, N, A) * (int64_t)sizeof(float))) return rc;
    if (n == 0) return SGW_OK;
    IqnBwdParams b{};
    IqnFwdParams& p = b.f;
    iqn_network_fill(p, d);
    p.h = const_cast<float*>(d->h);           // (read only here)
    b.grad = d->grad_quantiles;
    float* w = static_cast<float*>(d->workspace);
    b.z = w; b.y = b.z + M * L; b.dy = b.y + M * L; b.de = b.dy + M * L; b.c = b.de + M * L; b.dO = b.c + M * SGW_IQN_N_COS; b.dhp = b.dO + M * (A + 1);
    b.out_dh = d->out_grad_h;
    IqnWgradParams g{};
    int32_t tiles = 0;
    auto job = [&](int i, const float* G, int64_t gs, int64_t J, const void* act, int64_t as, int64_t K, int64_t rows, bool u8, float* out_w, float* out_b) {
        IqnWgradJob& jb = g.job[i];
        jb.G = G; jb.act = act; jb.out_w = out_w; jb.out_b = out_b;
        jb.M = rows; jb.gs = gs; jb.as = as;
        jb.J = (int32_t)J; jb.K = (int32_t)K; jb.u8 = u8;
        // the column tiles that hold something asked for: all of [0, K) for the weight, the one of column K for the bias
        const int32_t last = (int32_t)(K / 32);
        jb.kt0 = out_w ? 0 : last;
        jb.kts = out_w ? (out_b ? last + 1 : (int32_t)ceil_div(K, 32)) : (out_b ? 1 : 0);
        jb.tile0 = tiles;
        tiles += jb.kts * (int32_t)ceil_div(J, 32);
    };
    job(0, b.dO, A + 1, A, b.y, L, L, M, false, d->out_w_adv, d->out_b_adv);
    job(1, b.dO + A, A + 1, 1, b.y, L, L, M, false, d->out_w_val, d->out_b_val);
    job(2, b.dy, L, L, b.z, L, L, M, false, d->out_w_ff, d->out_b_ff);
    job(3, b.de, L, L, b.c, SGW_IQN_N_COS, SGW_IQN_N_COS, M, false, d->out_w_cos, d->out_b_cos);
    job(4, b.dhp, L, L, d->states, d->state_stride, D, n, p.u8 != 0, d->out_w_head, d->out_b_head);
    g.tiles = tiles;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(iqn_bwd_rows_kernel, dim3((unsigned)std::min<int64_t>(p.q_tiles, kFwdMaxBlocks)), dim3(kFwdThreads), 0, s, b);
    HIP_TRY(hipGetLastError());
    if (tiles > 0) {
        hipLaunchKernelGGL(iqn_wgrad_kernel, dim3((unsigned)ceil_div(tiles, kBwdWaves)), dim3(64 * kBwdWaves), 0, s, g);
        HIP_TRY(hipGetLastError());
    }
    return SGW_OK;
}

// ---------------------------------------------------------------- the noisy layers' weights (noisy.h)
static int noisy_launch(const sgw_noisy_weights_desc* d, const sgw_learn_clock* clock, const char* who, void* stream) {
    if (d->mode != SGW_NOISY_FORWARD && d->mode != SGW_NOISY_BACKWARD) return fail(SGW_EINVAL, "%s: unknown mode %d", who, d->mode);
    if (d->num_jobs < 0 || d->num_jobs > SGW_NOISY_MAX_JOBS) return fail(SGW_EINVAL, "%s: num_jobs = %d outside [0, %d]", who, d->num_jobs, SGW_NOISY_MAX_JOBS);
    if (d->reserved0 || d->reserved1) return fail(SGW_EINVAL, "%s: reserved fields must be 0", who);
    const bool backward = d->mode == SGW_NOISY_BACKWARD;
    NoisyParams p{};
    int64_t chunks = 0;
    for (int k = 0; k < SGW_NOISY_MAX_JOBS; ++k) {
        NoisyJob& o = p.job[k];
        o.chunk0 = INT32_MAX;
        if (k >= d->num_jobs) continue;
        const sgw_noisy_job& j = d->jobs[k];
        if (backward) {
            if (!j.grad_eff || !j.eps_in || !j.out_grad_sigma) return fail(SGW_EINVAL, "%s: job %d: grad_eff, eps_in and out_grad_sigma must not be NULL (backward)", who, k);
            if (j.weight || j.sigma || j.out_eff || j.out_eps) return fail(SGW_EINVAL, "%s: job %d: weight, sigma, out_eff and out_eps must be NULL (backward)", who, k);
        } else {
            if (!j.weight || !j.sigma || !j.out_eff) return fail(SGW_EINVAL, "%s: job %d: weight, sigma and out_eff must not be NULL (forward)", who, k);
            if (j.grad_eff || j.out_grad_sigma) return fail(SGW_EINVAL, "%s: job %d: grad_eff and out_grad_sigma must be NULL (forward)", who, k);
            if (j.tensor_id < 0 || j.tensor_id >= (1 << 28)) return fail(SGW_EINVAL, "%s: job %d: tensor_id = %d outside [0, 2^28)", who, k, j.tensor_id);
        }
        if (j.count < 0 || j.count > ((int64_t)1 << 32)) return fail(SGW_EINVAL, "%s: job %d: count = %lld outside [0, 2^32]", who, k, (long long)j.count);
        if (j.reserved) return fail(SGW_EINVAL, "%s: job %d: reserved fields must be 0", who, k);
        if (misaligned(3, {j.weight, j.sigma, j.eps_in, j.grad_eff, j.out_eff, j.out_eps, j.out_grad_sigma}))
            return fail(SGW_EINVAL, "%s: job %d: misaligned float32 pointer", who, k);
        o.a = backward ? j.grad_eff : j.weight;
        o.b = j.sigma;
        o.eps = j.eps_in;
        o.out = backward ? j.out_grad_sigma : j.out_eff;
        o.out_eps = j.out_eps;
        o.count = j.count;
        o.c3 = ((uint32_t)j.tensor_id << 4) | (uint32_t)SGW_STREAM_NOISE;
        o.chunk0 = (int32_t)chunks;               // (at most 24 * 2^22 chunks)
        chunks += ceil_div(j.count, kNoisyChunk);
    }
    if (chunks == 0) return SGW_OK;
    p.seed_lo = (uint32_t)d->seed; p.seed_hi = (uint32_t)(d->seed >> 32);
    p.draw_lo = (uint32_t)d->draw; p.draw_hi = (uint32_t)(d->draw >> 32);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (backward) LAUNCH_TRY(noisy_kernel<true>, (unsigned)chunks, s, p);               // (draws nothing: the clock is not read)
    else if (clock) LAUNCH_CLOCKED_TRY(noisy_clocked_kernel, (unsigned)chunks, s, p, clock);
    else LAUNCH_TRY(noisy_kernel<false>, (unsigned)chunks, s, p);
    return SGW_OK;
}

int sgw_noisy_weights(const sgw_noisy_weights_desc* d, void* stream) {
    if (!d) return fail(SGW_EINVAL, "sgw_noisy_weights: desc is NULL");
    return noisy_launch(d, nullptr, "sgw_noisy_weights", stream);
}

int sgw_noisy_weights_clocked(const sgw_noisy_weights_desc* d, const sgw_learn_clock* clock, void* stream) {
    const char* who = "sgw_noisy_weights_clocked";
    if (!d) return fail(SGW_EINVAL, "%s: desc is NULL", who);
    if (int rc = clock_refused(who, clock)) return rc;
    if (d->draw) return fail(SGW_EINVAL, "%s: draw = %llu must be 0 (the draw is the clock's count)", who, (unsigned long long)d->draw);
    return noisy_launch(d, clock, who, stream);
}

// ---------------------------------------------------------------- Adam, clipping and the soft update (adam_step.h)
int64_t sgw_adam_plan_bytes(int64_t num_tensors, int64_t total_numel) {
    if (num_tensors < 1 || num_tensors > kAdamMaxTensors) return fail(SGW_EINVAL, "sgw_adam_plan_bytes: num_tensors = %lld outside [1, %d]", (long long)num_tensors, kAdamMaxTensors);
    if (total_numel < 0) return fail(SGW_EINVAL, "sgw_adam_plan_bytes: total_numel = %lld", (long long)total_numel);
    // (every tensor ends in at most one chunk that is not full)
    return num_tensors * (int64_t)sizeof(AdamRec) + (total_numel / kAdamChunk + num_tensors) * (int64_t)sizeof(AdamChunk);
}

int sgw_adam_plan(const sgw_adam_tensor* records, int64_t T, int32_t dtype, void* host_image, int64_t image_bytes, sgw_adam_plan_info* info) {
    if (!records || !host_image || !info) return fail(SGW_EINVAL, "sgw_adam_plan: records, host_image and info must not be NULL");
    if (T < 1 || T > kAdamMaxTensors) return fail(SGW_EINVAL, "sgw_adam_plan: num_tensors = %lld outside [1, %d]", (long long)T, kAdamMaxTensors);
    if (!is_float_type(dtype)) return fail(SGW_EINVAL, "sgw_adam_plan: unknown dtype %d", dtype);
    if (misaligned(7, {host_image})) return fail(SGW_EINVAL, "sgw_adam_plan: misaligned 8-byte pointer (host_image)");
    int64_t chunks = 0, total = 0;
    for (int64_t k = 0; k < T; ++k) {
        const sgw_adam_tensor& r = records[k];
        if (!r.param) return fail(SGW_EINVAL, "sgw_adam_plan: tensor %lld: param must not be NULL", (long long)k);
        if (r.grad && (!r.exp_avg || !r.exp_avg_sq)) return fail(SGW_EINVAL, "sgw_adam_plan: tensor %lld: exp_avg and exp_avg_sq must not be NULL where grad is given", (long long)k);
        if (r.numel < 0) return fail(SGW_EINVAL, "sgw_adam_plan: tensor %lld: numel = %lld", (long long)k, (long long)r.numel);
        if (!std::isfinite(r.lr)) return fail(SGW_EINVAL, "sgw_adam_plan: tensor %lld: lr = %g must be finite", (long long)k, r.lr);
        if (r.reserved) return fail(SGW_EINVAL, "sgw_adam_plan: tensor %lld: reserved fields must be 0", (long long)k);
        if (misaligned(float_mask(dtype), {r.param, r.grad, r.exp_avg, r.exp_avg_sq, r.target}))
            return fail(SGW_EINVAL, "sgw_adam_plan: tensor %lld: a pointer is not aligned to its element type", (long long)k);
        if (r.grad && r.numel > 0) {
            chunks += adam_chunks(r.numel);
            total += r.numel;
            if (chunks > INT32_MAX) return fail(SGW_EINVAL, "sgw_adam_plan: 2^31 chunks or more");
        }
    }
    const int64_t need = T * (int64_t)sizeof(AdamRec) + chunks * (int64_t)sizeof(AdamChunk);
    if (image_bytes < need) return fail(SGW_EINVAL, "sgw_adam_plan: the image needs %lld bytes (sgw_adam_plan_bytes); got %lld", (long long)need, (long long)image_bytes);
    AdamRec* recs = static_cast<AdamRec*>(host_image);
    AdamChunk* map = reinterpret_cast<AdamChunk*>(recs + T);
    int64_t at_chunk = 0;
    for (int64_t k = 0; k < T; ++k) {
        const sgw_adam_tensor& r = records[k];
        AdamRec o{};
        o.p = r.param; o.g = r.grad; o.m = r.exp_avg; o.v = r.exp_avg_sq; o.t = r.target;
        o.numel = r.numel; o.lr = r.lr;
        o.first_chunk = (int32_t)at_chunk;
        o.flags = misaligned(15, {r.param, r.grad, r.exp_avg, r.exp_avg_sq, r.target}) ? 0 : kAdamVec;
        recs[k] = o;
        const int64_t nc = r.grad && r.numel > 0 ? adam_chunks(r.numel) : 0;
        for (int64_t j = 0; j < nc; ++j) map[at_chunk + j] = AdamChunk{(int32_t)k, (int32_t)j};
        at_chunk += nc;
    }
    info->num_chunks = chunks;
    info->workspace_bytes = chunks * (int64_t)sizeof(double);
    info->image_bytes = need;
    info->total_numel = total;
    return SGW_OK;
}

int sgw_adam_step(const sgw_adam_step_desc* d, void* stream) {
    if (!d) return fail(SGW_EINVAL, "sgw_adam_step: desc is NULL");
    if (!d->plan) return fail(SGW_EINVAL, "sgw_adam_step: plan must not be NULL");
    if (d->num_tensors < 1 || d->num_tensors > kAdamMaxTensors) return fail(SGW_EINVAL, "sgw_adam_step: num_tensors = %lld outside [1, %d]", (long long)d->num_tensors, kAdamMaxTensors);
    if (d->num_chunks < 0 || d->num_chunks > INT32_MAX) return fail(SGW_EINVAL, "sgw_adam_step: num_chunks = %lld outside [0, 2^31)", (long long)d->num_chunks);
    if (!is_float_type(d->dtype)) return fail(SGW_EINVAL, "sgw_adam_step: unknown dtype %d", d->dtype);
    if (d->clip_mode != SGW_ADAM_CLIP_NONE && d->clip_mode != SGW_ADAM_CLIP_NORM && d->clip_mode != SGW_ADAM_CLIP_COEF) return fail(SGW_EINVAL, "sgw_adam_step: unknown clip_mode %d", d->clip_mode);
    if (d->flags & ~SGW_ADAM_ZERO_GRADS) return fail(SGW_EINVAL, "sgw_adam_step: unknown flags 0x%x", (unsigned)d->flags);
    if (d->reserved0 || d->reserved1) return fail(SGW_EINVAL, "sgw_adam_step: reserved fields must be 0");
    if (!std::isfinite(d->max_norm) || !std::isfinite(d->beta1) || !std::isfinite(d->beta2) || !std::isfinite(d->eps) || !std::isfinite(d->tau))
        return fail(SGW_EINVAL, "sgw_adam_step: max_norm = %g, beta1 = %g, beta2 = %g, eps = %g and tau = %g must be finite", d->max_norm, d->beta1, d->beta2, d->eps, d->tau);
    if (d->beta1 < 0.0 || d->beta1 >= 1.0 || d->beta2 < 0.0 || d->beta2 >= 1.0) return fail(SGW_EINVAL, "sgw_adam_step: beta1 = %g, beta2 = %g outside [0, 1)", d->beta1, d->beta2);
    if (1.0 - d->beta1 >= 0.5) return fail(SGW_EINVAL, "sgw_adam_step: 1 - beta1 = %g must be below 0.5 (the lerp's other branch is out of scope)", 1.0 - d->beta1);
    if (d->step_state ? d->step != 0 : d->step < 1) return fail(SGW_EINVAL, "sgw_adam_step: step = %lld (>= 1 without a step_state, 0 with one)", (long long)d->step);
    if (d->clip_mode == SGW_ADAM_CLIP_COEF && !d->clip_coef) return fail(SGW_EINVAL, "sgw_adam_step: SGW_ADAM_CLIP_COEF needs clip_coef");
    if (misaligned(float_mask(d->dtype), {d->clip_coef})) return fail(SGW_EINVAL, "sgw_adam_step: clip_coef is not aligned to its element type");
    if (misaligned(7, {d->plan, d->step_state, d->out_norm, d->workspace})) return fail(SGW_EINVAL, "sgw_adam_step: misaligned 8-byte pointer (plan, step_state, out_norm or workspace)");
    const int64_t image = d->num_tensors * (int64_t)sizeof(AdamRec) + d->num_chunks * (int64_t)sizeof(AdamChunk);
    if (d->plan_bytes < image) return fail(SGW_EINVAL, "sgw_adam_step: a plan of %lld tensors and %lld chunks has %lld bytes; got %lld", (long long)d->num_tensors, (long long)d->num_chunks, (long long)image, (long long)d->plan_bytes);
    const bool norm = d->clip_mode == SGW_ADAM_CLIP_NORM;
    if (norm)
        if (int rc = workspace_short("sgw_adam_step", d->workspace, d->workspace_bytes, d->num_chunks * (int64_t)sizeof(double), " SGW_ADAM_CLIP_NORM")) return rc;
    AdamParams p{};
    p.recs = static_cast<const AdamRec*>(d->plan);
    p.map = reinterpret_cast<const AdamChunk*>(p.recs + d->num_tensors);
    p.partials = static_cast<double*>(d->workspace);
    p.coef = d->clip_coef; p.state = d->step_state; p.out_norm = d->out_norm;
    p.max_norm = d->max_norm; p.beta1 = d->beta1; p.beta2 = d->beta2; p.omb1 = 1.0 - d->beta1; p.omb2 = 1.0 - d->beta2;
    p.eps = d->eps; p.tau = d->tau; p.omtau = 1.0 - d->tau;
    if (!d->step_state) {
        p.bc1 = 1.0 - std::pow(d->beta1, (double)d->step);
        p.bc2_sqrt = std::pow(1.0 - std::pow(d->beta2, (double)d->step), 0.5);
    }
    p.T = (int32_t)d->num_tensors; p.nchunks = (int32_t)d->num_chunks; p.zero = d->flags & SGW_ADAM_ZERO_GRADS;
    const bool f64 = d->dtype == SGW_POLICY_F64;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (d->step_state || (norm && d->num_chunks > 0)) {
        const unsigned blocks = norm ? adam_blocks(d->num_chunks) : 1u;
        if (f64) hipLaunchKernelGGL(adam_norm_kernel<double>, dim3(blocks), dim3(kBlock), 0, s, p, (int)norm);
        else hipLaunchKernelGGL(adam_norm_kernel<float>, dim3(blocks), dim3(kBlock), 0, s, p, (int)norm);
        HIP_TRY(hipGetLastError());
    }
    if (d->num_chunks == 0 && !d->out_norm) return SGW_OK;
    if (f64) launch_adam_apply<double>(p, d->clip_mode, adam_blocks(d->num_chunks), s);
    else launch_adam_apply<float>(p, d->clip_mode, adam_blocks(d->num_chunks), s);
    HIP_TRY(hipGetLastError());
    return SGW_OK;
}

int sgw_choose_actions(sgw_engine* e, const float* values, const int64_t* idx, int64_t n, uint32_t epoch, uint32_t turn, int64_t* out, void* stream) {
    if (!e || !values || !out) return fail(SGW_EINVAL, "sgw_choose_actions: NULL argument");
    if (n < 0 || n > (int64_t)e->cfg.num_envs * e->cfg.num_agents) return fail(SGW_EINVAL, "sgw_choose_actions: n = %lld outside [0, E * A]", (long long)n);
    if ((reinterpret_cast<uintptr_t>(values) & 3) || (reinterpret_cast<uintptr_t>(out) & 7) || (reinterpret_cast<uintptr_t>(idx) & 7))
        return fail(SGW_EINVAL, "sgw_choose_actions: misaligned pointer");
    if (n == 0) return SGW_OK;
    const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(n, kBlock), (int64_t)e->num_cus * 16);
    hipLaunchKernelGGL(choose_actions_kernel, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), e->d_turn, values, (int)e->cfg.num_actions,
                       idx, n, (int64_t)e->cfg.num_envs, (uint32_t)e->cfg.first_env_id, epoch, turn, (uint32_t)e->cfg.seed, (uint32_t)(e->cfg.seed >> 32), out);
    HIP_TRY(hipGetLastError());
    return SGW_OK;
}

int sgw_turn_prev_rows(sgw_engine* e, int32_t agent, int32_t count, void* out, void* stream) {
    if (!e || !out) return fail(SGW_EINVAL, "sgw_turn_prev_rows: NULL argument");
    if (agent < 0 || agent >= e->cfg.num_agents) return fail(SGW_EINVAL, "sgw_turn_prev_rows: agent %d out of range", agent);
    if (e->turn_cap[agent] <= 0) return fail(SGW_EINVAL, "sgw_turn_prev_rows: agent %d has no replay states bound (sgw_turn_bind)", agent);
    if (count < 1 || count > e->turn_cap[agent]) return fail(SGW_EINVAL, "sgw_turn_prev_rows: count must be in [1, capacity = %lld]", (long long)e->turn_cap[agent]);
    const int64_t rb = e->turn_row_bytes[agent];
    const bool v16 = (rb & 15) == 0 && ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(e->turn_states[agent])) & 15) == 0;
    const bool v4 = (rb & 3) == 0 && ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(e->turn_states[agent])) & 3) == 0;
    const int vec = v16 ? 16 : (v4 ? 4 : 1);
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(rb / vec * count, kBlock), (int64_t)e->num_cus * 16));
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* o = static_cast<uint8_t*>(out);
    if (vec == 16) hipLaunchKernelGGL((turn_prev_rows_kernel<16>), dim3(blocks), dim3(kBlock), 0, s, e->d_turn, agent, count, o, rb);
    else if (vec == 4) hipLaunchKernelGGL((turn_prev_rows_kernel<4>), dim3(blocks), dim3(kBlock), 0, s, e->d_turn, agent, count, o, rb);
    else hipLaunchKernelGGL((turn_prev_rows_kernel<1>), dim3(blocks), dim3(kBlock), 0, s, e->d_turn, agent, count, o, rb);
    HIP_TRY(hipGetLastError());
    return SGW_OK;
}

int sgw_turn_end(sgw_engine* e, const void* obs, void* stream) {
    if (!e) return fail(SGW_EINVAL, "sgw_turn_end: NULL engine");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int A = e->cfg.num_agents;
    const int N = e->base.C * e->base.VV;
    if (e->turn_rows && obs) {   // this turn's windows -> the agents' replay rows
        const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div((int64_t)e->cfg.num_envs * A, kBlock / 64), (int64_t)e->num_cus * 32));   // a wave per window
        const bool even = (N & 1) == 0 && e->turn_rows_even && (reinterpret_cast<uintptr_t>(obs) & 7) == 0;
        if (e->obs_format == SGW_OBS_U8) {
            hipLaunchKernelGGL((turn_commit_kernel<uint8_t, 1>), dim3(blocks), dim3(kBlock), 0, s, e->d_turn, static_cast<const uint8_t*>(obs), (int64_t)e->cfg.num_envs, A, N);
        } else if (even) {
            hipLaunchKernelGGL((turn_commit_kernel<float, 2>), dim3(blocks), dim3(kBlock), 0, s, e->d_turn, static_cast<const float*>(obs), (int64_t)e->cfg.num_envs, A, N);
        } else {
            hipLaunchKernelGGL((turn_commit_kernel<float, 1>), dim3(blocks), dim3(kBlock), 0, s, e->d_turn, static_cast<const float*>(obs), (int64_t)e->cfg.num_envs, A, N);
        }
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(turn_advance_kernel, dim3(1), dim3(SGW_MAX_AGENTS), 0, s, e->d_turn, A);   // every ring advances; the turn counts as completed
    HIP_TRY(hipGetLastError());
    return SGW_OK;
}

int sgw_turn_state(sgw_engine* e, uint32_t* epoch_turn, int64_t* rows, void* stream) {
    if (!e || !epoch_turn) return fail(SGW_EINVAL, "sgw_turn_state: NULL argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    TurnState h;
    HIP_TRY(hipMemcpyAsync(&h, e->d_turn, sizeof(h), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    epoch_turn[0] = h.epoch; epoch_turn[1] = h.turn;
    if (rows) for (int a = 0; a < e->cfg.num_agents; ++a) rows[a] = h.row[a];
    return SGW_OK;
}

int sgw_set_obs_format(sgw_engine* e, int format) {
    if (!e) return fail(SGW_EINVAL, "sgw_set_obs_format: NULL engine");
    if (format != SGW_OBS_F32 && format != SGW_OBS_U8) return fail(SGW_EINVAL, "unknown observation format %d", format);
    if (format == SGW_OBS_U8 && !e->onehot)
        return fail(SGW_EINVAL, "SGW_OBS_U8 needs a one-hot appearance table (counts are exact small integers)");
    e->obs_format = format;
    return SGW_OK;
}

int sgw_bind_agent_state(sgw_engine* e, uint8_t* agent_state, uint8_t* state_at_pov) {
    if (!e) return fail(SGW_EINVAL, "sgw_bind_agent_state: NULL engine");
    if (!agent_state && state_at_pov) return fail(SGW_EINVAL, "sgw_bind_agent_state: state_at_pov without agent_state");
    e->agent_state = agent_state;
    e->state_at_pov = state_at_pov;
    return SGW_OK;
}

int sgw_bind_row_tail(sgw_engine* e, int kind, int tail_len, const float* table) {
    if (!e) return fail(SGW_EINVAL, "sgw_bind_row_tail: NULL engine");
    if (kind == SGW_TAIL_NONE) { e->tail_kind = SGW_TAIL_NONE; e->tail_len = 0; e->tail_table = nullptr; return SGW_OK; }
    // the whole-env instance of sgw_sweep_observe_rows has a twin that writes the tail (round 6): compiled / loaded HERE, not inside a stream-ordered call; a
    // refusal only costs the capability bit (the sweep alone + sgw_observe_rows do the same in two launches)
    auto tail_twin = [&]() {
        std::string err;
        (void)resolve_instance(e, e->k_sweep_rows_tail, 0, &err);   // (its LDS limit is left as it is)
    };
    if (kind == SGW_TAIL_AGENT_IS_IT) {
        if (e->cfg.agent_rule != SGW_AGENT_RULE_TAG) return fail(SGW_EINVAL, "SGW_TAIL_AGENT_IS_IT is the tail of SGW_AGENT_RULE_TAG agents");
        e->tail_kind = kind; e->tail_len = 1; e->tail_table = nullptr;
        tail_twin();
        return SGW_OK;
    }
    if (kind != SGW_TAIL_POSITION_TABLE) return fail(SGW_EINVAL, "sgw_bind_row_tail: unknown kind %d", kind);
    if (tail_len < 1 || tail_len > 4096 || !table) return fail(SGW_EINVAL, "SGW_TAIL_POSITION_TABLE needs a device table of [H][W][tail_len] floats, 1 <= tail_len <= 4096");
    e->tail_kind = kind; e->tail_len = tail_len; e->tail_table = table;
    tail_twin();
    return SGW_OK;
}

int sgw_bind_target_types(sgw_engine* e, uint8_t* target_types) {
    if (!e) return fail(SGW_EINVAL, "sgw_bind_target_types: NULL engine");
    if (target_types && e->cfg.agent_rule != SGW_AGENT_RULE_MOVE)
        return fail(SGW_EINVAL, "sgw_bind_target_types: the record is kept by the acts of SGW_AGENT_RULE_MOVE");
    if (target_types)
        if (int rc = resolve_twins(e)) return rc;
    // kept in the launch parameters every call starts from: every act sees it, and an unbound engine launches what it launched before
    e->base.target_types = target_types;
    e->base.extras = (e->base.extras & ~kExtraTargets) | (target_types ? kExtraTargets : 0u);
    return SGW_OK;
}

int sgw_bind_encounters(sgw_engine* e, int64_t* counts, const uint8_t* slot_of_type, int32_t num_slots) {
    if (!e) return fail(SGW_EINVAL, "sgw_bind_encounters: NULL engine");
    if (!counts) {   // (an unbound engine launches what it launched before)
        e->base.enc_counts = nullptr;
        e->base.enc_slots = 0;
        e->base.extras &= ~kExtraEncounters;
        return SGW_OK;
    }
    if (e->cfg.agent_rule != SGW_AGENT_RULE_MOVE && e->cfg.agent_rule != SGW_AGENT_RULE_CLEANUP)
        return fail(SGW_EINVAL, "sgw_bind_encounters: the counts are kept by the acts of SGW_AGENT_RULE_MOVE and SGW_AGENT_RULE_CLEANUP");
    if (!slot_of_type) return fail(SGW_EINVAL, "sgw_bind_encounters: slot_of_type is NULL");
    if (num_slots < 1 || num_slots > 32) return fail(SGW_EINVAL, "sgw_bind_encounters: num_slots must be in 1..32, not %d", (int)num_slots);
    if (reinterpret_cast<uintptr_t>(counts) & 7u) return fail(SGW_EINVAL, "sgw_bind_encounters: counts must be 8-byte aligned");
    uint8_t slots[SGW_MAX_TYPES];
    memset(slots, SGW_NO_SLOT, sizeof(slots));
    for (int t = 0; t < e->cfg.num_types; ++t) {
        if (slot_of_type[t] != SGW_NO_SLOT && slot_of_type[t] >= num_slots)
            return fail(SGW_EINVAL, "sgw_bind_encounters: slot_of_type[%d] = %d is neither SGW_NO_SLOT nor below num_slots = %d", t, (int)slot_of_type[t], (int)num_slots);
        slots[t] = slot_of_type[t];
    }
    if (int rc = resolve_twins(e)) return rc;    // (compiled / loaded HERE, not inside a stream-ordered call)
    // the slot table joins the engine's device tables (a blocking copy: binding is not stream-ordered); the rest is kept in the launch
    // parameters every call starts from, like target_types
    HIP_TRY(hipMemcpy(reinterpret_cast<char*>(e->d_tab) + offsetof(DevTables, enc_slot), slots, sizeof(slots), hipMemcpyHostToDevice));
    memcpy(e->h_tab.enc_slot, slots, sizeof(slots));
    e->base.enc_counts = counts;
    e->base.enc_slots = num_slots;
    e->base.extras |= kExtraEncounters;
    return SGW_OK;
}

int sgw_bind_agent_dir(sgw_engine* e, uint8_t* agent_dir) {
    if (!e) return fail(SGW_EINVAL, "sgw_bind_agent_dir: NULL engine");
    e->agent_dir = agent_dir;
    return SGW_OK;
}

int sgw_init_agent_state(sgw_engine* e, uint8_t* agent_state, void* stream) {
    if (!e || !agent_state) return fail(SGW_EINVAL, "sgw_init_agent_state: NULL argument");
    Params p = e->base;
    p.agent_state = agent_state;
    const int blocks = (int)std::min<int64_t>(ceil_div(p.E, kBlock), (int64_t)e->num_cus * 8);
    hipLaunchKernelGGL(init_agent_state_kernel, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), p);
    HIP_TRY(hipGetLastError());
    return SGW_OK;
}

int sgw_random_actions(sgw_engine* e, uint8_t* actions, uint32_t epoch, uint32_t turn, void* stream) {
    if (!e || !actions) return fail(SGW_EINVAL, "sgw_random_actions: NULL argument");
    Params p = e->base;
    p.actions = actions; p.epoch = epoch; p.turn = turn;
    const int64_t n = p.E * p.A;
    const int blocks = (int)std::min<int64_t>(ceil_div(n, kBlock), (int64_t)e->num_cus * 8);
    hipLaunchKernelGGL(random_actions_kernel, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), p);
    HIP_TRY(hipGetLastError());
    return SGW_OK;
}

int sgw_reduce_metrics(sgw_engine* e, const double* total_reward, double* out, void* stream) {
    if (!e || !total_reward || !out) return fail(SGW_EINVAL, "sgw_reduce_metrics: NULL argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(reduce_stage1, dim3(kRedBlocks), dim3(kBlock), 0, s, total_reward, e->cfg.num_envs, e->d_part);
    hipLaunchKernelGGL(reduce_stage2, dim3(1), dim3(kBlock), 0, s, e->d_part, e->cfg.num_envs, out);
    HIP_TRY(hipGetLastError());
    return SGW_OK;
}

int sgw_get_status(sgw_engine* e, int32_t* status_out, void* stream) {
    if (!e || !status_out) return fail(SGW_EINVAL, "sgw_get_status: NULL argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t v = 0;
    HIP_TRY(hipMemcpyAsync(&v, e->d_status, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(e->d_status, 0, sizeof(int32_t), s));
    HIP_TRY(hipStreamSynchronize(s));
    *status_out = v;
    return SGW_OK;
}

int sgw_set_timing(sgw_engine* e, int enable) {
    if (!e) return fail(SGW_EINVAL, "sgw_set_timing: NULL engine");
    if (enable && e->ev0.empty()) {
        e->ev0.resize(kEventPool);
        e->ev1.resize(kEventPool);
        for (int i = 0; i < kEventPool; ++i) {
            HIP_TRY(hipEventCreate(&e->ev0[i]));
            HIP_TRY(hipEventCreate(&e->ev1[i]));
        }
    }
    e->timing = enable != 0;
    e->ev_used = 0;
    e->ms_acc = 0.0;
    e->launches = 0;
    e->series.clear();
    e->series_dropped = 0;
    return SGW_OK;
}

int sgw_get_step_time_ms(sgw_engine* e, double* total_ms, int64_t* launches) {
    if (!e || !total_ms || !launches) return fail(SGW_EINVAL, "sgw_get_step_time_ms: NULL argument");
    if (int rc = time_drain(e)) return rc;
    *total_ms = e->ms_acc;
    *launches = e->launches;
    e->ms_acc = 0.0;
    e->launches = 0;
    return SGW_OK;
}

int sgw_get_step_times_ms(sgw_engine* e, float* out_ms, int64_t capacity, int64_t* count) {
    if (!e || !count || (capacity > 0 && !out_ms)) return fail(SGW_EINVAL, "sgw_get_step_times_ms: NULL argument");
    if (int rc = time_drain(e)) return rc;
    const int64_t n = std::min<int64_t>((int64_t)e->series.size(), std::max<int64_t>(capacity, 0));
    for (int64_t i = 0; i < n; ++i) out_ms[i] = e->series[(size_t)i];
    const int64_t lost = (int64_t)e->series.size() - n + e->series_dropped;
    *count = n;
    e->series.clear();
    e->series_dropped = 0;
    if (lost > 0) {   // the durations read are right; the caller learns that the series is not complete
        fail(SGW_OK, "sgw_get_step_times_ms: %lld launches not returned (capacity %lld, series cap %lld)", (long long)lost,
             (long long)capacity, (long long)kSeriesCap);
        return 1;
    }
    return SGW_OK;
}

int sgw_set_auto_reset(sgw_engine* e, uint32_t max_turns, double* episode_return) {
    if (!e) return fail(SGW_EINVAL, "sgw_set_auto_reset: NULL engine");
    e->auto_max_turns = max_turns;
    e->episode_return = max_turns ? episode_return : nullptr;
    return SGW_OK;
}

int sgw_set_wg_per_cu(sgw_engine* e, int wg_per_cu) {
    if (!e) return fail(SGW_EINVAL, "sgw_set_wg_per_cu: NULL engine");
    if (wg_per_cu < -1 || wg_per_cu > 8) return fail(SGW_EINVAL, "wg_per_cu must be -1 (never cap), 0 (automatic) or 1..8");
    e->wg_per_cu = wg_per_cu;
    return SGW_OK;
}

int sgw_launch_info(sgw_engine* e, char* buf, int64_t capacity) {
    if (!e || !buf || capacity < 1) return fail(SGW_EINVAL, "sgw_launch_info: NULL argument");
    // what a whole-batch, whole-turn sgw_step with 16-byte-aligned observations launches: the kernel, the LDS bytes it
    // REQUESTS (a workgroup-per-CU cap is part of that request) and the workgroups per CU the runtime then admits
    Params p = e->base;
    p.a0 = 0; p.a1 = p.A; p.flags = SGW_STEP_SWEEP | SGW_STEP_RANDOM_ACTIONS; p.do_move = 1;
    p.obs = reinterpret_cast<float*>(16); p.obs_u8 = e->obs_format == SGW_OBS_U8 ? 1 : 0;
    StepLaunch d;
    if (int rc = step_launch(e, p, nullptr, &d)) return rc;
    Kernel& k = *d.k;   // (such a call is no single phase: always an instance of the plan)
    if (d.walk) (void)resolve_kernel(e, k);
    int per_cu = 0;
    hipError_t oe = k.jit ? hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.jit, (int)d.threads, d.lds_info)
                          : (k.host ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.host, (int)d.threads, d.lds_info) : hipErrorInvalidValue);
    if (oe != hipSuccess) per_cu = -1;
    const char* phase = e->k_rows.usable() ? e->k_rows.name() : (e->phase_ok ? (e->onehot ? "phase_kernel<true>" : "phase_kernel<false>") : "the step kernel");
    const char* srows = e->k_sweep_rows.usable() ? ((e->tail_kind != SGW_TAIL_NONE && e->fast && !e->sweep_rows_chunked && e->k_sweep_rows_tail.jit) ? e->k_sweep_rows_tail.name()
                                                                                                                                                   : e->k_sweep_rows.name()) : "-";   // what sgw_sweep_observe_rows launches
    snprintf(buf, (size_t)capacity, "%s group=%d threads=%d lds=%zu env_lds=%d obs_stage=%d stage_agents=%d grid=%d wg_per_cu=%d cap=%s%d phase=%s big_stage=%d specialised=%d sweep_rows=%s",
             k.name(),
             (e->fast || e->big) ? (e->big ? e->big_threads : e->wpe * kWave) : e->group,
             (int)d.threads, d.lds_info, e->step_env_lds, e->obs_stage, e->stage_agents,
             (int)d.blocks, per_cu,
             e->wg_per_cu == 0 ? "auto:" : (e->wg_per_cu < 0 ? "never:" : "forced:"), d.cap, phase, d.big_stage,
             k.jit ? 1 : 0, srows);
    return SGW_OK;
}

}  // extern "C"
