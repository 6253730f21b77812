// plan.h -- host side of sgw.hip (included inside its anonymous namespace): the planner.
// Which of the prebuilt and specialised kernel instances runs for a world, and under which LDS layout, is decided HERE and
// nowhere else: make_plan is a pure function (config, options, CUs, LDS per workgroup) -> Plan, with no HIP call and no
// engine (sgw_plan runs it without a device; tests/test_plan.py pins its answers).  sgw.hip keeps the engine, the launchers
// and the C entry points; it reads the Plan and never re-derives it.
//
// Kernel instances are typed: a prebuilt step_fast / step_big instance is ONE table row (FAST_ROW / BIG_ROW) that yields its
// template arguments as a value, the host function and the name together; the specialised twin of a row is "the same
// arguments with this engine's constants", built from the value -- no kernel name is ever parsed.  What else has to know
// which rows exist (LDS slack for run-time channel counts, compile-time shapes, compile-time tables) asks the pick functions.
#pragma once

// One launchable kernel of an engine: a prebuilt instance of the library, and / or the instance specialised for this engine
// that hipRTC compiles (at sgw_create for the whole-turn kernel, at first use for the others).
struct Kernel {
    const void* host = nullptr;     // prebuilt instance (nullptr: none that fits this engine's plan)
    const char* host_name = "-";
    std::string want;               // template-id of the specialised instance ("" : none wanted)
    bool x_twin = false;            // the template has an `_x` twin (step_fast, step_big, step_kernel, phase_rows: the kernels in which agents act)
    bool compile_time_tables = false;   // `host` is a step_fast instance with compile-time tables (C != 0): no code for the extras, its `_x` twin serves them
    hipFunction_t jit = nullptr;
    hipFunction_t jit_x = nullptr;  // ... and its twin with drawn values / target_types compiled in (common.h: kExtrasDefault), when the engine needs it
    bool tried_x = false;
    bool tried = false;             // the specialised instance has been asked for (and, if jit is still null, was refused)
    bool usable() const { return host != nullptr || !want.empty(); }
    const char* name() const { return (jit || (!host && !want.empty())) ? want.c_str() : host_name; }
};

uint64_t prob_threshold(double pr) {
    const double t = std::floor(pr * 4294967296.0);
    if (!(t > 0.0)) return 0;
    if (t >= 4294967296.0) return 4294967296ull;
    return (uint64_t)t;
}

int validate(const sgw_config* c) {
    if (!c) return fail(SGW_EINVAL, "config is NULL");
    if (c->height < 3 || c->width < 3 || c->height > SGW_MAX_DIM || c->width > SGW_MAX_DIM)
        return fail(SGW_EINVAL, "height/width must be in [3, %d] (got %dx%d)", SGW_MAX_DIM, c->height, c->width);
    if (c->layers < 1 || c->layers > SGW_MAX_LAYERS)
        return fail(SGW_EINVAL, "layers must be in [1, %d] (got %d)", SGW_MAX_LAYERS, c->layers);
    if (c->num_agents < 1 || c->num_agents > SGW_MAX_AGENTS)
        return fail(SGW_EINVAL, "num_agents must be in [1, %d] (got %d)", SGW_MAX_AGENTS, c->num_agents);
    if (c->num_agents > (c->height - 2) * (c->width - 2))
        return fail(SGW_EINVAL, "more agents (%d) than interior cells", c->num_agents);
    if (c->vision_radius < 0 || c->vision_radius > (std::min(c->height, c->width) - 1) / 2)
        return fail(SGW_EINVAL, "vision_radius %d invalid: visual_field needs r <= (min(H,W)-1)//2 = %d",
                    c->vision_radius, (std::min(c->height, c->width) - 1) / 2);
    if (c->num_types < 1 || c->num_types > SGW_MAX_TYPES)
        return fail(SGW_EINVAL, "num_types must be in [1, %d] (got %d)", SGW_MAX_TYPES, c->num_types);
    if (c->num_channels < 1 || c->num_channels > SGW_MAX_CHANNELS)
        return fail(SGW_EINVAL, "num_channels must be in [1, %d] (got %d)", SGW_MAX_CHANNELS, c->num_channels);
    if (c->num_actions < 1 || c->num_actions > SGW_MAX_ACTIONS)
        return fail(SGW_EINVAL, "num_actions must be in [1, %d] (got %d)", SGW_MAX_ACTIONS, c->num_actions);
    for (int i = 0; i < c->num_actions; ++i)
        if (c->action_dy[i] < -1 || c->action_dy[i] > 1 || c->action_dx[i] < -1 || c->action_dx[i] > 1)
            return fail(SGW_EINVAL, "action %d: (dy, dx) must be in {-1,0,1}", i);
    if (c->agent_layer < 0 || c->agent_layer >= c->layers) return fail(SGW_EINVAL, "agent_layer out of range");
    if (c->default_type < 0 || c->default_type >= c->num_types) return fail(SGW_EINVAL, "default_type out of range");
    if (c->fill_type < 0 || c->fill_type >= c->num_types) return fail(SGW_EINVAL, "fill_type out of range");
    for (int a = 0; a < c->num_agents; ++a) {
        if (c->agent_type[a] >= c->num_types) return fail(SGW_EINVAL, "agent_type[%d] out of range", a);
        if (c->type_rule[c->agent_type[a]] != SGW_RULE_NONE)
            return fail(SGW_EINVAL, "agent types are skipped by the sweep and must have SGW_RULE_NONE");
    }
    for (int t = 0; t < c->num_types; ++t) {
        if (c->type_rule[t] == SGW_RULE_NONE) continue;
        if (c->type_rule[t] == SGW_RULE_BECOME_IF) {
            if (c->rule_layer[t] >= c->layers) return fail(SGW_EINVAL, "type %d: rule_layer out of range", t);
            if (c->rule_become[t] >= c->num_types) return fail(SGW_EINVAL, "type %d: rule_become out of range", t);
            continue;
        }
        if (c->type_rule[t] != SGW_RULE_SPAWN)
            return fail(SGW_EINVAL, "type %d: unsupported transition rule %d", t, (int)c->type_rule[t]);
        if (c->spawn_count[t] < 1 || c->spawn_count[t] > SGW_MAX_CHOICES)
            return fail(SGW_EINVAL, "type %d: spawn_count must be in [1, %d]", t, SGW_MAX_CHOICES);
        for (int k = 0; k < c->spawn_count[t]; ++k)
            if (c->spawn_choice[t][k] >= c->num_types) return fail(SGW_EINVAL, "type %d: spawn choice out of range", t);
        if (!(c->spawn_prob[t] >= 0.0 && c->spawn_prob[t] <= 1.0))
            return fail(SGW_EINVAL, "type %d: spawn_prob must be in [0, 1]", t);
    }
    for (int z = 0; z < c->layers; ++z) {
        if (c->layer_fill_type[z] >= c->num_types) return fail(SGW_EINVAL, "layer_fill_type[%d] out of range", z);
        if (c->layer_border_type[z] != SGW_NO_BORDER && c->layer_border_type[z] >= c->num_types)
            return fail(SGW_EINVAL, "layer_border_type[%d] out of range", z);
    }
    if (c->dense_count > SGW_MAX_CHOICES) return fail(SGW_EINVAL, "dense_count too large");
    for (int k = 0; k < c->dense_count; ++k)
        if (c->dense_choice[k] >= c->num_types) return fail(SGW_EINVAL, "dense choice out of range");
    if (!(c->dense_prob >= 0.0 && c->dense_prob <= 1.0)) return fail(SGW_EINVAL, "dense_prob must be in [0, 1]");
    if (c->agent_rule != SGW_AGENT_RULE_MOVE && c->agent_rule != SGW_AGENT_RULE_TAG && c->agent_rule != SGW_AGENT_RULE_CLEANUP)
        return fail(SGW_EINVAL, "unknown agent_rule %d", (int)c->agent_rule);
    if (c->agent_rule == SGW_AGENT_RULE_CLEANUP) {
        if (c->beam_radius < 0 || 3 * c->beam_radius > 64) return fail(SGW_EINVAL, "beam_radius must be in [0, 21]");
        if (c->clean_beam_type >= c->num_types || c->zap_beam_type >= c->num_types)
            return fail(SGW_EINVAL, "beam types out of range");
        for (int i = 0; i < c->num_actions; ++i)
            if (c->action_kind[i] > SGW_ACTION_ZAP) return fail(SGW_EINVAL, "action %d: unknown action kind", i);
    }
    if (c->agent_rule == SGW_AGENT_RULE_TAG) {
        if (c->tag_it_type >= c->num_types || c->tag_notit_type >= c->num_types || c->tag_it_type == c->tag_notit_type)
            return fail(SGW_EINVAL, "tag_it_type / tag_notit_type must be two distinct registered types");
        if (c->type_passable[c->tag_it_type] || c->type_passable[c->tag_notit_type])
            return fail(SGW_EINVAL, "tag agent types must be impassable");
    }
    for (int t = 0; t < c->num_types; ++t) {   // drawn values (sgw.h: type_value_alt / value_alt_prob)
        if (!(c->value_alt_prob[t] >= 0.0 && c->value_alt_prob[t] <= 1.0))
            return fail(SGW_EINVAL, "type %d: value_alt_prob must be in [0, 1]", t);
        if (!std::isfinite(c->type_value_alt[t])) return fail(SGW_EINVAL, "type %d: type_value_alt must be finite", t);
        if (c->value_alt_prob[t] == 0.0) continue;
        if (c->agent_rule != SGW_AGENT_RULE_MOVE)
            return fail(SGW_EINVAL, "type %d: a drawn value needs SGW_AGENT_RULE_MOVE (Tag ignores values, Cleanup sums every layer of the target)", t);
        for (int a = 0; a < c->num_agents; ++a)
            if (c->agent_type[a] == t) return fail(SGW_EINVAL, "type %d: an agent type cannot have a drawn value", t);
    }
    if (c->obs_post != SGW_OBS_POST_NONE && c->obs_post != SGW_OBS_POST_CLIP255_DIV255)
        return fail(SGW_EINVAL, "unknown obs_post %d", c->obs_post);
    if (c->grid_env_stride != 0 && c->grid_env_stride < (int64_t)c->layers * c->height * c->width)
        return fail(SGW_EINVAL, "grid_env_stride is smaller than one env");
    if (c->num_envs < 1) return fail(SGW_EINVAL, "num_envs must be >= 1");
    if (c->first_env_id + (uint64_t)c->num_envs > 4294967296ull)
        return fail(SGW_EINVAL, "global env ids must fit 32 bits");
    return SGW_OK;
}

using StepFn = void (*)(const Params);
using RowsFn = void (*)(const Params, const RowPtrs);

// ---- prebuilt instances (the path when hipRTC is absent; also what a specialised instance falls back to) -----------
#define PICK(...)                                             \
    do {                                                      \
        *name = #__VA_ARGS__;                                 \
        return reinterpret_cast<const void*>(static_cast<StepFn>(__VA_ARGS__)); \
    } while (0)

#define PICK2(...)                                            \
    do {                                                      \
        *name = #__VA_ARGS__;                                 \
        return reinterpret_cast<const void*>(static_cast<RowsFn>(__VA_ARGS__)); \
    } while (0)

// step_kernel<G, ONEHOT, L, C, RULE, r, H, W, MULTI>: the single-turn instance, or (multi) the one with sgw_rollout's turn loop.
// A compile-time radius for the examples as shipped (Tag 11x11 / 9x9 windows 116-119 -> 107-108 us, Treasurehunt 5x5 51.0 -> 46.2 us at
// 65 536 envs); everything else about a user's own world comes from the specialised instance (jit.h).
#define PICK_SK(G_, OH, L_, C_, RULE_, R_, H_, W_, NAME)                          \
    do {                                                                          \
        *name = multi ? NAME " (turn loop)" : NAME;                               \
        return multi ? reinterpret_cast<const void*>(static_cast<RowsFn>(step_kernel<G_, OH, L_, C_, RULE_, R_, H_, W_, true>)) \
                     : reinterpret_cast<const void*>(static_cast<RowsFn>(step_kernel<G_, OH, L_, C_, RULE_, R_, H_, W_, false>)); \
    } while (0)
// (round 5) The library holds the turn-loop (sgw_rollout) instance of the packed / wave-per-env kernels for plain movers only, plus the Tag
// example as shipped: every run-time-shape turn-loop instance of the Tag / Cleanup rules and every one of the workgroup-per-env form
// (G = 256) spilled registers to scratch (12-100 bytes per lane; tools/regs.py), and with hipRTC the normal path they were fallbacks of
// fallbacks.  Without one, sgw_rollout is a loop of single-turn launches (the specialised instance, where hipRTC is there, has none of that).
#define PICK_SK1(G_, OH, L_, C_, RULE_, R_, H_, W_, NAME)                         \
    do {                                                                          \
        *name = multi ? "-" : NAME;                                               \
        return multi ? nullptr : reinterpret_cast<const void*>(static_cast<RowsFn>(step_kernel<G_, OH, L_, C_, RULE_, R_, H_, W_, false>)); \
    } while (0)
template <int G>
const void* pick_step_g(bool onehot, int L, int C, int rule, int r, int H, int W, bool multi, const char** name) {
    constexpr int kMove = SGW_AGENT_RULE_MOVE, kTag = SGW_AGENT_RULE_TAG, kCleanup = SGW_AGENT_RULE_CLEANUP;
    if (rule == SGW_AGENT_RULE_CLEANUP) {
        if (onehot) PICK_SK1(G, true, 0, 0, kCleanup, 0, 0, 0, "step_kernel<G, true, 0, 0, SGW_AGENT_RULE_CLEANUP>");
        PICK_SK1(G, false, 0, 0, kCleanup, 0, 0, 0, "step_kernel<G, false, 0, 0, SGW_AGENT_RULE_CLEANUP>");
    }
    if (rule == SGW_AGENT_RULE_TAG) {
        if constexpr (G == 32) {
            if (onehot && L == 1 && C == 4 && r == 4 && H == 11 && W == 11) PICK_SK(32, true, 1, 4, kTag, 4, 11, 11, "step_kernel<32, true, 1, 4, SGW_AGENT_RULE_TAG, 4, 11, 11>");   // the Tag example as shipped
            if (onehot && L == 1 && C == 4 && r == 4) PICK_SK1(32, true, 1, 4, kTag, 4, 0, 0, "step_kernel<32, true, 1, 4, SGW_AGENT_RULE_TAG, 4>");
            if (onehot && L == 1 && C == 4 && r == 3) PICK_SK1(32, true, 1, 4, kTag, 3, 0, 0, "step_kernel<32, true, 1, 4, SGW_AGENT_RULE_TAG, 3>");
        }
        if (onehot && L == 1 && C == 4) PICK_SK1(G, true, 1, 4, kTag, 0, 0, 0, "step_kernel<G, true, 1, 4, SGW_AGENT_RULE_TAG>");   // the Tag example's tables
        if (onehot) PICK_SK1(G, true, 0, 0, kTag, 0, 0, 0, "step_kernel<G, true, 0, 0, SGW_AGENT_RULE_TAG>");
        PICK_SK1(G, false, 0, 0, kTag, 0, 0, 0, "step_kernel<G, false, 0, 0, SGW_AGENT_RULE_TAG>");
    }
    if constexpr (G == 256) {      // a workgroup per env: single-turn instances only
        if (onehot && L == 2 && C == 6) PICK_SK1(G, true, 2, 6, kMove, 0, 0, 0, "step_kernel<G, true, 2, 6>");
        if (onehot) PICK_SK1(G, true, 0, 0, kMove, 0, 0, 0, "step_kernel<G, true>");
        PICK_SK1(G, false, 0, 0, kMove, 0, 0, 0, "step_kernel<G, false>");
    } else {
        if constexpr (G == 16)
            if (onehot && L == 2 && C == 6 && r == 2) PICK_SK(16, true, 2, 6, kMove, 2, 0, 0, "step_kernel<16, true, 2, 6, SGW_AGENT_RULE_MOVE, 2>");   // the Treasurehunt example's 5x5 windows
        if (onehot && L == 2 && C == 6) PICK_SK(G, true, 2, 6, kMove, 0, 0, 0, "step_kernel<G, true, 2, 6>");                             // Treasurehunt-shaped tables
        if (onehot) PICK_SK(G, true, 0, 0, kMove, 0, 0, 0, "step_kernel<G, true>");
        PICK_SK(G, false, 0, 0, kMove, 0, 0, 0, "step_kernel<G, false>");
    }
}
#undef PICK_SK
#undef PICK_SK1

// more than 64 agents (round 6): the workgroup-per-env instances with 128-entry per-agent arrays; prebuilt with run-time shapes only (single-turn: a rollout
// is a loop of launches without hipRTC)
const void* pick_step_many(bool onehot, int rule, bool multi, const char** name) {
    if (multi) return nullptr;
    if (rule == SGW_AGENT_RULE_CLEANUP) {
        if (onehot) PICK2(step_kernel<256, true, 0, 0, SGW_AGENT_RULE_CLEANUP, 0, 0, 0, false, SGW_MAX_AGENTS>);
        PICK2(step_kernel<256, false, 0, 0, SGW_AGENT_RULE_CLEANUP, 0, 0, 0, false, SGW_MAX_AGENTS>);
    }
    if (rule == SGW_AGENT_RULE_TAG) {
        if (onehot) PICK2(step_kernel<256, true, 0, 0, SGW_AGENT_RULE_TAG, 0, 0, 0, false, SGW_MAX_AGENTS>);
        PICK2(step_kernel<256, false, 0, 0, SGW_AGENT_RULE_TAG, 0, 0, 0, false, SGW_MAX_AGENTS>);
    }
    if (onehot) PICK2(step_kernel<256, true, 0, 0, SGW_AGENT_RULE_MOVE, 0, 0, 0, false, SGW_MAX_AGENTS>);
    PICK2(step_kernel<256, false, 0, 0, SGW_AGENT_RULE_MOVE, 0, 0, 0, false, SGW_MAX_AGENTS>);
}
const void* pick_step(const Options& o, int group, bool onehot, int L, int C, int rule, int r, int H, int W, bool multi, const char** name) {
    if (group == 16) return pick_step_g<16>(onehot, L, C, rule, r, H, W, multi, name);
    if (group == 32) return pick_step_g<32>(onehot, L, C, rule, r, H, W, multi, name);
    if (group == 64) return pick_step_g<64>(onehot, L, C, rule, r, H, W, multi, name);
    return pick_step_g<256>(onehot, L, C, rule, r, H, W, multi, name);
}
// ---- template-ids of the specialised instances (spelled like the prebuilt names: trailing default arguments dropped, so an instance the
// library already holds is recognised and not compiled again)
std::string join_args(const char* tmpl, std::vector<std::string> a, size_t keep, const char* drop) {
    while (a.size() > keep && a.back() == drop) a.pop_back();
    std::string s = std::string(tmpl) + "<";
    for (size_t i = 0; i < a.size(); ++i) s += (i ? ", " : "") + a[i];
    return s + ">";
}
const char* tf(bool b) { return b ? "true" : "false"; }

// ---- step_fast<ONEHOT, L, C, r, H, W, TAG, RULES, STAGE, MULTI, P3, I16>: an instance as a value
struct FastInst {
    bool onehot;
    int L, C, r, H, W;
    bool tag, rules, stage, multi, p3, i16;
    std::string id() const {
        return join_args("step_fast", {tf(onehot), std::to_string(L), std::to_string(C), std::to_string(r), std::to_string(H), std::to_string(W),
                                       tf(tag), tf(rules), tf(stage), tf(multi), tf(p3), tf(i16)}, 6, "false");
    }
    // the same instance with an engine's own constants in place of the numeric arguments (the I16 instances keep a run-time map)
    FastInst shaped(int l, int c, int rr, int h, int w) const {
        FastInst d = *this;
        d.L = l; d.C = c; d.r = rr; d.H = i16 ? 0 : h; d.W = i16 ? 0 : w;
        return d;
    }
    FastInst turn_loop() const { FastInst d = *this; d.multi = true; return d; }
    // the ROWX twin of a chunk-staging instance (one-hot, STAGE, single-turn, not the 16-bit colour instance); "" for any other
    std::string rowsx_id() const {
        if (!onehot || !stage || multi || i16) return "";
        return "step_fast_rowsx<" + std::to_string(L) + ", " + std::to_string(C) + ", " + std::to_string(r) + ", " + std::to_string(H) + ", " + std::to_string(W) + ", " +
               tf(tag) + ", " + tf(rules) + ", " + tf(p3) + ">";
    }
};
// step_big<ONEHOT, L, C, r, MULTI, WALK, TAG, THREADS>
struct BigInst {
    bool onehot;
    int L, C, r;
    bool multi, walk, tag;
    int threads = kBigThreads;
};
// a row of the prebuilt tables: the arguments, the host function and the name, written once (fn == nullptr: the library holds no such instance)
struct FastRow { FastInst d{}; const void* fn = nullptr; const char* name = "-"; };
struct BigRow { BigInst d{}; const void* fn = nullptr; const char* name = "-"; };
#define FAST_ROW(...) FastRow{FastInst{__VA_ARGS__}, reinterpret_cast<const void*>(static_cast<StepFn>(step_fast<__VA_ARGS__>)), "step_fast<" #__VA_ARGS__ ">"}
#define BIG_ROW(...) BigRow{BigInst{__VA_ARGS__}, reinterpret_cast<const void*>(static_cast<RowsFn>(step_big<__VA_ARGS__>)), "step_big<" #__VA_ARGS__ ">"}

// the MULTI (turn-loop) instantiations of step_fast that sgw_rollout launches; an empty row: no such variant, the rollout is
// a loop of single-turn launches
FastRow pick_fast_multi(const Options& o, bool onehot, int L, int C, int r, int H, int W, bool tag, bool rules, bool stage) {
    const bool p3 = onehot && rules && C <= 10 && L <= 7 && o.pack3;
    if (p3 && stage && L == 3 && C == 9) return FAST_ROW(true, 3, 9, 0, 0, 0, false, true, true, true, true);   // Cleanup
    if (p3 && stage) return FAST_ROW(true, 0, 0, 0, 0, 0, false, true, true, true, true);    // layered rule sets
    if (onehot && rules && stage && L == 3 && C == 9) return FAST_ROW(true, 3, 9, 0, 0, 0, false, true, true, true);
    if (onehot && rules && stage) return FAST_ROW(true, 0, 0, 0, 0, 0, false, true, true, true);
    if (!onehot || tag || rules || L != 2 || C != 6) return FastRow{};
    if (r == 3 && H == 32 && W == 32) return FAST_ROW(true, 2, 6, 3, 32, 32, false, false, false, true);
    if (r == 2 && H == 16 && W == 16) return FAST_ROW(true, 2, 6, 2, 16, 16, false, false, false, true);
    if (stage) return FAST_ROW(true, 2, 6, 0, 0, 0, false, false, true, true);
    return FastRow{};
}

StepFn pick_reset(int wpe) { return wpe == 1 ? reset_kernel<1> : reset_kernel<4>; }

BigRow pick_big(bool onehot, int L, int C, int r, bool tag, int threads) {
    if (tag) {   // TagAgent.act on the workgroup-per-env kernel (moves in registers, the "it" token walked by wave 0)
        if (threads == 256) {
            if (onehot && L == 1 && C == 4 && r == 4) return BIG_ROW(true, 1, 4, 4, false, false, true, 256);
            if (onehot) return BIG_ROW(true, 0, 0, 0, false, false, true, 256);
        }
        if (onehot && L == 1 && C == 4 && r == 4) return BIG_ROW(true, 1, 4, 4, false, false, true);   // the Tag example's tables and 9x9 window
        if (onehot) return BIG_ROW(true, 0, 0, 0, false, false, true);
        return BIG_ROW(false, 0, 0, 0, false, false, true);
    }
    if (!onehot) return BIG_ROW(false, 0, 0, 0);
    if (threads == 256) {   // up to 32 agents: four waves per workgroup
        if (L == 2 && C == 6 && r == 5) return BIG_ROW(true, 2, 6, 5, false, false, false, 256);
        return BIG_ROW(true, 0, 0, 0, false, false, false, 256);
    }
    if (L == 2 && C == 6 && r == 5) return BIG_ROW(true, 2, 6, 5);   // BASELINE config 5
    return BIG_ROW(true, 0, 0, 0);
}

// which of pick_big's choices run 256 threads (the others: kBigThreads): worlds whose windows are little work for eight waves --
// agents x window cells up to 2 048 (round 3, 8 192 envs, us at 512 -> 256 threads: 90x90x2 A16 r3 123 -> 98, 100x100x2 A8 r5 106 -> 89,
// Tag 128x128 A32 r3 143 -> 119, Tag 160x160 A16 r4 141 -> 135, 128x128x2 A16 r3 194 -> 200; but 128x128x2 A32 r5 211 -> 243, config 5 352 -> 394)
int big_threads_for(const Options& o, bool onehot, int num_agents, int window_cells) {
    if (o.big_threads == 256 || o.big_threads == 512) return onehot ? o.big_threads : kBigThreads;   // A/B and test hook
    return (onehot && num_agents * window_cells <= 2048) ? 256 : kBigThreads;
}

BigRow pick_big_multi(bool onehot, int L, int C, int r) {
    if (!onehot) return BIG_ROW(false, 0, 0, 0, true);
    if (L == 2 && C == 6 && r == 5) return BIG_ROW(true, 2, 6, 5, true);
    return BigRow{};   // (round 5: the run-time-table turn-loop instance used 28 bytes of scratch per lane; without hipRTC such a world's rollout
                       // is a loop of single-turn launches)
}

BigRow pick_big_walk(bool onehot, int L, int C, int r, int threads) {
    if (!onehot) return BIG_ROW(false, 0, 0, 0, false, true);
    if (threads == 256) {
        if (L == 2 && C == 6 && r == 5) return BIG_ROW(true, 2, 6, 5, false, true, false, 256);
        return BIG_ROW(true, 0, 0, 0, false, true, false, 256);
    }
    if (L == 2 && C == 6 && r == 5) return BIG_ROW(true, 2, 6, 5, false, true);
    return BIG_ROW(true, 0, 0, 0, false, true);
}

// phase_rows instances: layers x counter words (channels / 4) x vision radius.  Shapes outside the table are compiled on demand
// (jit.h); without hipRTC they keep the staging kernels (worlds <= 4 KiB) or phase_kernel (above).
const void* pick_rows(int L, int NW, int r, const char** name, const void** obs_fn, const char** obs_name) {
#define ROWS_CASE(l, n, rr)                           \
    if (L == l && NW == n && r == rr) {               \
        *obs_fn = reinterpret_cast<const void*>(static_cast<RowsFn>(observe_rows<l, n, rr>)); \
        *obs_name = "observe_rows<" #l ", " #n ", " #rr ">"; \
        PICK(phase_rows<l, n, rr>);                   \
    }
    ROWS_CASE(2, 2, 3);   // BASELINE configs 3 / 4
    ROWS_CASE(2, 2, 2);   // BASELINE config 2, the Treasurehunt example
    ROWS_CASE(2, 2, 5);   // BASELINE config 5
#undef ROWS_CASE
    return nullptr;
}

FastRow pick_fast(const Options& o, bool onehot, bool rgb16, int L, int C, int r, int H, int W, bool tag, bool rules, bool stage) {
    if (rgb16 && stage && !rules && C == 3) {   // integer colour tables behind clip / 255 (the reference's RGBObservationSpec): 16-bit counters, result table
        if (tag) return FAST_ROW(true, 0, 3, 0, 0, 0, true, false, true, false, false, true);
        return FAST_ROW(true, 0, 3, 0, 0, 0, false, false, true, false, false, true);
    }
    if (rules) {
        // one-hot tables of <= 10 channels: 3-bit packed counters (ONE table word per cell and layer instead of ceil(C / 4))
        const bool p3 = onehot && C <= 10 && L <= 7 && o.pack3;
        if (p3 && L == 3 && C == 9 && stage && r == 5 && H == 21 && W == 31)
            return FAST_ROW(true, 3, 9, 5, 21, 31, false, true, true, false, true);   // Cleanup as shipped (21x31x3 map, 11x11 windows)
        if (p3 && stage) return FAST_ROW(true, 0, 0, 0, 0, 0, false, true, true, false, true);
        if (p3) return FAST_ROW(true, 0, 0, 0, 0, 0, false, true, false, false, true);
        if (onehot && stage) return FAST_ROW(true, 0, 0, 0, 0, 0, false, true, true);
        if (onehot) return FAST_ROW(true, 0, 0, 0, 0, 0, false, true);
        return FAST_ROW(false, 0, 0, 0, 0, 0, false, true);
    }
    if (tag) {
        if (onehot && L == 1 && C == 4 && r == 3 && H == 32 && W == 32) return FAST_ROW(true, 1, 4, 3, 32, 32, true);   // Tag on the headline's map
        const bool p3t = onehot && stage && C <= 10 && L <= 7 && o.pack3;   // 3-bit packed counters
        if (p3t) return FAST_ROW(true, 0, 0, 0, 0, 0, true, false, true, false, true);
        if (onehot && stage) return FAST_ROW(true, 0, 0, 0, 0, 0, true, false, true);
        if (onehot) return FAST_ROW(true, 0, 0, 0, 0, 0, true);
        return FAST_ROW(false, 0, 0, 0, 0, 0, true);
    }
    if (!onehot) return FAST_ROW(false, 0, 0, 0, 0, 0);
    if (L == 2 && C == 6 && r == 3 && H == 32 && W == 32) return FAST_ROW(true, 2, 6, 3, 32, 32);   // BASELINE configs 3/4 (headline)
    if (L == 2 && C == 6 && r == 2 && H == 16 && W == 16) return FAST_ROW(true, 2, 6, 2, 16, 16);   // BASELINE config 2
    if (L == 2 && C == 6) {   // treasurehunt-shaped, any size
        if (stage) return FAST_ROW(true, 2, 6, 0, 0, 0, false, false, true);
        return FAST_ROW(true, 2, 6, 0, 0, 0);
    }
    // any other one-hot table of <= 10 channels: 3-bit packed counters (ONE table word per cell and layer instead of four, ten
    // guarded channel planes instead of sixteen)
    const bool p3 = onehot && stage && C <= 10 && L <= 7 && o.pack3;
    if (p3) return FAST_ROW(true, 0, 0, 0, 0, 0, false, false, true, false, true);
    if (stage) return FAST_ROW(true, 0, 0, 0, 0, 0, false, false, true);
    return FAST_ROW(true, 0, 0, 0, 0, 0);
}

// Does the row a one-hot plain / Tag world of this shape gets have a compile-time map (H / W)?  Asked of pick_fast itself, so that a new
// row cannot be forgotten here.  (One-hot tables are assumed whatever the world's own: the packing rule has always asked this of Tag worlds
// without looking at their tables, and a Tag world of 32x32x1, 4 channels, radius 3 with other tables keeps that answer.)
bool fixed_fast_shape(const Options& o, int L, int C, int r, int H, int W, bool tag) {
    return pick_fast(o, true, false, L, C, r, H, W, tag, false, false).d.H != 0;
}

std::string fast_rows_id(int L, int C, int r, int H, int W, bool tag = false, bool tail = false) {
    return "step_fast_rows<" + std::to_string(L) + ", " + std::to_string(C) + ", " + std::to_string(r) + ", " + std::to_string(H) + ", " + std::to_string(W) +
           (tail ? (tag ? ", true, true>" : ", false, true>") : (tag ? ", true>" : ">"));
}
std::string generic_id(int G, bool onehot, int L, int C, int rule, int r, int H, int W, bool multi, bool many = false, bool rows = false) {
    if (rows)        // (the ROWS instance: every argument spelled)
        return join_args("step_kernel", {std::to_string(G), tf(onehot), std::to_string(L), std::to_string(C), std::to_string(rule), std::to_string(r),
                                         std::to_string(H), std::to_string(W), "false", std::to_string(many ? SGW_MAX_AGENTS : 64), "true"}, 11, "");
    if (many)        // (128-entry per-agent arrays: every argument spelled)
        return join_args("step_kernel", {std::to_string(G), tf(onehot), std::to_string(L), std::to_string(C), std::to_string(rule), std::to_string(r),
                                         std::to_string(H), std::to_string(W), tf(multi), std::to_string(SGW_MAX_AGENTS)}, 10, "");
    return join_args("step_kernel", {std::to_string(G), tf(onehot), std::to_string(L), std::to_string(C), std::to_string(rule), std::to_string(r),
                                     std::to_string(H), std::to_string(W), tf(multi)}, 8, "false");
}
std::string big_id(bool onehot, int L, int C, int r, bool multi, bool walk, bool tag, int threads, bool rows = false) {
    std::vector<std::string> a = {tf(onehot), std::to_string(L), std::to_string(C), std::to_string(r), tf(multi), tf(walk), tf(tag), std::to_string(threads)};
    if (rows) { a.push_back("true"); return join_args("step_big", a, 9, ""); }      // (the ROWS instance: every argument spelled)
    if (threads == kBigThreads) a.pop_back();
    return join_args("step_big", a, 4, threads == kBigThreads ? "false" : "");
}
std::string rows_id(const char* tmpl, int L, int NW, int r) {
    return std::string(tmpl) + "<" + std::to_string(L) + ", " + std::to_string(NW) + ", " + std::to_string(r) + ">";
}

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// workgroups of `threads` threads and `lds` dynamic bytes a CU holds at once when the kernel is compiled for `waves_per_simd` (its
// __launch_bounds__): what hipOccupancyMaxActiveBlocksPerMultiprocessor answers, as pure arithmetic (sgw_plan makes no HIP call)
int resident_per_cu(int threads, size_t lds, int waves_per_simd) {
    const int by_waves = std::max(1, (waves_per_simd * 4) / std::max(1, threads / kWave));
    const int by_lds = lds ? (int)(kLdsPerCu / (((lds + 1023) & ~(size_t)1023))) : by_waves;
    return std::max(1, std::min(by_waves, by_lds));
}

// Everything the planner decides.  make_plan writes all of it, starting from Plan(); the engine (struct sgw_engine : Plan) reads it.
// Written after planning, and only these: base.tab / tmpl / status (sgw_create: the device allocations), base.extras /
// base.target_types (sgw_bind_target_types), multi_turn (sgw_rollout: cleared when the turn-loop instance is refused), and in
// every Kernel the handles jit / jit_x / tried / tried_x (resolve_instance, resolve_twin: compiling is not planning).
struct Plan {
    Params base{};        // everything except per-call fields
    DevTables h_tab{};    // host copy of the tables (sgw_create uploads it)
    int wpe = 1;          // waves per env
    int group = 64;       // generic step kernel: threads per env (16 / 32: several envs share a wave)
    bool onehot = true;
    bool rgb16 = false;   // integer appearance tables behind clip / 255: step_fast's I16 instances
    int plain_tab_bytes = 0;   // ... whose direct-store variant is the float64 kernel with its own, larger table area
    bool fast = false;    // step_fast specialisation applies
    bool big = false;     // step_big (workgroup per env, pipelined agents) applies
    bool jit = false;     // the plan counts on instances specialised for this engine (hipRTC)
    bool whole_env_burst = false;   // step_fast with a compile-time shape: the whole env's windows leave in one burst
    Kernel k_step;        // a whole turn (sgw_step of all agents, sgw_observe)
    Kernel k_plain;       // STAGE kernels: the direct-store variant for calls that cannot be staged
    Kernel k_multi;       // sgw_rollout's turns in one launch
    Kernel k_walk;        // step_big<..., WALK>: resident workgroups walking the batch
    Kernel k_rows;        // phase_rows<L, NW, R>: a policy-driven phase with a lane per window row (one-hot, plain moves)
    Kernel k_obs_rows;    // observe_rows<L, NW, R>: a range of agents, per-agent destinations
    Kernel k_sweep_rows;  // step_fast_rows<L, C, R, H, W>: the sweep + every agent's window into per-agent destinations, one launch (step_big<..., ROWS> for worlds above 4 KiB)
    Kernel k_sweep_rows_tail;          // ... step_fast_rows<..., TAIL = true>: the same with the bound row tail behind every window (resolved by sgw_bind_row_tail)
    bool sweep_rows_chunked = false;   // ... it is a step_fast_rowsx instance (a chunk-staging kernel: any env_stride, row tails)
    int walk_blocks = 0;                            // how many workgroups of the walking kernel the chip holds at once
    int64_t walk_min_envs = 0, walk_max_envs = 0;  // batches above min and up to max take it (multiples of what the plain kernel holds at once)
    int64_t big_stage_min_envs = 0;                // step_big stages its windows for batches above this
    int stage_agents = 0;      // agents per staged chunk (STAGE kernels)
    bool phase_ok = false;     // the phase kernel applies (plain moves)
    int rows_wpb = 0;          // windows per 256-thread workgroup of observe_rows
    int rows_epb = 0;          // envs per 256-thread workgroup of it
    size_t rows_lds = 0;
    bool multi_turn = false;   // the step kernel in use runs sgw_rollout's turns in one launch
    void (*reset_fn)(const Params) = nullptr;
    size_t lds_bytes = 0;       // reset / generic step
    size_t step_lds_bytes = 0;  // step kernel actually launched
    bool fast_rules = false;   // the RULES variant of step_fast applies
    int step_env_lds = 0;
    int obs_stage = 0;     // bytes of LDS observation staging per wave (step_fast, one-hot)
    int big_stage = 0;     // ... per wave of step_big (0: direct stores)
    int big_threads = kBigThreads;   // threads per workgroup of the step_big instance in use (the rollout instance: always kBigThreads)
    int fast_tab_bytes = 0;
    int big_tab_bytes = 0;   // step_big: only the counter words of the channels in use
    int grid_blocks = 1;
    int fast_wg_cap = 5;   // step_fast workgroups per CU when writing large float32 observations of a large batch (0: no cap)
    bool fast_wg_cap_forced = false;   // option fast_wg_per_cu given: that value for the staged path too (default there: 6)
    int reset_blocks = 1;
};

// what the stages of make_plan hand on to each other besides the Plan: the inputs, and the facts about the world that a later stage asks for again
struct Planning {
    const sgw_config& c;
    const Options& o;
    const int num_cus;
    const bool jit;       // specialised instances may be counted on
    int nspawn = 0;       // types with a spawn rule
    bool plain_move = false, tagk = false, many_agents = false;
    bool fast_8k = false;      // a plain / Tag world of 4-11 KiB on the wave-per-env kernel
    int epb = 1;               // envs per 256-thread workgroup at this plan's waves per env
    int epb_step = 1;          // ... of the step kernel (packed: several per wave)
    bool rgb16_fast = false, bytes_ok = false;
    bool fixed_shape = false;  // a compile-time-shape instance of step_fast whose whole env leaves in one burst
    bool stage_kernel = false; // a STAGE kernel (bursts of agents) applies
};
#define PLANNING_INPUTS                  \
    const sgw_config& c = w.c;           \
    const Options& o = w.o;              \
    const bool jit = w.jit;              \
    Params& p = e->base;                 \
    const bool onehot = e->onehot;       \
    (void)c; (void)o; (void)jit; (void)p; (void)onehot

// The engine's kernels in ONE list; who walks a part of it names the part.
enum KernelSet : unsigned {
    kWholeStep = 1,         // launched with the step kernel's LDS request: their dynamic-LDS limit is raised with it
    kTwinAtBind = 2,        // agents act in them: their `_x` twins are compiled when the engine learns that it needs them, not inside a stream-ordered call
    kResolvedAtCreate = 4,  // compiled / loaded by sgw_create (a refusal re-plans); the tail twin waits for sgw_bind_row_tail
    kHasPrebuiltTwin = 8,   // may turn out to be exactly an instance the library holds
};
const struct { Kernel Plan::*k; unsigned sets; } kKernels[] = {
    {&Plan::k_step, kWholeStep | kTwinAtBind | kResolvedAtCreate | kHasPrebuiltTwin},
    {&Plan::k_plain, kWholeStep | kTwinAtBind | kResolvedAtCreate | kHasPrebuiltTwin},
    {&Plan::k_multi, kWholeStep | kTwinAtBind | kResolvedAtCreate | kHasPrebuiltTwin},
    {&Plan::k_walk, kWholeStep | kTwinAtBind | kResolvedAtCreate | kHasPrebuiltTwin},
    {&Plan::k_rows, kTwinAtBind | kResolvedAtCreate},
    {&Plan::k_obs_rows, kResolvedAtCreate},
    {&Plan::k_sweep_rows, kResolvedAtCreate | kHasPrebuiltTwin},
    {&Plan::k_sweep_rows_tail, 0},
};
// f(Kernel&) for every kernel of `set`, in that order; the first non-zero answer ends the walk and is returned
template <class F>
int for_each_kernel(Plan& p, unsigned set, F f) {
    for (const auto& s : kKernels)
        if (s.sets & set)
            if (int rc = f(p.*(s.k))) return rc;
    return 0;
}

// ---- stage 1: the device tables; whether the appearance table is one-hot / an integer colour table
void plan_tables(const sgw_config& c, Plan* e) {
    DevTables& h = e->h_tab;
    memset(&h, 0, sizeof(h));   // (padding too: the struct goes to the device as bytes)
    bool onehot = true;
    for (int t = 0; t < c.num_types; ++t) {
        int ones = 0, ch = -1;
        bool other = false;
        for (int k = 0; k < c.num_channels; ++k) {
            const double v = c.appearance[t][k];
            h.appearance[t][k] = v;
            if (v == 1.0) { ++ones; ch = k; }
            else if (v != 0.0) other = true;
        }
        if (other || ones > 1) onehot = false;
        if (ones == 1 && !other) h.delta[ch >> 2][t] = 1u << (8 * (ch & 3));
        if (ones == 1 && !other && ch < 10) h.delta3[t] = 1u << (3 * ch);
        h.value[t] = c.type_value[t];
        h.value_alt[t] = c.type_value_alt[t];
        h.alt_thr[t] = prob_threshold(c.value_alt_prob[t]);
        h.thr_lo[t] = (uint32_t)(prob_threshold(c.spawn_prob[t]) & 0xFFFFFFFFull);
        h.spawn_count[t] = c.spawn_count[t];
        memcpy(h.spawn_choice[t], c.spawn_choice[t], SGW_MAX_CHOICES);
    }
    for (int t = 0; t < c.num_types; ++t) {
        h.rule[t] = c.type_rule[t];
        h.rule_layer[t] = c.rule_layer[t];
        h.rule_become[t] = c.rule_become[t];
        h.rule_mask[t] = c.rule_mask[t];
    }
    memcpy(h.agent_type, c.agent_type, SGW_MAX_AGENTS);
    memcpy(h.dense_choice, c.dense_choice, SGW_MAX_CHOICES);
    memcpy(h.layer_fill, c.layer_fill_type, 8);
    memcpy(h.layer_border, c.layer_border_type, 8);
    if (c.obs_post != SGW_OBS_POST_NONE) onehot = false;   // post-processing lives on the general float64 path
    e->onehot = onehot;
    // ... except the reference's RGBObservationSpec as it builds its own maps (uint8 colours, clip / 255): integer tables of <= 4
    // channels take the byte-staging window pipeline with 16-bit counters and a table of the 256 possible results (step_fast.h, I16)
    bool rgb16 = c.obs_post == SGW_OBS_POST_CLIP255_DIV255 && c.num_channels <= 4 && c.layers <= 7;
    for (int t = 0; t < c.num_types && rgb16; ++t)
        for (int k = 0; k < c.num_channels; ++k) {
            const double v = c.appearance[t][k];
            if (!(v >= 0.0 && v <= 9362.0 && v == std::floor(v))) rgb16 = false;
        }
    if (rgb16) {
        for (int t = 0; t < c.num_types; ++t)
            for (int k = 0; k < c.num_channels; ++k) h.delta16[k >> 1][t] |= (uint32_t)c.appearance[t][k] << (16 * (k & 1));
        for (int k = 0; k < 256; ++k) h.post_lut[k] = (float)(std::fmin(std::fmax((double)k, 0.0), 255.0) / 255.0);   // = obs_finish of an integer sum
    }
    e->rgb16 = rgb16;
}

// ---- stage 2: the static launch parameters
void plan_params(Planning& w, Plan* e) {
    PLANNING_INPUTS;
    const DevTables& h = e->h_tab;
    memset(&p, 0, sizeof(p));
    p.H = c.height; p.W = c.width; p.L = c.layers; p.A = c.num_agents; p.r = c.vision_radius;
    p.V = 2 * c.vision_radius + 1; p.VV = p.V * p.V; p.C = c.num_channels; p.T = c.num_types;
    p.nact = c.num_actions; p.zA = c.agent_layer;
    p.cells = c.layers * c.height * c.width;
    p.cells_pad = (p.cells + 15) & ~15;
    p.env_stride = c.grid_env_stride > 0 ? c.grid_env_stride : p.cells;
    p.env_lds = p.cells_pad + agent_lds_bytes(c.num_agents > 64 ? SGW_MAX_AGENTS : 64);      // (the generic kernel's per-agent LDS arrays: its AC template argument)
    p.tab_bytes = onehot ? kTabFastBytes : kTabAllBytes;
    p.default_type = (uint32_t)c.default_type;
    p.fill_type = (uint32_t)c.fill_type;
    for (int t = 0; t < c.num_types; ++t) {
        if (c.type_rule[t] == SGW_RULE_SPAWN) {
            p.spawn_mask |= 1u << t;
            if (prob_threshold(c.spawn_prob[t]) >= 4294967296ull) p.thr_full_mask |= 1u << t;
        }
        if (c.type_passable[t]) p.pass_mask |= 1u << t;
        if (h.alt_thr[t]) p.drawn_mask |= 1u << t;
    }
    p.extras = p.drawn_mask ? kExtraDrawn : 0u;
    for (int a = 0; a < c.num_actions; ++a) {
        p.dy_pack |= (uint32_t)(c.action_dy[a] + 1) << (2 * a);
        p.dx_pack |= (uint32_t)(c.action_dx[a] + 1) << (2 * a);
    }
    for (int q = 0; q < 4; ++q) p.fill_delta[q] = h.delta[q][c.fill_type];
    p.fill_delta3 = h.delta3[c.fill_type];
    p.fill_delta16[0] = h.delta16[0][c.fill_type];
    p.fill_delta16[1] = h.delta16[1][c.fill_type];
    int& nspawn = w.nspawn;
    p.spawn_pat = 0xFFFFFFFFu;   // matches no valid type id
    for (int t = 0; t < c.num_types; ++t) {
        if (c.type_rule[t] != SGW_RULE_SPAWN) continue;
        ++nspawn;
        p.spawn_pat = 0x01010101u * (uint32_t)t;
        const uint64_t thr = prob_threshold(c.spawn_prob[t]);
        p.spawn_thr = (uint32_t)(thr & 0xFFFFFFFFull);
        p.spawn_full = thr >= 4294967296ull ? 1u : 0u;
        p.spawn_n = c.spawn_count[t];
        p.choice_lo = p.choice_hi = 0;
        for (int k = 0; k < c.spawn_count[t]; ++k) {
            if (k < 4) p.choice_lo |= (uint32_t)c.spawn_choice[t][k] << (8 * k);
            else p.choice_hi |= (uint32_t)c.spawn_choice[t][k] << (8 * (k - 4));
        }
    }
    p.single_spawner = nspawn <= 1 ? 1 : 0;
    p.onehot = onehot ? 1 : 0;
    p.nturns = 1;
    p.obs_A = c.num_agents;      // observations go to the [E][A][C][V][V] tensor unless a call says otherwise
    p.obs_a0 = 0;
    p.seed_lo = (uint32_t)c.seed;
    p.seed_hi = (uint32_t)(c.seed >> 32);
    p.first_env = (uint32_t)c.first_env_id;
    p.E = c.num_envs;
    p.dense_thr = prob_threshold(c.dense_prob);
    p.dense_count = c.dense_count;
    p.obs_post = c.obs_post;
    p.agent_rule = c.agent_rule;
    p.tag_it = c.tag_it_type;
    p.tag_notit = c.tag_notit_type;
    p.tag_reward = c.tag_reward;
    p.agent_mask = 0;
    for (int a = 0; a < c.num_agents; ++a) p.agent_mask |= 1u << (c.agent_type[a] & 31u);
    if (c.agent_rule == SGW_AGENT_RULE_TAG) p.agent_mask |= (1u << (c.tag_it_type & 31u)) | (1u << (c.tag_notit_type & 31u));
    p.has_become = 0;
    p.become_mask = 0;
    for (int t = 0; t < c.num_types; ++t)
        if (c.type_rule[t] == SGW_RULE_BECOME_IF) {
            p.has_become = 1;
            p.become_mask |= 1u << t;
        }
    p.quiet0 = p.quiet1 = 0xFFFFFFFFu;         // (four pad bytes: never cells)
    for (int z = 0; z < c.layers; ++z) {
        const uint32_t t = c.layer_fill_type[z];
        if (t >= (uint32_t)c.num_types || c.type_rule[t] != SGW_RULE_NONE) continue;
        const uint32_t w = 0x01010101u * t;
        if (p.quiet0 == 0xFFFFFFFFu || p.quiet0 == w) p.quiet0 = w;
        else if (p.quiet1 == 0xFFFFFFFFu || p.quiet1 == w) p.quiet1 = w;
    }
    p.kind_pack = 0;
    for (int a = 0; a < c.num_actions; ++a) p.kind_pack |= (uint32_t)(c.action_kind[a] & 3u) << (2 * a);
    p.beam_radius = c.beam_radius;
    p.clean_beam = c.clean_beam_type;
    p.zap_beam = c.zap_beam_type;
    p.beam_block_mask = c.beam_block_mask;
    p.total_factor = c.reward_total_factor > 0 ? c.reward_total_factor : 1;
}

// ---- stage 3: kernel family -- one wave per env while a slice stays small, else a workgroup per env
void plan_family(Planning& w, Plan* e) {
    PLANNING_INPUTS;
    const int nspawn = w.nspawn;
    const bool plain_move = c.agent_rule == SGW_AGENT_RULE_MOVE;   // step_big implements MovingAgent.act only
    const bool tagk = c.agent_rule == SGW_AGENT_RULE_TAG;
    const bool simple_rules = !p.has_become && c.agent_rule != SGW_AGENT_RULE_CLEANUP;   // else: generic kernel
    const bool vec16 = (p.env_stride & 15) == 0 && p.env_stride >= p.cells_pad;   // 16-byte loads/stores per env are legal
    // Layered rule sets (BECOME_IF, Cleanup) stay on the wave-per-env RULES kernel up to 8 KiB per env: above 4 KiB their
    // alternative is the ticket-ordered workgroup-per-env generic kernel, where every act is a hand-off between waves
    // (Cleanup 48x48x3, 4 096 envs: 95 us there against 74.5 here); up to 11 KiB from 16 384 envs on, as for the plain worlds below
    // (Cleanup 56x64x3 at 4 096 / 16 384 / 65 536 envs 97 / 394 / 1 499 us on the generic kernel, 107 / 308 / 1 229 here)
    const int rules_units = (c.num_envs >= 16384 || o.rules_11k) ? kMaxUnitsPlain : kMaxUnitsRules;
    bool rules_8k = !simple_rules && !tagk && vec16 && p.cells_pad > 4096 && (p.cells_pad >> 4) <= 64 * rules_units && p.VV <= 128;
    if (!o.fast_rules || o.force_generic) rules_8k = false;
    // Plain and Tag worlds between 4 and 8 KiB per env: a LARGE batch of them also runs a wave per env (step_big spends a 512-thread
    // workgroup and three barriers on an env; per env that is about twice the time of the wave-per-env kernel, which pays only when the
    // batch is too small to fill the chip with waves).  tools/mid_world_probe.py, us per turn at 2 048 / 4 096 / 8 192 / 65 536 envs,
    // workgroup per env -> wave per env: 48x48x2 A8 r5 23 / 40 / 73 / 640 -> 22 / 31 / 56 / 373; 64x64x2 A16 r3 33 / 57 / 107 / 858 ->
    // 28 / 39 / 69 / 488; 50x50x2 A8 r3 26 / 46 / 84 / 686 -> 19 / 25 / 41 / 272; Tag 72x72 A16 r4 23 / 41 / 74 / 727 -> 25 / 34 / 61 / 447;
    // Tag 90x90 A12 r3 27 / 48 / 90 / 741 -> 20 / 25 / 48 / 347.  Option fast_8k = 0 / 1: never / whatever the batch.
    const bool fast_8k_ok = simple_rules && (onehot || (e->rgb16 && c.num_channels == 3)) && vec16 && nspawn <= 1 && p.cells_pad > 4096 && (p.cells_pad >> 4) <= 64 * kMaxUnitsPlain && p.VV <= 128;
    // (between 8 and 11 KiB -- three workgroups per CU -- from 16 384 envs on: 72x72x2 A8 r5 at 4 096 / 16 384 / 32 768 envs 47 / 166 / 429 ->
    // 55 / 156 / 341 us, Tag 100x100 A16 r4 43 / 219 / 429 -> 49 / 140 / 306; above that two workgroups per CU no longer pay: 90x90x2 555 -> 640)
    bool fast_8k = fast_8k_ok && c.num_envs >= (p.cells_pad <= 8192 ? 4096 : 16384);
    if (o.fast_8k == 0) fast_8k = false;
    if (o.fast_8k == 1) fast_8k = fast_8k_ok;
    if (o.force_generic) fast_8k = false;
    e->wpe = (p.cells_pad <= 4096 || rules_8k || fast_8k) ? 1 : 4;
    if (o.force_big && simple_rules && !o.force_generic) e->wpe = 4;
    // More than 64 agents (round 6): the wave- and workgroup-per-env kernels keep an agent per LANE of one wave; such worlds run on the generic kernel
    // with a workgroup per env (an agent phase = the work of one wave behind the LDS ticket, per-agent state in LDS arrays of SGW_MAX_AGENTS), any size
    const bool many_agents = c.num_agents > 64;
    if (many_agents) e->wpe = 4;
    const int epb = kBlock / (e->wpe * kWave);
    e->lds_bytes = (size_t)p.tab_bytes + (size_t)epb * p.env_lds;
    e->fast = e->wpe == 1 && vec16 && (p.cells_pad >> 4) <= 64 * (fast_8k ? kMaxUnitsPlain : kMaxUnits) && nspawn <= 1 && p.VV <= 128 && simple_rules;   // MovingAgent.act and TagAgent.act
    // the layered rule set on the wave-per-env kernel (RULES variant): any spawners, BECOME_IF rules, Cleanup or plain agents
    e->fast_rules = !e->fast && e->wpe == 1 && vec16 && (p.cells_pad >> 4) <= 64 * rules_units && p.VV <= 128 &&
                    !tagk && (p.cells_pad <= 4096 || rules_8k);
    if (!o.fast_rules) e->fast_rules = false;   // test hook: generic kernel instead
    e->fast = e->fast || e->fast_rules;
    if (many_agents) e->fast = e->fast_rules = false;
    // fast kernel: wave-private LDS = [one-hot counter words | appearance table][grid]
    // (the integer-table RGB instances exist for three channels, plain or Tag movers, worlds <= 4 KiB)
    const bool rgb16_fast = e->rgb16 && e->fast && !e->fast_rules && c.num_channels == 3;
    const bool bytes_ok = onehot || rgb16_fast;        // the byte-staging window pipeline applies
    e->fast_tab_bytes = bytes_ok ? 4 * SGW_MAX_TYPES * 4 : SGW_MAX_TYPES * SGW_MAX_CHANNELS * 8;
    bool agents_impassable = true;
    for (int a = 0; a < c.num_agents; ++a) agents_impassable = agents_impassable && !c.type_passable[c.agent_type[a]];
    const bool tag_move = tagk;      // TagAgent.act moves like MovingAgent.act; step_big<..., TAG> walks the "it" token
    e->big = e->wpe == 4 && vec16 && nspawn <= 1 && p.VV <= 128 && agents_impassable && (plain_move || tag_move) && simple_rules && !many_agents;
    e->big_threads = kBigThreads;
    if (e->big) e->big_threads = big_threads_for(o, onehot, c.num_agents, p.VV);
    w.plain_move = plain_move; w.tagk = tagk; w.many_agents = many_agents; w.fast_8k = fast_8k; w.epb = epb;
    w.rgb16_fast = rgb16_fast; w.bytes_ok = bytes_ok;
}

// ---- stage 4: LDS staging of the observations of the wave-per-env kernels
void plan_obs_staging(Planning& w, Plan* e) {
    PLANNING_INPUTS;
    const bool tagk = w.tagk, fast_8k = w.fast_8k, bytes_ok = w.bytes_ok;
    bool stage_kernel = false;   // a STAGE kernel (bursts of agents) applies
    const int ob_elems = c.num_agents * c.num_channels * p.VV;
    // a compile-time-shape instance of step_fast whose whole env leaves in ONE burst (the headline's way): a prebuilt one, or -- with
    // specialised instances -- any one-hot plain / Tag world of <= 4 KiB whose windows are a multiple of 4 elements and <= 4 KiB of bytes
    bool fixed_shape = !e->fast_rules && fixed_fast_shape(o, c.layers, c.num_channels, c.vision_radius, c.height, c.width, tagk);
    if (jit && !fixed_shape && e->fast && !e->fast_rules && onehot && p.cells_pad <= 4096 && (ob_elems & 3) == 0 && ob_elems <= 4096 && o.burst != 2) {
        // ... while the wave's LDS (tables + grid + the env's window bytes) still lets SIX workgroups share a CU; beyond that the
        // chunked bursts keep the occupancy (option burst = 1: whenever legal).  (profiles/r04_jit_probe.txt, whole / chunks: 32x32x2 C8
        // 143.6 / 148.0 us, 30x30 r4 174.3 / 183.0, 40x40 163.3 / 165.6 -- six per CU; 32x32x3 C10, five per CU: 191.2 / 182.3)
        const size_t per_wave = (size_t)e->fast_tab_bytes + p.cells_pad + ((ob_elems + 15) & ~15);
        fixed_shape = o.burst == 1 || per_wave * 4 + 1024 <= kLdsPerCu / 6;
    }
    if (jit && (o.burst == 2 || o.stage_agents >= 0)) fixed_shape = false;   // (a forced burst size asks for the chunked emit)
    {   // LDS staging of one-hot observations
        const int per_agent = c.num_channels * p.VV;
        if (e->fast && onehot && fixed_shape) {   // (never an RGB world: six channels)
            // whole envs of a multiple of 4 elements, at most 4 KiB of byte counts
            if ((ob_elems & 3) == 0 && ob_elems <= 4096) e->obs_stage = (ob_elems + 15) & ~15;
        } else if (e->fast && bytes_ok) {
            // run-time shapes: as many agents per burst as fit the wave's share of LDS at full occupancy (8 workgroups
            // of 4 waves per CU, 1 KiB granules: 5 120 bytes per wave); if not even one agent fits, at 5 workgroups per CU
            const int base = e->fast_tab_bytes + (e->fast_rules ? kRuleLds : 0) + p.cells_pad;
            // The RULES kernels (layered rule sets: big windows over three layers) stage for FIVE workgroups per CU: longer bursts and
            // fewer half-written observation streams open at once beat the extra waves, as for the occupancy cap of the plain
            // kernels -- Cleanup 21x31x3 at 65 536 envs, agents per burst 1 / 2 / 3 / 4 / 5 / 10: 666 / 695 / 643-680 / 640 / 643 / 850 us
            // (16 384 envs: 201 / 193 / 185-190 / 188 / 181 / 240).
            // instances with a run-time channel count write their planes in groups of four: up to three planes of slack behind a chunk
            // (asked of pick_fast: the row this world gets with STAGE, the only case in which the answer is used.  Exception kept from the
            // hand-written rule this replaces: the I16 instances have a compile-time C = 3 and have always been given the slack all the same.)
            const bool static_channels = jit || (!w.rgb16_fast && pick_fast(o, true, false, c.layers, c.num_channels, c.vision_radius, c.height, c.width,
                                                                            tagk, e->fast_rules, true).d.C != 0);
            const int slack = 48 + (static_channels ? 0 : 3 * p.VV);
            int budget = e->fast_rules ? (int)((kLdsPerCu / 5 - 1024) / 4) - base - slack : (int)(kLdsPerCu / 8 / 4) - base - slack;
            for (int wg = 4; (e->fast_rules || fast_8k) && budget < per_agent && wg >= 2; --wg)      // big envs: fewer workgroups per CU until a window fits
                budget = (int)((kLdsPerCu / wg - 1024) / 4) - base - slack;
            if (budget < per_agent) budget = (int)((kLdsPerCu / 5 - 1024) / 4) - base - slack;
            int apc = budget >= per_agent ? std::min(c.num_agents, budget / per_agent) : 0;
            if (o.stage_agents >= 0) apc = std::min(c.num_agents, o.stage_agents);   // A/B hook
            if (apc > 0) {
                e->stage_agents = apc;
                e->obs_stage = (apc * per_agent + slack - 48 + 31 + 15) & ~15;   // + 31: the chunk's offset from a 128-byte line of global memory (step_fast.h: emit_chunk)
                stage_kernel = true;
            }
        }
        if (!o.stage) { e->obs_stage = 0; stage_kernel = false; e->stage_agents = 0; }   // test / tuning hook
    }
    w.fixed_shape = fixed_shape; w.stage_kernel = stage_kernel;
}

// ---- stage 5: lanes per env (the packing rule), then what is left of the staging and the step kernel's LDS
void plan_packing(Planning& w, Plan* e) {
    PLANNING_INPUTS;
    const bool tagk = w.tagk, rgb16_fast = w.rgb16_fast, fixed_shape = w.fixed_shape;
    const int epb = w.epb;
    bool& stage_kernel = w.stage_kernel;
    if (o.force_generic) e->fast = e->big = e->fast_rules = false;   // test hook: the generic kernel on shapes the specialised ones would take
    // Small worlds: two or four envs per wave on the LDS-resident generic kernel (step_kernel<16 / 32>).  A wave-per-env
    // kernel spends most of a small world's life on per-env work that keeps few lanes busy (a 21x21x2 world: 29 of 64
    // lanes in the sweep, 25 in the 5x5 gather, one in the moves), and at ~700 instructions per env it is bound by
    // instruction issue, not memory; packed, that stream is shared.  Rule from tools/group_sweep.py (65 536 envs, us per
    // step, wave-per-env / 16 lanes / 32 lanes per env -- profiles/r02_group_sweep.txt):
    //   10x10 A2 r2 88/29/42   16x16 A4 r2 81/46/55   21x21 A2 r2 90/46/55   21x21 A8 r2 132/118/105
    //   24x24 A4 r3 134/137/124   32x32 A2 r2 93/96/78   28x28 A8 r3 167/243/223   32x32 A8 r3 118/282/206
    //   Tag 11x11 A5 r4 171/155/111   Tag 32x32 A8 r3 194/156/140   Cleanup 21x31x3 A10 r5 694/1383/1246
    // i.e. pack while the observation work per env (A * V * V window cells) is small, and only for batches that still
    // fill the chip twice over once packed (a small batch is latency-bound: config 2, 4 096 envs, 11 us wave-per-env
    // against 16-19 us packed).  Option group = 16 / 32 forces a packing, 64 forbids it.
    e->group = e->wpe * kWave;
    if (e->wpe == 1) {
        const int64_t avv = (int64_t)c.num_agents * p.VV;
        // (round 3: the batch a packing needs, re-measured on the single-turn instances -- us per step at 1 024 / 4 096 / 8 192 / 16 384 /
        // 32 768 envs, wave per env | 32 lanes | 16 lanes: 16x16 A4 r2 7.6 / 11.1 / 15.9 / 26.1 / 45.4 | 8.6 / 10.2 / 12.6 / 19.3 / 31.2 |
        // 10.5 / 11.6 / 13.0 / 17.4 / 28.1; 10x10 A2 r2 7.2 / 9.2 / 12.8 / 21.1 / 36.8 | 7.2 / 8.2 / 10.1 / 15.1 / 24.1 | 7.5 / 8.0 / 9.1 /
        // 11.2 / 18.0: two envs per wave from 4 096 envs on, four from 12 288)
        auto enough = [&](int G) { return c.num_agents <= G && (int64_t)c.num_envs * G / kWave >= (G == 16 ? 3072 : 2048); };
        int g = 0;
        // (Tag on a map with a compile-time-shape wave-per-env instance stays there: 32x32 / 8 agents 117 us against 143 packed)
        // (round 3, tools/tag_group_probe.py, two envs per wave / wave per env: 11x11 A5 r4 99 / 131 us, 16x16 A4 r3 51 / 104, 20x20 A5 r4 116 / 127,
        // 24x24 A6 r3 80 / 125, 28x28 A6 r3 96 / 115, but 30x30 A6 r4 183 / 128, 32x32 A8 r4 217 / 148, 40x40 A8 r3 163 / 135, 48x48 A10 r4 323 / 180, 64x64 A8 r3 221 / 183
        // (wave-per-env: the 3-bit-counter Tag instance): pack while map bytes + 2 x window cells of all agents stay below 1 500)
        if (tagk)
            g = (enough(32) && p.cells_pad + 2 * avv < 1500 && !(e->fast && fixed_fast_shape(o, c.layers, c.num_channels, c.vision_radius, c.height, c.width, true))) ? 32 : 0;
        else if (c.agent_rule == SGW_AGENT_RULE_MOVE && !p.has_become) {
            // (round 3, profiles/r03_group_sweep.txt -- the wave-per-env kernels have gained more than the packed ones since the rule
            // was set: 24x24 A4 r3 98 / 157 / 122 us, 32x32 A8 r2 136 / 193 / 152, 32x32 A4 r3 90 / 197 / 144, while 21x21 A8 r2
            // 122 / 132 / 105 and 32x32 A2 r2 94 / 104 / 80 still pack: two envs per wave only while the windows OR the map are small)
            if (avv <= 100 && p.cells_pad <= 1024 && enough(16)) g = 16;
            else if (avv <= 200 && (avv <= 100 || p.cells_pad <= 1024) && enough(32)) g = 32;
        }
        if (o.group) g = o.group;
        const bool fits = (g == 16 || g == 32) && c.num_agents <= g &&
                          (c.agent_rule != SGW_AGENT_RULE_CLEANUP || 3 * c.beam_radius <= g);
        if (fits) {
            e->group = g;
            e->fast = e->fast_rules = false;
        }
    }
    if (!e->fast) { e->obs_stage = 0; stage_kernel = false; e->stage_agents = 0; }
    e->rgb16 = rgb16_fast && e->fast && stage_kernel;      // the I16 instances are STAGE kernels: no staging area, no integer path
    if (!onehot && !e->rgb16) {
        e->fast_tab_bytes = SGW_MAX_TYPES * SGW_MAX_CHANNELS * 8;
        e->obs_stage = 0;
        stage_kernel = false;
        e->stage_agents = 0;
    }
    e->whole_env_burst = e->fast && onehot && fixed_shape && e->obs_stage > 0;
    // what the float64 kernel (calls the STAGE kernel cannot serve: agent ranges, OBS_NEXT, unaligned tensors) needs instead
    e->plain_tab_bytes = e->rgb16 ? SGW_MAX_TYPES * SGW_MAX_CHANNELS * 8 : 0;
    const int epb_step = (e->fast || e->big) ? epb : kBlock / e->group;   // envs per workgroup of the step kernel
    e->step_env_lds = e->fast ? e->fast_tab_bytes + (e->fast_rules ? kRuleLds : 0) + p.cells_pad + e->obs_stage : p.env_lds;
    e->step_lds_bytes = e->fast ? (size_t)epb * e->step_env_lds + (e->rgb16 ? 1024 : 0) : (size_t)p.tab_bytes + (size_t)epb_step * e->step_env_lds;   // (+ the I16 result table)
    w.epb_step = epb_step;
}

// ---- stage 6: the LDS layout of step_big
void plan_big_lds(Planning& w, Plan* e) {
    PLANNING_INPUTS;
    const bool tagk = w.tagk;
    p.big_pitch = c.width;
    if (e->big) {
        // LDS of a workgroup: [counter words of the channels in use | appearance table][agent arrays][grid image][staging].
        // Staging of the one-hot windows (a wave's window leaves as line-aligned 16-byte streaming stores, step_big.h phase
        // R): on for instances with compile-time tables (config 5: 434 -> 347-372 us per turn at 8 192 envs); an instance with run-time
        // tables pays more for the byte staging than the stores give back (64x64 / 16 agents / 7x7 windows: 229 -> 270 us) and is
        // compiled without it.  Option big_stage = 0: never.
        // Padded rows (W + 16: the ~3 rows a 32-lane group of the window gather touches fall on disjoint banks) where a row
        // is whole 16-byte units -- unless the padding costs a workgroup per CU (LDS is handed out in 1 KiB granules): with
        // the staging, config 5's image fits four times into a CU only unpadded (39 936 bytes: exactly), and a fourth workgroup is
        // worth more than the conflict-free gather (1 280 envs: 55 us at four per CU, 71 at three).
        const bool static_tables = onehot && (jit || pick_big(onehot, c.layers, c.num_channels, c.vision_radius, tagk, e->big_threads).d.C != 0);   // (asked of pick_big)
        e->big_tab_bytes = static_tables ? ((c.num_channels + 3) / 4) * SGW_MAX_TYPES * 4 : e->fast_tab_bytes;   // (the run-time instance adds all four counter words)
        const size_t fixed = (size_t)e->big_tab_bytes + big_agent_lds(tagk);
        bool stage_on = static_tables && !tagk;   // (the Tag example's 9x9x4 windows are ten lines each: staged 54 / 79 us, direct 47 / 74, 128x128 at 2 048 envs / 72x72 at 8 192)
        if (o.big_stage == 0) stage_on = false;
        e->big_stage = stage_on ? (c.num_channels * p.VV + 31 + 3) & ~3 : 0;
        const size_t stage_all = (size_t)(e->big_threads / 64) * e->big_stage;
        auto per_cu = [&](size_t bytes) { return std::min<size_t>(4, kLdsPerCu / (((bytes + 1023) & ~(size_t)1023) + 1024)); };   // (a workgroup's request must stay 1 KiB below its share)
        const size_t plain_img = (size_t)p.cells_pad, padded_img = (size_t)c.layers * c.height * (c.width + 16);
        const bool can_pad = (c.width & 15) == 0 && (p.cells & 15) == 0;
        if (can_pad && per_cu(fixed + padded_img + stage_all) >= per_cu(fixed + plain_img + stage_all)) p.big_pitch = c.width + 16;
        e->step_lds_bytes = fixed + (p.big_pitch == c.width ? plain_img : padded_img);
        if (e->big_stage) {
            p.big_stage_off = (int)e->step_lds_bytes;        // (a multiple of 16: every piece before it is)
            e->step_lds_bytes += stage_all;
        }
    }
}

// ---- stage 7: the instances of the step kernels
void set_prebuilt(Kernel& k, const FastRow& row) { k.host = row.fn; k.host_name = row.name; k.compile_time_tables = row.d.C != 0; }
void set_prebuilt(Kernel& k, const BigRow& row) { k.host = row.fn; k.host_name = row.name; }
void plan_fast_instances(Planning& w, Plan* e) {
    PLANNING_INPUTS;
    const bool tagk = w.tagk, stage_kernel = w.stage_kernel;
    const int L = c.layers, C = c.num_channels, r = c.vision_radius, H = c.height, W = c.width;
    const bool static_map = p.cells_pad <= 4096;   // step_fast: the whole grid in NU <= 4 register units per lane
    const int jh = static_map ? H : 0, jw = static_map ? W : 0;
    const FastRow plain = pick_fast(o, e->onehot, false, L, C, r, H, W, tagk, e->fast_rules, false);
    const FastRow step = pick_fast(o, e->onehot, e->rgb16, L, C, r, H, W, tagk, e->fast_rules, stage_kernel);
    const FastRow multi = pick_fast_multi(o, e->onehot, L, C, r, H, W, tagk, e->fast_rules, stage_kernel);
    set_prebuilt(e->k_plain, plain);
    set_prebuilt(e->k_step, step);
    set_prebuilt(e->k_multi, multi);
    if (jit) {   // the specialised twin of a prebuilt choice: the same arguments with this engine's L, C, r, H, W (a run-time map above 4 KiB)
        if (e->whole_env_burst) {
            const FastInst whole{true, L, C, r, jh, jw, tagk};
            e->k_step.want = whole.id();
            e->k_multi.want = tagk ? "" : whole.turn_loop().id();
            if (step.d.H == 0) e->k_step.host = e->k_multi.host = nullptr;   // (no prebuilt twin stages a whole env of this shape)
            e->k_plain = Kernel();                                           // the same instance serves agent ranges with direct stores
        } else {
            e->k_step.want = step.d.shaped(L, C, r, jh, jw).id();
            e->k_plain.want = plain.d.shaped(L, C, r, jh, jw).id();
            if (multi.fn) e->k_multi.want = multi.d.shaped(L, C, r, jh, jw).id();
            else if (stage_kernel && e->onehot && !tagk && !e->rgb16) e->k_multi.want = step.d.shaped(L, C, r, jh, jw).turn_loop().id();
        }
    } else if (e->whole_env_burst) {
        e->k_plain = Kernel();
    }
    // the policy turn's first launch into per-agent rows (sgw_sweep_observe_rows): plain movers whose env leaves as one burst
    if (e->whole_env_burst && static_map && !e->fast_rules && ((C * (2 * r + 1) * (2 * r + 1)) & 1) == 0) {      // (round 6: Tag movers too)
        if (L == 2 && C == 6 && r == 3 && H == 32 && W == 32 && !tagk) {
            e->k_sweep_rows.host = reinterpret_cast<const void*>(&step_fast_rows<2, 6, 3, 32, 32>);
            e->k_sweep_rows.host_name = "step_fast_rows<2, 6, 3, 32, 32>";
        }
        if (jit) e->k_sweep_rows.want = fast_rows_id(L, C, r, H, W, tagk);
        if (jit) e->k_sweep_rows_tail.want = fast_rows_id(L, C, r, H, W, tagk, true);       // (compiled when a tail is bound: sgw_bind_row_tail)
    }
    // ... and on the chunk-staging instances (layered rule sets, Tag, run-time maps): the ROWX twin, specialised only (round 6)
    if (jit && !e->whole_env_burst && stage_kernel && e->onehot && !e->rgb16 && e->stage_agents >= 1) {
        e->k_sweep_rows.want = step.d.shaped(L, C, r, jh, jw).rowsx_id();
        e->sweep_rows_chunked = !e->k_sweep_rows.want.empty();
    }
}
void plan_instances(Planning& w, Plan* e) {
    PLANNING_INPUTS;
    const bool tagk = w.tagk, many_agents = w.many_agents;
    const bool tag_move = tagk;      // TagAgent.act moves like MovingAgent.act; step_big<..., TAG> walks the "it" token
    const int L = c.layers, C = c.num_channels, r = c.vision_radius, H = c.height, W = c.width;
    for (Kernel* k : {&e->k_step, &e->k_plain, &e->k_multi, &e->k_walk}) k->x_twin = true;
    e->k_sweep_rows.x_twin = !e->fast;   // (step_big<..., ROWS> / step_kernel<..., ROWS>; step_fast_rows has no twin)
    if (e->fast) {
        plan_fast_instances(w, e);
    } else if (e->big) {
        set_prebuilt(e->k_step, pick_big(e->onehot, L, C, r, tag_move, e->big_threads));
        if (!tag_move) set_prebuilt(e->k_multi, pick_big_multi(e->onehot, L, C, r));
        if (!tag_move && ((p.cells + 15) >> 4) <= 4 * e->big_threads)   // the prefetch holds one 4-unit round per thread
            set_prebuilt(e->k_walk, pick_big_walk(e->onehot, L, C, r, e->big_threads));
        if (jit) {
            e->k_sweep_rows.want = big_id(e->onehot, L, C, r, false, false, tag_move, e->big_threads, true);   // (round 6: the fused sweep + rows launch; specialised only)
            e->k_step.want = big_id(e->onehot, L, C, r, false, false, tag_move, e->big_threads);
            if (!tag_move) e->k_multi.want = big_id(e->onehot, L, C, r, true, false, false, kBigThreads);   // (whether or not the library holds a twin)
            if (e->k_walk.host) e->k_walk.want = big_id(e->onehot, L, C, r, false, true, false, e->big_threads);
        }
    } else {
        if (many_agents) {      // (group == 256: set above)
            e->k_step.host = pick_step_many(e->onehot, c.agent_rule, false, &e->k_step.host_name);
            e->k_multi.host = nullptr;
        } else {
            e->k_step.host = pick_step(o, e->group, e->onehot, L, C, c.agent_rule, r, H, W, false, &e->k_step.host_name);
            e->k_multi.host = pick_step(o, e->group, e->onehot, L, C, c.agent_rule, r, H, W, true, &e->k_multi.host_name);   // the generic kernel's instance with the turn loop
        }
        if (jit) {
            e->k_step.want = generic_id(e->group, e->onehot, L, C, c.agent_rule, r, H, W, false, many_agents);
            e->k_multi.want = generic_id(e->group, e->onehot, L, C, c.agent_rule, r, H, W, true, many_agents);
            e->k_sweep_rows.want = generic_id(e->group, e->onehot, L, C, c.agent_rule, r, H, W, false, many_agents, true);   // (round 6: the fused sweep + rows launch)
        }
    }
    if (!o.big_walk) e->k_walk = Kernel();   // A/B hook
    for_each_kernel(*e, kHasPrebuiltTwin, [](Kernel& k) {
        if (k.host && k.want == k.host_name) k.want.clear();   // the library already holds exactly this instance
        return 0;
    });
    e->multi_turn = e->k_multi.usable();   // kernels with sgw_rollout's turn loop
}

// ---- stage 8: the phase / row kernels
void plan_row_kernels(Planning& w, Plan* e) {
    PLANNING_INPUTS;
    const bool plain_move = w.plain_move;
    const int L = c.layers, C = c.num_channels, r = c.vision_radius;
    e->reset_fn = pick_reset(e->wpe);
    // Worlds above 4 KiB only: there, gathering one window from global memory beats staging 32 KiB through LDS (config 5:
    // 14.9 against 24.4 us per phase launch); a 2 KiB env is staged with four coalesced 16-byte loads per lane and the
    // byte gather from global is the slower way (config 3: 62.9 against 46.1 us).  Option phase_kernel = 0 / 1 forces.
    e->phase_ok = plain_move && e->wpe == 4;
    if (o.phase_kernel >= 0) e->phase_ok = plain_move && o.phase_kernel == 1;
    if (e->onehot && p.cells >= 8 && o.phase_rows) {
        // (observe_rows renders windows whatever the agents do when they act: every agent rule; phase_rows moves plain movers only)
        const int NW = (C + 3) / 4;
        e->k_rows.x_twin = true;
        e->k_rows.host = pick_rows(L, NW, r, &e->k_rows.host_name, &e->k_obs_rows.host, &e->k_obs_rows.host_name);
        if (jit && !e->k_rows.host && r >= 1 && r <= 7) {
            e->k_rows.want = rows_id("phase_rows", L, NW, r);
            e->k_obs_rows.want = rows_id("observe_rows", L, NW, r);
        }
        if (!plain_move) e->k_rows = Kernel();
        if (e->k_obs_rows.usable()) {
            const int V = 2 * r + 1;
            e->rows_epb = e->rows_wpb = 4 * (64 / (V <= 4 ? 4 : (V <= 8 ? 8 : 16)));
            // per wave: counter words, the value table, the staging bytes of the windows it carries
            e->rows_lds = (size_t)4 * (NW * 34 * 4 + SGW_MAX_TYPES * 8 + (((e->rows_epb / 4) * C * V * V + 15) & ~15));
        }
    }
}

// ---- stage 9: the walk window and the launch geometry
void plan_geometry(Planning& w, Plan* e) {
    PLANNING_INPUTS;
    const int epb = w.epb, epb_step = w.epb_step;
    p.stage_agents = e->stage_agents;
    if (o.fast_wg_per_cu > 0) { e->fast_wg_cap = o.fast_wg_per_cu; e->fast_wg_cap_forced = true; }   // tuning hook
    e->grid_blocks = (int)ceil_div(p.E, (e->fast || e->big) ? epb : epb_step);   // every step kernel: one env per group, the dispatcher balances
    if (e->k_walk.usable()) {
        // workgroups a CU holds at once: the walking variant is compiled for SGW_WALK_WAVES waves per SIMD (76 VGPRs: three 512-thread
        // workgroups per CU), the plain kernel for 6 (the hardware admits a fourth workgroup while the request stays 1 KiB below a quarter
        // of the CU's LDS -- 1 280 envs of config 5: 55 us there, 71 above)
        const size_t walk_lds = e->step_lds_bytes - (size_t)(e->big_threads / 64) * e->big_stage;   // (the walking variant stores directly: no staging area)
        const int per_cu = resident_per_cu(e->big_threads, walk_lds, SGW_WALK_WAVES);
        const int plain_per_cu = resident_per_cu(e->big_threads, e->step_lds_bytes, SGW_BIG_WAVES);
        // Engaged for batches of 1.5x to 3x what the plain kernel holds at once (one env per workgroup, four
        // workgroups per CU at config 5 = 1 024 envs), measured on config 5's shape, same box, us per launch, walking
        // against plain: 1 280 envs 53 / 55, 1 536 74-77 / 70-72, 2 048 88-96 / 109-118, 3 072 161-183 / 174-178,
        // 4 096 206 / 224, 8 192 511 / 436.  Fewer walking workgroups are resident (76 VGPRs: three per CU), they
        // run in lockstep and each env's prefetch waits for the previous env's stores, so over many rounds the
        // dispatcher's four per CU win; over two or three rounds the hidden drain does.  Also measured at 2 048 envs:
        // 683 workgroups (three envs each, evenly) 100 us, 512 100 us, 1 024 / 1 365 (oversubscribed) 93-107 us, a
        // 64-VGPR build (four per CU, six spilled registers) 95-98 us, staggered starts 96-101 us.
        e->walk_blocks = per_cu * w.num_cus;
        // Round 3, with the staged windows (config 5, us per launch, plain direct / walking direct / plain staged): 1 024 envs
        // 47 / - / 59, 1 280 54 / 54 / 69, 1 536 70 / 76 / 78, 2 048 105 / 91 / 97, 2 560 132 / 128 / 117, 3 072 155 / 168 / 141,
        // 4 096 216 / - / 174-181, 8 192 415 / - / 347: the window is 1.5x to 2.25x now, staging takes over above it.
        e->walk_min_envs = (int64_t)plain_per_cu * w.num_cus * 3 / 2;
        e->walk_max_envs = e->big_stage ? (int64_t)plain_per_cu * w.num_cus * 9 / 4 : (int64_t)plain_per_cu * w.num_cus * 3;
        if (o.big_walk_blocks > 0) {   // tuning / test hook: this many workgroups, whatever the batch
            e->walk_blocks = o.big_walk_blocks;
            e->walk_min_envs = e->walk_blocks;
            e->walk_max_envs = INT64_MAX;
        }
    }
    // staged windows pay once the batch is a few rounds of workgroups (a single round is latency-bound, and the staging adds
    // an LDS round trip per window): above 1.75x what the chip holds at once (see the table above)
    if (e->big) {
        const int64_t by_lds = (int64_t)(kLdsPerCu / (((e->step_lds_bytes + 1023) & ~(size_t)1023) + 1024));
        const int64_t resident = std::max<int64_t>(1, std::min<int64_t>(2048 / e->big_threads, by_lds));   // workgroups a CU holds at once
        e->big_stage_min_envs = resident * w.num_cus * 7 / 4;
        if (o.big_stage == 1) e->big_stage_min_envs = 0;   // test hook: staged whatever the batch
    }
    e->reset_blocks = (int)ceil_div(p.E, epb);   // one env per group and launch
}

// Everything sgw_create decides, as a function of (config, options, CUs, LDS per workgroup) alone: kernel family, lanes per env, LDS
// layout, staging, walk window, the instances to launch.  No HIP call (sgw_plan runs it without a device; tests/test_plan.py
// enumerates it).  `jit`: specialised instances may be counted on.  The stages run in this order and each reads only the ones before it;
// the order of an option's override relative to the automatic rule it overrides is behaviour.
int make_plan(const sgw_config& c, const Options& o, int num_cus, size_t /* lds_cap: no rule asks for it yet */, bool jit, Plan* out) {
    *out = Plan();
    out->jit = jit;
    Planning w{c, o, num_cus, jit};
    plan_tables(c, out);
    plan_params(w, out);
    plan_family(w, out);
    plan_obs_staging(w, out);
    plan_packing(w, out);
    plan_big_lds(w, out);
    const size_t lds_max = 160 * 1024;
    if (out->lds_bytes > lds_max)
        return fail(SGW_EINVAL, "world of %d bytes per env does not fit the %zu-byte LDS-resident path", out->base.cells, lds_max);
    plan_instances(w, out);
    plan_row_kernels(w, out);
    plan_geometry(w, out);
    return SGW_OK;
}
#undef PLANNING_INPUTS
