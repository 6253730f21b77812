// Sampling from a batch of categorical action distributions (sgw_policy_sample): what sorrel/models/pytorch/ppo.py:121-137
// (ActorCritic.act: Categorical(probs).sample(), .log_prob()) and :139-152 (evaluate: .entropy()) compute per agent and turn, for
// every row of an [n][num_actions] tensor in one launch.  include/sgw.h states the arithmetic; this file follows it term by term.
//
// One lane per row; the 64 lanes of a wave take 64 adjacent rows, 256 threads a tile of 256, and a capped grid strides over the tiles.
// Rows of up to 16 actions live in registers (compile-time buckets 4 / 8 / 16): one read of the row -- with 16-byte loads where the
// base, the stride and the row's byte count are multiples of 16, so that a wave's load of 64 contiguous rows uses every line it
// fetches -- then the sum, the search, the one log and (only when the entropy is asked for) the other logs without touching memory
// again.  Rows of 17..256 actions take a plain loop per pass that re-reads the row through the cache: two passes for
// probabilities (sum; search + entropy), three for logits (the maximum first), one more when the chosen weight is read back.
// Every sum is SERIAL per row, in index order and in float64, on purpose: a parallel scan re-associates the running sums and loses
// equality with the restatement (and the running sum c_i that meets the threshold must be the very sum that ended at S).
// The body is compiled with fp contract off: q_i * l_i is rounded before it enters the entropy's sum.
// The draw is keyed -- Philox of (seed, env, epoch, turn, agent), stream SGW_STREAM_POLICY, the layout of SGW_STREAM_EXPLORE -- so a
// row's action is a function of its distribution and its key: nothing is consumed, re-sharding the batch changes nothing.
// Outputs are written once: non-temporal stores.  No atomics, no LDS, no cross-lane traffic.
#pragma once

constexpr int kPolicyMaxBlocks = 2048;        // grid cap: 8 workgroups per CU on 256 CUs; more row tiles than that and the workgroups stride
constexpr int kPolicyMaxActions = 256;

struct PolicyParams {
    const void* dist;
    const int64_t* idx;
    int64_t* out_actions;
    float* out_log_probs;                     // with `ts`: the BASE of a [capacity][num_envs] ring; the kernel adds the agent's row
    float* out_entropy;
    const TurnState* ts;                      // sgw_turn_policy_sample: epoch, the turn in flight and the ring row come from the device's turn state
    int64_t n, num_envs, stride, tiles;
    int32_t nact, agent0, mode;
    uint32_t seed_lo, seed_hi, first_env, epoch, turn;
};

// NA: 4 / 8 / 16 = the register-resident buckets (nact <= NA), 0 = the generic loop (nact <= 256).  VEC: 16-byte loads.
template <int NA, bool F64, bool VEC>
__global__ __launch_bounds__(kBlock) void policy_sample_kernel(const PolicyParams p) {
#pragma clang fp contract(off)                    // for the whole body: no product may fuse into the sum it feeds
    const double inf = __builtin_huge_val();
    const float nanf_ = __builtin_nanf("");
    const bool logits = p.mode == SGW_POLICY_LOGITS;
    const int nact = p.nact;
    uint32_t epoch = p.epoch, turn = p.turn;
    float* lp_out = p.out_log_probs;
    if (p.ts) {                                   // (uniform: scalar loads)
        epoch = p.ts->epoch;
        turn = p.ts->turn + 1u;
        if (lp_out) lp_out = p.ts->cap[p.agent0] > 0 ? lp_out + p.ts->row[p.agent0] * p.num_envs : nullptr;
    }
    const uint32_t c3 = (epoch << 4) | SGW_STREAM_POLICY;
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t k = tile * kBlock + threadIdx.x;
        if (k >= p.n) continue;                   // (no cross-lane traffic below: a lane past the last row simply leaves)
        // the row's key
        int64_t env, agent;
        if (p.idx) {
            const int64_t r = p.idx[k];
            env = r % p.num_envs;
            agent = r / p.num_envs;
        } else {
            env = k % p.num_envs;
            agent = p.agent0 + k / p.num_envs;
        }
        bool bad = agent < 0 || agent >= SGW_MAX_AGENTS || env < 0;      // (a key the host could not see: the row is refused, nothing else is)
        const U4 w4 = philox4x32_10((uint32_t)agent >> 2, turn, p.first_env + (uint32_t)env, c3, p.seed_lo, p.seed_hi);
        const double uh = ((double)word_of(w4, (int)(agent & 3)) + 0.5) * 0x1p-32;
        const int64_t at0 = k * p.stride;
        int action = 255;
        double wa = 0.0, S = 0.0, acc = 0.0;
        if constexpr (NA > 0) {
            double x[NA];
            const double pad = logits ? -inf : 0.0;   // a weight of exactly 0: never chosen, adds nothing to any sum
            cat_load_row<NA, F64, VEC>(p.dist, at0, nact, pad, x);
            if (logits) bad |= cat_weights<NA>(x);
            S = cat_sum<NA>(x, bad);
            const double t = uh * S;
            double c = 0.0;
            bool found = false;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                c += x[i];
                if (!found && c > t) { found = true; action = i; wa = x[i]; }
            }
            if (p.out_entropy) {
#pragma unroll
                for (int i = 0; i < NA; ++i) {
                    if (i < nact) {
                        const double q = x[i] / S;
                        const double prod = q * policy_clamped_log(q);
                        acc += prod;
                    }
                }
            }
        } else {
            double m = 0.0;
            if (logits) {
                m = cat_row_max<F64>(p.dist, at0, nact);
                bad |= !(m < inf);
            }
            for (int i = 0; i < nact; ++i) {
                const double w = cat_weight<F64>(p.dist, at0 + i, logits, m);
                bad |= !(w >= 0.0);
                S += w;
            }
            const double t = uh * S;
            double c = 0.0;
            bool found = false;
            const bool ent = p.out_entropy != nullptr;
            for (int i = 0; i < nact; ++i) {
                const double w = cat_weight<F64>(p.dist, at0 + i, logits, m);
                c += w;
                if (!found && c > t) { found = true; action = i; wa = w; }
                if (ent) {
                    const double q = w / S;
                    const double prod = q * policy_clamped_log(q);
                    acc += prod;
                } else if (found) {
                    break;
                }
            }
        }
        bad |= !(S > 0.0 && S < inf);
        float lp = (float)policy_clamped_log(wa / S), en = (float)(-acc);
        if (bad) { action = 255; lp = nanf_; en = nanf_; }
        __builtin_nontemporal_store((int64_t)action, p.out_actions + k);
        if (lp_out) __builtin_nontemporal_store(lp, lp_out + k);
        if (p.out_entropy) __builtin_nontemporal_store(en, p.out_entropy + k);
    }
}

// host side
template <bool F64>
void launch_policy(const PolicyParams& p, const bool vec, const unsigned blocks, hipStream_t s) {
    dispatch_actions(p.nact, vec, [&](auto na, auto v) { hipLaunchKernelGGL((policy_sample_kernel<na(), F64, v()>), dim3(blocks), dim3(kBlock), 0, s, p); });
}
