// IQN's quantile Huber loss and its gradient (sgw_iqn_loss): what sorrel/models/pytorch/iqn.py:359-405 and calculate_huber_loss
// (:451-464) -- the body of iRainbowModel.train_step between the three network outputs and loss.backward() -- compute through some
// thirty small torch launches forward and as many backward, for every row of a batch in one launch.  include/sgw.h states the
// arithmetic; this file follows it term by term.
//
// The layout: a row is 3 N A floats plus N^2 pair terms, and the reference's batch is 64 rows, so a lane per row (ppo_loss.h) would
// leave most of the machine idle and read with a stride of a whole row.  A GROUP of G lanes -- the power of two at or above N, a
// compile-time bucket 1 .. 64 -- owns one batch row: a wave holds 64 / G rows, 256 threads a tile of 256 / G rows, and a capped grid
// strides over the tiles.  A group never straddles a wave, so its lanes talk through cross-lane moves alone; every such move is
// executed by the whole wave (the loops around them have wave-uniform trip counts, and a group past the last row only skips its loads
// and stores).  For one row:
//   1  lane l takes actions l, l + G, ...: it adds its column of q_next_local serially over the quantiles (adjacent lanes read adjacent
//      addresses) and keeps its first maximum; a butterfly over the group merges (value, index) pairs under one total order -- a NaN
//      before any number, then the larger value, then the smaller index -- so every lane ends with the row's a*
//   2  lane j loads q_next_target[b][j][a*] and forms T_j;  3  lane i loads X_i and tau_i
//   4  lane i walks j = 0 .. N-1, fetching T_j from lane j, and carries the float64 sums of ql_ij and e_ij
//   5  the row term: those N sums added serially in i (fetched lane by lane)
//   6  the gradient row [N][A] leaves as coalesced stores by the whole group: zeros, and lane i's value where a == actions_b -- 16 bytes
//      per lane where A is a multiple of 4 and the base is 16-byte aligned (a quad then lies inside one quantile's actions)
// Lane 0 of a group adds the row term to a float64 sum it carries over the tiles; a workgroup adds its threads' sums in a pairwise tree
// over LDS whose order depends on the thread index alone and writes ONE partial to the workspace; iqn_loss_merge_kernel adds the
// partials in a fixed order (ppo_loss_merge_kernel's scheme, for one sum and this loss's divisor) and writes L.  No floating-point
// atomics: two runs give the same bits.  Every function that multiplies carries fp contract off (the pragma is lexical).  No array
// lives in registers, so nothing is indexed by a lane's value.  The gradient and td_error are written once: non-temporal stores.
#pragma once

constexpr int kIqnMaxBlocks = 2048;           // grid cap: 8 workgroups per CU on 256 CUs; more row tiles than that and the workgroups stride
constexpr int kIqnMaxQuantiles = 64;
constexpr int kIqnMaxActions = 256;
constexpr int kIqnNoAction = 0x7fffffff;      // the index of "no candidate yet": loses against every action

struct IqnLossParams {
    const float* q_next_local;
    const float* q_next_target;
    const float* q_expected;
    const float* taus;
    const void* actions;
    const float* rewards;
    const float* dones;
    const void* valid;
    float* grad;
    int64_t* next_actions;
    double* row_terms;
    float* td_error;
    double* out_terms;
    double* partials;                         // [workgroups of the first launch]
    int64_t n, tiles;
    double inv, count;                        // 1.0 / (n N N) and (double)(n N N)
    float discount;
    int32_t N, A, atype, vtype, nparts;
};

// is candidate (ov, oa) before (v, a) in the order of phase 1?
__device__ __forceinline__ bool iqn_before(const float ov, const int oa, const float v, const int a) {
    if (oa == kIqnNoAction) return false;
    if (a == kIqnNoAction) return true;
    const bool on = ov != ov, mn = v != v;
    if (on || mn) return on && (!mn || oa < a);
    return ov > v || (ov == v && oa < a);
}

// G: the lanes of a group (1 .. 64, a power of two, >= N).  VEC: 16-byte gradient stores (A % 4 == 0, the base 16-byte aligned).
template <int G, bool VEC>
__global__ __launch_bounds__(kBlock) void iqn_loss_kernel(const IqnLossParams p) {
#pragma clang fp contract(off)                    // for the whole body: no product may fuse into the sum it feeds
    constexpr int R = kBlock / G;                 // rows of a tile
    const int tid = threadIdx.x, l = tid % G, r = tid / G;
    const int N = p.N, A = p.A;
    const int64_t rowq = (int64_t)N * A;
    const float nan_f = __builtin_nanf("");
    const float fn = (float)N;
    double sum = 0.0;
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t b = tile * R + r;
        const bool active = b < p.n;
        const int64_t base = active ? b * rowq : 0;
        // 1: the action the local net prefers in the next state
        float best = 0.0f;
        int besta = kIqnNoAction;
        if (active) {
            const float* q = p.q_next_local + base;
            for (int a = l; a < A; a += G) {
                float s = q[a];
                for (int k = 1; k < N; ++k) s += q[(int64_t)k * A + a];
                const float m = s / fn;
                if (besta == kIqnNoAction || m > best || (m != m && best == best)) {
                    best = m;
                    besta = a;
                }
            }
        }
#pragma unroll
        for (int off = 1; off < G; off <<= 1) {
            const float ov = __shfl_xor(best, off);
            const int oa = __shfl_xor(besta, off);
            if (iqn_before(ov, oa, best, besta)) {
                best = ov;
                besta = oa;
            }
        }
        // 2, 3: the row's scalars, this lane's target and its expected quantile
        int64_t act = 0;
        bool bad = false;
        float rew = 0.0f, done = 0.0f, T = 0.0f, X = 0.0f, tau = 0.0f;
        double valid = 0.0;
        if (active) {
            act = load_action(p.actions, p.atype, b);
            bad = act < 0 || act >= A;
            rew = p.rewards[b];
            done = p.dones[b];
            valid = load_float(p.valid, p.vtype, b);
            if (l < N) {
                const float qt = p.q_next_target[base + (int64_t)l * A + besta];     // (besta is in [0, A): lane 0 always has a candidate)
                const float dq = p.discount * qt;
                const float keep = 1.0f - done;
                const float tail = dq * keep;
                T = rew + tail;
                X = bad ? nan_f : p.q_expected[base + (int64_t)l * A + act];
                tau = p.taus[b * N + l];
            }
        }
        // 4: lane i over the targets
        float* const tdrow = (p.td_error && active && l < N) ? p.td_error + (b * N + l) * N : nullptr;
        double sq = 0.0, se = 0.0;
        for (int j = 0; j < N; ++j) {
            const float Tj = __shfl(T, j, G);
            const float td = Tj - X;
            const float mag = fabsf(td);
            const bool small = mag <= 1.0f;
            const float sqr = td * td;
            const float h = small ? 0.5f * sqr : mag - 0.5f;
            const float neg = td < 0.0f ? 1.0f : 0.0f;
            const float w = fabsf(tau - neg);
            const double hv = (double)h * valid;
            const double ql = (double)w * hv;
            sq += ql;
            const double iw = p.inv * (double)w;
            const float g = (float)(iw * valid);
            const float sg = (td > 0.0f ? 1.0f : 0.0f) - neg;
            const float gt = g * td;
            const float gs = g * sg;
            const float e = small ? gt : gs;
            se += (double)e;
            if (tdrow) __builtin_nontemporal_store(td, tdrow + j);
        }
        // 5: the row term
        double S = 0.0;
        for (int i = 0; i < N; ++i) S += __shfl(sq, i, G);
        const float gval = (float)(-se);
        if (active && l == 0) {
            const double term = bad ? (double)nan_f : S;
            sum += term;
            if (p.row_terms) __builtin_nontemporal_store(term, p.row_terms + b);
            if (p.next_actions) __builtin_nontemporal_store((int64_t)besta, p.next_actions + b);
        }
        // 6: the whole gradient row
        if (p.grad) {
            if constexpr (VEC) {
                const int Aq = A >> 2, total = N * Aq;
                const int iters = (total + G - 1) / G, di = G / Aq, da = G % Aq;
                int k = l, i = l / Aq, aq = l % Aq;
                for (int it = 0; it < iters; ++it) {
                    const float gv = __shfl(gval, i < N ? i : 0, G);
                    if (active && k < total) {
                        const int a0 = aq << 2;
                        cat_f4 o;
                        o.x = bad ? nan_f : ((int64_t)a0 == act ? gv : 0.0f);
                        o.y = bad ? nan_f : ((int64_t)(a0 + 1) == act ? gv : 0.0f);
                        o.z = bad ? nan_f : ((int64_t)(a0 + 2) == act ? gv : 0.0f);
                        o.w = bad ? nan_f : ((int64_t)(a0 + 3) == act ? gv : 0.0f);
                        __builtin_nontemporal_store(o, reinterpret_cast<cat_f4*>(p.grad + base) + k);
                    }
                    k += G; i += di; aq += da;
                    if (aq >= Aq) { aq -= Aq; ++i; }
                }
            } else {
                const int total = N * A;
                const int iters = (total + G - 1) / G, di = G / A, da = G % A;
                int k = l, i = l / A, a = l % A;
                for (int it = 0; it < iters; ++it) {
                    const float gv = __shfl(gval, i < N ? i : 0, G);
                    if (active && k < total) __builtin_nontemporal_store(bad ? nan_f : ((int64_t)a == act ? gv : 0.0f), p.grad + base + k);
                    k += G; i += di; a += da;
                    if (a >= A) { a -= A; ++i; }
                }
            }
        }
    }
    // the workgroup's sum: a pairwise tree whose order depends on nothing but the thread index
    __shared__ double red[1][kBlock];
    const double sums[1] = {sum};
    block_tree<1>(sums, red, TreeSum{});
    if (tid == 0) p.partials[blockIdx.x] = red[0][0];
}

// second launch, one workgroup: thread i adds partials i, i + 256, ... in that order, the same tree merges the threads, thread 0 writes L
__global__ __launch_bounds__(kBlock) void iqn_loss_merge_kernel(const IqnLossParams p) {
    __shared__ double red[1][kBlock];
    double sums[1];
    partials_sum<1>(p.partials, p.nparts, sums);
    block_tree<1>(sums, red, TreeSum{});
    if (threadIdx.x == 0) p.out_terms[0] = red[0][0] / p.count;
}

// host side
inline int iqn_loss_group(const int num_quantiles) {
    int g = 1;
    while (g < num_quantiles) g <<= 1;
    return g;
}

inline int64_t iqn_loss_tiles(const int64_t n, const int num_quantiles) {
    const int64_t rows = kBlock / iqn_loss_group(num_quantiles);
    return n / rows + (n % rows ? 1 : 0);
}

inline int64_t iqn_loss_blocks(const int64_t n, const int num_quantiles) { return std::min<int64_t>(iqn_loss_tiles(n, num_quantiles), kIqnMaxBlocks); }

template <int G>
void launch_iqn_loss_group(const IqnLossParams& p, const bool vec, const unsigned blocks, hipStream_t s) {
    if (vec) hipLaunchKernelGGL((iqn_loss_kernel<G, true>), dim3(blocks), dim3(kBlock), 0, s, p);
    else hipLaunchKernelGGL((iqn_loss_kernel<G, false>), dim3(blocks), dim3(kBlock), 0, s, p);
}

inline void launch_iqn_loss(const IqnLossParams& p, const bool vec, const unsigned blocks, hipStream_t s) {
    switch (iqn_loss_group(p.N)) {
        case 1: launch_iqn_loss_group<1>(p, vec, blocks, s); break;
        case 2: launch_iqn_loss_group<2>(p, vec, blocks, s); break;
        case 4: launch_iqn_loss_group<4>(p, vec, blocks, s); break;
        case 8: launch_iqn_loss_group<8>(p, vec, blocks, s); break;
        case 16: launch_iqn_loss_group<16>(p, vec, blocks, s); break;
        case 32: launch_iqn_loss_group<32>(p, vec, blocks, s); break;
        default: launch_iqn_loss_group<64>(p, vec, blocks, s); break;
    }
}
