// PPO's clipped loss and its gradients (sgw_ppo_loss): what sorrel/models/pytorch/ppo.py:259-285 -- the body of train_step's k_epochs
// loop between the networks' outputs and optimizer.step -- computes through a few dozen elementwise torch launches and an autograd
// graph, for every row of a ring segment in one launch.  include/sgw.h states the arithmetic; this file follows it term by term.
//
// The layout is policy.h's: one lane per row; the 64 lanes of a wave take 64 adjacent rows, 256 threads a tile of 256, and a capped
// grid strides over the tiles.  Rows of up to 16 actions live in registers (compile-time buckets 4 / 8 / 16): the row is read ONCE --
// with 16-byte loads where the base, the stride and the row's byte count are multiples of 16 -- and its gradient leaves with stores of
// the same width.  Rows of 17..256 actions take a plain loop per pass that re-reads the row through the cache (the maximum for logits,
// the sum, the entropy and t, then the gradient, which computes every gq_i a second time rather than keep 256 of them).
// Every sum over a row is SERIAL, in index order and in float64, and the kernel bodies AND the two helpers they call are compiled with
// fp contract off (the pragma is lexical, so each function that multiplies carries its own): the restatement
// (tests/ppo_loss_common.py) and this file round the same intermediate values.
// The means: each lane carries float64 sums of P, d^2 and H over the tiles it walks; a workgroup adds its lanes' sums in a pairwise tree
// over LDS whose order depends on the thread index alone and writes ONE partial to the workspace; ppo_loss_merge_kernel adds the
// partials in a fixed order and writes out_terms.  No floating-point atomics: two runs give the same bits.  The gradients need n and
// nothing else of the batch, so they are final after the first launch.  Gradients and row terms are written once: non-temporal stores.
#pragma once

constexpr int kPpoMaxBlocks = 2048;           // grid cap: 8 workgroups per CU on 256 CUs; more row tiles than that and the workgroups stride
constexpr int kPpoMaxActions = 256;

struct PpoLossParams {
    const void* dist;
    const void* values;
    const void* actions;
    const float* old_lp;
    const void* returns;
    void* g_dist;
    void* g_values;
    double* row_terms;
    double* out_terms;
    double* partials;                         // [workgroups of the first launch][3] = sums of (P, d^2, H)
    int64_t n, stride, tiles;
    double lo, hi, c, vc;
    int32_t nact, mode, vtype, atype, rtype, nparts;
};

// gq_i of include/sgw.h for one weight: q = w / S, l = the clamped log; at the action taken (`taken`) gr r is subtracted from c q
// (a subtraction IS the addition of the negation, and no unary minus is left for the optimiser to fold into the product gr r)
__device__ __forceinline__ double ppo_gq(const double w, const double S, const double c, const double grr, const bool taken, double& q, double& l) {
#pragma clang fp contract(off)                    // (the pragma is lexical: it does not reach a helper from the kernel body that calls it)
    constexpr double lo = 0x1p-52, hi = 1.0 - 0x1p-52;
    q = w / S;
    l = policy_clamped_log(q);
    const double cq = c * q;
    const double gl = taken ? cq - grr : cq;
    const double through = (q >= lo && q <= hi) ? gl / q : 0.0;
    const double cl = c * l;
    return through + cl;
}

// the row's scalar part: P, d^2, gr r and dL/dv from lp (include/sgw.h: loss, dL/dr, dL/dv)
struct PpoRow {
    double P, d2, grr, gv;
};

__device__ __forceinline__ PpoRow ppo_row_scalars(const PpoLossParams& p, const double lp, const double old, const double v, const double R, const double dn) {
#pragma clang fp contract(off)
    const double r = exp(lp - old);
    const double A = R - v;
    const double rc = r < p.lo ? p.lo : (r > p.hi ? p.hi : r);      // (a NaN passes through both comparisons, as torch.clamp lets it)
    const double s1 = r * A;
    const double s2 = rc * A;
    const bool inside = r >= p.lo && r <= p.hi;
    const double half = A / 2.0;
    double gr;
    if (s1 < s2) gr = A;
    else if (s1 > s2) gr = inside ? A : 0.0;
    else gr = half + (inside ? half : 0.0);
    const double d = v - R;
    PpoRow o;
    o.P = -((s1 < s2 || s1 != s1) ? s1 : s2);                        // torch.min: a NaN wins
    o.d2 = d * d;
    o.grr = gr * r;
    const double two = 2.0 * p.vc;
    const double num = two * d;
    o.gv = num / dn;
    return o;
}

// NA: 4 / 8 / 16 = the register-resident buckets (nact <= NA), 0 = the generic loop (nact <= 256).  VEC: 16-byte loads and stores.
template <int NA, bool F64, bool VEC>
__global__ __launch_bounds__(kBlock) void ppo_loss_kernel(const PpoLossParams p) {
#pragma clang fp contract(off)                    // for the whole body: no product may fuse into the sum it feeds
    const double inf = __builtin_huge_val();
    const double nan_ = __builtin_nan("");
    const bool logits = p.mode == SGW_POLICY_LOGITS;
    const int nact = p.nact;
    const double dn = (double)p.n, c = p.c;
    double sumP = 0.0, sumD = 0.0, sumH = 0.0;
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t k = tile * kBlock + threadIdx.x;
        if (k >= p.n) continue;                   // (the barrier sits behind the loop: a lane past the last row simply adds nothing)
        const int64_t at0 = k * p.stride;
        const int64_t act = load_action(p.actions, p.atype, k);
        const double v = load_float(p.values, p.vtype, k), R = load_float(p.returns, p.rtype, k), old = (double)p.old_lp[k];
        bool bad = act < 0 || act >= nact;
        double S = 0.0, acc = 0.0;
        PpoRow row;
        if constexpr (NA > 0) {
            double x[NA], g[NA];
            const double pad = logits ? -inf : 0.0;   // a weight of exactly 0: adds nothing to any sum
            cat_load_row<NA, F64, VEC>(p.dist, at0, nact, pad, x);
            if (logits) bad |= cat_weights<NA>(x);
            S = cat_sum<NA>(x, bad);
            double wa = 0.0;
#pragma unroll
            for (int i = 0; i < NA; ++i) wa = (int64_t)i == act ? x[i] : wa;      // (a select per element: no register array is indexed by a lane's value)
            bad |= !(S > 0.0 && S < inf);
            row = ppo_row_scalars(p, policy_clamped_log(wa / S), old, v, R, dn);
            double t = 0.0;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                g[i] = 0.0;
                if (i < nact) {
                    double q, l;
                    g[i] = ppo_gq(x[i], S, c, row.grr, (int64_t)i == act, q, l);
                    const double ql = q * l;
                    acc += ql;
                    const double gqq = g[i] * q;
                    t += gqq;
                }
            }
            if (p.g_dist) {
#pragma unroll
                for (int i = 0; i < NA; ++i) {
                    const double diff = g[i] - t;
                    double o;
                    if (logits) {
                        const double q = x[i] / S;
                        const double prod = q * diff;
                        o = prod / dn;
                    } else {
                        const double per = diff / S;
                        o = per / dn;
                    }
                    g[i] = bad ? nan_ : o;
                }
                cat_store_row<NA, F64, VEC>(p.g_dist, at0, nact, g);
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
            bad |= !(S > 0.0 && S < inf);
            const double wa = cat_weight<F64>(p.dist, at0 + (act < 0 || act >= nact ? 0 : act), logits, m);    // (an action out of range reads element 0; the row is NaN)
            row = ppo_row_scalars(p, policy_clamped_log(wa / S), old, v, R, dn);
            double t = 0.0;
            for (int i = 0; i < nact; ++i) {
                const double w = cat_weight<F64>(p.dist, at0 + i, logits, m);
                double q, l;
                const double gq = ppo_gq(w, S, c, row.grr, (int64_t)i == act, q, l);
                const double ql = q * l;
                acc += ql;
                const double gqq = gq * q;
                t += gqq;
            }
            if (p.g_dist) {
                for (int i = 0; i < nact; ++i) {
                    const double w = cat_weight<F64>(p.dist, at0 + i, logits, m);
                    double q, l;
                    const double diff = ppo_gq(w, S, c, row.grr, (int64_t)i == act, q, l) - t;
                    double o;
                    if (logits) {
                        const double prod = q * diff;
                        o = prod / dn;
                    } else {
                        const double per = diff / S;
                        o = per / dn;
                    }
                    policy_store_elem<F64>(p.g_dist, at0 + i, bad ? nan_ : o);
                }
            }
        }
        double P = row.P, d2 = row.d2, H = -acc, gv = row.gv;
        if (bad) { P = nan_; d2 = nan_; H = nan_; gv = nan_; }
        sumP += P;
        sumD += d2;
        sumH += H;
        if (p.g_values) store_float(p.g_values, p.vtype, k, gv);
        if (p.row_terms) {
            __builtin_nontemporal_store(P, p.row_terms + 3 * k);
            __builtin_nontemporal_store(d2, p.row_terms + 3 * k + 1);
            __builtin_nontemporal_store(H, p.row_terms + 3 * k + 2);
        }
    }
    // the workgroup's sums: a pairwise tree whose order depends on nothing but the thread index
    __shared__ double red[3][kBlock];
    const double sums[3] = {sumP, sumD, sumH};
    block_tree<3>(sums, red, TreeSum{});
    if (threadIdx.x == 0) {
        p.partials[3 * blockIdx.x] = red[0][0];
        p.partials[3 * blockIdx.x + 1] = red[1][0];
        p.partials[3 * blockIdx.x + 2] = red[2][0];
    }
}

// second launch, one workgroup: thread i adds partials i, i + 256, ... in that order, the same tree merges the threads, thread 0 writes
// out_terms = (L, Pm, M, Hm)
__global__ __launch_bounds__(kBlock) void ppo_loss_merge_kernel(const PpoLossParams p) {
#pragma clang fp contract(off)
    __shared__ double red[3][kBlock];
    double sums[3];
    partials_sum<3>(p.partials, p.nparts, sums);
    block_tree<3>(sums, red, TreeSum{});
    if (threadIdx.x == 0) {
        const double dn = (double)p.n;
        const double Pm = red[0][0] / dn, M = red[1][0] / dn, Hm = red[2][0] / dn;
        const double vm = p.vc * M;
        const double ch = p.c * Hm;
        const double pv = Pm + vm;
        p.out_terms[0] = pv - ch;
        p.out_terms[1] = Pm;
        p.out_terms[2] = M;
        p.out_terms[3] = Hm;
    }
}

// host side
inline int64_t ppo_loss_blocks(const int64_t n) { return std::min<int64_t>((n + kBlock - 1) / kBlock, kPpoMaxBlocks); }

template <bool F64>
void launch_ppo_loss(const PpoLossParams& p, const bool vec, const unsigned blocks, hipStream_t s) {
    dispatch_actions(p.nact, vec, [&](auto na, auto v) { hipLaunchKernelGGL((ppo_loss_kernel<na(), F64, v()>), dim3(blocks), dim3(kBlock), 0, s, p); });
}
