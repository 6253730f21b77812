// IQN's network forward (sgw_iqn_forward): what sorrel/models/pytorch/iqn.py:110-167 (IQN.forward, get_qvalues) and layers.py's
// NoisyLinear compute through a dozen torch launches, for every row of a batch in two.  include/sgw.h states the arithmetic; this file
// follows it term by term.
//
// Two launches, because the two GEMM stages have different M: the head layer has one row per state (M = n, K = D), everything behind it
// one row per (state, quantile) (M = n N).  A workgroup that owned whole states through both would run the head's K = D product for the
// 64 / N states of its tile on a matrix unit whose tile has 32 rows -- at the reference's N = 12 five rows of 32 would carry data, and the
// head would cost more than the rest -- and would read all of w_head once per five states.  So iqn_head_kernel is a plain
// [n][D] x [D][L] GEMM over tiles of 64 states that leaves h [n][L] in the workspace (L floats per state: 1 / N of what a single
// [n N][L] intermediate of the torch path takes), and iqn_quantile_kernel does the rest for tiles of R = 64 / N whole states = R N <= 64
// quantile rows: taus (read, or drawn keyed), the 64 x 64 cosines into LDS, the embedding GEMM (K = 64), the product with h in the
// GEMM's epilogue, the noisy layer's GEMM (K = L) from LDS back into the same LDS image, the dueling head on the vector unit (A + 1 <= 65
// columns: less than one more column tile) and the two serial means.  Nothing of size n N L leaves the chip.
//
// Every product runs on __builtin_amdgcn_mfma_f32_32x32x2f32, whose result is bit for bit the k-ordered fmaf chain that starts at C: the
// accumulators start at the bias, k ascends, nothing is split.  A tile is 64 rows x up to 256 columns, a workgroup 512 threads: wave w
// of 8 owns the 32-column tile w for both 32-row tiles (2 accumulators of 16 registers; two waves per SIMD give the matrix unit four
// independent chains); column tiles past L and the second row tile of a tile with <= 32 rows are skipped (wave-uniform).  Operands:
// lane l feeds A[row l & 31][k = l >> 5] and B[k = l >> 5][column l & 31]; its 16 results are column l & 31, rows
// (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).  Weights are [out][in], so B[k][j] = W[j][k]: a weight tile of 32 k is staged through LDS as
// Wl[j][33] with loads that run along k (lane t & 31 = k: 128 contiguous bytes per weight row), one k-tile ahead in registers so the
// loads of tile t + 1 fly during the products of tile t.  Odd row strides (33, 65, 257 floats) put the 32 rows a half-wave reads for one k
// on 32 banks.  Padding: k past K is +0 in A and -0 in W (their product -0 is the one addend that leaves EVERY accumulator as it is, a -0
// included); columns past L are forced to +0 when a stage's result becomes the next stage's A; rows past the tile's last are +0 in A and
// skip their stores.  A NaN or an infinity stays in its row: rows of A never mix.
// No atomics, no cross-workgroup traffic: two runs give the same bits.  fp contract is off in every body; the chains are explicit fmaf.
#pragma once
#include "learn_clock.h"

constexpr int kFwdM = 64;                     // rows of a tile (two 32-row MFMA tiles)
constexpr int kFwdKT = 32;                    // k of a staged weight tile
constexpr int kFwdWS = kFwdKT + 1;            // row stride of the staged tiles, floats
constexpr int kFwdCS = 65;                    // ... of the cosine image (and of the dueling head's A + 1 results)
constexpr int kFwdXS = 257;                   // ... of the activation image
constexpr int kFwdMaxL = 256;
constexpr int kFwdThreads = 512;              // 8 waves: one per 32-column tile of the widest layer
constexpr int kFwdMaxBlocks = 1 << 20;        // grid cap: more tiles than that and the workgroups stride

typedef float fwd_f16 __attribute__((ext_vector_type(16)));

struct IqnFwdParams {
    const void* states;
    const float *w_head, *b_head, *w_cos, *b_cos, *w_ff, *b_ff, *w_adv, *b_adv, *w_val, *b_val, *taus;
    const int64_t* idx;
    float *out_q, *out_quant, *out_taus, *out_cos;
    float* h;                                 // the workspace: [n][L]
    const TurnState* ts;                      // sgw_turn_iqn_forward: epoch and the turn in flight come from the device's turn state
    int64_t n, stride, num_envs, head_tiles, q_tiles;
    int32_t D, L, N, A, u8, agent0, R;
    uint32_t seed_lo, seed_hi, first_env, epoch, turn;
};

__device__ __forceinline__ float fwd_relu(const float x) { return x > 0.0f ? x : (x != x ? x : 0.0f); }

// acc[rt] += A[64][K] x W[rows][K]^T for the calling wave's column tile w, rt = the 32-row tile.
// HEAD: A's k-tile is staged from the states (row0 .. row0 + mrows) into As beside the weights; else A is an LDS image of stride `as`
// that holds every k < ceil32(K).  Ends with a barrier: the caller may overwrite A and Wl.
// TRANS: W is [K][rows] (the product with a weight's transpose: the backward's dz); its tile is staged with loads that run along the rows.
template <bool HEAD, bool U8, bool TRANS = false>
__device__ __forceinline__ void fwd_gemm(fwd_f16 (&acc)[2], const float* A, const int as, float* As, const IqnFwdParams& p, const int64_t row0,
                                         const int mrows, const float* __restrict__ W, const int rows, const int K, float* Wl, const int CT, const bool two) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 31, lk = lane >> 5;
    const int kq = tid & 31, j0 = tid >> 5;
    const bool c0 = w < CT;
    float wreg[16], areg[4];
    // every load is unconditional at a clamped address and its value is not looked at before the NEXT k-tile's LDS write, where the
    // padding is a select: no branch around a load, no wait per element, and the loads stay in flight during this tile's products
    const int jmax = rows - 1, kmax = K - 1, rmax = mrows - 1;
    auto load = [&](const int k0) {
        const int k = k0 + kq, kc = k < kmax ? k : kmax;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if constexpr (TRANS) {
                const int j = kq + 32 * (i & 7), jc = j < jmax ? j : jmax, kt = k0 + j0 + 16 * (i >> 3), ktc = kt < kmax ? kt : kmax;
                wreg[i] = W[(int64_t)ktc * rows + jc];
            } else {
                const int j = j0 + 16 * i, jc = j < jmax ? j : jmax;
                wreg[i] = W[(int64_t)jc * K + kc];
            }
        }
        if constexpr (HEAD) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = j0 + 16 * i, rc = r < rmax ? r : rmax;
                const int64_t at = (row0 + rc) * p.stride + kc;
                if constexpr (U8) areg[i] = (float)static_cast<const uint8_t*>(p.states)[at];
                else areg[i] = static_cast<const float*>(p.states)[at];
            }
        }
    };
    load(0);
    for (int k0 = 0; k0 < K; k0 += kFwdKT) {
        const bool kin = k0 + kq < K;
        __syncthreads();                      // the products of the previous k-tile have read Wl (and As)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if constexpr (TRANS) {
                const int j = kq + 32 * (i & 7), kt = j0 + 16 * (i >> 3);
                Wl[j * kFwdWS + kt] = (k0 + kt < K && j < rows) ? wreg[i] : -0.0f;
            } else {
                Wl[(j0 + 16 * i) * kFwdWS + kq] = (kin && j0 + 16 * i < rows) ? wreg[i] : -0.0f;
            }
        }
        if constexpr (HEAD) {
#pragma unroll
            for (int i = 0; i < 4; ++i) As[(j0 + 16 * i) * kFwdWS + kq] = (kin && j0 + 16 * i < mrows) ? areg[i] : 0.0f;
        }
        __syncthreads();
        if (k0 + kFwdKT < K) load(k0 + kFwdKT);
        if (!c0) continue;                    // (wave-uniform: a column tile past L has nothing to compute; the barriers above are shared)
        const float* a_at = HEAD ? As + lr * kFwdWS + lk : A + lr * as + k0 + lk;
        const int as_ = HEAD ? kFwdWS : as;
        const float* b_at = Wl + (w * 32 + lr) * kFwdWS + lk;
        if (two) {
#pragma unroll
            for (int s = 0; s < kFwdKT; s += 2) {
                const float b = b_at[s];
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_at[s], b, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_at[32 * as_ + s], b, acc[1], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int s = 0; s < kFwdKT; s += 2) acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_at[s], b_at[s], acc[0], 0, 0, 0);
        }
    }
    __syncthreads();
}

// every accumulator of the wave starts at its column's bias (a column past L: +0)
__device__ __forceinline__ void fwd_bias(fwd_f16 (&acc)[2], const float* __restrict__ bias, const int L) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lr = lane & 31;
    const int col = w * 32 + lr;
    const float b = col < L ? bias[col] : 0.0f;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[rt][r] = b;
}

// f(row of the tile, column, value) for every result the wave holds, if its column tile is below CT
template <typename F>
__device__ __forceinline__ void fwd_each(const fwd_f16 (&acc)[2], const int CT, const bool two, F f) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lr = lane & 31, lk = lane >> 5;
    if (w >= CT) return;
    const int col = w * 32 + lr;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        if (rt == 1 && !two) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) f(rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk, col, acc[rt][r]);
    }
}

// first launch: h = relu(states x w_head^T + b_head) for tiles of 64 states (U8: the states are uint8)
template <bool U8>
__global__ __launch_bounds__(kFwdThreads) void iqn_head_kernel(const IqnFwdParams p) {
#pragma clang fp contract(off)
    __shared__ float As[kFwdM * kFwdWS];
    __shared__ float Wl[kFwdMaxL * kFwdWS];
    const int L = p.L, CT = (L + 31) >> 5;
    for (int64_t tile = blockIdx.x; tile < p.head_tiles; tile += gridDim.x) {
        const int64_t row0 = tile * kFwdM;
        const int mrows = (int)(p.n - row0 < kFwdM ? p.n - row0 : kFwdM);
        const bool two = mrows > 32;
        fwd_f16 acc[2];
        fwd_bias(acc, p.b_head, L);
        fwd_gemm<true, U8>(acc, nullptr, 0, As, p, row0, mrows, p.w_head, L, p.D, Wl, CT, two);
        fwd_each(acc, CT, two, [&](const int row, const int col, const float v) {
            if (row < mrows && col < L) p.h[(row0 + row) * L + col] = fwd_relu(v);
        });
    }
}

// second launch: everything behind the head for tiles of R whole states = R N quantile rows.  CLOCKED (iqn_quantile_clocked_kernel): the drawn
// taus' turn is the low word of the learner clock's count, read once here; the epoch is the descriptor's
template <bool CLOCKED>
__device__ __forceinline__ void iqn_quantile_tiles(const IqnFwdParams& p, const sgw_learn_clock* clock) {
#pragma clang fp contract(off)
    __shared__ float X[kFwdM * kFwdXS];       // z, then y: [quantile row][L padded to whole column tiles]
    __shared__ float Cb[kFwdM * kFwdCS];      // the cosines [quantile row][64]; then adv_0 .. adv_(A-1), val of every quantile row
    __shared__ float Wl[kFwdMaxL * kFwdWS];
    __shared__ float tau_s[kFwdM], mean_s[kFwdM];
    __shared__ int state_s[kFwdM];            // the state (of the tile) a quantile row belongs to
    const int tid = threadIdx.x;
    const int N = p.N, A = p.A, L = p.L, R = p.R, CT = (L + 31) >> 5;
    uint32_t epoch = p.epoch, turn = p.turn;
    if constexpr (CLOCKED) {
        turn = (uint32_t)learn_clock_count(clock);
    } else if (p.ts) {                        // (uniform: scalar loads)
        epoch = p.ts->epoch;
        turn = p.ts->turn + 1u;
    }
    const uint32_t c3 = (epoch << 4) | SGW_STREAM_TAU;
    const float nan_f = __builtin_nanf("");
    for (int64_t tile = blockIdx.x; tile < p.q_tiles; tile += gridDim.x) {
        const int64_t row0 = tile * R;
        const int srows = (int)(p.n - row0 < R ? p.n - row0 : R);
        const int mv = srows * N;             // quantile rows that exist: they are rows row0 N .. row0 N + mv of every [n N] output
        const int64_t q0 = row0 * N;
        const bool two = mv > 32;
        // 1: taus
        if (tid < kFwdM) {
            float tau = 0.0f;
            int st = 0;
            if (tid < mv) {
                st = tid / N;
                const int q = tid - st * N;
                const int64_t k = row0 + st;
                if (p.taus) {
                    tau = p.taus[k * N + q];
                } else {
                    int64_t env, agent;
                    if (p.idx) {
                        const int64_t r = p.idx[k];
                        env = r % p.num_envs;
                        agent = r / p.num_envs;
                    } else {
                        env = k % p.num_envs;
                        agent = p.agent0 + k / p.num_envs;
                    }
                    const bool bad = agent < 0 || agent >= SGW_MAX_AGENTS || env < 0;      // (a key the host could not see)
                    const U4 w4 = philox4x32_10(((uint32_t)agent << 4) | (uint32_t)(q >> 2), turn, p.first_env + (uint32_t)env, c3, p.seed_lo, p.seed_hi);
                    tau = bad ? nan_f : (float)(word_of(w4, q & 3) >> 8) * 0x1p-24f;
                }
                if (p.out_taus) p.out_taus[q0 + tid] = tau;
            }
            tau_s[tid] = tau;
            state_s[tid] = st;
        }
        __syncthreads();
        // 2: the cosines
#pragma unroll 1
        for (int e = tid; e < kFwdM * SGW_IQN_N_COS; e += kFwdThreads) {
            const int m = e >> 6, i = e & 63;
            float c = 0.0f;
            if (m < mv) {
                const float pi_i = (float)(3.14159265358979323846 * (double)(i + 1));
                const float arg = tau_s[m] * pi_i;
                c = cosf(arg);
                if (p.out_cos) p.out_cos[q0 * SGW_IQN_N_COS + e] = c;
            }
            Cb[m * kFwdCS + i] = c;
        }
        // 3: e = relu(cos x w_cos^T + b_cos); z = h * e   (fwd_gemm's first barrier orders the writes of Cb before its reads)
        fwd_f16 acc[2];
        fwd_bias(acc, p.b_cos, L);
        fwd_gemm<false, false>(acc, Cb, kFwdCS, nullptr, p, 0, 0, p.w_cos, L, SGW_IQN_N_COS, Wl, CT, two);
        fwd_each(acc, CT, two, [&](const int m, const int col, const float v) {
            float z = 0.0f;
            if (m < mv && col < L) {
                const float hv = p.h[(row0 + state_s[m]) * L + col];
                z = hv * fwd_relu(v);
            }
            X[m * kFwdXS + col] = z;
        });
        // 4: y = relu(z x w_ff^T + b_ff), back into X once every wave has read z
        fwd_bias(acc, p.b_ff, L);
        fwd_gemm<false, false>(acc, X, kFwdXS, nullptr, p, 0, 0, p.w_ff, L, L, Wl, CT, two);
        fwd_each(acc, CT, two, [&](const int m, const int col, const float v) { X[m * kFwdXS + col] = col < L ? fwd_relu(v) : 0.0f; });
        __syncthreads();
        // 5: the dueling head: lane = quantile row, wave g takes outputs g, g + 8, ... (output A is the value); the weight row is wave-uniform
        {
            const int m = tid & 63, g = __builtin_amdgcn_readfirstlane(tid >> 6);
            const bool live = m < mv;
#pragma unroll 1
            for (int o = g; o <= A; o += 8) {
                const float* __restrict__ wrow = o < A ? p.w_adv + (int64_t)o * L : p.w_val;
                float s = o < A ? p.b_adv[o] : p.b_val[0];
                if (live)
                    for (int k = 0; k < L; ++k) s = fmaf(X[m * kFwdXS + k], wrow[k], s);
                Cb[m * kFwdCS + o] = s;
            }
        }
        __syncthreads();
        // 6: the mean over the actions, the quantiles
        if (tid < mv) {
            float s = Cb[tid * kFwdCS];
            for (int a = 1; a < A; ++a) s += Cb[tid * kFwdCS + a];
            mean_s[tid] = s / (float)A;
        }
        __syncthreads();
        for (int e = tid; e < mv * A; e += kFwdThreads) {
            const int m = e / A, a = e - m * A;
            const float sum = Cb[m * kFwdCS + A] + Cb[m * kFwdCS + a];
            const float qv = sum - mean_s[m];
            Cb[m * kFwdCS + a] = qv;
            if (p.out_quant) p.out_quant[q0 * A + e] = qv;
        }
        __syncthreads();
        // 7: the mean over the quantiles
        if (p.out_q) {
            for (int e = tid; e < srows * A; e += kFwdThreads) {
                const int st = e / A, a = e - st * A;
                float s = Cb[(st * N) * kFwdCS + a];
                for (int q = 1; q < N; ++q) s += Cb[(st * N + q) * kFwdCS + a];
                p.out_q[row0 * A + e] = s / (float)N;
            }
        }
        __syncthreads();                      // the next tile rewrites tau_s and Cb
    }
}

__global__ __launch_bounds__(kFwdThreads) void iqn_quantile_kernel(const IqnFwdParams p) { iqn_quantile_tiles<false>(p, nullptr); }

// sgw_iqn_forward_clocked's second launch (the head draws nothing: iqn_head_kernel serves both)
__global__ __launch_bounds__(kFwdThreads) void iqn_quantile_clocked_kernel(const IqnFwdParams p, const sgw_learn_clock* clock) {
    iqn_quantile_tiles<true>(p, clock);
}
