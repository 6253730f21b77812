// IQN's network backward (sgw_iqn_backward): from dL/dquantiles to the gradients of the ten effective weights, what torch's autograd does
// behind sorrel/models/pytorch/iqn.py:322-412's loss.backward() through two dozen launches.  include/sgw.h states the arithmetic; this file
// follows it term by term.
//
// Two launches.  iqn_bwd_rows_kernel is iqn_quantile_kernel run forwards and then backwards for the same tiles of R = 64 / N whole states:
// taus -> cosines -> the embedding GEMM and z -> the noisy GEMM and y (the forward's own device functions: the same bits), then dO (the
// dueling head's backward), dy on the vector unit (A + 1 <= 65 terms per element, as the forward's head), dz = dy x w_ff (fwd_gemm over
// w_ff TRANSPOSED, staged with loads that run along the output index), de and the serial sum over a state's quantiles that is dh.  e waits
// in de's place of the workspace between the two passes: dz lands in the thread that computed e.  A learner's batch is a sampled one (64 states
// = 768 quantile rows in the reference), so the [n N][L] intermediates z, y, dy, de (and c, dO, dhp) go through the workspace on purpose.
// iqn_wgrad_kernel then forms every weight gradient as ONE chain over the batch rows: a wave owns one 32 x 32 tile of one gradient and
// runs __builtin_amdgcn_mfma_f32_32x32x2f32 over ALL rows m ascending, two per instruction, with G[m][j0 .. j0 + 31] as A and
// Act[m][k0 .. k0 + 31] as B read straight from memory (128 contiguous bytes per half-wave), kBwdAhead row pairs ahead in registers.  The
// bias gradient is the column behind the last of Act, whose value is 1.  Five jobs (advantage, value, noisy, embedding, head) share the
// launch through a table in the argument block.  Serial in M: the time grows with the batch and no more than (tiles) waves work; a
// split-M variant would need a merge and is not built.  Padding as in the forward: a row past the last (an odd M) and a column past the
// edge are +0 in A and -0 in B; rows past the edge skip their stores.  No atomics, no LDS in the second launch: two runs give the same bits.
#pragma once

constexpr int kBwdJobs = 5;
constexpr int kBwdWaves = 4;                  // waves (= tiles) of an iqn_wgrad_kernel workgroup
constexpr int kBwdAhead = 8;                  // row pairs a wave loads ahead of its matrix instructions

struct IqnBwdParams {
    IqnFwdParams f;                           // states, the weights, taus, h, the sizes and the tiling of iqn_quantile_kernel
    const float* grad;                        // dL/dquantiles [n N][A]
    float *z, *y, *dy, *de, *c, *dO, *dhp;    // the workspace: [n N][L] x 4, [n N][64], [n N][A + 1], [n][L]
    float* out_dh;                            // [n][L], or NULL
};

struct IqnWgradJob {
    const float* G;                           // [M] rows of J gradients, gs elements apart
    const void* act;                          // [M] rows of K activations (float32, or uint8: u8), as elements apart
    float *out_w, *out_b;                     // [J][K] and [J]; either may be NULL
    int64_t M, gs, as;
    int32_t J, K, u8, kt0, kts, tile0;        // the job's column tiles kt0 .. kt0 + kts (the bias column is column K); tile0: its first tile of the launch
};

struct IqnWgradParams {
    IqnWgradJob job[kBwdJobs];
    int32_t tiles;
};

// torch's threshold_backward on the stored activation: 0 at 0, a NaN passes the gradient
__device__ __forceinline__ bool bwd_mask(const float x) { return !(x <= 0.0f); }

// first launch: the forward behind h again, then its backward down to de and dhp, for tiles of R whole states = R N quantile rows
__global__ __launch_bounds__(kFwdThreads) void iqn_bwd_rows_kernel(const IqnBwdParams b) {
#pragma clang fp contract(off)
    __shared__ float X[kFwdM * kFwdXS];       // z, y, dy, then dz * e: [quantile row][L padded to whole column tiles]
    __shared__ float Cb[kFwdM * kFwdCS];      // the cosines [quantile row][64]; then dO [quantile row][A + 1]
    __shared__ float Wl[kFwdMaxL * kFwdWS];
    __shared__ float tau_s[kFwdM];
    __shared__ int state_s[kFwdM];
    const IqnFwdParams& p = b.f;
    const int tid = threadIdx.x;
    const int N = p.N, A = p.A, R = p.R, CT = (p.L + 31) >> 5;
    for (int64_t tile = blockIdx.x; tile < p.q_tiles; tile += gridDim.x) {
        // (L is opaque per tile: the addresses of three GEMMs' staged loads and of the epilogues' elements, hoisted out of this loop, would
        // not fit the registers)
        int L = p.L;
        asm volatile("" : "+s"(L));
        const int64_t row0 = tile * R;
        const int srows = (int)(p.n - row0 < R ? p.n - row0 : R);
        const int mv = srows * N;
        const int64_t q0 = row0 * N;
        const bool two = mv > 32;
        // the tile's part of every [n N] and [n] array: a uniform base, so an element's address is one 32-bit offset
        const float* __restrict__ ht = p.h + row0 * L;
        float* __restrict__ zt = b.z + q0 * L;
        float* __restrict__ yt = b.y + q0 * L;
        float* __restrict__ dyt = b.dy + q0 * L;
        float* __restrict__ det = b.de + q0 * L;
        float* __restrict__ dOt = b.dO + q0 * (A + 1);
        // 1: taus
        if (tid < kFwdM) {
            const bool live = tid < mv;
            tau_s[tid] = live ? p.taus[q0 + tid] : 0.0f;
            state_s[tid] = live ? tid / N : 0;
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
                b.c[q0 * SGW_IQN_N_COS + e] = c;
            }
            Cb[m * kFwdCS + i] = c;
        }
        // 3: e = relu(cos x w_cos^T + b_cos), which waits in de's place for step 8; z = h * e
        fwd_f16 acc[2];
        fwd_bias(acc, p.b_cos, L);
        fwd_gemm<false, false>(acc, Cb, kFwdCS, nullptr, p, 0, 0, p.w_cos, L, SGW_IQN_N_COS, Wl, CT, two);
        fwd_each(acc, CT, two, [&](const int m, const int col, const float v) {
            float z = 0.0f;
            if (m < mv && col < L) {
                const float hv = ht[state_s[m] * L + col];
                const float e = fwd_relu(v);
                z = hv * e;
                zt[m * L + col] = z;
                det[m * L + col] = e;
            }
            X[m * kFwdXS + col] = z;
        });
        // 4: y = relu(z x w_ff^T + b_ff), back into X once every wave has read z
        fwd_bias(acc, p.b_ff, L);
        fwd_gemm<false, false>(acc, X, kFwdXS, nullptr, p, 0, 0, p.w_ff, L, L, Wl, CT, two);
        fwd_each(acc, CT, two, [&](const int m, const int col, const float v) {
            const float y = col < L ? fwd_relu(v) : 0.0f;
            if (m < mv && col < L) yt[m * L + col] = y;
            X[m * kFwdXS + col] = y;
        });
        // 5: dO = (dadv_0 .. dadv_(A-1), dval) of every quantile row, over the cosines (the embedding GEMM ended with a barrier)
        if (tid < mv) {
            const float* __restrict__ g = b.grad + q0 * A + tid * A;
            float G = g[0];
            for (int a = 1; a < A; ++a) G += g[a];
            const float share = G / (float)A;
            for (int a = 0; a < A; ++a) {
                const float d = g[a] - share;
                Cb[tid * kFwdCS + a] = d;
                dOt[tid * (A + 1) + a] = d;
            }
            Cb[tid * kFwdCS + A] = G;
            dOt[tid * (A + 1) + A] = G;
        }
        __syncthreads();
        // 6: dy over y: lane = quantile row, wave g takes columns g, g + 8, ...; the weight column is wave-uniform
        {
            const int m = tid & 63, g = __builtin_amdgcn_readfirstlane(tid >> 6);
            const bool live = m < mv;
#pragma unroll 1
            for (int j = g; j < L; j += 8) {
                float s = 0.0f;
                if (live) {
                    for (int o = 0; o < A; ++o) s = fmaf(Cb[m * kFwdCS + o], p.w_adv[(int64_t)o * L + j], s);
                    s = fmaf(Cb[m * kFwdCS + A], p.w_val[j], s);
                }
                const float y = X[m * kFwdXS + j];
                X[m * kFwdXS + j] = live && bwd_mask(y) ? s : 0.0f;
            }
        }
        __syncthreads();
        for (int e = tid; e < mv * L; e += kFwdThreads) {
            const int m = e / L, col = e - m * L;
            dyt[e] = X[m * kFwdXS + col];
        }
        // 7: dz = dy x w_ff: the chains start at +0 and run over w_ff's rows
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[rt][r] = 0.0f;
        fwd_gemm<false, false, true>(acc, X, kFwdXS, nullptr, p, 0, 0, p.w_ff, L, L, Wl, CT, two);
        // 8: de = relu'(e) dz h over e (the thread that wrote e reads it: dz lands in the lane and register that computed e); dz * e into
        // X for the sums over the quantiles
        fwd_each(acc, CT, two, [&](const int m, const int col, const float dz) {
            if (m < mv && col < L) {
                const float hv = ht[state_s[m] * L + col];
                const float e = det[m * L + col];
                const float de = dz * hv;
                det[m * L + col] = bwd_mask(e) ? de : 0.0f;
                X[m * kFwdXS + col] = dz * e;
            }
        });
        __syncthreads();
        for (int e = tid; e < srows * L; e += kFwdThreads) {
            const int st = e / L, k = e - st * L;
            float s = X[(st * N) * kFwdXS + k];
            for (int q = 1; q < N; ++q) s += X[(st * N + q) * kFwdXS + k];
            if (b.out_dh) b.out_dh[row0 * L + e] = s;
            b.dhp[row0 * L + e] = bwd_mask(ht[e]) ? s : 0.0f;
        }
        __syncthreads();                      // the next tile rewrites tau_s, Cb and X
    }
}

// second launch: wave = one 32 x 32 tile of one job's out[j][k] = chain over m of G[m][j] * act[m][k] (column K: act = 1, the bias)
__global__ __launch_bounds__(64 * kBwdWaves) void iqn_wgrad_kernel(const IqnWgradParams p) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, lr = lane & 31, lk = lane >> 5;
    const int tile = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kBwdWaves + (threadIdx.x >> 6)));
    if (tile >= p.tiles) return;
    int ji = 0;
#pragma unroll
    for (int i = 1; i < kBwdJobs; ++i) ji = tile >= p.job[i].tile0 ? i : ji;
    const IqnWgradJob& jb = p.job[ji];
    const int t = tile - jb.tile0, jt = t / jb.kts, kt = jb.kt0 + t - jt * jb.kts;
    const int J = jb.J, K = jb.K;
    const int j = jt * 32 + lr, col = kt * 32 + lr;
    const bool jin = j < J, cin = col <= K, one = col == K;
    const int64_t M = jb.M, gs = jb.gs, as = jb.as;
    const float* __restrict__ G = jb.G + (jin ? j : J - 1);
    const int cc = col < K ? col : K - 1;
    const float* __restrict__ actf = static_cast<const float*>(jb.act) + cc;
    const uint8_t* __restrict__ actb = static_cast<const uint8_t*>(jb.act) + cc;
    const bool u8 = jb.u8 != 0;
    // every load is unconditional at a clamped address; the padding is a select where the value is used
    auto load = [&](const int64_t m0, float (&a)[kBwdAhead], float (&v)[kBwdAhead]) {
#pragma unroll
        for (int i = 0; i < kBwdAhead; ++i) {
            const int64_t m = m0 + 2 * i + lk, mc = m < M ? m : M - 1;
            a[i] = G[mc * gs];
            v[i] = u8 ? (float)actb[mc * as] : actf[mc * as];
        }
    };
    fwd_f16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    float a[kBwdAhead], v[kBwdAhead], na[kBwdAhead], nv[kBwdAhead];
    load(0, a, v);
    for (int64_t m0 = 0; m0 < M; m0 += 2 * kBwdAhead) {
        load(m0 + 2 * kBwdAhead, na, nv);
#pragma unroll
        for (int i = 0; i < kBwdAhead; ++i) {
            if (m0 + 2 * i < M) {             // (wave-uniform)
                const bool in = m0 + 2 * i + lk < M;
                const float av = in && jin ? a[i] : 0.0f;
                const float bv = in && cin ? (one ? 1.0f : v[i]) : -0.0f;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
            }
            a[i] = na[i];
            v[i] = nv[i];
        }
    }
    if (!cin) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = jt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (row >= J) continue;
        if (!one) {
            if (jb.out_w) jb.out_w[(int64_t)row * K + col] = acc[r];
        } else if (jb.out_b) {
            jb.out_b[row] = acc[r];
        }
    }
}
