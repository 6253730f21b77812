// The noisy layers' weights (sgw_noisy_weights): what layers.py's NoisyLinear.forward does in front of F.linear -- epsilon.normal_(),
// weight + sigma * epsilon, for the weight and the bias of three layers, in each of the three network calls of a learner's step: 54 torch
// launches -- and what autograd does behind it for sigma (grad * epsilon), as ONE launch each way over a table of up to
// SGW_NOISY_MAX_JOBS tensors.  include/sgw.h states the arithmetic and the key of the drawn normals.
//
// The job table lies in the argument block (as iqn_wgrad_kernel's).  A workgroup of kBlock threads takes one chunk of kNoisyChunk = 4 kBlock
// elements of one job, found from the prefix of the jobs' chunk counts; a thread takes four consecutive elements, which is one Philox
// block, so a drawn block is computed once.  Tensors are aligned to their element only (value.bias has one element, a bias follows its
// weight anywhere), so every load and store is one dword.  No atomics, no LDS, no scratch; the product is rounded before the sum.
#pragma once
#include "learn_clock.h"

constexpr int kNoisyChunk = 4 * kBlock;

struct NoisyJob {
    const float *a, *b, *eps;                 // forward: weight, sigma, eps_in (or NULL: drawn); backward: grad_eff, -, eps
    float *out, *out_eps;                     // forward: out_eff, out_eps (or NULL); backward: out_grad_sigma, -
    int64_t count;
    uint32_t c3;                              // the draw's fourth counter word: tensor_id << 4 | SGW_STREAM_NOISE
    int32_t chunk0;                           // the job's first chunk of the launch (INT32_MAX in an unused slot)
};

struct NoisyParams {
    NoisyJob job[SGW_NOISY_MAX_JOBS];
    uint32_t seed_lo, seed_hi, draw_lo, draw_hi;
};

// the four normals of Philox block `blk` of draw (draw_lo, draw_hi): Box-Muller over the word pairs (x, y) and (z, w)
__device__ __forceinline__ void noisy_normals(const NoisyParams& p, const uint32_t draw_lo, const uint32_t draw_hi, const uint32_t c3, const uint32_t blk,
                                              float (&n)[4]) {
#pragma clang fp contract(off)
    const U4 w = philox4x32_10(blk, draw_lo, draw_hi, c3, p.seed_lo, p.seed_hi);
    const uint32_t wa[2] = {w.x, w.z}, wb[2] = {w.y, w.w};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float u1 = (float)((wa[h] >> 8) + 1u) * 0x1p-24f;          // (0, 1]: exact
        const float u2 = (float)(wb[h] >> 8) * 0x1p-24f;                 // [0, 1): exact
        const float r = sqrtf(-2.0f * logf(u1));
        const float arg = 6.28318530717958647692f * u2;
        n[2 * h] = r * cosf(arg);
        n[2 * h + 1] = r * sinf(arg);
    }
}

// one chunk of one job; the draw's two words come from the argument block (noisy_kernel) or from the learner clock (noisy_clocked_kernel)
template <bool BACKWARD>
__device__ __forceinline__ void noisy_chunk(const NoisyParams& p, const uint32_t draw_lo, const uint32_t draw_hi) {
#pragma clang fp contract(off)
    const int chunk = (int)blockIdx.x;
    int ji = 0;
#pragma unroll
    for (int i = 1; i < SGW_NOISY_MAX_JOBS; ++i) ji = chunk >= p.job[i].chunk0 ? i : ji;
    const NoisyJob& jb = p.job[ji];
    const int64_t count = jb.count;
    const int64_t i0 = (int64_t)(chunk - jb.chunk0) * kNoisyChunk + 4 * (int64_t)threadIdx.x;
    if (i0 >= count) return;
    if constexpr (BACKWARD) {
        const float* __restrict__ g = jb.a;
        const float* __restrict__ eps = jb.eps;
        float* __restrict__ out = jb.out;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = i0 + k;
            if (i < count) out[i] = g[i] * eps[i];
        }
    } else {
        const float* __restrict__ weight = jb.a;
        const float* __restrict__ sigma = jb.b;
        const float* __restrict__ eps_in = jb.eps;
        float* __restrict__ out = jb.out;
        float* __restrict__ out_eps = jb.out_eps;
        float n[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (!eps_in) noisy_normals(p, draw_lo, draw_hi, jb.c3, (uint32_t)(i0 >> 2), n);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = i0 + k;
            if (i < count) {
                const float e = eps_in ? eps_in[i] : n[k];
                const float prod = sigma[i] * e;
                out[i] = weight[i] + prod;
                if (out_eps) out_eps[i] = e;
            }
        }
    }
}

template <bool BACKWARD>
__global__ __launch_bounds__(kBlock) void noisy_kernel(const NoisyParams p) {
    noisy_chunk<BACKWARD>(p, p.draw_lo, p.draw_hi);
}

// sgw_noisy_weights_clocked, forward mode (the backward draws nothing: it launches noisy_kernel<true>): draw = clock->count, both words
__global__ __launch_bounds__(kBlock) void noisy_clocked_kernel(const NoisyParams p, const sgw_learn_clock* clock) {
    const uint64_t draw = learn_clock_count(clock);
    noisy_chunk<false>(p, (uint32_t)draw, (uint32_t)(draw >> 32));
}
