// Adam, gradient clipping and the soft update (sgw_adam_step): what sorrel/models/pytorch/iqn.py:405-410 -- clip_grad_norm_,
// optimizer.step(), soft_update() -- and ppo.py:283-285 run after loss.backward(), some eighty small torch launches on device tensors,
// for a whole parameter list in two launches (one when nothing is clipped and the step is counted by the host).  include/sgw.h states
// the arithmetic; this file follows it term by term.
//
// The layout: a multi-tensor kernel over a table in device memory (so that a call can be recorded).  sgw_adam_plan cuts every tensor
// that has a gradient into chunks of kAdamChunk elements and writes T records and the chunk map; at most kAdamMaxBlocks workgroups
// stride over the map.  Lane t of a workgroup owns four groups of four consecutive elements of its chunk -- elements 4 (t + 256 r) + e --
// and reads and writes each group as 16 bytes (float32) or twice 16 bytes (float64) where every base of the tensor is 16-byte aligned;
// a tensor with an unaligned base and the ragged end of a last chunk go element by element.  The ownership does not depend on the
// access width, so neither does the order of the norm's sum.
//   adam_norm_kernel    (SGW_ADAM_CLIP_NORM, or a device step_state)  one float64 partial per CHUNK -- lane sums in element order, the
//                       block tree of block_reduce.h -- so the result does not depend on the grid; block 0 advances the step state
//   adam_apply_kernel   every workgroup first re-merges the partials in the contract's order (chunks serially into tensor sums, lane i
//                       takes tensors i, i + 256, ..., the tree merges the lanes: a few hundred doubles for the networks at hand),
//                       forms c, then updates its own chunks: p, g, m, v, t in; p, m, v, t and optionally g out
// No grid barrier, no "last block" counter, no floating-point atomics.  Every function that does arithmetic carries fp contract off (the
// pragma is lexical); the two fusions of the contract are explicit fma calls.  p, m, v and t are read again by the next step: plain stores.
#pragma once

constexpr int kAdamChunk = SGW_ADAM_CHUNK;
constexpr int kAdamMaxBlocks = 2048;          // grid cap: 8 workgroups per CU on 256 CUs
constexpr int kAdamMaxTensors = SGW_ADAM_MAX_TENSORS;
constexpr int kAdamVec = 1;                   // AdamRec::flags: every base of the tensor is 16-byte aligned
static_assert(kAdamChunk == 16 * kBlock, "a lane owns four groups of four elements");

struct AdamRec {                              // the device's record: sgw_adam_tensor with the reserved word put to use
    void* p;
    void* g;
    void* m;
    void* v;
    void* t;
    int64_t numel;
    double lr;
    int32_t first_chunk, flags;
};
static_assert(sizeof(AdamRec) == sizeof(sgw_adam_tensor) && sizeof(AdamRec) == 64, "the image holds T records of 64 bytes");
struct AdamChunk { int32_t tensor, chunk; };

struct AdamParams {
    const AdamRec* recs;
    const AdamChunk* map;
    double* partials;                         // [chunks]
    const void* coef;
    sgw_adam_step_state* state;
    double* out_norm;
    double max_norm, beta1, beta2, omb1, omb2, eps, tau, omtau, bc1, bc2_sqrt;
    int32_t T, nchunks, zero;
};

__device__ __forceinline__ int64_t adam_chunks_of(const void* grad, const int64_t numel) { return grad && numel > 0 ? (numel + (kAdamChunk - 1)) / kAdamChunk : 0; }

// the table hands out pointers whose address space the compiler cannot see: say that they are global memory (global_load / global_store
// instead of flat ones)
#define ADAM_GLOBAL __attribute__((address_space(1)))

// a group of four elements from `at` on, of which `left` exist (a missing one reads as +0); 16-byte accesses for a whole group of a VEC tensor
template <class F>
__device__ __forceinline__ void adam_load4(const void* base, const int64_t at, const int left, const bool vec, F (&x)[4]) {
    const ADAM_GLOBAL F* q = (const ADAM_GLOBAL F*)base + at;
    if (vec && left >= 4) {
        if constexpr (sizeof(F) == 8) {
            const cat_d2 a = ((const ADAM_GLOBAL cat_d2*)q)[0], b = ((const ADAM_GLOBAL cat_d2*)q)[1];
            x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y;
        } else {
            const cat_f4 a = ((const ADAM_GLOBAL cat_f4*)q)[0];
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = e < left ? q[e] : (F)0;
    }
}

template <class F>
__device__ __forceinline__ void adam_store4(void* base, const int64_t at, const int left, const bool vec, const F (&x)[4]) {
    ADAM_GLOBAL F* q = (ADAM_GLOBAL F*)base + at;
    if (vec && left >= 4) {
        if constexpr (sizeof(F) == 8) {
            cat_d2 a, b;
            a.x = x[0]; a.y = x[1]; b.x = x[2]; b.y = x[3];
            ((ADAM_GLOBAL cat_d2*)q)[0] = a;
            ((ADAM_GLOBAL cat_d2*)q)[1] = b;
        } else {
            cat_f4 a;
            a.x = x[0]; a.y = x[1]; a.z = x[2]; a.w = x[3];
            ((ADAM_GLOBAL cat_f4*)q)[0] = a;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < left) q[e] = x[e];
    }
}

__device__ __forceinline__ float adam_sqrt(const float x) { return sqrtf(x); }
__device__ __forceinline__ double adam_sqrt(const double x) { return sqrt(x); }
__device__ __forceinline__ float adam_fma(const float a, const float b, const float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double adam_fma(const double a, const double b, const double c) { return fma(a, b, c); }

// first launch: one partial per chunk; block 0 advances the step state
template <class F>
__global__ __launch_bounds__(kBlock) void adam_norm_kernel(const AdamParams p, const int norm) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    if (p.state && blockIdx.x == 0 && tid == 0) {
        p.state->step += 1;
        p.state->beta1_pow *= p.beta1;
        p.state->beta2_pow *= p.beta2;
    }
    if (!norm) return;
    __shared__ double red[1][kBlock];
    for (int chunk = blockIdx.x; chunk < p.nchunks; chunk += gridDim.x) {
        const AdamChunk ce = p.map[chunk];
        const AdamRec rec = p.recs[ce.tensor];
        const int64_t base = (int64_t)ce.chunk * kAdamChunk;
        const int n = (int)(rec.numel - base < kAdamChunk ? rec.numel - base : kAdamChunk);
        const bool vec = rec.flags & kAdamVec;
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int first = 4 * (tid + kBlock * r), left = n - first;
            if (left > 0) {
                F g[4];
                adam_load4<F>(rec.g, base + first, left, vec, g);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double sq = (double)g[e] * (double)g[e];       // (a missing element adds +0 to a sum that is never -0)
                    acc += sq;
                }
            }
        }
        const double sums[1] = {acc};
        block_tree<1>(sums, red, TreeSum{});
        if (tid == 0) p.partials[chunk] = red[0][0];
    }
}

// CLIP: SGW_ADAM_CLIP_*
template <class F, int CLIP>
__global__ __launch_bounds__(kBlock) void adam_apply_kernel(const AdamParams p) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    F c = (F)1;
    double norm = __builtin_nan("");
    if constexpr (CLIP == SGW_ADAM_CLIP_NORM) {
        __shared__ double red[1][kBlock];
        double s = 0.0;
        for (int k = tid; k < p.T; k += kBlock) {
            const AdamRec* rec = p.recs + k;
            const int64_t nc = adam_chunks_of(rec->g, rec->numel);
            const double* part = p.partials + rec->first_chunk;
            double sk = 0.0;
            for (int64_t j = 0; j < nc; ++j) sk += part[j];
            s += sk;
        }
        const double sums[1] = {s};
        block_tree<1>(sums, red, TreeSum{});
        norm = sqrt(red[0][0]);
        const F room = (F)norm + (F)1e-6;
        c = (F)p.max_norm / room;
        c = c > (F)1 ? (F)1 : c;
    } else if constexpr (CLIP == SGW_ADAM_CLIP_COEF) {
        c = *reinterpret_cast<const F*>(p.coef);
    }
    if (p.out_norm && blockIdx.x == 0 && tid == 0) {
        p.out_norm[0] = norm;
        p.out_norm[1] = (double)c;
    }
    double bc1 = p.bc1, bc2_sqrt = p.bc2_sqrt;
    if (p.state) {
        bc1 = 1.0 - p.state->beta1_pow;
        const double bc2 = 1.0 - p.state->beta2_pow;
        bc2_sqrt = sqrt(bc2);
    }
    const F omb1 = (F)p.omb1, omb2 = (F)p.omb2, b2 = (F)p.beta2, bcs = (F)bc2_sqrt, eps = (F)p.eps, tau = (F)p.tau, omtau = (F)p.omtau;
    for (int chunk = blockIdx.x; chunk < p.nchunks; chunk += gridDim.x) {
        const AdamChunk ce = p.map[chunk];
        const AdamRec rec = p.recs[ce.tensor];
        const int64_t base = (int64_t)ce.chunk * kAdamChunk;
        const int n = (int)(rec.numel - base < kAdamChunk ? rec.numel - base : kAdamChunk);
        const bool vec = rec.flags & kAdamVec;
        const double step_size = rec.lr / bc1;
        const F nss = (F)(-step_size);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int first = 4 * (tid + kBlock * r), left = n - first;
            if (left <= 0) continue;
            const int64_t at = base + first;
            F pp[4], g[4], m[4], v[4], t[4] = {(F)0, (F)0, (F)0, (F)0};
            adam_load4<F>(rec.p, at, left, vec, pp);
            adam_load4<F>(rec.g, at, left, vec, g);
            adam_load4<F>(rec.m, at, left, vec, m);
            adam_load4<F>(rec.v, at, left, vec, v);
            if (rec.t) adam_load4<F>(rec.t, at, left, vec, t);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const F ge = CLIP == SGW_ADAM_CLIP_NONE ? g[e] : g[e] * c;
                const F d = ge - m[e];
                m[e] = adam_fma(omb1, d, m[e]);
                const F vb = v[e] * b2;
                const F w = omb2 * ge;
                v[e] = adam_fma(w, ge, vb);
                const F root = adam_sqrt(v[e]);
                const F scaled = root / bcs;
                const F denom = scaled + eps;
                const F num = nss * m[e];
                const F quo = num / denom;
                pp[e] = pp[e] + quo;
                const F a = tau * pp[e];
                const F b = omtau * t[e];
                t[e] = a + b;
                g[e] = (F)0;
            }
            adam_store4<F>(rec.p, at, left, vec, pp);
            adam_store4<F>(rec.m, at, left, vec, m);
            adam_store4<F>(rec.v, at, left, vec, v);
            if (rec.t) adam_store4<F>(rec.t, at, left, vec, t);
            if (p.zero) adam_store4<F>(rec.g, at, left, vec, g);
        }
    }
}

// host side
inline int64_t adam_chunks(const int64_t numel) { return numel / kAdamChunk + (numel % kAdamChunk ? 1 : 0); }
inline unsigned adam_blocks(const int64_t chunks) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(chunks, kAdamMaxBlocks)); }

template <class F>
void launch_adam_apply(const AdamParams& p, const int clip, const unsigned blocks, hipStream_t s) {
    if (clip == SGW_ADAM_CLIP_NORM) hipLaunchKernelGGL((adam_apply_kernel<F, SGW_ADAM_CLIP_NORM>), dim3(blocks), dim3(kBlock), 0, s, p);
    else if (clip == SGW_ADAM_CLIP_COEF) hipLaunchKernelGGL((adam_apply_kernel<F, SGW_ADAM_CLIP_COEF>), dim3(blocks), dim3(kBlock), 0, s, p);
    else hipLaunchKernelGGL((adam_apply_kernel<F, SGW_ADAM_CLIP_NONE>), dim3(blocks), dim3(kBlock), 0, s, p);
}
