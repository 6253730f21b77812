// Replay batches (sgw_sample): a frame-stacked batch gathered from a replay ring in one launch.
//
// Work item w = k * (F + 1) + j is ONE source row: frame j of sample k, row (t + j, e) of the ring.  It is read once and stored to
// out_states frame j (j < F) and to out_next_states frame j - 1 (j >= 1): F + 1 row reads per sample instead of the 2 F of two
// separate gathers.  A wave takes a row; the waves of the grid stride over the items.  A row moves in pieces of kSamplePieces loads
// per lane, and the loop is software-pipelined over the pieces of ALL the rows of a wave: the loads of the next piece (the next row,
// when this was the row's last piece) are issued before the stores of the current one, so two pieces are in flight per wave.
// Indices are wave-uniform: read from starts / envs, or recomputed by every wave from one Philox block (no index pre-pass).
#pragma once
#include "learn_clock.h"

constexpr int kSamplePieces = 8;            // loads per lane and piece (dword variant); the 16-byte variant issues kSamplePieces / 2
constexpr int kSampleMaxBlocks = 1536;      // grid cap: 6144 waves, 24 per CU on 256 CUs (all resident at once: the kernels reach 7 waves per
                                            // SIMD) -- more items than that and the waves stride

struct SampleParams {
    const void* states;
    const void* actions;
    const float* rewards;
    const float* dones;
    const int64_t* starts;
    const int64_t* envs;
    const uint64_t* draw_count;
    float* out_states;
    float* out_next;
    int64_t* out_actions;
    float* out_rewards;
    float* out_dones;
    float* out_valid;
    int64_t* out_index;
    int64_t n, num_envs, num_starts, R;
    int64_t step_k;                                 // the grid's waves / (F + 1) ...
    int64_t sts, ses, scs, sce;                     // state / scalar strides (turn, env), in elements
    uint64_t draw;
    uint32_t seed_lo, seed_hi;
    int32_t step_j;                                 // ... and % (F + 1): how far a wave's item moves per row
    int32_t F, act_u8, pieces;                      // pieces per row = ceil(R / (64 * loads per piece * VEC))
};

// where one work item reads and writes (wave-uniform)
struct SampleRow {
    int64_t src;      // element offset of the row in `states` (0 -- a row that exists -- when the sample's index is out of range)
    int64_t dst;      // element offset of frame j of sample k in out_states; out_next_states holds it one frame earlier
    bool to_states, to_next;      // both false: nothing is stored
};

// Wave-uniform reads of the ring's scalars and of the index lists go through the constant address space: the compiler then issues
// scalar loads, which the vector loads in flight do not have to be waited for (vmcnt counts in order).  Nothing read this way is
// written by this kernel.
#define SGW_CONSTANT_AS __attribute__((address_space(4)))
template <typename T>
__device__ __forceinline__ T uniform_load(const T* q, const int64_t i) {
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    return ((const SGW_CONSTANT_AS T*)q)[i];
#pragma clang diagnostic pop
}

template <int VEC, bool U8>
struct SamplePiece {
    typedef float vfloat4 __attribute__((ext_vector_type(4)));
    static constexpr int N = VEC == 4 ? kSamplePieces / 2 : kSamplePieces;
    typedef typename std::conditional<VEC == 4, vfloat4, float>::type Out;
    typedef typename std::conditional<U8, typename std::conditional<VEC == 4, uint32_t, uint8_t>::type, Out>::type In;
    In v[N];

    static __device__ __forceinline__ Out widen(const In x) {
        if constexpr (!U8) return x;
        else if constexpr (VEC == 4) return Out{(float)(x & 0xffu), (float)((x >> 8) & 0xffu), (float)((x >> 16) & 0xffu), (float)(x >> 24)};
        else return (float)x;
    }
    // units of VEC elements: lane l of load i of piece c takes unit (c * N + i) * 64 + l.  Loads are unconditional -- a lane past the
    // row's end reads the row's last unit again -- so that no branch sits between them and the compiler can count them.
    __device__ __forceinline__ void load(const SampleParams& p, const SampleRow& r, const int c, const int lane) {
        const In* s = reinterpret_cast<const In*>(p.states) + r.src / VEC;
        const int last = (int)(p.R / VEC) - 1;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int u = (c * N + i) * 64 + lane;
            v[i] = s[u < last ? u : last];
        }
    }
    __device__ __forceinline__ void store(const SampleParams& p, const SampleRow& r, const int c, const int lane) const {
        const int units = (int)(p.R / VEC);
        Out* d0 = reinterpret_cast<Out*>(p.out_states) + r.dst / VEC;
        Out* d1 = reinterpret_cast<Out*>(p.out_next) + (r.to_next ? r.dst - p.R : 0) / VEC;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int u = (c * N + i) * 64 + lane;
            const Out x = widen(v[i]);
            if (u < units && r.to_states) __builtin_nontemporal_store(x, d0 + u);
            if (u < units && r.to_next) __builtin_nontemporal_store(x, d1 + u);
        }
    }
};

// Frame j of sample k: the sample's (start, env) -- given or drawn --, the row's addresses, and (the wave of the sample's last stacked
// frame, lane 0) the sample's scalars.
__device__ __forceinline__ SampleRow sample_locate(const SampleParams& p, const int64_t num_starts, const int64_t k, const int j, const uint64_t counter,
                                                   const int lane) {
    const int F = p.F;
    int64_t t, e;
    if (p.starts) {
        t = uniform_load(p.starts, k);
        e = uniform_load(p.envs, k);
    } else {
        // u32 numbers 2k and 2k + 1 of the stream: words (0, 1) or (2, 3) of block k >> 1
        const U4 b = philox4x32_10((uint32_t)(k >> 1), (uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)SGW_STREAM_SAMPLE, p.seed_lo, p.seed_hi);
        const bool odd = (k & 1) != 0;
        t = __builtin_amdgcn_readfirstlane(__umulhi(odd ? b.z : b.x, (uint32_t)num_starts));
        e = __builtin_amdgcn_readfirstlane(__umulhi(odd ? b.w : b.y, (uint32_t)p.num_envs));
    }
    SampleRow r;
    const bool ok = t >= 0 && t < num_starts && e >= 0 && e < p.num_envs;      // a given index out of range: no address is formed from it
    r.to_states = ok && j < F;
    r.to_next = ok && j >= 1;
    r.src = r.dst = 0;
    if (!ok) return r;
    r.src = (t + j) * p.sts + e * p.ses;
    r.dst = (k * F + j) * p.R;
    if (j == F - 1) {
        const int64_t at = (t + j) * p.scs + e * p.sce;
        const int64_t action = p.act_u8 ? (int64_t)uniform_load(reinterpret_cast<const uint8_t*>(p.actions), at) : uniform_load(reinterpret_cast<const int64_t*>(p.actions), at);
        const float reward = uniform_load(p.rewards, at), done = uniform_load(p.dones, at);
        bool ended = false;
        for (int f = 0; f < F - 1; ++f) ended |= uniform_load(p.dones, (t + f) * p.scs + e * p.sce) != 0.0f;
        if (lane == 0) {
            p.out_actions[k] = action;
            p.out_rewards[k] = reward;
            p.out_dones[k] = done;
            p.out_valid[k] = ended ? 0.0f : 1.0f;
            if (p.out_index) {
                p.out_index[2 * k] = t;
                p.out_index[2 * k + 1] = e;
            }
        }
    }
    return r;
}

// the gather; num_starts bounds the drawn (and the given) starts: the argument block's (sample_rows_kernel) or the learner clock's, clamped
// (sample_rows_clocked_kernel)
template <int VEC, bool U8>
__device__ __forceinline__ void sample_rows(const SampleParams& p, const int64_t num_starts) {
    const int lane = threadIdx.x & 63;
    const int F1 = p.F + 1;
    const uint32_t w0 = blockIdx.x * (kBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);       // below the grid's wave count
    // item w = k * (F + 1) + j, and w advances by the grid's waves: (k, j) advance by (step_k, step_j) with a carry -- no 64-bit division
    int64_t k = w0 / (uint32_t)F1;
    int j = (int)(w0 % (uint32_t)F1);
    if (k >= p.n) return;
    const uint64_t counter = p.starts ? 0 : (p.draw_count ? uniform_load(p.draw_count, 0) : p.draw);
    const int pieces = p.pieces;
    SamplePiece<VEC, U8> cur, nxt;
    SampleRow row = sample_locate(p, num_starts, k, j, counter, lane), nrow = row;
    int c = 0;
    cur.load(p, row, c, lane);
    for (;;) {
        int nc = c + 1;
        bool more = true;
        if (nc == pieces) {
            nc = 0;
            k += p.step_k;
            j += p.step_j;
            if (j >= F1) {
                j -= F1;
                ++k;
            }
            more = k < p.n;
            if (more) nrow = sample_locate(p, num_starts, k, j, counter, lane);
        }
        if (!more) nc = c;                  // (the last piece is loaded once more rather than branching around the loads)
        nxt.load(p, nrow, nc, lane);
        cur.store(p, row, c, lane);
        if (!more) break;
        cur = nxt;
        row = nrow;
        c = nc;
    }
}

template <int VEC, bool U8>
__global__ __launch_bounds__(kBlock) void sample_rows_kernel(const SampleParams p) {
    sample_rows<VEC, U8>(p, p.num_starts);
}

// sgw_sample_clocked: the draws' bound is the learner clock's num_starts, read once and clamped HERE to [1, p.num_starts] -- the bound the host
// checked against the ring's capacity -- so that whatever the clock holds, no row read lies outside the ring
template <int VEC, bool U8>
__global__ __launch_bounds__(kBlock) void sample_rows_clocked_kernel(const SampleParams p, const sgw_learn_clock* clock) {
    const int64_t now = learn_clock_num_starts(clock);
    const int64_t least = now > 1 ? now : 1;
    sample_rows<VEC, U8>(p, least < p.num_starts ? least : p.num_starts);
}

// *count += 1, after the gather that read it (same stream): the next call -- or the next replay of a recorded graph -- draws anew
__global__ void sample_count_kernel(uint64_t* count) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        *count = *count + 1;
    }
}
