// Discounted returns (sgw_returns): what sorrel/models/pytorch/ppo.py:226-239 computes at the head of train_step, for every
// (env, agent) column of a replay ring in one launch.
//
// One lane per column; the 64 lanes of a wave take 64 adjacent columns, so a wave's load of one ring row is one contiguous segment
// (col_stride 1) or one element per agent group (col_stride A).  Time runs BACKWARDS over `count` ring rows that start at row
// `first` and wrap at `capacity` (a compare and a subtract):
//     d = 0 at every done != 0;   d = fl32(r + fl32(g * d))
// in float32 with the product and the sum rounded separately -- the reference's arithmetic under NumPy's promotion rules (float32
// rewards, a Python-float gamma).  The recurrence is kept SERIAL per column on purpose: a parallel scan over time re-associates the
// float32 sums and products and loses bit equality with the reference.  Parallelism comes from the columns, and the memory
// latency is hidden by a software pipeline over chunks of kReturnsChunk turns: the 2 K loads of the next chunk are issued before the
// K dependent steps and the K stores of the current one.  Loads are unconditional and clamped (a turn before the segment reads turn 0
// again, a lane past the last column reads the last column), so that no branch sits between them.
//
// Normalisation, float64, (x - mean) / (std + 1e-7) with the unbiased std:
//   COLUMN  per column, in the same launch.  The statistics are running (Welford) moments taken in the backward sweep; a second,
//           forward sweep re-reads the returns and writes the normalised values.
//   ALL     one mean / std over count * cols values.  Every lane carries running moments over the columns it walks; a workgroup
//           merges its lanes' (n, mean, M2) in a fixed tree and writes ONE partial to the workspace.  A second launch merges the
//           partials -- every workgroup does, in the same fixed order, so all of them hold the same bits -- and normalises.  No
//           floating-point atomics: two runs give identical results.
#pragma once

constexpr int kReturnsChunk = 8;              // K: turns per pipeline stage (2 K loads in flight per lane, 4 K with the next stage's)
constexpr int kReturnsMaxBlocks = 2048;       // grid cap: 8 workgroups per CU on 256 CUs; more column tiles than that and the workgroups stride

struct ReturnsParams {
    const float* rewards;
    const float* dones;
    float* out_returns;
    void* out_norm;
    double* out_stats;
    double* partials;                          // [workgroups of the first launch][3] = (n, mean, M2)
    int64_t first, count, capacity, cols;
    int64_t ts, cs;                            // turn / column stride of rewards and dones, in elements
    int64_t tiles;                             // ceil(cols / kBlock)
    float gamma;
    int32_t nparts;
};

struct Moments {
    double n, mean, m2;
};

__device__ __forceinline__ void moments_push(Moments& m, const double x) {
    m.n += 1.0;
    const double d = x - m.mean;
    m.mean += d / m.n;
    m.m2 += d * (x - m.mean);
}

// (Chan, Golub & LeVeque's pairwise update)
__device__ __forceinline__ Moments moments_merge(const Moments a, const Moments b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double n = a.n + b.n, d = b.mean - a.mean;
    return Moments{n, a.mean + d * (b.n / n), a.m2 + b.m2 + d * d * (a.n * b.n / n)};
}

// the workgroup's moments, merged pairwise in an order that depends on nothing but the thread index; every thread gets the result
// (block_reduce.h's tree with moments_merge as its operation; like moments_push and moments_merge, WITHOUT fp contract off)
__device__ __forceinline__ Moments moments_block_merge(const Moments m, double (*red)[kBlock]) {
    const double v[3] = {m.n, m.mean, m.m2};
    block_tree<3>(v, red, [](double (&a)[3], const double (&b)[3]) {
        const Moments r = moments_merge(Moments{a[0], a[1], a[2]}, Moments{b[0], b[1], b[2]});
        a[0] = r.n;
        a[1] = r.mean;
        a[2] = r.m2;
    });
    return Moments{red[0][0], red[1][0], red[2][0]};
}

__device__ __forceinline__ double moments_std(const Moments m) { return sqrt(m.m2 / (m.n - 1.0)); }      // one value: 0 / 0 = NaN, as torch's std

template <bool OUT32>
__device__ __forceinline__ void returns_store_norm(void* out, const int64_t at, const double v) {
    if constexpr (OUT32) __builtin_nontemporal_store((float)v, reinterpret_cast<float*>(out) + at);
    else __builtin_nontemporal_store(v, reinterpret_cast<double*>(out) + at);
}

// Chunk j of a column holds the turns t = count - 1 - j K - i, i = 0 .. K-1 (the last chunk may reach below turn 0: clamped)
struct ReturnsChunk {
    float r[kReturnsChunk], d[kReturnsChunk];

    __device__ __forceinline__ void load(const ReturnsParams& p, const int64_t col_off, const int64_t j) {
        const int64_t top = p.count - 1 - j * kReturnsChunk;
#pragma unroll
        for (int i = 0; i < kReturnsChunk; ++i) {
            int64_t t = top - i;
            t = t < 0 ? 0 : t;
            int64_t row = p.first + t;                       // first < capacity and t < count <= capacity: one subtraction wraps
            row = row >= p.capacity ? row - p.capacity : row;
            const int64_t at = row * p.ts + col_off;
            r[i] = p.rewards[at];
            d[i] = p.dones[at];
        }
    }
};

template <int NORM, bool OUT32>
__global__ __launch_bounds__(kBlock) void returns_kernel(const ReturnsParams p) {
#pragma clang fp contract(off)                    // for the whole body: the recurrence below must not become a fused multiply-add
    constexpr int K = kReturnsChunk;
    const int64_t chunks = (p.count + K - 1) / K;
    Moments all{0.0, 0.0, 0.0};
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t col = tile * kBlock + threadIdx.x;
        const bool live = col < p.cols;
        const int64_t col_off = (live ? col : p.cols - 1) * p.cs;
        Moments m = NORM == SGW_RETURNS_NORM_ALL ? all : Moments{0.0, 0.0, 0.0};
        float disc = 0.0f;
        ReturnsChunk cur, nxt;
        cur.load(p, col_off, 0);
        for (int64_t j = 0; j < chunks; ++j) {
            nxt.load(p, col_off, j + 1 < chunks ? j + 1 : j);      // (the last chunk is loaded once more rather than branching around the loads)
            const int64_t top = p.count - 1 - j * K;
            float x[K];
#pragma unroll
            for (int i = 0; i < K; ++i) {
                if (cur.d[i] != 0.0f) disc = 0.0f;                   // truthiness, as the reference's `if done:`
                const float prod = p.gamma * disc;                   // (two roundings: the contract(off) above keeps hipcc from fusing them;
                disc = cur.r[i] + prod;                              //  __fadd_rn(r, __fmul_rn(g, d)) IS fused -- the intrinsics are plain * and +)
                x[i] = disc;
                if (NORM != SGW_RETURNS_NORM_NONE && top - i >= 0) moments_push(m, (double)disc);
            }
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const int64_t t = top - i;
                if (live && t >= 0) {
                    float* q = p.out_returns + t * p.cols + col;
                    // re-read below (COLUMN) or by the next launch (ALL): an ordinary store there
                    if constexpr (NORM == SGW_RETURNS_NORM_NONE) __builtin_nontemporal_store(x[i], q);
                    else *q = x[i];
                }
            }
            cur = nxt;
        }
        if constexpr (NORM == SGW_RETURNS_NORM_ALL) {
            if (live) all = m;                                       // (a lane past the last column walked a copy of the last one)
        }
        if constexpr (NORM == SGW_RETURNS_NORM_COLUMN) {
            // The forward sweep reads out_returns[t][col] for THIS lane's column only: every address it loads was stored above by this
            // same thread, and a thread's load of an address follows its own earlier store to it in program order -- no other thread
            // writes the column, so no fence or barrier is involved.
            if (live) {
                const double mean = m.mean, sd = moments_std(m), denom = sd + 1e-7;
                if (p.out_stats) {
                    p.out_stats[2 * col] = mean;
                    p.out_stats[2 * col + 1] = sd;
                }
                for (int64_t t0 = 0; t0 < p.count; t0 += K) {
                    float y[K];
#pragma unroll
                    for (int i = 0; i < K; ++i) {
                        const int64_t t = t0 + i < p.count ? t0 + i : p.count - 1;
                        y[i] = p.out_returns[t * p.cols + col];
                    }
#pragma unroll
                    for (int i = 0; i < K; ++i) {
                        if (t0 + i < p.count) returns_store_norm<OUT32>(p.out_norm, (t0 + i) * p.cols + col, ((double)y[i] - mean) / denom);
                    }
                }
            }
        }
    }
    if constexpr (NORM == SGW_RETURNS_NORM_ALL) {
        __shared__ double red[3][kBlock];
        const Moments b = moments_block_merge(all, red);
        if (threadIdx.x == 0) {
            p.partials[3 * blockIdx.x] = b.n;
            p.partials[3 * blockIdx.x + 1] = b.mean;
            p.partials[3 * blockIdx.x + 2] = b.m2;
        }
    }
}

// NORM_ALL, second launch: the partials of the first -> one (mean, std); then out_normalized over the contiguous [count][cols] returns
template <bool OUT32>
__global__ __launch_bounds__(kBlock) void returns_normalize_all_kernel(const ReturnsParams p) {
    __shared__ double red[3][kBlock];
    Moments m{0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < p.nparts; i += kBlock) m = moments_merge(m, Moments{p.partials[3 * i], p.partials[3 * i + 1], p.partials[3 * i + 2]});
    m = moments_block_merge(m, red);
    const double mean = m.mean, sd = moments_std(m), denom = sd + 1e-7;
    if (blockIdx.x == 0 && threadIdx.x == 0 && p.out_stats) {
        p.out_stats[0] = mean;
        p.out_stats[1] = sd;
    }
    constexpr int U = 4;
    const int64_t total = p.count * p.cols, step = (int64_t)gridDim.x * kBlock * U;
    for (int64_t base = (int64_t)blockIdx.x * kBlock * U + threadIdx.x; base < total; base += step) {
        float y[U];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int64_t at = base + (int64_t)i * kBlock;
            y[i] = p.out_returns[at < total ? at : total - 1];
        }
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int64_t at = base + (int64_t)i * kBlock;
            if (at < total) returns_store_norm<OUT32>(p.out_norm, at, ((double)y[i] - mean) / denom);
        }
    }
}

// host side
inline int64_t returns_blocks(const int64_t cols) { return std::min<int64_t>((cols + kBlock - 1) / kBlock, kReturnsMaxBlocks); }

template <int NORM>
void launch_returns(const ReturnsParams& p, bool out32, unsigned blocks, hipStream_t s) {
    if (out32) hipLaunchKernelGGL((returns_kernel<NORM, true>), dim3(blocks), dim3(kBlock), 0, s, p);
    else hipLaunchKernelGGL((returns_kernel<NORM, false>), dim3(blocks), dim3(kBlock), 0, s, p);
}
