// The deterministic workgroup reduction every learner kernel ends in (ppo_loss.h, iqn_loss.h, returns.h, reduce_stage1/2), once:
// kBlock slots of LDS per value, a halving tree s = kBlock / 2 .. 1 in which thread tid combines slot tid with slot tid + s, one partial
// per workgroup; a second launch of one workgroup in which thread i takes partials i, i + kBlock, ... in that order and the same tree
// merges the threads.  The order depends on the thread index alone -- two runs give the same bits -- and is part of the tested contract
// (tests/iqn_loss_common.py::tree restates it).
// fp contract: the tree only combines values it has just loaded from LDS, so its own flag cannot change a result; the functor's can.
// TreeSum and partials_sum carry contract(off), which the loss kernels promise for every operation done on their behalf; returns.h's
// moments_merge runs contracted, as it always has, and must stay so.
#pragma once

// op(a, b) folds b, the K values of slot tid + s, into a, those of slot tid.  red[k][0] is the result, behind a barrier: any thread may read it.
template <int K, class Op>
__device__ __forceinline__ void block_tree(const double (&v)[K], double (*red)[kBlock], const Op op) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) red[k][tid] = v[k];
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if (tid < s) {
            double a[K], b[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                a[k] = red[k][tid];
                b[k] = red[k][tid + s];
            }
            op(a, b);
#pragma unroll
            for (int k = 0; k < K; ++k) red[k][tid] = a[k];
        }
        __syncthreads();
    }
}

struct TreeSum {
    template <int K>
    __device__ __forceinline__ void operator()(double (&a)[K], const double (&b)[K]) const {
#pragma clang fp contract(off)
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] += b[k];
    }
};

// second launch: thread i adds partials i, i + kBlock, ... of [nparts][K], in that order
template <int K>
__device__ __forceinline__ void partials_sum(const double* partials, const int nparts, double (&v)[K]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.0;
    for (int i = threadIdx.x; i < nparts; i += kBlock) {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += partials[K * i + k];
    }
}
