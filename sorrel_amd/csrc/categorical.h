// One row of a Categorical distribution as policy.h and ppo_loss.h both read it, and the typed loads and stores the learner kernels
// share.  include/sgw.h states the arithmetic; the `bad`-row rules and the clamped log live HERE and nowhere else.  The generic path's
// passes differ between the kernels (policy.h leaves its search early when no entropy is asked for) and stay in them.
// fp contract is lexical: it does not reach a helper from the kernel body that calls it, so every function here that adds, subtracts,
// multiplies or divides carries its own contract(off).
#pragma once

typedef float cat_f4 __attribute__((ext_vector_type(4)));       // (ext_vector_type: what __builtin_nontemporal_store accepts)
typedef double cat_d2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double policy_clamped_log(const double q) {
    // torch's probs_to_logits: log(clamp(q, eps, 1 - eps)) with eps = 2^-52 (a NaN passes through both comparisons)
    constexpr double lo = 0x1p-52, hi = 1.0 - 0x1p-52;
    return log(q < lo ? lo : (q > hi ? hi : q));
}

// ---------------------------------------------------------------- typed loads and stores (the stores: written once, non-temporal)
template <bool F64>
__device__ __forceinline__ double policy_elem(const void* base, const int64_t at) {
    if constexpr (F64) return reinterpret_cast<const double*>(base)[at];
    else return (double)reinterpret_cast<const float*>(base)[at];
}
template <bool F64>
__device__ __forceinline__ void policy_store_elem(void* base, const int64_t at, const double v) {
    if constexpr (F64) __builtin_nontemporal_store(v, reinterpret_cast<double*>(base) + at);
    else __builtin_nontemporal_store((float)v, reinterpret_cast<float*>(base) + at);
}
// ... by a type code known only at run time (SGW_POLICY_F32 / _F64, SGW_PPO_ACT_U8 / _I64; uniform over the launch)
__device__ __forceinline__ double load_float(const void* base, const int type, const int64_t k) {
    return type == SGW_POLICY_F64 ? policy_elem<true>(base, k) : policy_elem<false>(base, k);
}
__device__ __forceinline__ void store_float(void* base, const int type, const int64_t k, const double v) {
    if (type == SGW_POLICY_F64) policy_store_elem<true>(base, k, v);
    else policy_store_elem<false>(base, k, v);
}
__device__ __forceinline__ int64_t load_action(const void* base, const int type, const int64_t k) {
    return type == SGW_PPO_ACT_U8 ? (int64_t)reinterpret_cast<const uint8_t*>(base)[k] : reinterpret_cast<const int64_t*>(base)[k];
}

// ---------------------------------------------------------------- the register path
// One read of the row; VEC: 16 bytes per load (the caller found the base, the stride and the row's byte count to be multiples of 16).
// `pad`: -inf for logits, 0 for probabilities = a weight of exactly 0: never chosen, adds nothing to any sum.
template <int NA, bool F64, bool VEC>
__device__ __forceinline__ void cat_load_row(const void* dist, const int64_t at0, const int nact, const double pad, double (&x)[NA]) {
    if constexpr (VEC) {
        constexpr int PER = F64 ? 2 : 4;
#pragma unroll
        for (int c = 0; c < NA / PER; ++c) {
            if (c * PER >= nact) {                // (nact is a multiple of PER on this path)
#pragma unroll
                for (int j = 0; j < PER; ++j) x[PER * c + j] = pad;
            } else if constexpr (F64) {
                const cat_d2 v = reinterpret_cast<const cat_d2*>(reinterpret_cast<const double*>(dist) + at0)[c];
                x[2 * c] = v.x; x[2 * c + 1] = v.y;
            } else {
                // four floats off a pointer declared 16-byte aligned: the backend makes ONE 16-byte load of them (tests/test_learner_codegen.py
                // counts them); read through a cat_f4 the row costs registers and occupancy (profiles/learner_refactor.txt)
                const float* q = static_cast<const float*>(__builtin_assume_aligned(reinterpret_cast<const float*>(dist) + at0, 16)) + 4 * c;
                x[4 * c] = (double)q[0]; x[4 * c + 1] = (double)q[1]; x[4 * c + 2] = (double)q[2]; x[4 * c + 3] = (double)q[3];
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < NA; ++i) x[i] = i < nact ? policy_elem<F64>(dist, at0 + i) : pad;
    }
}

// the first nact of g, with stores of the width cat_load_row read with
template <int NA, bool F64, bool VEC>
__device__ __forceinline__ void cat_store_row(void* out, const int64_t at0, const int nact, const double (&g)[NA]) {
    if constexpr (VEC) {
        constexpr int PER = F64 ? 2 : 4;
#pragma unroll
        for (int c = 0; c < NA / PER; ++c) {
            if (c * PER >= nact) continue;
            if constexpr (F64) {
                cat_d2 o;
                o.x = g[2 * c]; o.y = g[2 * c + 1];
                __builtin_nontemporal_store(o, reinterpret_cast<cat_d2*>(reinterpret_cast<double*>(out) + at0) + c);
            } else {
                cat_f4 o;
                o.x = (float)g[4 * c]; o.y = (float)g[4 * c + 1]; o.z = (float)g[4 * c + 2]; o.w = (float)g[4 * c + 3];
                __builtin_nontemporal_store(o, reinterpret_cast<cat_f4*>(reinterpret_cast<float*>(out) + at0) + c);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < NA; ++i)
            if (i < nact) policy_store_elem<F64>(out, at0 + i, g[i]);
    }
}

// logits -> weights exp(x_i - m); true: the row has no finite maximum and is refused
template <int NA>
__device__ __forceinline__ bool cat_weights(double (&x)[NA]) {
#pragma clang fp contract(off)
    double m = x[0];
#pragma unroll
    for (int i = 1; i < NA; ++i) m = x[i] > m || m != m ? x[i] : m;      // (a NaN is replaced; a NaN entry gives a NaN weight below)
#pragma unroll
    for (int i = 0; i < NA; ++i) x[i] = exp(x[i] - m);
    return !(m < __builtin_huge_val());
}

// S: serial, in index order and in float64; a weight that is negative or a NaN refuses the row
template <int NA>
__device__ __forceinline__ double cat_sum(const double (&x)[NA], bool& bad) {
#pragma clang fp contract(off)
    double S = 0.0;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        bad |= !(x[i] >= 0.0);
        S += x[i];
    }
    return S;
}

// ---------------------------------------------------------------- the generic path
// the maximum of a row of logits (a NaN is replaced); the caller refuses the row on !(m < inf)
template <bool F64>
__device__ __forceinline__ double cat_row_max(const void* dist, const int64_t at0, const int nact) {
    double m = policy_elem<F64>(dist, at0);
    for (int i = 1; i < nact; ++i) {
        const double v = policy_elem<F64>(dist, at0 + i);
        m = v > m || m != m ? v : m;
    }
    return m;
}

// the weight of the element at `at`
template <bool F64>
__device__ __forceinline__ double cat_weight(const void* dist, const int64_t at, const bool logits, const double m) {
#pragma clang fp contract(off)
    const double v = policy_elem<F64>(dist, at);
    return logits ? exp(v - m) : v;
}

// ---------------------------------------------------------------- host side
// f(NA, VEC) as std::integral_constants: the bucket 4 / 8 / 16 that holds nact, with or without 16-byte accesses, or the generic loop (0)
template <int NA, class F>
auto dispatch_vec(const bool vec, F& f) {
    return vec ? f(std::integral_constant<int, NA>{}, std::true_type{}) : f(std::integral_constant<int, NA>{}, std::false_type{});
}
template <class F>
auto dispatch_actions(const int nact, const bool vec, F f) {
    if (nact <= 4) return dispatch_vec<4>(vec, f);
    if (nact <= 8) return dispatch_vec<8>(vec, f);
    if (nact <= 16) return dispatch_vec<16>(vec, f);
    return f(std::integral_constant<int, 0>{}, std::false_type{});
}
