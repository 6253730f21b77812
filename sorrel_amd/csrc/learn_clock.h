// The learner clock (sgw_learn_clock, include/sgw.h): the scalars of a learner's step that change from one step to the next -- the count of
// steps done, which keys the noise and the taus, and the replay ring's filled rows -- in device memory, so that a recorded graph, whose argument
// blocks are frozen, reads them anew at every replay.
//
// A clocked kernel reads the clock ONCE, at its top, through the constant address space: the compiler then issues a scalar load into SGPRs, the
// value is wave-uniform by construction (no readfirstlane, no vector load to wait for), and nothing a clocked kernel reads this way is written by
// it: the clock changes only between kernels, by sgw_learn_clock_advance or a copy on the same stream, and the scalar cache is invalidated at a
// kernel's start.  The clocked kernels are instantiations of their own (a pointer appended to the argument block), so the unclocked kernels keep
// their names, their argument blocks and their registers.
#pragma once

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
__device__ __forceinline__ uint64_t learn_clock_count(const sgw_learn_clock* c) {
    return ((const __attribute__((address_space(4))) sgw_learn_clock*)c)->count;
}
__device__ __forceinline__ int64_t learn_clock_num_starts(const sgw_learn_clock* c) {
    return ((const __attribute__((address_space(4))) sgw_learn_clock*)c)->num_starts;
}
#pragma clang diagnostic pop

// count += 1, behind the step that read it (same stream): the next step -- or the next replay of a recorded graph -- is keyed anew.  One thread,
// one vector load and one vector store.
__global__ void learn_clock_advance_kernel(sgw_learn_clock* clock) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        volatile uint64_t* count = &clock->count;
        *count = *count + 1;
    }
}
