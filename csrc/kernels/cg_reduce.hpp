// The deterministic grid reduction of the CG kernels (cg.hip) and of the
// preconditioner's dot epilogue (multigrid.hip): per-workgroup partials and a
// last-block finish in a fixed order (agent-scope release before the ticket,
// acquire after it, partials read on the vector path); no floating-point
// atomics, and no workgroup waits on another. Workgroups of kCgBlock threads.
#pragma once

#include <hip/hip_runtime.h>

#include "mxs/kernels/kernels.hpp"

#pragma clang fp contract(off)

namespace mxs {
namespace kernels {
namespace cgdev {

constexpr int kCgWaves = 4;  // side by side along x
constexpr int kCgBlock = kCgWaves * kWaveSize;

template <typename U>
__device__ __forceinline__ U umax(U a, U b) {
  return a > b ? a : b;
}

struct Pair {
  double sum;
  unsigned long long linf;  // bit pattern of a non-negative double (or a NaN)
};

// Workgroup reduction in a fixed order; valid in thread 0. lds: 2 * kCgWaves slots.
__device__ __forceinline__ Pair block_reduce(Pair v, unsigned long long* lds) {
#pragma unroll
  for (int off = kWaveSize / 2; off > 0; off >>= 1) {
    v.sum += __shfl_xor(v.sum, off);
    v.linf = umax(v.linf, static_cast<unsigned long long>(__shfl_xor(static_cast<long long>(v.linf), off)));
  }
  const int lane = threadIdx.x & (kWaveSize - 1), wave = threadIdx.x / kWaveSize;
  if (lane == 0) {
    lds[2 * wave] = static_cast<unsigned long long>(__double_as_longlong(v.sum));
    lds[2 * wave + 1] = v.linf;
  }
  __syncthreads();
  Pair r{0.0, 0ull};
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < kCgWaves; ++w) {
      r.sum += __longlong_as_double(static_cast<long long>(lds[2 * w]));
      r.linf = umax(r.linf, lds[2 * w + 1]);
    }
  }
  return r;
}

// The launch's total, valid in thread 0 of the last workgroup to arrive (`last`
// is workgroup-uniform). Every workgroup of the launch calls it exactly once.
// The last workgroup puts the ticket back to 0 for the next launch.
struct Total {
  bool last;
  double sum, linf;
};
// `bid` of `nblocks` is this workgroup's place in the launch (a 2-D grid numbers itself).
__device__ __forceinline__ Total grid_reduce_at(double acc, unsigned long long linf_bits, double* partials,
                                                unsigned* counter, unsigned bid, unsigned nblocks) {
  // ONE __shared__ object (the "is last" flag shares the array, as in dot.hip).
  __shared__ unsigned long long lds[4 * kCgWaves + 1];
  const Pair r = block_reduce(Pair{acc, linf_bits}, lds);
  volatile unsigned* flag = reinterpret_cast<volatile unsigned*>(lds + 4 * kCgWaves);
  if (threadIdx.x == 0) {
    partials[2 * index_t(bid)] = r.sum;
    partials[2 * index_t(bid) + 1] = __longlong_as_double(static_cast<long long>(r.linf));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the stores have left the wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // write back this XCD's L2 dirty lines
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned ticket = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *flag = (ticket == nblocks - 1) ? 1u : 0u;
  }
  __syncthreads();
  if (*flag == 0u) return Total{false, 0.0, 0.0};  // workgroup-uniform
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // drop this CU's (possibly stale) L1 lines
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  Pair t{0.0, 0ull};
  for (unsigned i = threadIdx.x; i < nblocks; i += kCgBlock) {  // fixed order per thread
    t.sum += partials[2 * index_t(i)];
    t.linf = umax(t.linf, static_cast<unsigned long long>(__double_as_longlong(partials[2 * index_t(i) + 1])));
  }
  const Pair total = block_reduce(t, lds + 2 * kCgWaves);
  if (threadIdx.x == 0) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return Total{true, total.sum, __longlong_as_double(static_cast<long long>(total.linf))};
}
__device__ __forceinline__ Total grid_reduce(double acc, unsigned long long linf_bits, double* partials,
                                             unsigned* counter) {
  return grid_reduce_at(acc, linf_bits, partials, counter, blockIdx.x, gridDim.x);
}

}  // namespace cgdev
}  // namespace kernels
}  // namespace mxs
