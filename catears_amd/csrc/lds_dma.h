// lds_dma.h -- device helpers shared by the LDS-DMA GEMM kernels
// (the bf16x6 GEMMs, gemm_bf16.hip, gemm_f16x3.hip, the int8 GEMMs).
#pragma once

#include <hip/hip_runtime.h>

namespace catears {
namespace dma {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// s_waitcnt vmcnt(N): all but this wave's N youngest vector-memory operations
// (LDS-DMAs included) are done.  A compiler barrier too.
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// global_load_lds_dwordx4: 16 bytes per lane from a per-lane global address
// into LDS at the wave-uniform base lds_dst + 16 * lane.
__device__ __forceinline__ void glds16(const char *src, char *lds_dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                   (__attribute__((address_space(3))) void *)lds_dst, 16, 0, 0);
}

// The same DMA through a buffer resource (buffer_load_dwordx4 ... lds): 16
// bytes per lane from base + voff into LDS at the wave-uniform lds_dst + 16 *
// lane.  A MUBUF access: the compiler counts it in vmcnt only, so LDS reads
// beside it keep exact lgkmcnt waits (a pending global_load_lds, a FLAT
// access, makes every LDS wait lgkmcnt(0)).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void *base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ void buf_lds16(__amdgpu_buffer_rsrc_t r, void *lds_dst, uint32_t voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void *)lds_dst, 16, voff, 0, 0, 0);
}

}  // namespace dma
}  // namespace catears
