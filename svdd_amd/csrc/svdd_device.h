// svdd_device.h — the device helpers that more than one translation unit uses, each defined here and nowhere else: the fp32 net
// kernels (svdd_nets.hip), the training GRU (svdd_gru_train.hip) and the split-precision kernels (svdd_lp_common.h,
// svdd_lp_gru_tail.hip) must give each other's bits, so they must run the same expressions. The host side is svdd_host.h.
#pragma once
#include <hip/hip_runtime.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));          // one MFMA accumulator / one 16-byte access
typedef __attribute__((address_space(3))) f32x4 LdsF4;            // ... read through an LDS byte address kept as an integer

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the GRU gates (v_exp_f32 / v_rcp_f32): the inference GRU, the training forward and the split-precision GRU share them
__device__ __forceinline__ float sigmoid_fast(float a) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896f * a));
}
__device__ __forceinline__ float tanh_fast(float a) {
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(2.88539008177793f * a));
}

template <int N>
__device__ __forceinline__ float row_ror(float v) {            // rotate right by N inside each 16-lane DPP row
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 + N, 0xf, 0xf, false));
}
__device__ __forceinline__ float group16_sum(float v) {        // sum over the 16 lanes sharing lane >> 4 (VALU DPP, no LDS)
  v += row_ror<8>(v); v += row_ror<4>(v); v += row_ror<2>(v); v += row_ror<1>(v);
  return v;
}

}  // namespace
