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

// s_waitcnt lgkmcnt(NOUT): wait until at most NOUT LDS reads are outstanding, vmcnt and expcnt untouched. The MFMA groups of the
// conv tower and of the backbone are fenced behind one such wait (svdd_nets.hip)
#define LGKM_WAIT(NOUT) __builtin_amdgcn_s_waitcnt(0xC07F | ((NOUT) << 8));

// The value net's tower the window and part rules are written for: TP_BLOCKS conv blocks after the stem. A row next to a window
// edge that is no sequence end sees zeros for its real neighbours and is wrong by up to two rows per block: TW_EDGE rows.
constexpr int TP_BLOCKS = 5;
constexpr int TW_EDGE = 2 * TP_BLOCKS;

// Head of a tower kernel that may run on candidate WINDOWS (the fp32 towers of svdd_nets.hip and tower_lp_kernel): A holds count /
// live_idx / win. Workgroup blockIdx.x computes candidate cand's rows [w0, w1), nt row tiles of 16, and KEEPS rows [keep_lo,
// keep_hi) of them (a window edge that is a sequence end is exact); every other row is its parent's. !WIN: all zero.
// CAND = TW_CAND_BRANCH or TW_CAND_SELECT: the same choice as a branch or as a select, each kernel's former shape (the other one
// changes its instructions).
#define TW_CAND_BRANCH(A) if (A.live_idx) cand = __builtin_amdgcn_readfirstlane(A.live_idx[blockIdx.x]);
#define TW_CAND_SELECT(A) cand = A.live_idx ? __builtin_amdgcn_readfirstlane(A.live_idx[blockIdx.x]) : (int)blockIdx.x;
#define TW_WIN_DECODE(A, WIN, CAND)                                                                           \
  int cand = blockIdx.x, w0 = 0, w1 = 0;                                                                      \
  if (WIN) {                                                                                                  \
    if (A.count && (int)blockIdx.x >= __builtin_amdgcn_readfirstlane(*A.count)) return;                       \
    CAND(A)                                                                                                   \
    w0 = __builtin_amdgcn_readfirstlane(A.win[2 * cand]);                                                     \
    w1 = __builtin_amdgcn_readfirstlane(A.win[2 * cand + 1]);                                                 \
  }                                                                                                           \
  const int nt = (w1 - w0) >> 4;
#define TW_WIN_KEEP(WIN, L)                                                                                   \
  const int keep_lo = !(WIN) ? 0 : (nt == 0 ? 0 : (w0 == 0 ? 0 : w0 + TW_EDGE));                              \
  const int keep_hi = !(WIN) ? 0 : (nt == 0 ? 0 : (w1 >= L ? L : w1 - TW_EDGE));

}  // namespace
