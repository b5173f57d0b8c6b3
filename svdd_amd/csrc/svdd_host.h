// svdd_host.h — the host side that all nine translation units share: the library's internal cross-file functions, the geometry
// constants that the fp32 and the split-precision kernels must agree on, the names of the profiling slots, and the ONE way a kernel
// is launched (svdd_launch / svdd_launch_timed). No device code lives here.
//
// An entry of the C ABI reads: validate (return SVDD_E_ARG before anything else happens) -> build the kernel's argument struct ->
// pick the kernel from its template arguments -> `return svdd_launch...(...)`. A timed entry takes its span first:
//     SvddSpan span(SVDD_SLOT_GRU);
//     return svdd_launch_timed(span.all(), kern, grid, block, lds, stream, args...);
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "svdd_hip.h"
#include "svdd_spt.h"

// ---- internal functions that cross translation units (each declared here and nowhere else)
extern "C" {
void svdd_internal_timed_events(int slot, hipEvent_t* e0, hipEvent_t* e1);   // svdd_kernels.hip: start / stop events of one span of `slot` (nullptrs when profiling is off)
int svdd_internal_num_cus();                        // svdd_nets.hip: compute units of the current device
int svdd_internal_fixed_spt();                      // svdd_nets.hip: svdd_set_backbone_packing's value
void svdd_internal_set_bb_split(int v);             // svdd_nets.hip        \.
void svdd_internal_set_bb_lp_version(int v);        // svdd_lp_backbone.hip  | the setters behind svdd_set_option
void svdd_internal_set_trunk_gemm_version(int v);   // svdd_trunk.hip        |
void svdd_internal_set_trunk_planes_f32(int v);     // svdd_trunk.hip       /
}

// ---- geometry shared by the fp32 kernels (svdd_nets.hip, svdd_gru_train.hip) and their split-precision twins (svdd_lp_*.hip)
constexpr int TW_ROWS = 208;               // rows of a workgroup tile of the conv tower and the backbone: 13 row tiles of 16
constexpr int TW_RT = 13;
constexpr int TW_MAXL = 8;                 // max conv layers of the tower after the stem
constexpr int BB_C = 128;                  // backbone channels
constexpr int BB_AP = BB_C + 4;            // fp32 LDS row stride of a backbone image (floats)
constexpr int BB_MAXL = 32;                // max backbone layers (dil[] of the argument structs)
constexpr int TS = 16;                     // sequences per GRU workgroup (MFMA M). backbone_split_kernel (svdd_nets.hip) has a LOCAL
                                           // TS of its own, the stride of a wave's row tiles: another quantity, it shadows this one there.
static_assert(TW_ROWS == 16 * TW_RT && TW_ROWS == SVDD_TILE_ROWS, "svdd_spt.h plans tiles of TW_ROWS rows");

// dil[BB_MAXL] of a backbone argument struct from the caller's list (1 beyond nlayers); false: a dilation <= 0
inline bool svdd_fill_dilations(int* dil, const int* dilations, int nlayers) {
  for (int i = 0; i < BB_MAXL; ++i) dil[i] = i < nlayers ? dilations[i] : 1;
  for (int i = 0; i < nlayers; ++i) if (dilations[i] <= 0) return false;
  return true;
}

// ---- profiling slots: svdd_profile_collect(slot, ...) sums the spans taken under one slot. bench.py, tools/ and
//      tests/test_configs_gpu.py use these NUMBERS: append, never renumber.
enum SvddProfileSlot {
  SVDD_SLOT_PROPOSE = 0,         // K1: svdd_propose, svdd_sample_categorical
  SVDD_SLOT_SELECT = 1,          // K2: svdd_select, svdd_select_compact
  SVDD_SLOT_CONV1D = 2,          // svdd_conv1d_cl_f32, svdd_conv1d_cl_gated_f32
  SVDD_SLOT_GRU = 3,             // svdd_gru_bidir_f32, svdd_gru_bidir_lp
  SVDD_SLOT_EPILOGUE_LN = 4,     // svdd_epilogue_ln_f32
  SVDD_SLOT_CONV_TOWER = 5,      // svdd_conv_tower[_windows]_{f32,lp}, svdd_reward_stem[_bwd]_f32
  SVDD_SLOT_BACKBONE = 6,        // svdd_backbone_cnn_{f32,save_f32,lp}, svdd_backbone_incr[2]_f32 (one span per forward)
  SVDD_SLOT_VALUE_TAIL = 7,      // svdd_value_tail_{f32,lp}, svdd_reward_tail_grad_f32
  SVDD_SLOT_TDS_RESAMPLE = 8,    // K4: svdd_tds_resample (one span over both phases)
  SVDD_SLOT_MT19937 = 9,         // K8: svdd_mt19937_uniform_f32
  SVDD_SLOT_BACKBONE_GRAD = 10,  // svdd_backbone_cnn_grad_f32
  SVDD_SLOT_GRU_TRAIN = 11,      // DPS: the GRU forward that saves its gates (svdd_gru_bidir_train[2]_f32)
  SVDD_SLOT_GRU_BPTT = 12,       // DPS: the GRU's back-propagation through time (svdd_gru_bidir_bwd[2]_f32)
  SVDD_SLOT_WITHIN = 13,         // svdd_within
  SVDD_SLOT_GREEDY_PICK = 14,    // svdd_greedy_pick
  SVDD_SLOT_EDIT_WITHIN = 15,    // svdd_edit_within
  SVDD_SLOT_COUNT
};

// The events of one launch of a span. An entry that times ONE span over several launches gives first() to its first launch and
// last() to its last one (launches in between go through svdd_launch); a single launch gets all().
struct SvddEvents { hipEvent_t start, stop; };
struct SvddSpan {
  hipEvent_t start, stop;
  explicit SvddSpan(SvddProfileSlot slot) { svdd_internal_timed_events(slot, &start, &stop); }
  SvddEvents all() const { return {start, stop}; }
  SvddEvents first() const { return {start, nullptr}; }
  SvddEvents last() const { return {nullptr, stop}; }
};

// ---- launching. Dynamic LDS of a launch: plain bytes, or svdd_lds_raised(bytes) where the launch must first raise the kernel's
//      limit to `bytes` (every kernel that takes more than the default 64 KB). The attribute is set on every such launch, not cached.
struct SvddLds {
  size_t bytes;
  bool raise;
  SvddLds(size_t b = 0, bool r = false) : bytes(b), raise(r) {}
};
inline SvddLds svdd_lds_raised(size_t bytes) { return SvddLds(bytes, true); }

template <typename... KA>
inline void svdd_raise_lds_limit(void (*kern)(KA...), size_t bytes) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
inline int svdd_launch_status() { return hipGetLastError() == hipSuccess ? SVDD_OK : SVDD_E_LAUNCH; }

// untimed launch -> SVDD_OK / SVDD_E_LAUNCH
template <typename... KA, typename... A>
inline int svdd_launch(void (*kern)(KA...), dim3 grid, dim3 block, SvddLds lds, void* stream, A&&... args) {
  if (lds.raise) svdd_raise_lds_limit(kern, lds.bytes);
  hipLaunchKernelGGL(kern, grid, block, lds.bytes, (hipStream_t)stream, static_cast<KA>(args)...);
  return svdd_launch_status();
}

// launch with a span's events bound to the dispatch itself (both may be nullptr: profiling off, or the middle of a span)
template <typename... KA, typename... A>
inline int svdd_launch_timed(SvddEvents ev, void (*kern)(KA...), dim3 grid, dim3 block, SvddLds lds, void* stream, A&&... args) {
  if (lds.raise) svdd_raise_lds_limit(kern, lds.bytes);
  hipExtLaunchKernelGGL(kern, grid, block, (uint32_t)lds.bytes, (hipStream_t)stream, ev.start, ev.stop, 0, static_cast<KA>(args)...);
  return svdd_launch_status();
}
