// svdd_nets.hip — gfx950 kernels for the two networks of the SVDD step (the masked-diffusion backbone and the
// ConvGRU value net), which are >99 % of a diffusion step and which PyTorch-ROCm/MIOpen runs badly at SVDD's
// shapes (256 / 2560 short sequences, 64-128 channels). Exact fp32 on the matrix cores throughout. Exposed through
// the C ABI of include/svdd_hip.h ("net kernels" section); used by svdd_amd/fused.py.
//
//   backbone_kernel     the whole dilated-CNN backbone forward in one launch (residual stream in registers,
//                       LayerNorm'd activations in LDS, weights from L2 straight into MFMA B operands)
//   conv_tower_kernel   the value net's conv tower (stem + 5 residual blocks) in one launch, activations in LDS
//   gru_bidir_kernel    bidirectional GRU 64 -> 64, one launch for all L timesteps (MIOpen: ~2900 launches, 11.7 ms
//                       per value forward at n = 2560, L = 200 [rocprof r01_v0]); 16 sequences of one direction per
//                       workgroup, gate weights in registers as MFMA B operands, hidden state in LDS
//   value_tail_kernel   direction sum + LayerNorm + FFN dense1 + ReLU + (dense2 o head) + mean over length
//   conv1d_cl_*_kernel  one dilated conv layer (layer-wise path, small batches) ; epilogue_ln_kernel its epilogue
#include "svdd_host.h"
#include "svdd_device.h"

namespace {

constexpr int H = 64;          // hidden = input width
// TS = 16 sequences per workgroup (MFMA M): svdd_host.h
constexpr int HPAD = H + 4;    // LDS row stride (floats): shifts rows by 16 B -> ds_read_b128 conflict-light

// x      [n, L, 64] fp32 (channels-last conv-tower output)
// wpack  [2 dirs][4 waves][64 lanes][96] : lane (j = lane&15, g = lane>>4) of wave w holds, for
//        hidden unit u = 16w + j and input k = 16g + s (s = 0..15):
//        [0:16) W_ir[u][k]  [16:32) W_hr[u][k]  [32:48) W_iz  [48:64) W_hz  [64:80) W_in  [80:96) W_hn
// bpack  [2 dirs][4][64] : b_ir+b_hr, b_iz+b_hz, b_in, b_hn
// out    [2 dirs][n, L, 64] : hidden state of each direction at every timestep
// BOTH = false: one workgroup (4 waves) per (16-sequence tile, direction), grid (tiles, 2).
// BOTH = true : one workgroup (8 waves) per tile of `ts` <= 16 sequences runs BOTH directions, two waves per SIMD
//               interleaving their MFMAs; with ts = ceil(n / 256) every CU gets exactly one workgroup (n = 2560:
//               ts = 10), instead of 320 single-direction workgroups leaving 3/4 of the chip idle for the second
//               half of the launch.
template <bool BOTH>
__global__ __launch_bounds__(BOTH ? 512 : 256) void gru_bidir_kernel(const float* __restrict__ x, const float* __restrict__ wpack,
                                                                     const float* __restrict__ bpack, float* __restrict__ out,
                                                                     int n_alloc, int L, int ts, const int* __restrict__ count) {
  __shared__ __attribute__((aligned(16))) float hbuf_all[BOTH ? 2 : 1][2][TS][HPAD];
  const int lane = threadIdx.x & 63;
  const int w = (threadIdx.x >> 6) & 3;
  // BOTH = false: unit u = blockIdx.x covers (tile u >> 1, direction u & 1), so that the units of a compacted batch are a
  // dense prefix of the grid: the dispatcher hands consecutive workgroups to different CUs, and with the dead tiles
  // interleaved (grid (tiles, 2)) 256 live units of 320 landed two to a CU on 32 CUs — 678 us instead of 368.
  const int dir = BOTH ? (int)(threadIdx.x >> 8) : (int)(blockIdx.x & 1);
  float (*hbuf)[TS][HPAD] = hbuf_all[BOTH ? dir : 0];
  const int j = lane & 15;            // hidden unit within the wave's 16 / sequence row for A operands
  const int g = lane >> 4;            // k-group of A/B operands ; row-group of C/D
  const int seq0 = (BOTH ? (int)blockIdx.x : (int)(blockIdx.x >> 1)) * ts;
  // n_alloc: rows the output tensor is laid out for ; n: valid rows (device scalar when the batch was compacted)
  const int n = count ? __builtin_amdgcn_readfirstlane(*count) : n_alloc;
  if (seq0 >= n) return;

  // B operands: this lane's 96 weights stay in registers for the whole sequence
  float wr[96];
  {
    const float4* wp = reinterpret_cast<const float4*>(wpack + (((size_t)dir * 4 + w) * 64 + lane) * 96);
#pragma unroll
    for (int i = 0; i < 24; ++i) {
      const float4 v = wp[i];
      wr[4 * i] = v.x; wr[4 * i + 1] = v.y; wr[4 * i + 2] = v.z; wr[4 * i + 3] = v.w;
    }
  }
  const int u = 16 * w + j;
  const float b_r = bpack[(dir * 4 + 0) * H + u], b_z = bpack[(dir * 4 + 1) * H + u];
  const float b_nx = bpack[(dir * 4 + 2) * H + u], b_nh = bpack[(dir * 4 + 3) * H + u];

  // A-operand source row for this lane (clamped for the ragged last tile)
  const int arow = min(seq0 + min(j, ts - 1), n - 1);
  const float* xrow = x + (size_t)arow * L * H + 16 * g;
  float hprev[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // h[seq = 4g + rho][u] of the previous step

  // h_0 = 0
  for (int i = threadIdx.x & 255; i < TS * HPAD; i += 256) (&hbuf[0][0][0])[i] = 0.0f;

  const int t0 = dir == 0 ? 0 : L - 1;
  const int dt = dir == 0 ? 1 : -1;
  float xa[16], xn[16];
  {
    const float4* xp = reinterpret_cast<const float4*>(xrow + (size_t)t0 * H);
#pragma unroll
    for (int i = 0; i < 4; ++i) { const float4 v = xp[i]; xa[4 * i] = v.x; xa[4 * i + 1] = v.y; xa[4 * i + 2] = v.z; xa[4 * i + 3] = v.w; }
  }
  // input projections of step 0 (they do not depend on h): acc = bias + x_0 W_i*
  f32x4 acc_r = {b_r, b_r, b_r, b_r}, acc_z = {b_z, b_z, b_z, b_z}, acc_nx = {b_nx, b_nx, b_nx, b_nx};
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    acc_r = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s], wr[s], acc_r, 0, 0, 0);
    acc_z = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s], wr[32 + s], acc_z, 0, 0, 0);
    acc_nx = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s], wr[64 + s], acc_nx, 0, 0, 0);
  }
  __syncthreads();

  // Per step the only serial chain is  barrier -> read h -> 48 recurrent MFMAs -> gates -> write h.
  // The 48 input-projection MFMAs of the NEXT step are issued between the h write and the barrier, so they cover
  // the barrier skew and the LDS write latency instead of adding to the chain.
  for (int step = 0; step < L; ++step) {
    const int t = t0 + dt * step;
    const int cur = step & 1;
    if (step + 1 < L) {             // prefetch x_{t+1}
      const float4* xp = reinterpret_cast<const float4*>(xrow + (size_t)(t + dt) * H);
#pragma unroll
      for (int i = 0; i < 4; ++i) { const float4 v = xp[i]; xn[4 * i] = v.x; xn[4 * i + 1] = v.y; xn[4 * i + 2] = v.z; xn[4 * i + 3] = v.w; }
    }
    float ha[16];
    {
      const float4* hp = reinterpret_cast<const float4*>(&hbuf[cur][j][16 * g]);
#pragma unroll
      for (int i = 0; i < 4; ++i) { const float4 v = hp[i]; ha[4 * i] = v.x; ha[4 * i + 1] = v.y; ha[4 * i + 2] = v.z; ha[4 * i + 3] = v.w; }
    }
    f32x4 acc_nh = {b_nh, b_nh, b_nh, b_nh};
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      acc_nh = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[s], wr[80 + s], acc_nh, 0, 0, 0);
      acc_r = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[s], wr[16 + s], acc_r, 0, 0, 0);
      acc_z = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[s], wr[48 + s], acc_z, 0, 0, 0);
    }
    // C/D layout: reg rho -> row (sequence) 4g + rho, column (unit) j
#pragma unroll
    for (int rho = 0; rho < 4; ++rho) {
      const float r = sigmoid_fast(acc_r[rho]);
      const float z = sigmoid_fast(acc_z[rho]);
      const float nn = tanh_fast(acc_nx[rho] + r * acc_nh[rho]);
      const float hn = (1.0f - z) * nn + z * hprev[rho];
      hprev[rho] = hn;
      const int srow = 4 * g + rho;
      hbuf[cur ^ 1][srow][u] = hn;
      if (srow < ts && seq0 + srow < n) out[(((size_t)dir * n_alloc + seq0 + srow) * L + t) * H + u] = hn;
    }
    // next step's input projections (independent of the barrier below)
    acc_r = f32x4{b_r, b_r, b_r, b_r}; acc_z = f32x4{b_z, b_z, b_z, b_z}; acc_nx = f32x4{b_nx, b_nx, b_nx, b_nx};
    if (step + 1 < L) {
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        acc_r = __builtin_amdgcn_mfma_f32_16x16x4f32(xn[s], wr[s], acc_r, 0, 0, 0);
        acc_z = __builtin_amdgcn_mfma_f32_16x16x4f32(xn[s], wr[32 + s], acc_z, 0, 0, 0);
        acc_nx = __builtin_amdgcn_mfma_f32_16x16x4f32(xn[s], wr[64 + s], acc_nx, 0, 0, 0);
      }
    }
    __syncthreads();
  }
}

// Producer / consumer variant of gru_bidir_kernel<false> (same bits: every accumulator sees the same products in the same
// order). Workgroup = 8 waves on one (tile of 16 sequences, direction): waves 0-3 are CONSUMERS and run the recurrence
// (read h_t and the input projections of step t from LDS -> 48 recurrent MFMAs -> gates -> write h_{t+1}); waves 4-7
// are PRODUCERS and compute bias + W_i* x of step t + 1 into an LDS ring one step ahead, from x rows they prefetched two
// further steps ahead. Consumer w and producer w + 4 share a SIMD and own the same 16 hidden units, so a producer lane's
// accumulators are exactly what its partner consumer lane continues from. The consumer's serial chain loses the 48
// input-projection MFMAs and the x loads. Measured (tools/gru_microbench.py): 369 -> 359 us at <= 256 units, 727 -> 670 us
// at n = 2560 — the step stays at ~1.8 us against the 1.28 us the 96 MFMAs of a wave pair need; wave priorities
// (s_setprio 3 for the consumers) changed nothing.
// (The 16-bit twin gru_lp_kernel, svdd_lp_gru_tail.hip, was built this way first.)
// The body is a device function so that gru_tower_parts_kernel (below the parts tower) can run it in its LEADING workgroups (the unit
// is blockIdx.x in both kernels); hbuf / xproj: the workgroup's LDS (GRU_PC_LDS_FLOATS in all).
constexpr int GRU_PC_LDS_FLOATS = 2 * TS * HPAD + 2 * 4 * 3 * 64 * 4;
__device__ __forceinline__ void gru_pc_body(const float* __restrict__ x, const float* __restrict__ wpack,
                                            const float* __restrict__ bpack, float* __restrict__ out, int n_alloc, int L,
                                            const int* __restrict__ count, float (*hbuf)[TS][HPAD],
                                            float (*xproj)[4][3][64 * 4]) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool producer = wv >= 4;
  const int w = wv & 3;
  const int dir = (int)(blockIdx.x & 1);               // unit u = (tile u >> 1, direction u & 1): dense prefix when compacted
  const int j = lane & 15, g = lane >> 4;
  const int seq0 = (int)(blockIdx.x >> 1) * TS;
  const int n = count ? __builtin_amdgcn_readfirstlane(*count) : n_alloc;
  if (seq0 >= n) return;
  const int u = 16 * w + j;
  const int t0 = dir == 0 ? 0 : L - 1;
  const int dt = dir == 0 ? 1 : -1;

  // this wave's half of the lane's 96 gate weights: producers W_ir, W_iz, W_in ; consumers W_hr, W_hz, W_hn
  float wr[3][16];
  {
    const float4* wp = reinterpret_cast<const float4*>(wpack + (((size_t)dir * 4 + w) * 64 + lane) * 96 + (producer ? 0 : 16));
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4 v = wp[8 * m + i];
        wr[m][4 * i] = v.x; wr[m][4 * i + 1] = v.y; wr[m][4 * i + 2] = v.z; wr[m][4 * i + 3] = v.w;
      }
  }
  for (int i = threadIdx.x; i < TS * HPAD; i += 512) (&hbuf[0][0][0])[i] = 0.0f;          // h_0 = 0
  float* myproj = &xproj[0][w][0][lane * 4];
  constexpr int SLOT = 4 * 3 * 64 * 4;                 // floats per ring slot

  if (producer) {
    const float b_r = bpack[(dir * 4 + 0) * H + u], b_z = bpack[(dir * 4 + 1) * H + u], b_nx = bpack[(dir * 4 + 2) * H + u];
    const int arow = min(seq0 + j, n - 1);             // clamped for the ragged last tile
    const float* xrow = x + (size_t)arow * L * H + 16 * g;
    float xa[2][16];                                   // two x rows in flight
    auto load_x = [&](int t, int bufi) {
      const float4* xp = reinterpret_cast<const float4*>(xrow + (size_t)t * H);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4 v = xp[i];
        xa[bufi][4 * i] = v.x; xa[bufi][4 * i + 1] = v.y; xa[bufi][4 * i + 2] = v.z; xa[bufi][4 * i + 3] = v.w;
      }
    };
    auto project = [&](int bufi, int slot) {           // bias + x W_i* of one step -> ring slot
      f32x4 pr = {b_r, b_r, b_r, b_r}, pz = {b_z, b_z, b_z, b_z}, pn = {b_nx, b_nx, b_nx, b_nx};
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        pr = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[bufi][s], wr[0][s], pr, 0, 0, 0);
        pz = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[bufi][s], wr[1][s], pz, 0, 0, 0);
        pn = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[bufi][s], wr[2][s], pn, 0, 0, 0);
      }
      float* dst = myproj + slot * SLOT;
      *reinterpret_cast<f32x4*>(dst) = pr;
      *reinterpret_cast<f32x4*>(dst + 256) = pz;
      *reinterpret_cast<f32x4*>(dst + 512) = pn;
    };
    // prologue: projections of step 0 in slot 0; x of steps 1 and 2 in flight
    load_x(t0, 0);
    if (L > 1) load_x(t0 + dt, 1);
    project(0, 0);
    if (L > 2) load_x(t0 + 2 * dt, 0);
    __syncthreads();
    // step s (consumers work on slot s & 1): project x_{s+1} into slot (s + 1) & 1, prefetch x_{s+3}
    // (the prefetches are unconditional — past the end they re-read the last row: with a load on one path only, the compiler's
    //  s_waitcnt before a projection became vmcnt(0) and drained the row issued just before it, not only the one it needs)
    for (int s = 0; s < L; s += 2) {
      if (s + 1 < L) project(1, 1);
      load_x(t0 + min(s + 3, L - 1) * dt, 1);
      __syncthreads();
      if (s + 1 >= L) break;
      if (s + 2 < L) project(0, 0);
      load_x(t0 + min(s + 4, L - 1) * dt, 0);
      __syncthreads();
    }
    return;
  }

  // ---- consumers
  const float b_nh = bpack[(dir * 4 + 3) * H + u];
  float hprev[4] = {0.0f, 0.0f, 0.0f, 0.0f};           // h[seq = 4g + rho][u] of the previous step
  __syncthreads();                                     // h_0 and slot 0 are ready
  for (int step = 0; step < L; ++step) {
    const int t = t0 + dt * step;
    const int cur = step & 1;
    float ha[16];
    {
      const float4* hp = reinterpret_cast<const float4*>(&hbuf[cur][j][16 * g]);
#pragma unroll
      for (int i = 0; i < 4; ++i) { const float4 v = hp[i]; ha[4 * i] = v.x; ha[4 * i + 1] = v.y; ha[4 * i + 2] = v.z; ha[4 * i + 3] = v.w; }
    }
    const float* src = myproj + cur * SLOT;
    f32x4 acc_r = *reinterpret_cast<const f32x4*>(src);
    f32x4 acc_z = *reinterpret_cast<const f32x4*>(src + 256);
    const f32x4 acc_nx = *reinterpret_cast<const f32x4*>(src + 512);
    f32x4 acc_nh = {b_nh, b_nh, b_nh, b_nh};
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      acc_nh = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[s], wr[2][s], acc_nh, 0, 0, 0);
      acc_r = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[s], wr[0][s], acc_r, 0, 0, 0);
      acc_z = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[s], wr[1][s], acc_z, 0, 0, 0);
    }
#pragma unroll
    for (int rho = 0; rho < 4; ++rho) {                // C/D layout: reg rho -> row (sequence) 4g + rho, column (unit) j
      const float r = sigmoid_fast(acc_r[rho]);
      const float z = sigmoid_fast(acc_z[rho]);
      const float nn = tanh_fast(acc_nx[rho] + r * acc_nh[rho]);
      const float hn = (1.0f - z) * nn + z * hprev[rho];
      hprev[rho] = hn;
      const int srow = 4 * g + rho;
      hbuf[cur ^ 1][srow][u] = hn;
      if (seq0 + srow < n) out[(((size_t)dir * n_alloc + seq0 + srow) * L + t) * H + u] = hn;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(512) void gru_pc_kernel(const float* __restrict__ x, const float* __restrict__ wpack,
                                                     const float* __restrict__ bpack, float* __restrict__ out,
                                                     int n_alloc, int L, const int* __restrict__ count) {
  __shared__ __attribute__((aligned(16))) float hbuf[2][TS][HPAD];
  __shared__ __attribute__((aligned(16))) float xproj[2][4][3][64 * 4];        // [slot][wave][gate][lane x 4]
  gru_pc_body(x, wpack, bpack, out, n_alloc, L, count, hbuf, xproj);
}

// ------------------------------------------------------------------ fused conv epilogue + LayerNorm ----
// Channels-last rows [R, C]. One pass replaces the bias-add, ReLU, residual-add, time-bias-add and
// LayerNorm kernels PyTorch launches between two convolutions of the dilated-CNN backbone
// (reference models/dnaconv.py:188-197) and of the value net's conv tower (Enformer.py:2269-2285):
//     t     = y + bias
//     f_out = act 0: relu(t) + f_prev | act 1: relu(t + f_prev) | act 2: t + f_prev      (f_prev optional)
//     hn    = LayerNorm(f_out + tb) * gamma + beta                    (optional; eps = 1e-5, biased variance)
// One wave per row, lane owns VPL = C/64 consecutive channels (8-16 B vector loads), mean/variance by
// xor-shuffle wave reduction (two-pass, like ATen's RowwiseMoments). HBM-bound: 2 reads + 1-2 writes.
struct EpiArgs {
  const float* y; const float* bias; const float* f_prev; const float* tb; const float* gamma; const float* beta;
  float* f_out; float* hn; int64_t R; int act;
};


template <int VPL>
__global__ __launch_bounds__(256) void epilogue_ln_kernel(EpiArgs a) {
  constexpr int C = 64 * VPL;
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const int c0 = lane * VPL;
  float bias[VPL], tb[VPL], gm[VPL], bt[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    bias[i] = a.bias ? a.bias[c0 + i] : 0.0f;
    tb[i] = (a.hn && a.tb) ? a.tb[c0 + i] : 0.0f;
    gm[i] = a.hn ? a.gamma[c0 + i] : 1.0f;
    bt[i] = a.hn ? a.beta[c0 + i] : 0.0f;
  }
  for (int64_t r = wave; r < a.R; r += nwaves) {
    const int64_t base = r * C + c0;
    float v[VPL], p[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) { v[i] = a.y[base + i]; p[i] = a.f_prev ? a.f_prev[base + i] : 0.0f; }
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const float t = v[i] + bias[i];
      v[i] = a.act == 0 ? fmaxf(t, 0.0f) + p[i] : a.act == 1 ? fmaxf(t + p[i], 0.0f) : t + p[i];
      if (a.f_out) a.f_out[base + i] = v[i];
      v[i] += tb[i];
      s += v[i];
    }
    if (a.hn) {
      const float mean = wave_sum(s) * (1.0f / C);
      float q = 0.0f;
#pragma unroll
      for (int i = 0; i < VPL; ++i) { const float d = v[i] - mean; q += d * d; }
      const float rstd = rsqrtf(wave_sum(q) * (1.0f / C) + 1e-5f);
#pragma unroll
      for (int i = 0; i < VPL; ++i) a.hn[base + i] = (v[i] - mean) * rstd * gm[i] + bt[i];
    }
  }
}

// ------------------------------------------------------------- dilated Conv1d, channels-last, fp32 MFMA ----
// y[n, l, co] = sum_{t, ci} x[n, l + (t - T/2) * dil, ci] * W[co, ci, t]      ("same" zero padding, no bias)
// as an implicit GEMM on the exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32). One workgroup owns a tile
// of whole sequences (<= 224 rows: one L=200 sequence, four L=50 sequences), so that
//   * the activations of the tile are staged into LDS ONCE per 32-channel chunk and re-used by all T taps
//     (a tap is just a row offset into the LDS image; out-of-range rows read a zero row);
//   * taps whose receptive rows are all padding are skipped, per 32-row MFMA tile — at L=200 the
//     dilation-64 layers only do 35 % of the nominal work, dilation-16 82 %;
//   * B = 256 sequences is exactly one workgroup per CU (no tail).
// Wave w owns output channels [32 (w % NCT), +32) and row tiles w / NCT, w / NCT + 4 / NCT, ...;
// accumulators stay in registers across the whole K loop (Cin * T).
constexpr int CONV_RT = 7;                 // 32-row MFMA tiles per workgroup tile
constexpr int CONV_ROWS = 32 * CONV_RT;    // 224
constexpr int CH = 32;                     // input-channel chunk
constexpr int CHP = CH + 4;                // padded LDS row stride (floats): conflict-free ds_read_b128

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ConvArgs {
  const float* x; const float* wpack; float* y;
  int n, L, spt /*sequences per tile*/, T, dil;
  const float* bias; const float* f_prev; int act;      // fused epilogue (static kernels): act -1 = raw conv output
  const float* tb; const float* gamma; const float* beta; float* hn;   // + LayerNorm(y + tb) of the next layer (hn != NULL)
};

// 16 MFMAs of one 32-row tile: A = 4 float4 (16 consecutive input channels of this lane's row), B = bf[16]
#define CONV_MMA16(ACC, A0, A1, A2, A3)                                                    \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A0.x, bf[0], ACC, 0, 0, 0);                   \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A0.y, bf[1], ACC, 0, 0, 0);                   \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A0.z, bf[2], ACC, 0, 0, 0);                   \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A0.w, bf[3], ACC, 0, 0, 0);                   \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A1.x, bf[4], ACC, 0, 0, 0);                   \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A1.y, bf[5], ACC, 0, 0, 0);                   \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A1.z, bf[6], ACC, 0, 0, 0);                   \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A1.w, bf[7], ACC, 0, 0, 0);                   \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A2.x, bf[8], ACC, 0, 0, 0);                   \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A2.y, bf[9], ACC, 0, 0, 0);                   \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A2.z, bf[10], ACC, 0, 0, 0);                  \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A2.w, bf[11], ACC, 0, 0, 0);                  \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A3.x, bf[12], ACC, 0, 0, 0);                  \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A3.y, bf[13], ACC, 0, 0, 0);                  \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A3.z, bf[14], ACC, 0, 0, 0);                  \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A3.w, bf[15], ACC, 0, 0, 0);

// two row tiles interleaved: consecutive MFMAs never share an accumulator (a dependent back-to-back pair
// stalls ~43 cycles as soon as ANY other instruction is scheduled between them)
#define CONV_MMA2(K, AV, BV)                                                               \
  acc[ra] = __builtin_amdgcn_mfma_f32_32x32x2f32(AV, bf[K], acc[ra], 0, 0, 0);            \
  acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(BV, bf[K], acc[rb], 0, 0, 0);
#define CONV_MMA32(X0, X1, X2, X3, Y0, Y1, Y2, Y3)                                         \
  CONV_MMA2(0, X0.x, Y0.x) CONV_MMA2(1, X0.y, Y0.y) CONV_MMA2(2, X0.z, Y0.z) CONV_MMA2(3, X0.w, Y0.w)       \
  CONV_MMA2(4, X1.x, Y1.x) CONV_MMA2(5, X1.y, Y1.y) CONV_MMA2(6, X1.z, Y1.z) CONV_MMA2(7, X1.w, Y1.w)       \
  CONV_MMA2(8, X2.x, Y2.x) CONV_MMA2(9, X2.y, Y2.y) CONV_MMA2(10, X2.z, Y2.z) CONV_MMA2(11, X2.w, Y2.w)     \
  CONV_MMA2(12, X3.x, Y3.x) CONV_MMA2(13, X3.y, Y3.y) CONV_MMA2(14, X3.z, Y3.z) CONV_MMA2(15, X3.w, Y3.w)

template <int CIN, int COUT>
__global__ __launch_bounds__(256) void conv1d_cl_kernel(ConvArgs a) {
  constexpr int NCHUNK = CIN / CH;
  constexpr int NCT = COUT / 32;                 // column tiles (2 or 4)
  constexpr int RGROUPS = 4 / NCT;               // waves sharing a column tile split the row tiles
  constexpr int MAXRT = (CONV_RT + RGROUPS - 1) / RGROUPS;
  constexpr int BLD = COUT * 8 / 256;            // float4 per thread to stage one W[t][c] tile (2 or 4)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                                      // [CONV_ROWS + 1][CHP]   (+1: the zero row)
  float* Bs = smem + (CONV_ROWS + 1) * CHP;              // [2][COUT][CHP]

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // wave-uniform (SGPR): keeps the tile-liveness branches scalar
  const int i = lane & 31, h = lane >> 5;
  const int ct = w % NCT, rg = w / NCT;
  const int L = a.L, T = a.T;
  const int tile_rows = a.spt * L;
  const int64_t row0 = (int64_t)blockIdx.x * tile_rows;   // first flattened (n*L) row of this tile
  const int64_t total_rows = (int64_t)a.n * L;
  const int half_t = T / 2;
  const int NIT = NCHUNK * T;

  f32x16 acc[MAXRT];
#pragma unroll
  for (int r = 0; r < MAXRT; ++r)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[r][e] = 0.0f;

  // this lane's A row per owned row tile: LDS byte-free offsets and the position inside its sequence
  int arow[MAXRT], apos[MAXRT];
#pragma unroll
  for (int r = 0; r < MAXRT; ++r) {
    const int rt = rg + r * RGROUPS;
    const int tr = 32 * rt + i;
    arow[r] = tr;
    apos[r] = (rt < CONV_RT && tr < tile_rows) ? tr % L : -(1 << 20);   // padding rows never match a tap
  }
  for (int e = threadIdx.x; e < CHP; e += 256) As[CONV_ROWS * CHP + e] = 0.0f;   // zero row

  // staging coordinates of this thread for the weight tile W[t][c] ([COUT][32] contiguous in wpack)
  const int b_r = threadIdx.x >> 3, b_q = threadIdx.x & 7;             // rows b_r + 32 k, 16-B column b_q
  float4 bp0, bp1, bp2, bp3;                                            // prefetched tile (named: must stay in VGPRs)
  bp0 = bp1 = bp2 = bp3 = float4{0.0f, 0.0f, 0.0f, 0.0f};

  // first live tap
  int it = 0;
  while (it < NIT) { const int d = (it % T - half_t) * a.dil; if (max(0, -d) < min(L, L - d)) break; ++it; }
  if (it < NIT) {
    const float* wsrc = a.wpack + ((size_t)((it % T) * NCHUNK + it / T) * COUT) * CH + b_r * CH + 4 * b_q;
    bp0 = *reinterpret_cast<const float4*>(wsrc);
    bp1 = *reinterpret_cast<const float4*>(wsrc + 32 * CH);
    if (BLD > 2) { bp2 = *reinterpret_cast<const float4*>(wsrc + 64 * CH); bp3 = *reinterpret_cast<const float4*>(wsrc + 96 * CH); }
    float* Bt = Bs + b_r * CHP + 4 * b_q;
    *reinterpret_cast<float4*>(Bt) = bp0;
    *reinterpret_cast<float4*>(Bt + 32 * CHP) = bp1;
    if (BLD > 2) { *reinterpret_cast<float4*>(Bt + 64 * CHP) = bp2; *reinterpret_cast<float4*>(Bt + 96 * CHP) = bp3; }
  }
  int par = 0, cur_c = -1;
  while (it < NIT) {
    const int c = it / T, t = it % T;
    if (c != cur_c) {                                        // new input-channel chunk: restage the activations
      __syncthreads();                                       // previous chunk's readers are done with As
      for (int e = threadIdx.x; e < CONV_ROWS * 8; e += 256) {
        const int r = e >> 3, q = e & 7;
        float4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (r < tile_rows && row0 + r < total_rows)
          v = *reinterpret_cast<const float4*>(a.x + (row0 + r) * CIN + c * CH + 4 * q);
        *reinterpret_cast<float4*>(As + r * CHP + 4 * q) = v;
      }
      cur_c = c;
    }
    // next live tap; its weight tile is fetched now and flies under this tap's MFMAs
    int nxt = it + 1;
    while (nxt < NIT) { const int d = (nxt % T - half_t) * a.dil; if (max(0, -d) < min(L, L - d)) break; ++nxt; }
    if (nxt < NIT) {
      const float* wsrc = a.wpack + ((size_t)((nxt % T) * NCHUNK + nxt / T) * COUT) * CH + b_r * CH + 4 * b_q;
      bp0 = *reinterpret_cast<const float4*>(wsrc);
      bp1 = *reinterpret_cast<const float4*>(wsrc + 32 * CH);
      if (BLD > 2) { bp2 = *reinterpret_cast<const float4*>(wsrc + 64 * CH); bp3 = *reinterpret_cast<const float4*>(wsrc + 96 * CH); }
    }
    __syncthreads();                                         // Bs[par] (and As) visible to every wave
    float bf[16];
    {
      const float4* bq = reinterpret_cast<const float4*>(Bs + par * COUT * CHP + (32 * ct + i) * CHP + 16 * h);
      const float4 v0 = bq[0], v1 = bq[1], v2 = bq[2], v3 = bq[3];
      bf[0] = v0.x; bf[1] = v0.y; bf[2] = v0.z; bf[3] = v0.w; bf[4] = v1.x; bf[5] = v1.y; bf[6] = v1.z; bf[7] = v1.w;
      bf[8] = v2.x; bf[9] = v2.y; bf[10] = v2.z; bf[11] = v2.w; bf[12] = v3.x; bf[13] = v3.y; bf[14] = v3.z; bf[15] = v3.w;
    }
    const int delta = (t - half_t) * a.dil;
    const int lo = max(0, -delta), hi = min(L, L - delta);   // rows l with 0 <= l + delta < L are live
    const float* Ah = As + 16 * h;
    // software pipeline over the row tiles: the 4 ds_read_b128 of tile r+1 are issued before the 16 MFMAs of tile r
    float4 x0, x1, x2, x3, y0, y1, y2, y3;
    x0 = x1 = x2 = x3 = y0 = y1 = y2 = y3 = float4{0.0f, 0.0f, 0.0f, 0.0f};
#define CONV_LIVE(R) ((rg + (R) * RGROUPS) < CONV_RT && (a.spt == 1 ? (lo < 32 * (rg + (R) * RGROUPS) + 32 && hi > 32 * (rg + (R) * RGROUPS)) \
                                                                      : 32 * (rg + (R) * RGROUPS) < tile_rows))
#define CONV_ALOAD(R, V0, V1, V2, V3)                                                                    \
  {                                                                                                       \
    const int p_ = apos[R] + delta;                                                                       \
    const float4* ap_ = reinterpret_cast<const float4*>(Ah + ((p_ >= 0 && p_ < L) ? arow[R] + delta : CONV_ROWS) * CHP); \
    V0 = ap_[0]; V1 = ap_[1]; V2 = ap_[2]; V3 = ap_[3];                                                    \
  }
    // row tiles in pairs (2 independent accumulator chains interleaved); dead tiles of a dilated tap are skipped
#pragma unroll
    for (int r = 0; r < MAXRT; r += 2) {
      const int ra = r, rb = (r + 1 < MAXRT) ? r + 1 : r;
      const bool la = CONV_LIVE(ra), lb = (r + 1 < MAXRT) && CONV_LIVE(rb);
      if (la && lb) {
        CONV_ALOAD(ra, x0, x1, x2, x3)
        CONV_ALOAD(rb, y0, y1, y2, y3)
        CONV_MMA32(x0, x1, x2, x3, y0, y1, y2, y3)
      } else if (la) {
        CONV_ALOAD(ra, x0, x1, x2, x3)
        CONV_MMA16(acc[ra], x0, x1, x2, x3)
      } else if (lb) {
        CONV_ALOAD(rb, y0, y1, y2, y3)
        CONV_MMA16(acc[rb], y0, y1, y2, y3)
      }
    }
    if (nxt < NIT) {                                        // other buffer: its last readers passed this tap's barrier
      float* Bt = Bs + (par ^ 1) * COUT * CHP + b_r * CHP + 4 * b_q;
      *reinterpret_cast<float4*>(Bt) = bp0;
      *reinterpret_cast<float4*>(Bt + 32 * CHP) = bp1;
      if (BLD > 2) { *reinterpret_cast<float4*>(Bt + 64 * CHP) = bp2; *reinterpret_cast<float4*>(Bt + 96 * CHP) = bp3; }
    }
    par ^= 1;
    it = nxt;
  }
#undef CONV_LIVE
#undef CONV_ALOAD
  // C/D layout of 32x32: reg e -> row (e & 3) + 8 (e >> 2) + 4 h, column i
#pragma unroll
  for (int r = 0; r < MAXRT; ++r) {
    const int rt = rg + r * RGROUPS;
    if (rt >= CONV_RT) continue;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int tr = 32 * rt + (e & 3) + 8 * (e >> 2) + 4 * h;
      if (tr < tile_rows && row0 + tr < total_rows) a.y[(row0 + tr) * COUT + 32 * ct + i] = acc[r][e];
    }
  }
}

// ---- statically scheduled variant: taps, dilation and sequence length are template parameters, so which
// (tap, 32-row tile) pairs touch only padding is known at compile time: no branch surrounds any MFMA, the
// accumulators stay in place, and the compiler software-pipelines the straight-line tap bodies.
constexpr bool conv_tap_live(int t, int T, int dil, int L) {
  const int d = (t - T / 2) * dil;
  const int lo = d < 0 ? -d : 0, hi = d > 0 ? L - d : L;
  return lo < hi;
}
constexpr bool conv_tile_live(int t, int rt, int T, int dil, int L, int spt) {
  const int d = (t - T / 2) * dil;
  const int lo = d < 0 ? -d : 0, hi = d > 0 ? L - d : L;
  if (lo >= hi) return false;
  if (32 * rt >= spt * L) return false;                       // pure padding tile
  if (spt != 1) return true;
  return lo < 32 * rt + 32 && hi > 32 * rt;
}

template <int CIN, int COUT, int T, int DIL, int LSEQ>
__global__ __launch_bounds__(256) void conv1d_cl_static_kernel(ConvArgs a) {
  constexpr int NCHUNK = CIN / CH;
  constexpr int NCT = COUT / 32;                 // 4 (128 channels) or 2 (64)
  constexpr int RGROUPS = 4 / NCT;               // waves sharing a column tile take interleaved row tiles
  constexpr int NRT = (CONV_RT + RGROUPS - 1) / RGROUPS;   // row tiles per wave (the last one of group 1 is padding)
  constexpr int BLD = COUT * 8 / 256;            // float4 per thread per weight tile
  constexpr int SPT = CONV_ROWS / LSEQ;
  constexpr int TILE_ROWS = SPT * LSEQ;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                                      // [CONV_ROWS + 1][CHP]
  float* Bs = smem + (CONV_ROWS + 1) * CHP;              // [2][COUT][CHP]

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ct = w % NCT, rg = w / NCT;                  // this wave's 32 output channels / row-tile group
  const int i = lane & 31, h = lane >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * TILE_ROWS;
  const int64_t total_rows = (int64_t)a.n * LSEQ;

  f32x16 acc[NRT];
#pragma unroll
  for (int r = 0; r < NRT; ++r)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[r][e] = 0.0f;

  // row tile r of this wave is tile rt = rg + r * RGROUPS; arow = its row for this lane, apos = position in its sequence
  int arow[NRT], apos[NRT];
#pragma unroll
  for (int r = 0; r < NRT; ++r) {
    arow[r] = 32 * (rg + r * RGROUPS) + i;
    apos[r] = (arow[r] < TILE_ROWS) ? arow[r] % LSEQ : -(1 << 20);      // padding rows read the zero row
  }
  for (int e = threadIdx.x; e < CHP; e += 256) As[CONV_ROWS * CHP + e] = 0.0f;   // zero row

  const int b_r = threadIdx.x >> 3, b_q = threadIdx.x & 7;
  const float* wbase = a.wpack + b_r * CH + 4 * b_q;
  float* bdst = Bs + b_r * CHP + 4 * b_q;
  float4 bp0, bp1, bp2, bp3;
  bp2 = bp3 = float4{0.0f, 0.0f, 0.0f, 0.0f};
  int par = 0;
  {                                                      // first live tap of chunk 0
    int t0 = 0;
#pragma unroll
    for (int t = T - 1; t >= 0; --t) if (conv_tap_live(t, T, DIL, LSEQ)) t0 = t;
    const float* wsrc = wbase + ((size_t)(t0 * NCHUNK) * COUT) * CH;
    bp0 = *reinterpret_cast<const float4*>(wsrc);
    bp1 = *reinterpret_cast<const float4*>(wsrc + 32 * CH);
    if (BLD > 2) { bp2 = *reinterpret_cast<const float4*>(wsrc + 64 * CH); bp3 = *reinterpret_cast<const float4*>(wsrc + 96 * CH); }
    *reinterpret_cast<float4*>(bdst) = bp0;
    *reinterpret_cast<float4*>(bdst + 32 * CHP) = bp1;
    if (BLD > 2) { *reinterpret_cast<float4*>(bdst + 64 * CHP) = bp2; *reinterpret_cast<float4*>(bdst + 96 * CHP) = bp3; }
  }
  const float* Ah = As + 16 * h;
  for (int c = 0; c < NCHUNK; ++c) {
    __syncthreads();                                       // previous chunk's readers are done with As
    for (int e = threadIdx.x; e < CONV_ROWS * 8; e += 256) {
      const int r = e >> 3, q = e & 7;
      float4 v = {0.0f, 0.0f, 0.0f, 0.0f};
      if (r < TILE_ROWS && row0 + r < total_rows)
        v = *reinterpret_cast<const float4*>(a.x + (row0 + r) * CIN + c * CH + 4 * q);
      *reinterpret_cast<float4*>(As + r * CHP + 4 * q) = v;
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      if (!conv_tap_live(t, T, DIL, LSEQ)) continue;       // compile-time
      // weight tile of the next live tap (next chunk's first live tap after the last one) flies under the MFMAs
      int tn = -1;
#pragma unroll
      for (int u = T - 1; u > t; --u) if (conv_tap_live(u, T, DIL, LSEQ)) tn = u;
      int cn = c;
      if (tn < 0) {
        cn = c + 1;
#pragma unroll
        for (int u = T - 1; u >= 0; --u) if (conv_tap_live(u, T, DIL, LSEQ)) tn = u;
      }
      const bool have_next = cn < NCHUNK;
      if (have_next) {
        const float* wsrc = wbase + ((size_t)(tn * NCHUNK + cn) * COUT) * CH;
        bp0 = *reinterpret_cast<const float4*>(wsrc);
        bp1 = *reinterpret_cast<const float4*>(wsrc + 32 * CH);
        if (BLD > 2) { bp2 = *reinterpret_cast<const float4*>(wsrc + 64 * CH); bp3 = *reinterpret_cast<const float4*>(wsrc + 96 * CH); }
      }
      __syncthreads();                                     // Bs[par] (and As) visible to every wave
      float bf[16];
      {
        const float4* bq = reinterpret_cast<const float4*>(Bs + par * COUT * CHP + (32 * ct + i) * CHP + 16 * h);
        const float4 v0 = bq[0], v1 = bq[1], v2 = bq[2], v3 = bq[3];
        bf[0] = v0.x; bf[1] = v0.y; bf[2] = v0.z; bf[3] = v0.w; bf[4] = v1.x; bf[5] = v1.y; bf[6] = v1.z; bf[7] = v1.w;
        bf[8] = v2.x; bf[9] = v2.y; bf[10] = v2.z; bf[11] = v2.w; bf[12] = v3.x; bf[13] = v3.y; bf[14] = v3.z; bf[15] = v3.w;
      }
      constexpr int dummy = 0; (void)dummy;
      const int delta = (t - T / 2) * DIL;
      // Tile liveness is a compile-time fact when every wave owns all row tiles (RGROUPS == 1); with two row
      // groups a tile's index depends on the wave, so only whole-tap skipping is static there.
#define SCONV_LIVE(R) (RGROUPS == 1 ? conv_tile_live(t, R, T, DIL, LSEQ, SPT) : true)
      float4 af[NRT][4];
#pragma unroll
      for (int r = 0; r < NRT; ++r) {
        if (!SCONV_LIVE(r)) continue;
        const int p = apos[r] + delta;
        const float4* ap = reinterpret_cast<const float4*>(Ah + ((p >= 0 && p < LSEQ) ? arow[r] + delta : CONV_ROWS) * CHP);
        af[r][0] = ap[0]; af[r][1] = ap[1]; af[r][2] = ap[2]; af[r][3] = ap[3];
      }
      // k-step outer, row tile inner: consecutive MFMAs never share an accumulator
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int r = 0; r < NRT; ++r)
          if (SCONV_LIVE(r)) acc[r] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[r][q].x, bf[4 * q], acc[r], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < NRT; ++r)
          if (SCONV_LIVE(r)) acc[r] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[r][q].y, bf[4 * q + 1], acc[r], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < NRT; ++r)
          if (SCONV_LIVE(r)) acc[r] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[r][q].z, bf[4 * q + 2], acc[r], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < NRT; ++r)
          if (SCONV_LIVE(r)) acc[r] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[r][q].w, bf[4 * q + 3], acc[r], 0, 0, 0);
      }
#undef SCONV_LIVE
      if (have_next) {                                    // other buffer: its last readers passed this tap's barrier
        float* bd = bdst + (par ^ 1) * COUT * CHP;
        *reinterpret_cast<float4*>(bd) = bp0;
        *reinterpret_cast<float4*>(bd + 32 * CHP) = bp1;
        if (BLD > 2) { *reinterpret_cast<float4*>(bd + 64 * CHP) = bp2; *reinterpret_cast<float4*>(bd + 96 * CHP) = bp3; }
      }
      par ^= 1;
    }
  }
  // ---- epilogue ----
  if (a.act < 0) {                                        // raw conv output straight from the accumulators
#pragma unroll
    for (int r = 0; r < NRT; ++r) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int tr = 32 * (rg + r * RGROUPS) + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (tr < TILE_ROWS && row0 + tr < total_rows) a.y[(row0 + tr) * COUT + 32 * ct + i] = acc[r][e];
      }
    }
    return;
  }
  // Fused: the accumulator tile goes through LDS (two halves of 128 rows: it does not fit at once) so that the
  // residual read, the f store and the LayerNorm run row-wise with fully coalesced 256/512-B rows:
  //   t = conv + bias ; f = act 0: relu(t) + f_prev | 1: relu(t + f_prev) | 2: t + f_prev ; hn = LN(f + tb)*gamma + beta
  constexpr int EP = COUT + 4;                            // LDS row stride of the epilogue tile
  constexpr int VPL = COUT / 64;                          // channels per lane in the row-wise pass
  float* Es = smem;
  const float bias_c = a.bias ? a.bias[32 * ct + i] : 0.0f;
  float tbv[VPL], gmv[VPL], btv[VPL];
#pragma unroll
  for (int k = 0; k < VPL; ++k) {
    tbv[k] = (a.hn && a.tb) ? a.tb[lane * VPL + k] : 0.0f;
    gmv[k] = a.hn ? a.gamma[lane * VPL + k] : 1.0f;
    btv[k] = a.hn ? a.beta[lane * VPL + k] : 0.0f;
  }
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    __syncthreads();                                      // main loop / previous half is done with this LDS
#pragma unroll
    for (int r = 0; r < NRT; ++r) {
      const int rt = rg + r * RGROUPS;
      if (rt / 4 != half || rt >= CONV_RT) continue;      // scalar-uniform
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int lr = 32 * (rt - 4 * half) + (e & 3) + 8 * (e >> 2) + 4 * h;
        Es[lr * EP + 32 * ct + i] = acc[r][e] + bias_c;
      }
    }
    __syncthreads();
    const int nrows = min(128, TILE_ROWS - 128 * half);
    constexpr int RB = 8;                                 // rows in flight per wave: the residual loads are issued together
    for (int base = 0; base < nrows; base += 4 * RB) {
      float p[RB][VPL], gt[RB][VPL];
#pragma unroll
      for (int j = 0; j < RB; ++j) {
        const int lr = base + 4 * j + w;
        const int64_t gr = row0 + 128 * half + lr;
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
          p[j][k] = (a.f_prev && lr < nrows && gr < total_rows) ? a.f_prev[gr * COUT + lane * VPL + k] : 0.0f;
          // act 3 (svdd_conv1d_cl_gated_f32, the backward pass of a ReLU layer): a.tb is a ROW tensor [rows][COUT], the forward
          // activation whose sign gates this gradient
          gt[j][k] = (a.act == 3 && lr < nrows && gr < total_rows) ? a.tb[gr * COUT + lane * VPL + k] : 1.0f;
        }
      }
#pragma unroll
      for (int j = 0; j < RB; ++j) {
        const int lr = base + 4 * j + w;
        const int64_t gr = row0 + 128 * half + lr;
        if (lr >= nrows || gr >= total_rows) continue;    // wave-uniform
        const int64_t o = gr * COUT + lane * VPL;
        float v[VPL];
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
          const float t = Es[lr * EP + lane * VPL + k];
          v[k] = a.act == 0 ? fmaxf(t, 0.0f) + p[j][k] : a.act == 1 ? fmaxf(t + p[j][k], 0.0f) :
                 a.act == 3 ? (gt[j][k] > 0.0f ? t + p[j][k] : 0.0f) : t + p[j][k];
          a.y[o + k] = v[k];
          v[k] += tbv[k];
          sum += v[k];
        }
        if (a.hn) {
          const float mean = wave_sum(sum) * (1.0f / COUT);
          float q = 0.0f;
#pragma unroll
          for (int k = 0; k < VPL; ++k) { const float d = v[k] - mean; q += d * d; }
          const float rstd = rsqrtf(wave_sum(q) * (1.0f / COUT) + 1e-5f);
#pragma unroll
          for (int k = 0; k < VPL; ++k) a.hn[o + k] = (v[k] - mean) * rstd * gmv[k] + btv[k];
        }
      }
    }
  }
}

// ------------------------------------------------------------------- fused conv tower (value network) ----
// The whole ConvTower of the ConvGRU value net (reference Enformer.py:1634-1751 with the Stem :1754-1804 and five
// ConvBlocks "CDNRA" :2176-2292; eval-mode BatchNorm folded into the weights by the host):
//     a0 = relu(conv15(onehot) + b0) ;  a_{k+1} = relu(conv5(a_k) + b_k + a_k)   (k = 0..4, 64 channels)
// in ONE launch, one workgroup per tile of whole sequences (<= 208 rows). The activations never leave the CU:
// they ping-pong between two LDS images [rows][64] and are the MFMA A operands directly (a tap is a row offset;
// rows outside the sequence read a zero row), so there is no activation traffic to HBM between layers (5 x 2 x
// 131 MB per value forward at n = 2560), no separate bias/residual/ReLU pass and no im2col staging. Only the
// weights stream through LDS (one [64][32] tile per (layer, tap, 32-channel chunk), register-prefetched).
// v_mfma_f32_16x16x4_f32 with 16-row tiles: 13 row tiles x 4 column tiles = 52 units = 13 per SIMD exactly
// (200 rows pad to 208: 4 % waste instead of 12 % with 32-row tiles). 8 waves: wave w owns column tile w & 3 and
// the row tiles of parity w >> 2, so the two waves of a SIMD interleave their MFMA streams.
// TW_ROWS = 208 rows = TW_RT = 13 row tiles of 16, TW_MAXL = 8 conv layers after the stem: svdd_host.h
constexpr int TW_C = 64;
constexpr int TW_AP = TW_C + 4;            // LDS row stride of the activation images (floats)

struct TowerArgs {
  const float* x;        // [n, L, 4] one-hot (value-function input)
  const float* tiles;    // [2 + 10*nlayers][64 cout][32] weight tiles in execution order:
                         //   stem: k = 4*tap + channel (60 real, 4 zero), chunks 0,1 ; then per layer, per 32-channel chunk, per tap
  const float* bias;     // [1 + nlayers][64]   stem bias, then the (BatchNorm-folded) layer biases
  float* out;            // [n, L, 64]
  int n, L, spt, nlayers, residual_mask;
  const int* count;      // device scalar: valid rows of a compacted batch (NULL: n) ; conv_tower_kernel only
};

// ------------------------------------------------------------------- the pieces of the fp32 tower family, defined ONCE ----
// conv_tower_kernel, conv_tower_win_kernel (generation 1), conv_tower2_kernel (generation 2) and conv_tower_parts_kernel must give
// each other's bits: a candidate's rows are either copied from its parent's tower output or recomputed, by whichever of them. So
// what decides a bit is text they share: the weight stream (which tile, which k-step feeds which MFMA), the order of the MFMAs of
// one accumulator, which image bytes a tap reads and what a row past the sequence reads (the zero rows -1 and TW_ROWS), and the
// epilogue bias -> residual -> ReLU. What MAY differ between kernels, and only that: which wave and lane owns which (row tile,
// column tile), the orientation of the accumulator (generation 2 is transposed), how many tiles are live and where a tile's first
// row lies, the schedule of fragment requests against MFMA groups, and which rows are staged, kept and stored. The pieces are macros
// on purpose, as BB_* / B2_* below: they name the locals of the kernel that uses them (wsrc, it, nit, actb, a_lo, a_hi, chk, delta,
// xs, acc ...), and textual sharing keeps every kernel's instruction stream what it was.
//
// Weight stream: BN = float4[2 CT], this lane's slice of the next tile for CT column tiles; B[CT][8] the current one, unpacked.
// TW_WLOAD1 / TW_UNPACK1 are one column tile of them, its two float4 named by the user; the *_ONE forms are for the kernels with one
// column tile per wave, which name them directly (generation 1: two variables, the parts kernel: bn[0], bn[1]): through the CT
// loop, or in generation 1 through an array, their instructions change.
#define TW_WLOAD1(BN0, BN1, SRC)                                                                              \
  BN0 = *reinterpret_cast<const float4*>(SRC);                                                                \
  BN1 = *reinterpret_cast<const float4*>((SRC) + 4);
#define TW_UNPACK1(B, BN0, BN1)                                                                               \
  B[0] = BN0.x; B[1] = BN0.y; B[2] = BN0.z; B[3] = BN0.w; B[4] = BN1.x; B[5] = BN1.y; B[6] = BN1.z; B[7] = BN1.w;
#define TW_WLOAD(BN, SRC, CT)                                                                                 \
  { const float* src_ = (SRC);                                                                                \
    _Pragma("unroll") for (int ct_ = 0; ct_ < CT; ++ct_) { TW_WLOAD1(BN[2 * ct_], BN[2 * ct_ + 1], src_ + ct_ * 16 * CH) } }
#define TW_WLOAD_ONE(BN0, BN1, SRC) { const float* src_ = (SRC); TW_WLOAD1(BN0, BN1, src_) }
#define TW_UNPACK(B, BN, CT)                                                                                  \
  float B[CT][8];                                                                                             \
  _Pragma("unroll") for (int ct_ = 0; ct_ < CT; ++ct_) { TW_UNPACK1(B[ct_], BN[2 * ct_], BN[2 * ct_ + 1]) }
#define TW_UNPACK_ONE(B, BN0, BN1) float B[1][8]; TW_UNPACK1(B[0], BN0, BN1)
// the tile of iteration it + 1 flies under the MFMAs of iteration it (tiles are stored in execution order)
#define TW_WNEXT(BN, CT) if (it + 1 < nit) TW_WLOAD(BN, wsrc + (size_t)(it + 1) * TW_C * CH, CT)
#define TW_WNEXT_ONE(BN0, BN1) if (it + 1 < nit) TW_WLOAD_ONE(BN0, BN1, wsrc + (size_t)(it + 1) * TW_C * CH)
// iteration ci of a conv block: 32-channel chunk chk, tap delta = -2 .. 2 ; dbytes = what both add to an image byte offset
#define TW_TAP(CI)                                                                                            \
  const int chk = (CI) / 5, delta = (CI) - 5 * chk - 2;                                                       \
  const int dbytes = delta * (TW_AP * 4) + chk * (CH * 4);
// A fragment V (float4[2]) of the image at byte offset OFF ; CLAMPED: one sequence per image, a row before / past the image reads
// the zero row -1 / TW_ROWS ; APOS: several sequences per image, POS = the row's position in its sequence
#define TW_ALOAD(V, OFF)                                                                                      \
  { const float4* ap_ = reinterpret_cast<const float4*>(actb + (OFF)); V[0] = ap_[0]; V[1] = ap_[1]; }
#define TW_ALOAD_CLAMPED(V, OFF) TW_ALOAD(V, min(max((OFF), a_lo + chk * (CH * 4)), a_hi + chk * (CH * 4)))
#define TW_ALOAD_APOS(V, POS, OFF) TW_ALOAD(V, (unsigned)((POS) + delta) < (unsigned)L ? (OFF) : a_hi + chk * (CH * 4))
// the stem's fragment: k = 32 ci + 8 g + s covers taps t0 = 8 ci + 2 g and t0 + 1 (4 channels each): V[Q] = one-hot row IDX
#define TW_XLOAD(V, Q, IDX) V[Q] = *reinterpret_cast<const float4*>(xs + 4 * (IDX));
// Generation 1: wave parity rh owns the row tiles rh + 2 r, r < 7 ; the last one (12 = 0 + 2 * 6) belongs to parity 0
#define TW_OWNED(R) (!((R) == 6 && rh == 1))
// Generation 1: the MFMAs of CNT row tiles R0 .. of one weight tile bf, k-step by k-step across the tiles (8 per accumulator, in
// k order); AF[r_] = tile R0 + r_'s fragment, LIVE (it may name r_) = the tile exists
#define TW_MM1(AF, R0, CNT, LIVE)                                                                             \
  _Pragma("unroll") for (int q_ = 0; q_ < 2; ++q_) {                                                          \
    _Pragma("unroll") for (int r_ = 0; r_ < CNT; ++r_) if (LIVE) acc[R0 + r_] = __builtin_amdgcn_mfma_f32_16x16x4f32(AF[r_][q_].x, bf[0][4 * q_], acc[R0 + r_], 0, 0, 0);     \
    _Pragma("unroll") for (int r_ = 0; r_ < CNT; ++r_) if (LIVE) acc[R0 + r_] = __builtin_amdgcn_mfma_f32_16x16x4f32(AF[r_][q_].y, bf[0][4 * q_ + 1], acc[R0 + r_], 0, 0, 0); \
    _Pragma("unroll") for (int r_ = 0; r_ < CNT; ++r_) if (LIVE) acc[R0 + r_] = __builtin_amdgcn_mfma_f32_16x16x4f32(AF[r_][q_].z, bf[0][4 * q_ + 2], acc[R0 + r_], 0, 0, 0); \
    _Pragma("unroll") for (int r_ = 0; r_ < CNT; ++r_) if (LIVE) acc[R0 + r_] = __builtin_amdgcn_mfma_f32_16x16x4f32(AF[r_][q_].w, bf[0][4 * q_ + 3], acc[R0 + r_], 0, 0, 0); \
  }
// Generation 1's schedule of a (chunk, tap) iteration: tile groups (0,1,2)(3,4)(5,6) through two register buffers, each group's
// reads one group ahead. LD(R, V) requests tile R's fragment (and skips tile 6 for parity 1), G3 / G2(AF, R0) = the MFMAs of 3 / 2 tiles
#define TW_SCHED322(LD, G3, G2)                                                                               \
  LD(0, fa[0]) LD(1, fa[1]) LD(2, fa[2])                                                                      \
  LD(3, fb[0]) LD(4, fb[1])                                                                                   \
  __builtin_amdgcn_sched_barrier(0);                                                                          \
  LGKM_WAIT(4)                                                                                                \
  G3(fa, 0)                                                                                                   \
  __builtin_amdgcn_sched_barrier(0);                                                                          \
  LD(5, fa[0]) LD(6, fa[1])                                                                                   \
  __builtin_amdgcn_sched_barrier(0);                                                                          \
  if (rh == 1) { LGKM_WAIT(2) } else { LGKM_WAIT(4) }                                                         \
  G2(fb, 3)                                                                                                   \
  __builtin_amdgcn_sched_barrier(0);                                                                          \
  LGKM_WAIT(0)                                                                                                \
  G2(fa, 5)                                                                                                   \
  __builtin_amdgcn_sched_barrier(0);
// Generation 1's layer epilogue (C/D layout: reg e -> row 4 g + e, column j): every wave must be done reading the image before its
// owners overwrite it (the stem reads xs, not the image); rows from NROWS on stay zero
#define TW_EPILOGUE1(LIVE, NROWS)                                                                             \
  if (layer >= 0) __syncthreads();                                                                            \
  const bool res = layer >= 0 && ((a.residual_mask >> layer) & 1);                                            \
  _Pragma("unroll") for (int r = 0; r < 7; ++r) {                                                             \
    if (!(LIVE)) continue;                                                                                    \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                           \
      const int row = 16 * (rh + 2 * r) + 4 * g + e;                                                          \
      const int o = row * TW_AP + 16 * cs + j;                                                                \
      const float v = acc[r][e] + (res ? act[o] : 0.0f);                                                      \
      act[o] = row < (NROWS) ? fmaxf(v, 0.0f) : 0.0f;                                                         \
    }                                                                                                         \
  }                                                                                                           \
  __syncthreads();                                       /* the image is complete */
// Generation 2 (transposed: the weight fragment is the A operand): the MFMAs of NL row tiles x CT column tiles of one weight tile b
#define TW_MM2(NL, CT)                                                                                        \
  _Pragma("unroll") for (int r = 0; r < NL; ++r)                                                              \
    _Pragma("unroll") for (int q = 0; q < 2; ++q) {                                                           \
      const float av[4] = {af[r][q].x, af[r][q].y, af[r][q].z, af[r][q].w};                                   \
      _Pragma("unroll") for (int s4 = 0; s4 < 4; ++s4)                                                        \
        _Pragma("unroll") for (int ct = 0; ct < CT; ++ct)                                                     \
          acc[r][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[ct][4 * q + s4], av[s4], acc[r][ct], 0, 0, 0);  \
    }
// Heads and tails. The one-hot image xs: rows -HALO .. TW_ROWS + HALO of a tile of whole sequences (zero outside the tile), or
// rows W0 - 8 .. of the sequence XC (real data beyond a window, zero outside the sequence)
#define TW_STAGE_SEQ(XC, HALO)                                                                                \
  for (int e = tid - (HALO); e < TW_ROWS + (HALO); e += 512) {                                                \
    float4 v = {0.0f, 0.0f, 0.0f, 0.0f};                                                                      \
    if (e >= 0 && e < tile_rows && row0 + e < total_rows) v = *reinterpret_cast<const float4*>((XC) + (row0 + e) * 4); \
    *reinterpret_cast<float4*>(xs + 4 * e) = v;                                                               \
  }
#define TW_STAGE_WIN(XC, W0)                                                                                  \
  for (int e = tid - 8; e < TW_ROWS + 8; e += 512) {                                                          \
    const int gl = (W0) + e;                                                                                  \
    float4 v = {0.0f, 0.0f, 0.0f, 0.0f};                                                                      \
    if (gl >= 0 && gl < L) v = *reinterpret_cast<const float4*>((XC) + (size_t)gl * 4);                       \
    *reinterpret_cast<float4*>(xs + 4 * e) = v;                                                               \
  }
// a window candidate's rows outside [keep_lo, keep_hi) are its parent's, straight from its output ; the kept ones are the image's
#define TW_COPY_PARENT_WIN(PAR)                                                                               \
  for (int e = tid; e < L * 16; e += 512) {                                                                   \
    const int row = e >> 4;                                                                                   \
    if (row < keep_lo || row >= keep_hi)                                                                      \
      *reinterpret_cast<float4*>(outc + (size_t)row * TW_C + 4 * (e & 15)) = *reinterpret_cast<const float4*>((PAR) + (size_t)row * TW_C + 4 * (e & 15)); \
  }
#define TW_STORE_WIN                                                                                          \
  for (int e = tid; e < L * 16; e += 512) {                                                                   \
    const int row = e >> 4, q = e & 15;                                                                       \
    if (row >= keep_lo && row < keep_hi)                                                                      \
      *reinterpret_cast<float4*>(outc + (size_t)row * TW_C + 4 * q) = *reinterpret_cast<const float4*>(act + (row - w0) * TW_AP + 4 * q); \
  }
// final image of a tile of whole sequences -> HBM, 16 B per thread, rows contiguous
#define TW_STORE_SEQ                                                                                          \
  for (int e = tid; e < tile_rows * 16; e += 512) {                                                           \
    const int row = e >> 4, q = e & 15;                                                                       \
    if (row0 + row < total_rows)                                                                              \
      *reinterpret_cast<float4*>(a.out + (row0 + row) * TW_C + 4 * q) = *reinterpret_cast<const float4*>(act + row * TW_AP + 4 * q); \
  }

// One LDS activation image only: a layer's outputs wait in the accumulators until every wave has finished reading
// the image, then each wave overwrites the positions it owns (reading its own residual first). 57 KB of LDS and
// <= 128 VGPRs per wave => TWO workgroups (16 waves) per CU, which overlap each other's barriers, LDS latency and
// global stores.
// Weight stream: each wave reads ITS [16 cout][32 k] slice of the (layer, chunk, tap) tile straight from L2 into the
// B-operand registers, one tile ahead: no LDS staging and no barrier per tap, so the waves of a workgroup run
// unsynchronised inside a layer. MFMA groups are fenced (sched_barrier) behind one explicit lgkmcnt wait: an
// s_waitcnt or ds_read between two MFMAs costs tens of cycles of matrix-pipe time on gfx950.
// SPT1 (one sequence per tile): image rows -1 and >= L are zero, so a tap is a clamped row offset.
template <bool SPT1>
__global__ __launch_bounds__(512, 4) void conv_tower_kernel(TowerArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* act = smem + TW_AP;                            // rows -1 .. TW_ROWS ; [-1] and [TW_ROWS] stay zero
  float* xs = smem + (TW_ROWS + 2) * TW_AP + 4;         // one-hot tile, rows -1 .. TW_ROWS ; [-1], [>= L], [TW_ROWS] zero

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cs = w & 3, rh = w >> 2;                    // column tile (16 channels) ; row-tile parity
  const int j = lane & 15, g = lane >> 4;
  const int L = a.L;
  const int tile_rows = a.spt * L;
  const int64_t row0 = (int64_t)blockIdx.x * tile_rows;
  const int64_t total_rows = (int64_t)(a.count ? __builtin_amdgcn_readfirstlane(*a.count) : a.n) * L;
  if (row0 >= total_rows) return;

  TW_STAGE_SEQ(a.x, 1)
  for (int e = tid; e < TW_AP; e += 512) { smem[e] = 0.0f; act[TW_ROWS * TW_AP + e] = 0.0f; }
  const float* wsrc = a.tiles + (16 * cs + j) * CH + 8 * g;
  float4 bn0, bn1;
  TW_WLOAD_ONE(bn0, bn1, wsrc)

  const int arow0 = 16 * rh + j;                        // this lane feeds rows arow0 + 32 r as the A operand
  int apos[SPT1 ? 1 : 7];
  if (!SPT1) {
#pragma unroll
    for (int r = 0; r < 7; ++r)
      apos[r] = (rh + 2 * r < TW_RT && arow0 + 32 * r < tile_rows) ? (arow0 + 32 * r) % L : -(1 << 20);
  }
  const int abase = ((16 * rh + j) * TW_AP + 8 * g) * 4;             // byte offset of (row 16 rh + j, col 8 g)
  const int a_lo = abase - (16 * rh + j + 1) * TW_AP * 4;            // row -1
  const int a_hi = abase + (TW_ROWS - 16 * rh - j) * TW_AP * 4;      // row TW_ROWS
  const char* actb = reinterpret_cast<const char*>(act);
  const int nit = 2 + 10 * a.nlayers;
  int it = 0;
  f32x4 acc[7];
  __syncthreads();                                       // xs and the zero rows are visible

#define TW_GROUP3(AF, R0) TW_MM1(AF, R0, 3, TW_OWNED((R0) + r_))
#define TW_GROUP2(AF, R0) TW_MM1(AF, R0, 2, TW_OWNED((R0) + r_))

  for (int layer = -1; layer < a.nlayers; ++layer) {     // layer -1 = the stem (15 taps x 4 channels as K = 64)
    const float bl = a.bias[(layer + 1) * TW_C + 16 * cs + j];
#pragma unroll
    for (int r = 0; r < 7; ++r) acc[r] = f32x4{bl, bl, bl, bl};
    const int niter = layer < 0 ? 2 : 10;
    for (int ci = 0; ci < niter; ++ci, ++it) {
      TW_UNPACK_ONE(bf, bn0, bn1)
      TW_WNEXT_ONE(bn0, bn1)
      if (layer < 0) {
        const int t0 = 8 * ci + 2 * g;
        float4 af[4][2];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int r0 = half ? 4 : 0, r1 = half ? 7 : 4;
#pragma unroll
          for (int r = r0; r < r1; ++r) {
            if (r == 6 && rh == 1) continue;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
              const int rr = arow0 + 32 * r + t0 + q - 7;
              int idx;
              if (SPT1) idx = min(max(rr, -1), TW_ROWS);
              else idx = (unsigned)(apos[SPT1 ? 0 : r] + t0 + q - 7) < (unsigned)L ? rr : TW_ROWS;
              TW_XLOAD(af[r - r0], q, idx)
            }
          }
          if (half == 0) { TW_MM1(af, 0, 4, TW_OWNED(r_)) } else { TW_MM1(af, 4, 3, TW_OWNED(4 + r_)) }
        }
      } else {
        TW_TAP(ci)
        float4 fa[3][2], fb[2][2];
#define TW_LD(R, V)                                                                                           \
        if (TW_OWNED(R)) {                                                                                    \
          if (SPT1) { TW_ALOAD_CLAMPED(V, abase + dbytes + (R) * (32 * TW_AP * 4)) }                          \
          else { TW_ALOAD_APOS(V, apos[SPT1 ? 0 : (R)], abase + dbytes + (R) * (32 * TW_AP * 4)) }            \
        }
        TW_SCHED322(TW_LD, TW_GROUP3, TW_GROUP2)
#undef TW_LD
      }
    }
    TW_EPILOGUE1(TW_OWNED(r), tile_rows)
  }
#undef TW_GROUP2
#undef TW_GROUP3
  TW_STORE_SEQ
}

// ---------------------------------------------- conv tower on candidate WINDOWS (SVDD-MC: M candidates per parent) ----
// The M candidates of a sample differ from their parent x_t only where a MASK was replaced this step (~L/steps
// positions), and the tower's receptive field is +-17 rows (stem 15 taps + 5 x 5 taps). So tower(candidate) equals
// tower(parent) outside +-17 rows of the changed positions, bit for bit (every output element accumulates the same
// products in the same order). This kernel computes, per candidate, only a contiguous row window [w0, w1) (multiples
// of 16) that covers the changed positions +-27 rows: +-17 for the receptive field, +10 because rows next to a window
// edge see zeros instead of their real neighbours and are wrong by up to 2 rows per conv layer (the stem reads the real
// one-hot rows beyond the window). Rows [w0 + TW_EDGE, w1 - TW_EDGE) come from this computation (a window edge that is a
// sequence end is exact), all other rows are copied from the parent's tower output (computed once per parent by
// conv_tower_kernel). At L = 200, 128 steps, M = 10: 42 % of the row tiles, 21 % of the candidates need none at all.
struct TowerWinArgs {
  TowerArgs t;             // x = candidates' one-hot [n, L, 4], out [n, L, 64]
  const int* win;          // [n][2]  (w0, w1) ; w0 == w1: the candidate equals its parent
  const float* parent_out; // [n / M, L, 64]
  int M;
  const int* live_idx;     // [count] candidate ids to process (NULL: identity); workgroup i writes out[i]
  const int* count;        // device scalar (NULL: n)
};

__global__ __launch_bounds__(512, 4) void conv_tower_win_kernel(TowerWinArgs wa) {
  const TowerArgs& a = wa.t;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* act = smem + TW_AP;                            // rows -1 .. TW_ROWS ; [-1] and [TW_ROWS] stay zero
  float* xs = smem + (TW_ROWS + 2) * TW_AP + 8 * 4;     // one-hot rows -8 .. TW_ROWS + 8 (real data beyond the window)

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cs = w & 3, rh = w >> 2;
  const int j = lane & 15, g = lane >> 4;
  const int L = a.L;
  TW_WIN_DECODE(wa, true, TW_CAND_SELECT)               // cand, w0, w1, nt = live row tiles
  const int lrows = min(L, w1) - w0;                    // valid local rows
  TW_WIN_KEEP(true, L)                                  // keep_lo, keep_hi
  float* outc = a.out + (size_t)blockIdx.x * L * TW_C;
  const float* par = wa.parent_out + (size_t)(cand / wa.M) * L * TW_C;

  TW_COPY_PARENT_WIN(par)
  if (nt == 0) return;

  const float* xc = a.x + (size_t)cand * L * 4;
  TW_STAGE_WIN(xc, w0)
  for (int e = tid; e < (TW_ROWS + 2) * TW_AP; e += 512) smem[e] = 0.0f;     // rows beyond the window must read as zero
  const float* wsrc = a.tiles + (16 * cs + j) * CH + 8 * g;
  float4 bn0, bn1;
  TW_WLOAD_ONE(bn0, bn1, wsrc)

  const int arow0 = 16 * rh + j;
  const int abase = ((16 * rh + j) * TW_AP + 8 * g) * 4;
  const int a_lo = abase - (16 * rh + j + 1) * TW_AP * 4;
  const int a_hi = abase + (TW_ROWS - 16 * rh - j) * TW_AP * 4;
  const char* actb = reinterpret_cast<const char*>(act);
  const int nlive = (nt - rh + 1) >> 1;                 // owned live tiles rh + 2 r, r < nlive (a prefix)
  const int nit = 2 + 10 * a.nlayers;
  int it = 0;
  f32x4 acc[7];
  __syncthreads();

  // the live tiles of a group are a prefix of it: straight-line MFMAs for each count, no per-tile predicate
#define TWW_GROUP3(AF, R0) { const int c_ = nlive - (R0); if (c_ >= 3) { TW_MM1(AF, R0, 3, true) } else if (c_ == 2) { TW_MM1(AF, R0, 2, true) } else if (c_ == 1) { TW_MM1(AF, R0, 1, true) } }
#define TWW_GROUP2(AF, R0) { const int c_ = nlive - (R0); if (c_ >= 2) { TW_MM1(AF, R0, 2, true) } else if (c_ == 1) { TW_MM1(AF, R0, 1, true) } }

  for (int layer = -1; layer < a.nlayers; ++layer) {
    const float bl = a.bias[(layer + 1) * TW_C + 16 * cs + j];
#pragma unroll
    for (int r = 0; r < 7; ++r) acc[r] = f32x4{bl, bl, bl, bl};
    const int niter = layer < 0 ? 2 : 10;
    for (int ci = 0; ci < niter; ++ci, ++it) {
      TW_UNPACK_ONE(bf, bn0, bn1)
      TW_WNEXT_ONE(bn0, bn1)
      float4 fa[3][2], fb[2][2];
      if (layer < 0) {                                   // xs holds real rows beyond the window and zero rows outside the sequence
        const int t0 = 8 * ci + 2 * g;
#define TWW_XLD(R, V) if ((R) < 6 || rh == 0) { TW_XLOAD(V, 0, arow0 + 32 * (R) + t0 - 7) TW_XLOAD(V, 1, arow0 + 32 * (R) + t0 - 7 + 1) }
        TW_SCHED322(TWW_XLD, TWW_GROUP3, TWW_GROUP2)
#undef TWW_XLD
      } else {
        TW_TAP(ci)
#define TWW_ALD(R, V) if ((R) < 6 || rh == 0) TW_ALOAD_CLAMPED(V, abase + dbytes + (R) * (32 * TW_AP * 4))
        TW_SCHED322(TWW_ALD, TWW_GROUP3, TWW_GROUP2)
#undef TWW_ALD
      }
    }
    TW_EPILOGUE1(r < nlive, lrows)
  }
#undef TWW_GROUP2
#undef TWW_GROUP3
  TW_STORE_WIN
}

// ----------------------------------------------------- conv tower, second generation (whole sequences AND windows) ----
// Same function, same bits as conv_tower_kernel / conv_tower_win_kernel (every output element accumulates the same
// products in the same order), restructured after what the 16-bit twin taught (svdd_lp_tower.hip):
//   * wave w owns 32 output channels (column tiles 2 cp, 2 cp + 1, cp = w & 1) of the row tiles rq + 4 r (rq = w >> 1), so
//     an A fragment (two ds_read_b128) feeds 16 MFMAs instead of 8: half the LDS read traffic;
//   * the number of live row tiles of a wave (4 / 3 for whole sequences, 0..4 for a window) is a TEMPLATE parameter of the
//     layer loop, chosen once per wave: straight-line code, no per-tile predicates;
//   * <= 128 VGPRs: two workgroups per CU.
struct TowerCtx2 {
  float* act;            // LDS image, row 0 ; rows -1 and TW_ROWS are zero
  const float* xs;       // LDS one-hot rows [row][4]
  const float* wsrc;     // this lane's slice of tile 0
  const float* bias;
  int L, tile_rows, nlayers, residual_mask;
  int rq, cp, j, g;
  int apos[7];
};

// CT = column tiles (16 output channels each) per wave: the 8 waves are 4 / CT channel groups x 2 CT row groups, wave
// (rq, cp) computes row tiles rq + 2 CT r, r < NL.
template <bool CLAMP, int NL, int CT>
__device__ __forceinline__ void tower2_layers(const TowerCtx2& c) {
  constexpr int RS = 2 * CT;                                     // row-tile stride of a wave
  constexpr int NA = NL > 0 ? NL : 1;
  const int j = c.j, g = c.g, L = c.L;
  const int arow0 = 16 * c.rq + j;
  const int abase = (arow0 * TW_AP + 8 * g) * 4;                 // byte offset of (row arow0, channel 8 g)
  const int a_lo = abase - (arow0 + 1) * TW_AP * 4;              // row -1
  const int a_hi = abase + (TW_ROWS - arow0) * TW_AP * 4;        // row TW_ROWS
  const char* actb = reinterpret_cast<const char*>(c.act);
  const int cb = 16 * CT * c.cp + 4 * g;                         // this lane's OUTPUT channels: cb + 16 ct + e (transposed tiles)
  const int nit = 2 + 10 * c.nlayers;
  const float* wsrc = c.wsrc;
  const float* xs = c.xs;
  float4 bn[2 * CT];                                             // [ct][half]: W[ch0 + 16 ct][8 g .. 8 g + 8] of the next tile
  TW_WLOAD(bn, wsrc, CT)
  int it = 0;
  f32x4 acc[NA][CT];

  for (int layer = -1; layer < c.nlayers; ++layer) {
    // TRANSPOSED accumulators (as in the 16-bit twin): lane (j, g) register e of column tile ct holds channel cb + 16 ct + e of
    // ONE position (row 16 (rq + RS r) + j): the epilogue is one 16-byte LDS load and store per (row tile, column tile)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const f32x4 bl = *reinterpret_cast<const f32x4*>(c.bias + (layer + 1) * TW_C + cb + 16 * ct);
#pragma unroll
      for (int r = 0; r < NL; ++r) acc[r][ct] = bl;
    }
    const int niter = layer < 0 ? 2 : 10;
    for (int ci = 0; ci < niter; ++ci, ++it) {
      TW_UNPACK(b, bn, CT)
      TW_WNEXT(bn, CT)
      float4 af[NA][2];
      if (layer < 0) {
        const int t0 = 8 * ci + 2 * g;
#pragma unroll
        for (int r = 0; r < NL; ++r)
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const int rr = arow0 + 16 * RS * r + t0 + q - 7;
            int idx;
            if (CLAMP) idx = rr;                                 // xs holds zero rows outside the sequence / window
            else idx = (unsigned)(c.apos[r] + t0 + q - 7) < (unsigned)L ? rr : TW_ROWS + 7;
            TW_XLOAD(af[r], q, idx)
          }
      } else {
        TW_TAP(ci)
#pragma unroll
        for (int r = 0; r < NL; ++r) {
          if (CLAMP) { TW_ALOAD_CLAMPED(af[r], abase + dbytes + r * (16 * RS * TW_AP * 4)) }
          else { TW_ALOAD_APOS(af[r], c.apos[r], abase + dbytes + r * (16 * RS * TW_AP * 4)) }
        }
      }
      TW_MM2(NL, CT)
    }
    if (layer >= 0) __syncthreads();                     // every wave is done reading the image (the stem reads xs)
    const bool res = layer >= 0 && ((c.residual_mask >> layer) & 1);
#pragma unroll
    for (int r = 0; r < NL; ++r) {
      const int row = 16 * (c.rq + RS * r) + j;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        f32x4* dst = reinterpret_cast<f32x4*>(c.act + row * TW_AP + cb + 16 * ct);
        const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
        const f32x4 v = acc[r][ct] + (res ? *dst : z);
        *dst = row < c.tile_rows ? __builtin_elementwise_max(v, z) : z;
      }
    }
    __syncthreads();                                     // the image is complete
  }
}

template <bool CLAMP, bool WIN, int CT>
__device__ __forceinline__ void tower2_dispatch(const TowerCtx2& c, int nlive) {
  if constexpr (CT == 2) {
    switch (nlive) {                                    // wave-uniform; every path runs the same barriers
      case 4: tower2_layers<CLAMP, 4, 2>(c); break;
      case 3: tower2_layers<CLAMP, 3, 2>(c); break;
      case 2: if constexpr (WIN) tower2_layers<CLAMP, 2, 2>(c); break;
      case 1: if constexpr (WIN) tower2_layers<CLAMP, 1, 2>(c); break;
      default: if constexpr (WIN) tower2_layers<CLAMP, 0, 2>(c); break;
    }
  } else {
    switch (nlive) {
      case 7: tower2_layers<CLAMP, 7, 1>(c); break;
      case 6: tower2_layers<CLAMP, 6, 1>(c); break;
      case 5: if constexpr (WIN) tower2_layers<CLAMP, 5, 1>(c); break;
      case 4: if constexpr (WIN) tower2_layers<CLAMP, 4, 1>(c); break;
      case 3: if constexpr (WIN) tower2_layers<CLAMP, 3, 1>(c); break;
      case 2: if constexpr (WIN) tower2_layers<CLAMP, 2, 1>(c); break;
      case 1: if constexpr (WIN) tower2_layers<CLAMP, 1, 1>(c); break;
      default: if constexpr (WIN) tower2_layers<CLAMP, 0, 1>(c); break;
    }
  }
}

template <bool SPT1, bool WIN, int CT>
__global__ __launch_bounds__(512, 4) void conv_tower2_kernel(TowerWinArgs wa) {
  const TowerArgs& a = wa.t;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* act = smem + TW_AP;                            // rows -1 .. TW_ROWS ; [-1] and [TW_ROWS] stay zero
  float* xs = smem + (TW_ROWS + 2) * TW_AP + 8 * 4;     // one-hot rows -8 .. TW_ROWS + 8

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = a.L;
  TW_WIN_DECODE(wa, WIN, TW_CAND_BRANCH)                // cand, w0, w1, nt
  const int tile_rows = WIN ? min(L, w1) - w0 : a.spt * L;
  const int64_t row0 = WIN ? 0 : (int64_t)blockIdx.x * tile_rows;
  const int64_t total_rows = (int64_t)((!WIN && a.count) ? __builtin_amdgcn_readfirstlane(*a.count) : a.n) * L;
  if (!WIN && row0 >= total_rows) return;
  TW_WIN_KEEP(WIN, L)                                   // keep_lo, keep_hi
  float* outc = a.out + (WIN ? (size_t)blockIdx.x * L * TW_C : 0);

  if (WIN) {
    const float* par = wa.parent_out + (size_t)(cand / wa.M) * L * TW_C;
    TW_COPY_PARENT_WIN(par)
    if (nt == 0) return;
  }
  {
    const float* xc = a.x + (WIN ? (size_t)cand * L * 4 : 0);
    if (WIN) { TW_STAGE_WIN(xc, w0) } else { TW_STAGE_SEQ(xc, 8) }
  }
  for (int e = tid; e < (TW_ROWS + 2) * TW_AP; e += 512) smem[e] = 0.0f;      // image incl. the zero rows

  TowerCtx2 c;
  c.act = act; c.xs = xs; c.bias = a.bias;
  c.L = L; c.tile_rows = tile_rows; c.nlayers = a.nlayers; c.residual_mask = a.residual_mask;
  constexpr int CG = 4 / CT, RS = 2 * CT;               // channel groups ; row-tile stride
  c.cp = w % CG; c.rq = w / CG; c.j = lane & 15; c.g = lane >> 4;
  c.wsrc = a.tiles + (16 * CT * c.cp + c.j) * CH + 8 * c.g;
#pragma unroll
  for (int r = 0; r < 7; ++r) {
    const int row = 16 * (c.rq + RS * r) + c.j;
    c.apos[r] = (!SPT1 && !WIN && row < tile_rows) ? row % L : -(1 << 20);
  }
  const int nlive = ((WIN ? nt : TW_ROWS / 16) - c.rq + RS - 1) / RS;
  __syncthreads();
  tower2_dispatch<SPT1 || WIN, WIN, CT>(c, nlive);
  if (WIN) { TW_STORE_WIN } else { TW_STORE_SEQ }
}

// (w0, w1) of every candidate: one wave per candidate compares it with its parent. TIGHT (svdd_candidate_windows_tight): the window
// starts AT the first row it needs, w0 = max(0, lo - margin), and only its length is a multiple of 16 — the window kernels address
// the one-hot rows, the LDS image, the keep range and the row stores relative to w0 and need nothing of w0 itself; w1 may then pass
// L rounded up to 16 (never by a whole tile: (w1 - w0) / 16 <= ceil(L / 16)).
template <bool TIGHT>
__global__ __launch_bounds__(256) void candidate_windows_kernel(const uint8_t* __restrict__ cand, const uint8_t* __restrict__ x,
                                                               int n, int L, int M, int margin, int* __restrict__ win,
                                                               int* __restrict__ flags) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= n) return;
  const int lane = threadIdx.x & 63;
  const uint8_t* cp = cand + (size_t)c * L;
  const uint8_t* xp = x + (size_t)(c / M) * L;
  int lo = 1 << 30, hi = -1;
  for (int l = lane; l < L; l += 64)
    if (cp[l] != xp[l]) { lo = min(lo, l); hi = max(hi, l); }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { lo = min(lo, __shfl_xor(lo, off, 64)); hi = max(hi, __shfl_xor(hi, off, 64)); }
  if (lane == 0) {
    int w0 = 0, w1 = 0;
    if (hi >= 0 && TIGHT) {
      w0 = max(0, lo - margin);
      w1 = w0 + ((min(L, hi + margin + 1) - w0 + 15) & ~15);
    } else if (hi >= 0) {
      w0 = max(0, lo - margin) & ~15;
      w1 = min((L + 15) & ~15, (hi + margin + 1 + 15) & ~15);
    }
    win[2 * c] = w0; win[2 * c + 1] = w1;
    if (flags) flags[c] = (w1 - w0) >> 4;              // row tiles of the window (>= 1) ; 0: the candidate is a copy of its parent
  }
}

// ------------------------------------------------ conv tower on candidate PARTS (per-layer row ranges, far changes apart) ----
// The tight window computes all six layers on one range [lo - 27, hi + 28). Two things in it nobody reads:
//   * only the stem needs +-27. Read from the output side, block 5 must be right on [lo - 17, hi + 18) (the rows that can differ
//     from the parent's), block 4 on two rows more per side, ... : layer k (0 = stem, 5 = last block) on +- (R + 2 (5 - k)), R = 17;
//   * changed positions far apart need no rows between them: the changed positions, ascending, are cut into PARTS wherever two
//     consecutive ones are >= G apart (at most TP_PARTS; further ones are merged into the last).
// Per part [a, b] and layer k the needed range is [max(0, a - R - 2 (5 - k)), min(L, b + R + 1 + 2 (5 - k))); the layer computes the
// 16-row tiles that cover it, counted from the range's own first row. Rows of a computed tile past the needed range hold GARBAGE
// (their inputs were outside the previous layer's needed range): the next layer's needed range is two rows shorter at each end
// and never reads them, and a row's result depends on no other row of its tile (one MFMA column). G >= 2 (R + 10) + 16 keeps two
// parts' computed tiles disjoint on every layer. A kept row is the same chain of MFMAs on the same inputs as in the whole-sequence
// kernel, whichever tile and lane it sits in: same bits (tests/test_tower_parts_gpu.py).
constexpr int TP_PARTS = 3;        // parts per candidate
// TP_BLOCKS = 5 conv blocks after the stem, the tower the part rule is written for: svdd_device.h
constexpr int TP_REACH = 17;       // receptive field of that tower, rows per side: the reach svdd_conv_tower_parts_f32 takes
constexpr int TP_LT = 16;          // stride of a layer's tile-origin list in LDS: <= TW_RT origins, [TP_LT - 1] = their number

// tile-layers of one part: sum over the six layers of the 16-row tiles covering the layer's needed range
__device__ __forceinline__ int tower_part_tile_layers(int a, int b, int L, int R) {
  int t = 0;
#pragma unroll
  for (int k = 0; k <= TP_BLOCKS; ++k) {
    const int h = R + 2 * (TP_BLOCKS - k);
    t += (min(L, b + h + 1) - max(0, a - h) + 15) >> 4;
  }
  return t;
}

// parts [n][3][2] = (first, last) changed position of each part, (-1, -1) where there is none; nparts [n]; flags [n] = tile-layers
// of the candidate (0: a copy of its parent); key [n] = ceil(flags / 6), 1 .. TW_RT: the average tiles per layer, a sort key within
// svdd_compact_by_key's 15 bins. One wave per candidate; the cut runs on wave-uniform values (a ballot per 64 positions).
__global__ __launch_bounds__(256) void candidate_parts_kernel(const uint8_t* __restrict__ cand, const uint8_t* __restrict__ x, int n, int L,
                                                             int M, int R, int G, int* __restrict__ parts, int* __restrict__ nparts,
                                                             int* __restrict__ flags, int* __restrict__ key) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= n) return;
  const int lane = threadIdx.x & 63;
  const uint8_t* cp = cand + (size_t)c * L;
  const uint8_t* xp = x + (size_t)(c / M) * L;
  int np = 0, prev = 0;
  int a0 = -1, a1 = -1, a2 = -1, b0 = -1, b1 = -1, b2 = -1;
  for (int l0 = 0; l0 < L; l0 += 64) {
    const int l = l0 + lane;
    unsigned long long m = __ballot(l < L && cp[l] != xp[l]);
    while (m) {
      const int p = l0 + __builtin_ctzll(m);
      m &= m - 1;
      if (np == 0 || (np < TP_PARTS && p - prev >= G)) {
        if (np == 0) a0 = p; else if (np == 1) a1 = p; else a2 = p;
        ++np;
      }
      if (np == 1) b0 = p; else if (np == 2) b1 = p; else b2 = p;
      prev = p;
    }
  }
  if (lane == 0) {
    int* pp = parts + (size_t)c * (2 * TP_PARTS);
    pp[0] = a0; pp[1] = b0; pp[2] = a1; pp[3] = b1; pp[4] = a2; pp[5] = b2;
    int t = 0;
    if (np > 0) t += tower_part_tile_layers(a0, b0, L, R);
    if (np > 1) t += tower_part_tile_layers(a1, b1, L, R);
    if (np > 2) t += tower_part_tile_layers(a2, b2, L, R);
    if (nparts) nparts[c] = np;
    if (flags) flags[c] = t;
    if (key) key[c] = (t + TP_BLOCKS) / (TP_BLOCKS + 1);
  }
}

struct TowerPartArgs {
  TowerArgs t;             // x = candidates' one-hot [n, L, 4], out [n, L, 64]
  const int* parts;        // [n][TP_PARTS][2] (first, last) changed position ; first < 0: no such part
  const float* parent_out; // [n / M, L, 64]
  int M, reach;
  const int* live_idx;     // [count] candidate ids to process (NULL: identity); workgroup i writes out[i]
  const int* count;        // device scalar (NULL: n)
};

// One layer (layer = -1: the stem) on this wave's NL tiles: the origins tl[rq], tl[rq + 2], ... of the layer's list. The image is
// addressed by SEQUENCE row (row r at act + r TW_AP). The layer is tower2_layers<true, NL, 1>'s, out of the same pieces (TW_UNPACK1 /
// TW_WLOAD1, TW_TAP, TW_ALOAD_CLAMPED, TW_XLOAD, TW_MM2), but its own text: as one body with tower2_layers this kernel's instructions change.
template <int NL>
__device__ __forceinline__ void tower_parts_layer(const TowerCtx2& c, int layer, const int* tl, float4 (&bn)[2], int& it) {
  constexpr int NA = NL > 0 ? NL : 1;
  const int niter = layer < 0 ? 2 : 10;
  const int nit = 2 + 10 * c.nlayers;
  const float* wsrc = c.wsrc;
  const float* xs = c.xs;
  if constexpr (NL == 0) {                                       // no tile on this layer: keep the weight stream and the barriers in step
    it += niter;
    if (it < nit) TW_WLOAD_ONE(bn[0], bn[1], wsrc + (size_t)it * TW_C * CH)
    if (layer >= 0) __syncthreads();
    __syncthreads();
    return;
  }
  const int j = c.j, g = c.g;
  int org[NA];                                                   // first sequence row of each tile (wave-uniform)
#pragma unroll
  for (int r = 0; r < NL; ++r) org[r] = __builtin_amdgcn_readfirstlane(tl[c.rq + 2 * r]);
  const int lbase = (j * TW_AP + 8 * g) * 4;                     // byte offset of (row j, channel 8 g)
  const int a_lo = (8 * g - TW_AP) * 4;                          // row -1
  const int a_hi = (TW_ROWS * TW_AP + 8 * g) * 4;                // row TW_ROWS
  const char* actb = reinterpret_cast<const char*>(c.act);
  const int cb = 16 * c.cp + 4 * g;                              // this lane's OUTPUT channels cb + e (transposed tiles)
  f32x4 acc[NA][1];
  {
    const f32x4 bl = *reinterpret_cast<const f32x4*>(c.bias + (layer + 1) * TW_C + cb);
#pragma unroll
    for (int r = 0; r < NL; ++r) acc[r][0] = bl;
  }
  for (int ci = 0; ci < niter; ++ci, ++it) {
    TW_UNPACK_ONE(b, bn[0], bn[1])
    TW_WNEXT_ONE(bn[0], bn[1])
    float4 af[NA][2];
    int og[NA];                                                  // the origins, opaque per iteration: the lane's addresses are summed
#pragma unroll                                                   // here, one at a time — hoisted out of the loop they would hold 7 VGPRs
    for (int r = 0; r < NL; ++r) { og[r] = org[r]; asm volatile("" : "+s"(og[r])); }
    if (layer < 0) {
      const int t0 = 8 * ci + 2 * g;                             // k = 32 ci + 8 g + s: taps t0, t0 + 1 (4 channels each)
#pragma unroll
      for (int r = 0; r < NL; ++r)
#pragma unroll
        for (int q = 0; q < 2; ++q)                              // xs holds zero rows outside the sequence, up to row TW_ROWS + 7
          { TW_XLOAD(af[r], q, min(og[r] + j + t0 + q - 7, TW_ROWS + 7)) }
    } else {
      TW_TAP(ci)
#pragma unroll
      for (int r = 0; r < NL; ++r) {                             // rows before 0 read the zero row -1, rows past TW_ROWS the zero row TW_ROWS
        TW_ALOAD_CLAMPED(af[r], lbase + dbytes + og[r] * (TW_AP * 4))
      }
    }
    TW_MM2(NL, 1)
  }
  if (layer >= 0) __syncthreads();                               // every wave is done reading the image (the stem reads xs)
  const bool res = layer >= 0 && ((c.residual_mask >> layer) & 1);
#pragma unroll
  for (int r = 0; r < NL; ++r) {
    const int row = org[r] + j;
    if (row < c.L) {                                             // rows from L on are never written: they stay the zeros the taps past the end read
      f32x4* dst = reinterpret_cast<f32x4*>(c.act + row * TW_AP + cb);
      const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
      const f32x4 v = acc[r][0] + (res ? *dst : z);
      *dst = __builtin_elementwise_max(v, z);
    }
  }
  __syncthreads();                                               // the image is complete
}

// The body is a device function so that gru_tower_parts_kernel can run it in the workgroups behind its GRU units: blk = the
// workgroup's place in this launch's list, smem its dynamic LDS (tower2_lds_bytes).
__device__ __forceinline__ void tower_parts_body(const TowerPartArgs& pa, unsigned blk, float* smem) {
  const TowerArgs& a = pa.t;
  __shared__ int tl[TP_BLOCKS + 1][TP_LT];              // per layer: the tile origins of all parts, then their number
  float* act = smem + TW_AP;                            // rows -1 .. TW_ROWS, by SEQUENCE row ; [-1] and [TW_ROWS] are zero where read
  float* xs = smem + (TW_ROWS + 2) * TW_AP + 8 * 4;     // one-hot rows -8 .. TW_ROWS + 8

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = a.L, R = pa.reach, nl = a.nlayers;
  if (pa.count && (int)blk >= __builtin_amdgcn_readfirstlane(*pa.count)) return;
  int cand = blk;
  if (pa.live_idx) cand = __builtin_amdgcn_readfirstlane(pa.live_idx[blk]);
  int np = 0, p0[TP_PARTS], p1[TP_PARTS];               // the parts, clamped into the sequence (whatever the array holds)
#pragma unroll
  for (int p = 0; p < TP_PARTS; ++p) {
    const int f = __builtin_amdgcn_readfirstlane(pa.parts[(size_t)cand * (2 * TP_PARTS) + 2 * p]);
    const int l = __builtin_amdgcn_readfirstlane(pa.parts[(size_t)cand * (2 * TP_PARTS) + 2 * p + 1]);
    p0[p] = min(max(f, 0), L - 1); p1[p] = min(max(l, p0[p]), L - 1);
    if (f >= 0 && np == p) np = p + 1;                  // parts are listed without holes
  }
  float* outc = a.out + (size_t)blk * L * TW_C;
  {
    const float* par = pa.parent_out + (size_t)(cand / pa.M) * L * TW_C;
    for (int e = tid; e < L * 16; e += 512) {           // rows that are the parent's, straight from its output
      const int row = e >> 4;
      bool kept = false;
#pragma unroll
      for (int p = 0; p < TP_PARTS; ++p) kept |= p < np && row >= p0[p] - R && row <= p1[p] + R;
      if (!kept)
        *reinterpret_cast<float4*>(outc + (size_t)row * TW_C + 4 * (e & 15)) = *reinterpret_cast<const float4*>(par + (size_t)row * TW_C + 4 * (e & 15));
    }
    if (np == 0) return;
  }
  {
    const float* xc = a.x + (size_t)cand * L * 4;
    TW_STAGE_WIN(xc, 0)                                 // the image is the whole sequence
  }
  // Zero only the image rows that are read: a block reads two rows around its tiles, so per part everything any layer reads lies
  // in [s - 2, e + 18), s / e = the stem's needed range (the tiles of a layer pass its needed end by at most 15 rows) — the rows
  // before 0 and from L on among them are the zero rows of the sequence ends and are never written.
  const int h0 = R + 2 * nl;
#pragma unroll
  for (int p = 0; p < TP_PARTS; ++p) {
    if (p >= np) break;
    const int z0 = max(-1, max(0, p0[p] - h0) - 2), z1 = min(TW_ROWS + 1, min(L, p1[p] + h0 + 1) + 18);
    const float4 z = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int e = tid; e < (z1 - z0) * (TW_AP / 4); e += 512) *reinterpret_cast<float4*>(act + z0 * TW_AP + 4 * e) = z;
  }
  if (tid <= nl) {                                      // layer tid's tile origins: every part's needed range in steps of 16 from its first row
    const int h = R + 2 * (nl - tid);
    int cnt = 0;
#pragma unroll
    for (int p = 0; p < TP_PARTS; ++p) {
      if (p >= np) break;
      const int e = min(L, p1[p] + h + 1);
      for (int o = max(0, p0[p] - h); o < e && cnt < TW_RT; o += 16) tl[tid][cnt++] = o;   // (disjoint ranges in <= 208 rows: <= TW_RT tiles)
    }
    tl[tid][TP_LT - 1] = cnt;
  }

  TowerCtx2 c;
  c.act = act; c.xs = xs; c.bias = a.bias;
  c.L = L; c.tile_rows = L; c.nlayers = nl; c.residual_mask = a.residual_mask;
  c.cp = w & 3; c.rq = w >> 2; c.j = lane & 15; c.g = lane >> 4;
  c.wsrc = a.tiles + (16 * c.cp + c.j) * CH + 8 * c.g;
  __syncthreads();
  float4 bn[2];
  TW_WLOAD_ONE(bn[0], bn[1], c.wsrc)
  int it = 0;
  for (int layer = -1; layer < nl; ++layer) {
    const int* tlk = tl[layer + 1];
    const int nlive = (__builtin_amdgcn_readfirstlane(tlk[TP_LT - 1]) - c.rq + 1) >> 1;
    switch (nlive) {                                    // wave-uniform; every path runs the same barriers
      case 7: tower_parts_layer<7>(c, layer, tlk, bn, it); break;
      case 6: tower_parts_layer<6>(c, layer, tlk, bn, it); break;
      case 5: tower_parts_layer<5>(c, layer, tlk, bn, it); break;
      case 4: tower_parts_layer<4>(c, layer, tlk, bn, it); break;
      case 3: tower_parts_layer<3>(c, layer, tlk, bn, it); break;
      case 2: tower_parts_layer<2>(c, layer, tlk, bn, it); break;
      case 1: tower_parts_layer<1>(c, layer, tlk, bn, it); break;
      default: tower_parts_layer<0>(c, layer, tlk, bn, it); break;
    }
  }
#pragma unroll
  for (int p = 0; p < TP_PARTS; ++p) {                  // the kept rows of each part: the last block's needed range
    if (p >= np) break;
    const int k0 = max(0, p0[p] - R), k1 = min(L, p1[p] + R + 1);
    for (int e = tid; e < (k1 - k0) * 16; e += 512) {
      const int row = k0 + (e >> 4), q = e & 15;
      *reinterpret_cast<float4*>(outc + (size_t)row * TW_C + 4 * q) = *reinterpret_cast<const float4*>(act + row * TW_AP + 4 * q);
    }
  }
}

__global__ __launch_bounds__(512, 4) void conv_tower_parts_kernel(TowerPartArgs pa) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  tower_parts_body(pa, blockIdx.x, smem);
}

// The middle launch of a two-part late step (svdd_value_late_step_f32): workgroups 0 .. gru_units - 1 run gru_pc_kernel's body on the
// second part's rows, the workgroups behind them conv_tower_parts_kernel's body on the first part's list. The GRU units come first:
// the dispatcher hands workgroups out in index order and their 200-step chains are the longest thing in the launch. Their LDS
// (33 KB) lies in the launch's dynamic LDS, which is the tower's (57 KB): as static LDS it would cost the tower its second workgroup
// per CU. Same bodies, same rows: same bits.
struct GruPartArgs {
  const float *x, *wpack, *bpack;
  float* out;
  int n_alloc, L;
  const int* count;
};
static_assert(GRU_PC_LDS_FLOATS <= (TW_ROWS + 2) * TW_AP, "the GRU unit's LDS must fit into the tower's image");

__global__ __launch_bounds__(512, 4) void gru_tower_parts_kernel(GruPartArgs ga, TowerPartArgs pa, unsigned gru_units) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if (blockIdx.x < gru_units) {
    gru_pc_body(ga.x, ga.wpack, ga.bpack, ga.out, ga.n_alloc, ga.L, ga.count, reinterpret_cast<float (*)[TS][HPAD]>(smem),
                reinterpret_cast<float (*)[4][3][64 * 4]>(smem + 2 * TS * HPAD));
    return;
  }
  tower_parts_body(pa, blockIdx.x - gru_units, smem);
}

// --------------------------------------------------------- fused dilated-CNN backbone (one launch per forward) ----
// The whole masked-diffusion backbone of the reference (models/dnaconv.py:176-210, sigma = 0):
//     f_0 = relu(conv9(onehot5(x)) + b)                      first layer as a 9-entry table lookup per output
//     hn_i = LayerNorm(f_i + tb_i) ; f_{i+1} = relu(conv9_dil_i(hn_i) + b_i) + f_i          i = 0..nl-1
//     logits = W2 relu(W1 f_nl + b1) + b2
// One workgroup per tile of whole sequences (<= 208 rows), 8 waves; every wave keeps its part of the residual stream f
// in registers, in the MFMA C/D layout, for the whole forward (work split: see the kernel). The only LDS-resident
// activation is the LayerNorm'd image hn [rows][128] that feeds the MFMA A operands (a tap = a row offset;
// out-of-sequence rows read a zero row). No activation ever goes to HBM: per forward the layer-wise path moved ~3 GB
// (conv in/out + the epilogue/LayerNorm pass per layer) and launched 41 kernels.
// v_mfma_f32_16x16x4_f32, 16-row tiles (200 rows -> 13 tiles, 4 % padding); row tiles whose rows all fall into the
// zero padding of a dilated tap are skipped (runtime, workgroup-uniform, from a schedule built once in LDS).
// Weights are NOT staged through LDS: each wave reads its [32 cout][32 k] slice of the (layer, chunk, tap) tile
// straight from L2 into the B-operand registers, one tile ahead, so there is no barrier inside a layer.
// LayerNorm statistics are two-pass (mean, then centred variance) with a 16-lane DPP reduction and a 4-way LDS
// exchange. Measurements and the PMC-guided history of this kernel: DESIGN.md section 4.
// BB_C = 128 channels, BB_AP = BB_C + 4 the LDS row stride, BB_MAXL = 32 layers: svdd_host.h

struct BackboneArgs {
  const uint8_t* x;        // [n, L] tokens 0..4
  const float* table0;     // [9][5][128]  W_first[co][c][t] -> [t][c][co]
  const float* tiles;      // [nl][4 chunks][9 taps][128][32] then final-1x1 [4][128][32]
  const float* vec;        // [nl + 2][4][128] : row 0: {b_first,-,-,-}; row 1+i: {bias_i, tb_i, gamma_i, beta_i}; last: {b_f1,-,-,-}
  const float* w2;         // [5][128] , then b2 [5]
  float* out;              // [n, L, 5]
  int n, L, spt, nl;
  int dil[BB_MAXL];
  const int* count;        // device scalar: valid rows (NULL: n) — exact work-skipping on a compacted batch
  const int* row_idx;      // [count] (NULL: identity): compact row r reads the tokens of sequence row_idx[r] of x ...
  int out_scatter;         // ... and writes its logits to row row_idx[r] of out (1) or to row r (0)
  int auto_spt, ncu;       // auto_spt: the workgroups pick the sequences per tile from the device-side row count (svdd_spt.h)
  SvddTilePlan plan;       // several sequences per tile, row count known on the host: which tile takes how many (svdd_spt.h)
  float* planes;           // PLN != 0: the carried stem planes [planes_P][n][208][128] (plane k - 1 = f after conv layer k - 1, k = 1 .. planes_P)
  int planes_P;
};

// What the gradient kernel (backbone_grad_kernel, DPS) needs from a forward, all in the forward kernel's LANE-PRIVATE layout — lane
// `tid` of workgroup `wg` owns element q = (r * 2 + ct) * 4 + e, q < 56: row 16 (rh + 2 r) + 4 g + e, column 32 cg + j + 16 ct —
// so every store / load of the pair of kernels is one fully coalesced 256-byte access per wave:
//   xhat [n][nl][56][512]  the LayerNorm'd value before the affine map, (h - mean) rstd, of every layer's input
//   rstd [n][nl][208]      1 / sqrt(var + eps) per row
//   mask [n][nl + 2][512]  bit q of a lane's 64-bit word: ReLU decision of the first layer (word 0), of layer i's conv (1 + i), of
//                          final_conv's first 1x1 (nl + 1)
struct BackboneSave {
  float* xhat;
  float* rstd;
  unsigned long long* mask;
};

// ---------------------------------------------------------------- the conv entry of the fp32 backbone family, defined ONCE ----
// backbone_kernel, backbone_grad_kernel, backbone_split_kernel and the segment kernels (svdd_seg_body.h) must give each other's
// bits, so the pieces of a (chunk, tap) entry are text they share, not text they copy. They are macros on purpose: they name the
// locals of the kernel that uses them (bf0 / bf1, arow0, a_lo, a_hi, sched, wsrc, tile_of, it, en, rh, dil ...), and textual sharing
// keeps every kernel's instruction stream what it was. Each kernel keeps its own entry SCHEDULE (which row tile's fragment is
// requested under which MFMA group): those differ.
//
// BB_MM16: the 16-MFMA group of one row tile, two column tiles x 8 k-steps alternating the accumulators ACC[0] / ACC[1]; U = the
// tile's A fragment (float4[2]), bf0 / bf1 = the unpacked weight tile, LIVE = the tile takes part in this entry. The user puts it
// between two sched_barrier(0) and behind its own s_waitcnt.
#define BB_MM16(ACC, U, LIVE)                                                                                \
      if (LIVE) {                                                                                            \
        _Pragma("unroll") for (int q_ = 0; q_ < 2; ++q_) {                                                   \
          ACC[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[q_].x, bf0[4 * q_], ACC[0], 0, 0, 0);              \
          ACC[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[q_].x, bf1[4 * q_], ACC[1], 0, 0, 0);              \
          ACC[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[q_].y, bf0[4 * q_ + 1], ACC[0], 0, 0, 0);          \
          ACC[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[q_].y, bf1[4 * q_ + 1], ACC[1], 0, 0, 0);          \
          ACC[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[q_].z, bf0[4 * q_ + 2], ACC[0], 0, 0, 0);          \
          ACC[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[q_].z, bf1[4 * q_ + 2], ACC[1], 0, 0, 0);          \
          ACC[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[q_].w, bf0[4 * q_ + 3], ACC[0], 0, 0, 0);          \
          ACC[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[q_].w, bf1[4 * q_ + 3], ACC[1], 0, 0, 0);          \
        }                                                                                                    \
      }
// the current weight tile (float4[4]: W[col0][8 g ..], W[col0 + 16][8 g ..]) as the B operands of the 8 k-steps
#define BB_UNPACK(BC)                                                                                        \
      const float bf0[8] = {BC[0].x, BC[0].y, BC[0].z, BC[0].w, BC[1].x, BC[1].y, BC[1].z, BC[1].w};         \
      const float bf1[8] = {BC[2].x, BC[2].y, BC[2].z, BC[2].w, BC[3].x, BC[3].y, BC[3].z, BC[3].w};
// a weight tile's four float4 of this lane, from SRC = wsrc + the tile's offset, into the register set B (prologue: the first
// tile; inside an entry: the next tile into the idle set)
#define BB_WLOAD(B, SRC)                                                                                     \
      { const float* src_ = (SRC);                                                                           \
        B[0] = *reinterpret_cast<const float4*>(src_);                                                       \
        B[1] = *reinterpret_cast<const float4*>(src_ + 4);                                                   \
        B[2] = *reinterpret_cast<const float4*>(src_ + 16 * CH);                                             \
        B[3] = *reinterpret_cast<const float4*>(src_ + 16 * CH + 4); }
// an A fragment (two ds_read_b128) from the LDS BYTE address ADDR, which already contains the image's base, into V (float4[2])
#define BB_ALOAD(V, ADDR)                                                                                    \
      { const LdsF4* ap_ = reinterpret_cast<const LdsF4*>(ADDR);                                             \
        const f32x4 t0_ = ap_[0], t1_ = ap_[1];                                                              \
        V[0] = make_float4(t0_[0], t0_[1], t0_[2], t0_[3]); V[1] = make_float4(t1_[0], t1_[1], t1_[2], t1_[3]); }
// ... with the address clamped to LO .. HI (the image's zero rows -1 and TW_ROWS).
// (VALU work does not run under fp32 MFMAs on this SIMD: the clamp is ONE v_med3_i32, and the fragment is read through an
//  LDS address kept as an integer that already contains the image's base — as "imgb + o_" every request carried a
//  v_add_u32 of the dynamic-LDS symbol, which is 0)
#define BB_ALOAD_CLAMPED(V, ADDR, LO, HI)                                                                    \
      { int o_;                                                                                              \
        asm("v_med3_i32 %0, %1, %2, %3" : "=v"(o_) : "v"(ADDR), "v"(LO), "v"(HI));                           \
        BB_ALOAD(V, o_) }

// ---- backbone_kernel's and backbone_grad_kernel's entry: the gradient pass walks the forward's work split with the forward's text.
#define B2_ALOAD(R, V, DELTA, COFF, DBYTES)                                                                  \
      BB_ALOAD_CLAMPED(V, arow0 + (DBYTES) + (R) * (32 * BB_AP * 4), a_lo + (COFF), a_hi + (COFF))
#define B2_MM(R, U, NOUT)                                                                                    \
      __builtin_amdgcn_sched_barrier(0);                                                                     \
      LGKM_WAIT(NOUT)                                                                                        \
      BB_MM16(acc[R], U, live & (1 << (2 * (R))))                                                            \
      __builtin_amdgcn_sched_barrier(0);
// entry parameters from a schedule word
#define B2_PARAMS(EN, DELTA, COFF, DBYTES)                                                                   \
      const int DELTA = ((((EN) >> 15) & 15) - 4) * dil;                                                     \
      const int COFF = (((EN) >> 13) & 3) * (CH * 4);                                                        \
      const int DBYTES = DELTA * (BB_AP * 4) + COFF;
// what every entry body begins with: the next schedule word is requested, the current tile unpacked, the next entry's tile sent to
// the idle set (after the last entry: this entry's again, never used — unconditional, so that the compiler's vmcnt model has one
// path), this entry's parameters decoded
#define B2_ENTRY_HEAD(BC, BN)                                                                                \
      const int nxt = en >> 19;                                                                              \
      const int en_next_v = sched[nxt < it_end ? nxt : it];                                                  \
      BB_UNPACK(BC)                                                                                          \
      BB_WLOAD(BN, wsrc + (size_t)tile_of(nxt < it_end ? nxt : it) * BB_C * CH)                              \
      B2_PARAMS(en, delta, coff, dbytes)                                                                     \
      const int live = en >> rh;                          /* bit 2 r = owned tile r */
// A fragments of row tiles 0 and 1 of an entry are requested during the LAST MFMA groups of the entry before it (first
// entry of a layer: right here), so that the matrix pipe does not run dry at every (chunk, tap) boundary while both waves
// of a SIMD wait for their first LDS reads (round 3; same bits: only the loads move). A wave with 7 row tiles ends an
// entry on the fragment set it began with, so its two sets trade roles from entry to entry (two copies of the body).
// one (chunk, tap) entry of a wave with 7 / 6 owned row tiles; UA holds (or is receiving) row tile 0, UB row tile 1
#define B2_ENTRY(UA, UB, BC, BN)                                                                             \
    { B2_ENTRY_HEAD(BC, BN)                                                                                  \
      /* (after a layer's last entry the "next entry" loads below read the dying image with the wrong dilation: clamped \
         addresses, values never used — the layer prologue reloads both sets; cheaper than a second copy of the MFMA groups) */ \
      B2_MM(0, UA, 3)                                     /* in flight: tile 1 (2 reads) + the schedule word */ \
      B2_ALOAD(2, UA, delta, coff, dbytes)                                                                   \
      B2_MM(1, UB, 2)                                                                                        \
      const int en2 = __builtin_amdgcn_readfirstlane(en_next_v);                                             \
      B2_PARAMS(en2, delta2, coff2, dbytes2)                                                                 \
      B2_ALOAD(3, UB, delta, coff, dbytes)                                                                   \
      B2_MM(2, UA, 2)                                                                                        \
      B2_ALOAD(4, UA, delta, coff, dbytes)                                                                   \
      B2_MM(3, UB, 2)                                                                                        \
      B2_ALOAD(5, UB, delta, coff, dbytes)                                                                   \
      B2_MM(4, UA, 2)                                                                                        \
      if (rh == 0) {                                                                                         \
        B2_ALOAD(6, UA, delta, coff, dbytes)                                                                 \
        B2_MM(5, UB, 2)                                                                                      \
        B2_ALOAD(0, UB, delta2, coff2, dbytes2)           /* next entry: tile 0 in UB, tile 1 in UA */       \
        B2_MM(6, UA, 2)                                                                                      \
        B2_ALOAD(1, UA, delta2, coff2, dbytes2)                                                              \
      } else {                                                                                               \
        B2_ALOAD(0, UA, delta2, coff2, dbytes2)                                                              \
        B2_MM(5, UB, 2)                                                                                      \
        B2_ALOAD(1, UB, delta2, coff2, dbytes2)                                                              \
      }                                                                                                      \
      it = nxt;                                                                                              \
      en = en2; }
// the same entry for a wave with at most FOUR / TWO owned row tiles (tiles of <= 8 / <= 4 row tiles): both waves of a SIMD take the
// same even number of slots, so the fragment sets keep their roles from entry to entry
#define B2_ENTRY4(UA, UB, BC, BN)                                                                            \
    { B2_ENTRY_HEAD(BC, BN)                                                                                  \
      B2_MM(0, UA, 3)                                                                                        \
      B2_ALOAD(2, UA, delta, coff, dbytes)                                                                   \
      B2_MM(1, UB, 2)                                                                                        \
      const int en2 = __builtin_amdgcn_readfirstlane(en_next_v);                                             \
      B2_PARAMS(en2, delta2, coff2, dbytes2)                                                                 \
      B2_ALOAD(3, UB, delta, coff, dbytes)                                                                   \
      B2_MM(2, UA, 2)                                                                                        \
      B2_ALOAD(0, UA, delta2, coff2, dbytes2)                                                                \
      B2_MM(3, UB, 2)                                                                                        \
      B2_ALOAD(1, UB, delta2, coff2, dbytes2)                                                                \
      it = nxt;                                                                                              \
      en = en2; }
#define B2_ENTRY2(UA, UB, BC, BN)                                                                            \
    { B2_ENTRY_HEAD(BC, BN)                                                                                  \
      B2_MM(0, UA, 3)                                                                                        \
      const int en2 = __builtin_amdgcn_readfirstlane(en_next_v);                                             \
      B2_PARAMS(en2, delta2, coff2, dbytes2)                                                                 \
      B2_ALOAD(0, UA, delta2, coff2, dbytes2)                                                                \
      B2_MM(1, UB, 2)                                                                                        \
      B2_ALOAD(1, UB, delta2, coff2, dbytes2)                                                                \
      it = nxt;                                                                                              \
      en = en2; }

// Work split: wave w owns 32 output channels (column group w & 3) of the row tiles of parity w >> 2 (7 / 6 tiles; the
// two waves of a SIMD share a column group and split the rows). An MFMA group is ONE row tile x two column tiles x
// 8 k-steps = 16 MFMAs alternating two accumulators, so
//   * an A fragment (two ds_read_b128 + one clamped address) feeds two column tiles;
//   * dead row tiles are skipped one by one;
//   * a LayerNorm row has two of its values in the same lane (half the DPP reductions, 4 partials per row).
// (A first version gave each wave 16 channels of all 13 row tiles and skipped tiles in pairs: twice the LDS reads and
//  address VALU per MFMA, 6 % more MFMAs; 2.31 vs 2.17 ms.)
// LDS image rows: row -1 and rows >= L of a one-sequence tile are zero, so a tap is a clamped row offset.
// PLN (the incremental stem, svdd_backbone_incr_f32): 1 = the forward also STORES f after each of the first planes_P conv layers
// (the first step of a decode fills the carried planes); 2 = the TAIL forward: f is loaded from plane planes_P and the layers
// planes_P .. nl - 1 plus final_conv run unchanged. Same operations on every element either way: same bits in `out`.
template <bool SPT1, bool SAVE = false, int PLN = 0>
__global__ __launch_bounds__(512, 2) void backbone_kernel(BackboneArgs a, BackboneSave sv) {
  static_assert(SPT1 || !SAVE, "the saving forward is the one-sequence-per-tile form");
  static_assert(SPT1 || PLN == 0, "the carried planes belong to the one-sequence-per-tile form");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* img = smem + BB_AP;                              // rows -1 .. TW_ROWS ; [-1] and [TW_ROWS] stay zero
  float* Bs = smem + (TW_ROWS + 2) * BB_AP;               // [9][5][128] the first layer's lookup table
  float* psum = Bs + 9 * 5 * BB_C;                        // [4][TW_ROWS]
  float* rstat = psum + 8 * TW_ROWS;                      // [TW_ROWS]
  int* toks = reinterpret_cast<int*>(rstat + TW_ROWS);    // [TW_ROWS]
  int* rpos = toks + TW_ROWS;                             // [TW_ROWS] position of a tile row inside its sequence
  int* sdil = rpos + TW_ROWS;                             // [BB_MAXL + 1]
  int* sched = sdil + BB_MAXL + 1;                        // [(nl + 1) * 36]

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cg = w & 3, rh = w >> 2;
  const int j = lane & 15, g = lane >> 4;
  const int col0 = 32 * cg + j;                           // this lane's columns: col0 and col0 + 16
  const int L = a.L;
  const int nvalid = a.count ? __builtin_amdgcn_readfirstlane(*a.count) : a.n;
  int seq0 = blockIdx.x, spt = 1;                         // this tile's first sequence and how many it takes
  if (!SPT1) {
    if ((int)blockIdx.x >= nvalid) return;                // a tile takes at least one sequence: no plan needed to know this one is empty
    SvddTilePlan pl = a.plan;
    if (a.auto_spt) pl = svdd_plan_tiles(nvalid, L, a.ncu, 9);
    svdd_plan_tile(pl, (int)blockIdx.x, seq0, spt);
    seq0 = __builtin_amdgcn_readfirstlane(seq0);
    spt = __builtin_amdgcn_readfirstlane(spt);
  }
  const int tile_rows = spt * L;
  if (seq0 >= nvalid) return;
  // Short tiles (round 6): a tile of nt < 13 row tiles leaves some of a wave's 7 / 6 row-tile slots dead — and a dead slot still cost
  // its fragment request, liveness test and wait in every (chunk, tap) entry, and its rows their LayerNorm passes (a 4-row-tile
  // workgroup: 10 dead slots per entry, 0.73 pipe occupancy in the loop, 14 % of its time in LayerNorm code for rows that do not exist;
  // profiles/r06_bb_small_tile_phases.txt). nro = the row-tile slots this wave really owns; the entry bodies come in three lengths
  // (7 / 4 / 2 slots) and the LayerNorm passes skip the slots beyond nro. Same operations on every live row: same bits.
  const int nt = SPT1 ? TW_RT : (tile_rows + 15) >> 4;
  const int nro = SPT1 ? 7 : __builtin_amdgcn_readfirstlane((nt - rh + 1) >> 1);
  const int body = SPT1 ? 7 : (nt <= 4 ? 2 : nt <= 8 ? 4 : 7);
#define BB_OWN(R) (SPT1 || (R) < nro)
  const int nl = a.nl;
  const int it_end = (nl + 1) * 36;
  constexpr int NR = 7;                                   // owned row tiles rh + 2 r (r = 6 only for rh = 0)

  // Several sequences per tile (!SPT1, L <= 104; round 5): the `spt` sequences are INTERLEAVED position-major — tile row
  // e = position * spt + q holds position e / spt of sequence seq0 + q. A dilated tap then is a row offset of spt * (t - 4) * dil that
  // leaves the tile exactly when the position leaves the sequence: the tile behaves like ONE sequence of spt * L rows with every
  // dilation multiplied by spt — clamped addressing and tile-granular liveness as for L = 200, instead of a position test per
  // fragment row and row tiles kept live by a few rows of each stacked sequence (the stacked layout issued 425 tile-taps per five
  // layers for 372 useful ones). Same products in the same order per output element: same bits.
  const int il = SPT1 ? 1 : spt;
  for (int e = tid; e < TW_ROWS; e += 512) {
    int tk = -1;
    const int q = SPT1 ? 0 : e % il, pos = SPT1 ? e : e / il;
    if (e < tile_rows && seq0 + q < nvalid) {
      const int64_t sq = a.row_idx ? (int64_t)a.row_idx[seq0 + q] : (int64_t)(seq0 + q);
      tk = a.x[sq * L + pos];
    }
    toks[e] = tk;
    rpos[e] = e < tile_rows ? pos : -(1 << 20);
  }
  for (int e = tid; e < BB_AP; e += 512) { smem[e] = 0.0f; img[TW_ROWS * BB_AP + e] = 0.0f; }
  if (!SPT1)                                              // rows of the slots nobody owns: zero once, never written again (taps read them as padding)
    for (int e = 16 * nt * BB_AP + tid; e < TW_ROWS * BB_AP; e += 512) img[e] = 0.0f;
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < BB_MAXL; ++i) sdil[i] = a.dil[i];
    sdil[BB_MAXL] = 1;
  }
  for (int e = tid; e < 9 * 5 * BB_C; e += 512) Bs[e] = a.table0[e];
  __syncthreads();
  // Schedule: index k = (layer*4 + chunk)*9 + tap. sched[k] = 0 for a tap that only sees zero padding, else
  //   bits 0-12: live row tiles ; 13-14 chunk ; 15-18 tap ; 19-28 index of the next live k.
  for (int k = tid; k < it_end; k += 512) {
    auto entry = [&](int kk) {
      const int layer = kk / 36, t = kk % 9;
      if (layer >= nl) return t == 4 ? 0x1fff : 0;
      const int d = (t - 4) * sdil[layer] * il;           // in tile rows (interleaved sequences: il rows per position)
      const int lo = d < 0 ? -d : 0, hi = d > 0 ? tile_rows - d : tile_rows;
      if (lo >= hi) return 0;
      int m = 0;
      for (int r = 0; r < TW_RT; ++r) if (lo < 16 * r + 16 && hi > 16 * r) m |= 1 << r;
      return m;
    };
    const int m = entry(k);
    int nx = k + 1;
    while (nx < it_end && entry(nx) == 0) ++nx;
    sched[k] = m ? (m | ((k % 36) / 9) << 13 | (k % 9) << 15 | nx << 19) : 0;
  }

  // ---- first layer: f[row][col] = relu(b + sum_t table[t][tok[row + t - 4]][col])   (dnaconv.py:177,184)
  f32x4 f[NR][2], acc[NR][2];
  unsigned long long relu_bits = 0ull;                    // SAVE: this lane's ReLU decisions of the current layer
  // the sequence's rows of plane 0 (PLN): plane k is pl_stride floats further on
  const size_t pl_stride = (size_t)a.n * TW_ROWS * BB_C;
  float* pl0 = PLN ? a.planes + (size_t)(a.row_idx ? a.row_idx[seq0] : seq0) * TW_ROWS * BB_C : nullptr;
  if (PLN == 2) {
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * (rh + 2 * r) + 4 * g + e;
          f[r][ct][e] = row < tile_rows ? pl0[(size_t)(a.planes_P - 1) * pl_stride + row * BB_C + col0 + 16 * ct] : 0.0f;
        }
  }
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    if (PLN == 2) break;
    const int col = col0 + 16 * ct;
    const float b0 = a.vec[col];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = 16 * (rh + 2 * r) + 4 * g + e;
        float v = b0;
        if (row < TW_ROWS) {
          const int pos = rpos[row];
#pragma unroll
          for (int t = 0; t < 9; ++t) {
            const int p = pos + t - 4;
            const int tk = (p >= 0 && p < L) ? toks[row + (t - 4) * il] : -1;
            if (tk >= 0) v += Bs[(t * 5 + tk) * BB_C + col];
          }
        }
        f[r][ct][e] = row < tile_rows ? fmaxf(v, 0.0f) : 0.0f;
        if (SAVE && row < tile_rows && v > 0.0f) relu_bits |= 1ull << ((r * 2 + ct) * 4 + e);
      }
  }
  if (SAVE) sv.mask[(size_t)blockIdx.x * (nl + 2) * 512 + tid] = relu_bits;
  __syncthreads();                                        // sched is visible

  // A operand addressing: this lane feeds row 16 (rh + 2 r) + j of its tiles, channels 32 c + 8 g .. + 8
  const int img_lds = (int)(unsigned)(size_t)(const __attribute__((address_space(3))) float*)img;              // LDS byte address of img
  const int arow0 = img_lds + ((16 * rh + j) * BB_AP + 8 * g) * 4;  // LDS byte address of (row 16 rh + j, col 8 g) of img
  const int a_lo = arow0 - (16 * rh + j + 1) * BB_AP * 4; // row -1
  const int a_hi = arow0 + (TW_ROWS - 16 * rh - j) * BB_AP * 4;     // row TW_ROWS

  // Weight stream: each lane reads W[col0][8 g ..] and W[col0 + 16][8 g ..] of the (layer, chunk, tap) tile straight
  // from L2 into the B-operand registers, one tile ahead (no LDS staging, no barrier inside a layer).
  const float* wsrc = a.tiles + col0 * CH + 8 * g;
  auto tile_of = [&](int k) { return k < nl * 36 ? k : nl * 36 + (k - nl * 36) / 9; };
  const int layer0 = PLN == 2 ? a.planes_P : 0;           // the tail forward starts behind the carried stem
  int it = layer0 * 36;
  while (it < it_end && sched[it] == 0) ++it;
  it = __builtin_amdgcn_readfirstlane(it);
  int en = __builtin_amdgcn_readfirstlane(sched[it]);
  // two weight-fragment sets that trade roles from entry to entry (round 4d: with ONE set refilled in place the current tile
  // had to be copied out first, 8 v_mov_b64 at each end of an entry, and VALU work does not run under fp32 MFMAs on this SIMD)
  float4 bA[4], bB[4];
  BB_WLOAD(bA, wsrc + (size_t)tile_of(it) * BB_C * CH)
  bB[0] = bA[0]; bB[1] = bA[1]; bB[2] = bA[2]; bB[3] = bA[3];

  for (int layer = layer0; layer <= nl; ++layer) {        // layer == nl: the first 1x1 conv of final_conv
    const float* vl = a.vec + (size_t)(layer + 1) * 4 * BB_C;
    if (layer < nl) {
      const float tb0 = vl[BB_C + col0], tb1 = vl[BB_C + col0 + 16];
      // pass 1: row means (this lane's two values of a row first, then the 16 lanes of the DPP row)
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (!BB_OWN(r)) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * (rh + 2 * r) + 4 * g + e;
          const float sm = group16_sum((f[r][0][e] + tb0) + (f[r][1][e] + tb1));
          if (j == 0 && row < TW_ROWS) psum[cg * TW_ROWS + row] = sm;
        }
      }
      __syncthreads();
      if (tid < TW_ROWS)
        rstat[tid] = ((psum[tid] + psum[TW_ROWS + tid]) + (psum[2 * TW_ROWS + tid] + psum[3 * TW_ROWS + tid])) * (1.0f / BB_C);
      __syncthreads();
      // pass 2: centred second moment
      // the four rows of a tile that a lane owns are adjacent: one 16-byte read per tile, issued one tile ahead (a read
      // placed next to its use would pay a full LDS round trip per row: the stores in between pin it in place)
      float4 st4 = *reinterpret_cast<const float4*>(rstat + min(16 * rh + 4 * g, TW_ROWS - 4));
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const float4 cur4 = st4;
        if (r + 1 < NR) st4 = *reinterpret_cast<const float4*>(rstat + min(16 * (rh + 2 * r + 2) + 4 * g, TW_ROWS - 4));
        const float mean4[4] = {cur4.x, cur4.y, cur4.z, cur4.w};
        if (!BB_OWN(r)) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * (rh + 2 * r) + 4 * g + e;
          const float mean = mean4[e];
          const float d0 = f[r][0][e] + tb0 - mean, d1 = f[r][1][e] + tb1 - mean;
          acc[r][0][e] = d0; acc[r][1][e] = d1;           // keep the centred values
          const float sq = group16_sum(d0 * d0 + d1 * d1);
          if (j == 0 && row < TW_ROWS) psum[cg * TW_ROWS + row] = sq;
        }
      }
      __syncthreads();
      if (tid < TW_ROWS)
        rstat[tid] = rsqrtf(((psum[tid] + psum[TW_ROWS + tid]) + (psum[2 * TW_ROWS + tid] + psum[3 * TW_ROWS + tid])) *
                            (1.0f / BB_C) + 1e-5f);
      __syncthreads();
      const float gm0 = vl[2 * BB_C + col0], gm1 = vl[2 * BB_C + col0 + 16];
      const float bt0 = vl[3 * BB_C + col0], bt1 = vl[3 * BB_C + col0 + 16];
      st4 = *reinterpret_cast<const float4*>(rstat + min(16 * rh + 4 * g, TW_ROWS - 4));
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const float4 cur4 = st4;
        if (r + 1 < NR) st4 = *reinterpret_cast<const float4*>(rstat + min(16 * (rh + 2 * r + 2) + 4 * g, TW_ROWS - 4));
        const float rs4[4] = {cur4.x, cur4.y, cur4.z, cur4.w};
        if (!BB_OWN(r)) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * (rh + 2 * r) + 4 * g + e;
          if (row < TW_ROWS) {
            const float rs = rs4[e];
            img[row * BB_AP + col0] = row < tile_rows ? acc[r][0][e] * rs * gm0 + bt0 : 0.0f;
            img[row * BB_AP + col0 + 16] = row < tile_rows ? acc[r][1][e] * rs * gm1 + bt1 : 0.0f;
            if (SAVE) {
              float* xh = sv.xhat + (((size_t)blockIdx.x * nl + layer) * 56 + (r * 2) * 4 + e) * 512 + tid;
              xh[0] = acc[r][0][e] * rs;
              xh[4 * 512] = acc[r][1][e] * rs;
            }
          }
        }
      }
      if (SAVE && tid < TW_ROWS) sv.rstd[((size_t)blockIdx.x * nl + layer) * TW_ROWS + tid] = rstat[tid];
    } else {
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (!BB_OWN(r)) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * (rh + 2 * r) + 4 * g + e;
          if (row < TW_ROWS) { img[row * BB_AP + col0] = f[r][0][e]; img[row * BB_AP + col0 + 16] = f[r][1][e]; }
        }
      }
    }
    // ---- implicit GEMM over (chunk, live tap)
    const float bl0 = vl[col0], bl1 = vl[col0 + 16];
#pragma unroll
    for (int r = 0; r < NR; ++r) { acc[r][0] = f32x4{bl0, bl0, bl0, bl0}; acc[r][1] = f32x4{bl1, bl1, bl1, bl1}; }
    const int dil = __builtin_amdgcn_readfirstlane(sdil[layer < nl ? layer : BB_MAXL]) * il;   // in tile rows
    const int layer_end = (layer + 1) * 36;
    __syncthreads();                                      // the image is complete
    // the entry loop: B2_* at file scope, shared with backbone_grad_kernel
    float4 ua[2], ub[2];
    if (it < layer_end) {
      B2_PARAMS(en, delta0, coff0, dbytes0)
      B2_ALOAD(0, ua, delta0, coff0, dbytes0)
      B2_ALOAD(1, ub, delta0, coff0, dbytes0)
    }
    // entries come in fours (the chunks of a tap), so a layer always ends on the second body and the sets keep their roles
    // from layer to layer; the odd exit is there for the bookkeeping only
    bool odd = false;
    if (!SPT1 && body == 4) {
      while (it < layer_end) {
        B2_ENTRY4(ua, ub, bA, bB)
        if (it >= layer_end) { odd = true; break; }
        B2_ENTRY4(ua, ub, bB, bA)
      }
    } else if (!SPT1 && body == 2) {
      while (it < layer_end) {
        B2_ENTRY2(ua, ub, bA, bB)
        if (it >= layer_end) { odd = true; break; }
        B2_ENTRY2(ua, ub, bB, bA)
      }
    } else if (rh == 0) {
      while (it < layer_end) {
        B2_ENTRY(ua, ub, bA, bB)
        if (it >= layer_end) { odd = true; break; }
        B2_ENTRY(ub, ua, bB, bA)
      }
    } else {
      while (it < layer_end) {
        B2_ENTRY(ua, ub, bA, bB)
        if (it >= layer_end) { odd = true; break; }
        B2_ENTRY(ua, ub, bB, bA)
      }
    }
    if (odd) { bA[0] = bB[0]; bA[1] = bB[1]; bA[2] = bB[2]; bA[3] = bB[3]; }
    __syncthreads();                                      // every wave is done reading the image
    if (SAVE) {
      relu_bits = 0ull;
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (acc[r][ct][e] > 0.0f) relu_bits |= 1ull << ((r * 2 + ct) * 4 + e);
      sv.mask[((size_t)blockIdx.x * (nl + 2) + 1 + layer) * 512 + tid] = relu_bits;
    }
    if (layer < nl) {
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (!BB_OWN(r)) continue;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
          for (int e = 0; e < 4; ++e) f[r][ct][e] = fmaxf(acc[r][ct][e], 0.0f) + f[r][ct][e];   // relu(conv + b) + f
      }
      if (PLN == 1 && layer < a.planes_P) {
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
          for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int row = 16 * (rh + 2 * r) + 4 * g + e;
              if (row < tile_rows) pl0[(size_t)layer * pl_stride + row * BB_C + col0 + 16 * ct] = f[r][ct][e];
            }
      }
    } else {
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (!BB_OWN(r)) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * (rh + 2 * r) + 4 * g + e;
          if (row < TW_ROWS) {
            img[row * BB_AP + col0] = fmaxf(acc[r][0][e], 0.0f);                                   // relu(W1 f + b1)
            img[row * BB_AP + col0 + 16] = fmaxf(acc[r][1][e], 0.0f);
          }
        }
      }
    }
  }
  __syncthreads();
  // ---- last 1x1 conv 128 -> 5: one (row, class) dot product per thread iteration
  for (int e = tid; e < tile_rows * 5; e += 512) {
    const int row = e / 5, v = e - 5 * row;
    const int q = SPT1 ? 0 : row % il, pos = SPT1 ? row : row / il;   // tile row -> (sequence seq0 + q, position)
    if (seq0 + q >= nvalid) continue;
    const float* hr = img + row * BB_AP;
    const float* wv = a.w2 + v * BB_C;
    float sm = a.w2[5 * BB_C + v];
#pragma unroll 8
    for (int k = 0; k < BB_C; ++k) sm += hr[k] * wv[k];
    const int64_t sq = (a.row_idx && a.out_scatter) ? (int64_t)a.row_idx[seq0 + q] : (int64_t)(seq0 + q);
    a.out[(sq * L + pos) * 5 + v] = sm;
  }
}
#undef BB_OWN

// ------------------------------------------------- incremental stem: only what a step's new tokens can reach (svdd_backbone_incr[2]_f32) ----
// The backbone does not see the time step, so a row's activations depend on its tokens alone, and between two decode steps a row's
// tokens change at a few positions. The leading run of P dilation-1 layers spreads a changed position p slowly: f after the first
// convolution differs from the previous step's inside p +- 4, f after conv layer k - 1 ("plane k") inside p +- (4 + 4 k) — everything
// else is the previous step's value, bit for bit. So f of every row is CARRIED in HBM across the decode, planes 1 .. P of
// [n][208][128] fp32, and per step
//   backbone_worklist_kernel   compares the old and the new tokens and writes, per layer, the row tiles inside the reach as items
//                              (first tile, tile count <= max_item) over runs of adjacent tiles;
//   backbone_order_kernel      (svdd_backbone_incr2_f32) packs each layer's non-empty items into a list, most tiles first, so that
//                              the dispatcher — which hands workgroups out in index order — balances the CUs by itself;
//   backbone_seg_kernel        one launch per layer k = 1 .. P, one workgroup per item: plane k - 1 of the item's tiles and of one
//                              halo tile on each side (k = 1: f_0 from the tokens, the table lookup of backbone_kernel's first
//                              layer) -> LayerNorm image in LDS -> the 9-tap convolution of the item's own tiles -> ReLU + residual ->
//                              plane k;
//   backbone_kernel<.., 2>     the tail: layers P .. nl - 1 and final_conv from plane P, one workgroup per sequence as ever.
// The work of the stem is then spread over the chip by ITEM, not tied to its row's CU (a per-row incremental kernel lasts as long
// as the row with the widest change: 0.90 of the full stage in the per-step maximum over 256 rows, 0.34 on average).
// Same bits: the segment kernel keeps backbone_kernel's lane-to-column ownership (wave = column group cg, lane (j, g) owns columns
// 32 cg + j and + 16 of rows 4 g + e), its LayerNorm summation tree (lane pair, group16_sum read at j = 0, the four psum partials as
// (p0 + p1) + (p2 + p3), the same rsqrtf), the accumulator start (the bias) and the (chunk outer, tap inner, 8 k-steps) order of
// products. At dilation 1 every tap of every row tile is live in backbone_kernel's schedule, so all 36 entries run; a tap that
// leaves the sequence reads a zero row there (clamped address) and a zero row of the halo tile here. A mask that marks too many
// tiles is still exact (an unchanged tile recomputes to the same bits); no workgroup waits for another: the stream orders the layers.
// svdd_backbone_incr3_f32 carries the planes on through the dilation-4 layers behind the stem: the reach grows by 16 rows per layer
// (BackboneReach), the same kernel runs them as backbone_seg_kernel<.., DIL = 4>, and the tail starts behind the last carried plane.
constexpr int SEG_SLOTS = 7;                   // items per (layer, row): 13 tiles in runs cut to <= 2 (or <= 4) tiles, at worst 7

struct BackboneSegArgs {
  const uint8_t* x;        // [n, L] the step's tokens (layer 1 builds f_0 from them)
  const float* table0;     // as BackboneArgs
  const float* tiles;
  const float* vec;
  float* planes;           // [P][n][208][128]
  const int* items;        // [P][n][SEG_SLOTS] : first tile | tile count << 8 ; 0 = empty slot
  int n, L, layer;         // layer k = 1 .. P: reads plane k - 1 (k = 1: the tokens), writes plane k
  const int* order;        // [P][order_stride] : row << 16 | item, the layer's non-empty items, most tiles first   (ORD kernels only)
  const int* order_count;  // [P] : entries of order[k] that are set
  int order_stride;        // n * (items per row)
};

// How far a changed position has spread in plane k, k = 1 .. P: r[k - 1] = 4 + sum over i < k of 4 dil[i] (4 + 4 k over the leading
// dilation-1 layers; 52, 68, 84, 100 over the four dilation-4 layers behind eight of them). lead1 = the leading dilation-1 layers:
// the marked tile-layers of planes 1 .. lead1 are counted in stat[0], those of the deeper planes in stat[1].
struct BackboneReach {
  int r[BB_MAXL];
  int lead1;
};
static BackboneReach backbone_reach(const int* dilations, int P, int lead1) {
  BackboneReach rc{};
  int reach = 4;
  for (int k = 1; k <= P; ++k) { reach += 4 * dilations[k - 1]; rc.r[k - 1] = reach; }
  rc.lead1 = lead1;
  return rc;
}

// One wave per row. Lane k - 1 cuts layer k's tile mask into items; stat (may be NULL) += the tile-layers marked (see BackboneReach).
// SLOTS = items per (layer, row): SEG_SLOTS for runs cut to 2 or 4 tiles, TW_RT for 1-tile items (the ordered entries only).
template <int SLOTS = SEG_SLOTS>
__global__ __launch_bounds__(256) void backbone_worklist_kernel(const uint8_t* __restrict__ x, uint8_t* __restrict__ x_prev, int n,
                                                                int L, int P, int max_item, int* __restrict__ items,
                                                                unsigned long long* __restrict__ stat, BackboneReach rc) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const int lane = threadIdx.x & 63;
  const uint8_t* xn = x + (size_t)row * L;
  uint8_t* xp = x_prev + (size_t)row * L;
  int changed = 0;                                        // bit q: position lane + 64 q differs
  for (int q = 0; q < 4; ++q) {
    const int l = lane + 64 * q;
    if (l < L && xn[l] != xp[l]) { changed |= 1 << q; xp[l] = xn[l]; }
  }
  int mine = 0;
  for (int k = 1; k <= P; ++k) {
    const int reach = rc.r[k - 1];
    int m = 0;
    for (int q = 0; q < 4; ++q)
      if (changed >> q & 1) {
        const int l = lane + 64 * q;
        const int tlo = max(0, l - reach) >> 4, thi = min(L - 1, l + reach) >> 4;
        m |= ((2 << thi) - 1) & ~((1 << tlo) - 1);
      }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m |= __shfl_xor(m, off, 64);
    if (lane == k - 1) mine = m;
  }
  if (stat) {                                             // one add per wave and counter: the lanes' adds to one address would queue up in L2
    int c0 = lane < rc.lead1 ? __popc(mine) : 0, c1 = lane < rc.lead1 ? 0 : __popc(mine);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { c0 += __shfl_xor(c0, off, 64); c1 += __shfl_xor(c1, off, 64); }
    if (lane == 0 && c0) atomicAdd(stat, (unsigned long long)c0);
    if (lane == 0 && c1) atomicAdd(stat + 1, (unsigned long long)c1);
  }
  if (lane >= P) return;
  int* it = items + ((size_t)lane * n + row) * SLOTS;
  int cnt = 0;
  for (int t = 0; t < TW_RT;) {
    if (!(mine >> t & 1)) { ++t; continue; }
    int len = 1;
    while (len < max_item && t + len < TW_RT && (mine >> (t + len) & 1)) ++len;
    it[cnt++] = t | len << 8;
    t += len;
  }
  for (; cnt < SLOTS; ++cnt) it[cnt] = 0;
}

// The size-ordered list of svdd_backbone_incr2_f32: workgroup k packs layer k + 1's non-empty items into order[k] as
// row << 16 | item, the items of 4 tiles first, then 3, 2, 1; inside a size class in (row, slot) order — a deterministic build (two
// passes over the rows: the class totals, then a block scan per class), so two forwards of the same tokens write the same list. The
// dispatcher hands workgroups out in index order: with the large items in front, a CU that finishes early draws the next one, and
// the empty workgroups all come after the work instead of between it.
template <int SLOTS>
__global__ __launch_bounds__(256) void backbone_order_kernel(const int* __restrict__ items, int n, int* __restrict__ order,
                                                             int* __restrict__ order_count) {
  __shared__ int wtot[4][4];                              // [wave][class]: class c holds the items of 4 - c tiles
  __shared__ int base[4];                                 // where the class continues in order[k]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int* it = items + (size_t)blockIdx.x * n * SLOTS;
  int* ord = order + (size_t)blockIdx.x * n * SLOTS;
  int cnt[4] = {0, 0, 0, 0};
  for (int r = tid; r < n; r += 256)
    for (int s = 0; s < SLOTS; ++s) {
      const int len = it[r * SLOTS + s] >> 8;
      for (int c = 0; c < 4; ++c) cnt[c] += len == 4 - c;
    }
  for (int c = 0; c < 4; ++c) {
    int v = cnt[c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) wtot[w][c] = v;
  }
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int c = 0; c < 4; ++c) { base[c] = run; run += wtot[0][c] + wtot[1][c] + wtot[2][c] + wtot[3][c]; }
    order_count[blockIdx.x] = run;
  }
  __syncthreads();
  for (int r0 = 0; r0 < n; r0 += 256) {
    const int r = r0 + tid;
    int item[SLOTS], pos[4];
    for (int c = 0; c < 4; ++c) cnt[c] = 0;
    for (int s = 0; s < SLOTS; ++s) {
      item[s] = r < n ? it[r * SLOTS + s] : 0;
      for (int c = 0; c < 4; ++c) cnt[c] += (item[s] >> 8) == 4 - c;
    }
    for (int c = 0; c < 4; ++c) {                         // inclusive scan inside the wave, wave totals through LDS
      int v = cnt[c];
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) { const int u = __shfl_up(v, off, 64); if (lane >= off) v += u; }
      pos[c] = v - cnt[c];
      if (lane == 63) wtot[w][c] = v;
    }
    __syncthreads();
    for (int c = 0; c < 4; ++c) {
      int at = base[c] + pos[c];
      for (int q = 0; q < w; ++q) at += wtot[q][c];
      for (int s = 0; s < SLOTS; ++s)
        if ((item[s] >> 8) == 4 - c) ord[at++] = r << 16 | item[s];
    }
    __syncthreads();
    if (tid < 4) base[tid] += wtot[0][tid] + wtot[1][tid] + wtot[2][tid] + wtot[3][tid];
    __syncthreads();
  }
}

// The list of svdd_backbone_incr4_f32 in ONE launch: workgroup k - 1 builds layer k's items of every row straight from the tokens
// (it compares 256 rows at a time, then thread t cuts row t's items in LDS) and then packs order[k - 1] as backbone_order_kernel
// does, from the registers when n <= 256.
// Every workgroup compares x with x_cur; workgroup 0 alone writes x into x_next, the OTHER buffer of the ping-pong pair, so no
// workgroup reads what another writes.
// Layers k <= rc.lead1 (dilation 1) get TIGHT items, origin row | tiles << 8: every maximal run [a, b] of rows within the reach of
// a changed position is covered by 16-row tiles at a, a + 16, ..; a tile that reaches the next run's first row takes that run into
// the same cover, so the tiles of a row are disjoint (at most 13, origins < L). Runs of adjacent tiles are cut to max_item as ever.
// Tight cutting can need SEG_SLOTS + 1 items (four 3-tile runs cut 2 + 1 each): such a (layer, row) takes the aligned cover, as
// origins 16 T. The deeper layers get backbone_worklist_kernel's aligned items, first tile | tiles << 8, unchanged. At dilation 1
// no bit depends on the origin: an output row's accumulator and a row's LayerNorm do not depend on which tile holds the row (the
// tight windows of the tower rest on the same fact), and the segment kernels run every tap of every own tile at dilation 1 (they
// mask taps only at DIL > 1). backbone_kernel's schedule runs the same taps EXCEPT where the last tile holds fewer than five live
// rows (L mod 16 in 1 .. 4): there it drops (last tile, tap + d) for every d >= L mod 16, all of whose rows read past the end. The
// segment kernels issue those MFMAs on image rows >= L, which are zero: every extra product is a zero, the accumulator (it starts
// at the bias) keeps its bits, and the two kernels still agree bit for bit (tests/test_lengths_gpu.py, every residue mod 16).
// stat[0] += the tiles cut for layers <= lead1, stat[1] += those of the deeper layers, one add per wave.
__global__ __launch_bounds__(256) void backbone_list_kernel(const uint8_t* __restrict__ x, const uint8_t* __restrict__ x_cur,
                                                            uint8_t* __restrict__ x_next, int n, int L, int max_item,
                                                            int* __restrict__ items, int* __restrict__ order,
                                                            int* __restrict__ order_count, unsigned long long* __restrict__ stat,
                                                            BackboneReach rc) {
  typedef unsigned long long u64;
  __shared__ u64 chs[256][4];                             // bit p & 63 of chs[row][p >> 6]: position p of the chunk's row differs
  __shared__ int its[256][SEG_SLOTS];                     // the chunk's items
  __shared__ int wtot[4][4];                              // [wave][class]: class c holds the items of 4 - c tiles
  __shared__ int base[4];                                 // where the class continues in order[k]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int reach = rc.r[blockIdx.x];
  const bool tight = (int)blockIdx.x < rc.lead1, keep = blockIdx.x == 0;
  int* itk = items + (size_t)blockIdx.x * n * SEG_SLOTS;
  int* ord = order + (size_t)blockIdx.x * n * SEG_SLOTS;
  const bool words = L % 8 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(x_cur) |
                                     reinterpret_cast<uintptr_t>(x_next)) & 7) == 0;
  // The compare, 256 rows at a time: lane (half, w8) of a wave takes positions 8 w8 .. + 7 of row 2 i + half, so one read of the
  // wave is two whole rows, and all 64 reads of a lane are in flight together. The 8 bits go to LDS, where thread t then finds the
  // 256 bits of row t. (A thread reading its own row word by word costs the CU 64 cache lines per instruction.)
  unsigned char* chb = reinterpret_cast<unsigned char*>(chs);
  const int half = lane >> 5, w8 = lane & 31;
  int tiles = 0, item[SEG_SLOTS], cnt4[4] = {0, 0, 0, 0};
  for (int r0 = 0; r0 < n; r0 += 256) {
    if (words) {
      u64 a[32], c[32];
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        const int rr = r0 + 64 * wave + 2 * i + half;
        const bool in = rr < n && 8 * w8 < L;
        const size_t at = in ? (size_t)rr * L + 8 * w8 : 0;
        a[i] = *reinterpret_cast<const u64*>(x + at);
        c[i] = *reinterpret_cast<const u64*>(x_cur + at);
        if (!in) c[i] = a[i];
      }
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        const int rl = 64 * wave + 2 * i + half;
        if (keep && r0 + rl < n && 8 * w8 < L) *reinterpret_cast<u64*>(x_next + (size_t)(r0 + rl) * L + 8 * w8) = a[i];
        const u64 d = a[i] ^ c[i];                        // -> bit e = byte e of d is not zero: high bit per non-zero byte, gathered by a multiply
        const unsigned dl = (unsigned)d, dh = (unsigned)(d >> 32);
        const unsigned zl = (((dl & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | dl) & 0x80808080u, zh = (((dh & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | dh) & 0x80808080u;
        const unsigned m = ((zl >> 7) * 0x10204080u) >> 28 | (((zh >> 7) * 0x10204080u) >> 28) << 4;
        chb[rl * 32 + w8] = (unsigned char)m;
      }
    } else {
      for (int i = 0; i < 32; ++i) {
        const int rl = 64 * wave + 2 * i + half, rr = r0 + rl;
        unsigned m = 0;
        if (rr < n)
          for (int e = 0; e < 8 && 8 * w8 + e < L; ++e) {
            const size_t at = (size_t)rr * L + 8 * w8 + e;
            const uint8_t a = x[at];
            if (keep) x_next[at] = a;
            m |= (unsigned)(a != x_cur[at]) << e;
          }
        chb[rl * 32 + w8] = (unsigned char)m;
      }
    }
    __syncthreads();
    const int r = r0 + tid;
    const u64 ch[4] = {chs[tid][0], chs[tid][1], chs[tid][2], chs[tid][3]};   // all zero for a row >= n
    int* it = its[tid];
    int cnt = 0, nt = 0;
    if (tight) {
      int cend = -1, io = 0, il = 0;                      // last row the cover holds ; the open item's origin and tiles
#pragma unroll
      for (int q = 0; q < 4; ++q)
        for (u64 b = ch[q]; b; b &= b - 1) {
          const int p = 64 * q + __builtin_ctzll(b);
          const int lo = max(0, p - reach), hi = min(L - 1, p + reach);
          int o = lo > cend ? lo : cend + 1;              // a new run starts its own cover; a run the cover has reached continues it
          for (; o <= hi; o += 16) {
            ++nt;
            if (il > 0 && il < max_item && o == io + 16 * il) { ++il; continue; }
            if (il > 0) { if (cnt < SEG_SLOTS) it[cnt] = io | il << 8; ++cnt; }
            io = o; il = 1;
          }
          cend = o - 1;
        }
      if (il > 0) { if (cnt < SEG_SLOTS) it[cnt] = io | il << 8; ++cnt; }
    }
    if (!tight || cnt > SEG_SLOTS) {                      // aligned tiles: backbone_worklist_kernel's mask and cut
      int m = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        for (u64 b = ch[q]; b; b &= b - 1) {
          const int p = 64 * q + __builtin_ctzll(b);
          const int tlo = max(0, p - reach) >> 4, thi = min(L - 1, p + reach) >> 4;
          m |= ((2 << thi) - 1) & ~((1 << tlo) - 1);
        }
      cnt = 0; nt = __popc(m);
      for (int t = 0; t < TW_RT;) {
        if (!(m >> t & 1)) { ++t; continue; }
        int len = 1;
        while (len < max_item && t + len < TW_RT && (m >> (t + len) & 1)) ++len;
        it[cnt++] = (tight ? 16 * t : t) | len << 8;
        t += len;
      }
    }
    for (; cnt < SEG_SLOTS; ++cnt) it[cnt] = 0;
    tiles += nt;
#pragma unroll
    for (int s = 0; s < SEG_SLOTS; ++s) {                 // the thread's own slots back into registers, and out
      item[s] = its[tid][s];
      if (r < n) itk[(size_t)r * SEG_SLOTS + s] = item[s];
#pragma unroll
      for (int c = 0; c < 4; ++c) cnt4[c] += (item[s] >> 8) == 4 - c;
    }
    __syncthreads();                                      // (the next 256 rows overwrite chs)
  }
  if (stat) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tiles += __shfl_xor(tiles, off, 64);
    if (lane == 0 && tiles) atomicAdd(stat + (tight ? 0 : 1), (unsigned long long)tiles);
  }
  // ---- order[k], as backbone_order_kernel packs it: the class totals, then a block scan per class over 256 rows at a time
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    int v = cnt4[c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) wtot[wave][c] = v;
  }
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int c = 0; c < 4; ++c) { base[c] = run; run += wtot[0][c] + wtot[1][c] + wtot[2][c] + wtot[3][c]; }
    order_count[blockIdx.x] = run;
  }
  __syncthreads();
  for (int r0 = 0; r0 < n; r0 += 256) {
    const int r = r0 + tid;
    int pos[4], cl[4] = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < SEG_SLOTS; ++s) {
      if (n > 256) item[s] = r < n ? itk[(size_t)r * SEG_SLOTS + s] : 0;   // one chunk: the registers still hold it
#pragma unroll
      for (int c = 0; c < 4; ++c) cl[c] += (item[s] >> 8) == 4 - c;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {                         // inclusive scan inside the wave, wave totals through LDS
      int v = cl[c];
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) { const int u = __shfl_up(v, off, 64); if (lane >= off) v += u; }
      pos[c] = v - cl[c];
      if (lane == 63) wtot[wave][c] = v;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      int at = base[c] + pos[c];
      for (int q = 0; q < wave; ++q) at += wtot[q][c];
#pragma unroll
      for (int s = 0; s < SEG_SLOTS; ++s)
        if ((item[s] >> 8) == 4 - c) ord[at++] = r << 16 | item[s];
    }
    __syncthreads();
    if (tid < 4) base[tid] += wtot[0][tid] + wtot[1][tid] + wtot[2][tid] + wtot[3][tid];
    __syncthreads();
  }
}

// The segment kernels: 4 waves, wave cg owns 32 output channels of EVERY tile of an item, so a weight fragment feeds up to NC row tiles
// and the register arrays are sized to the item. There are two LAYOUTS of an item's rows over the image and the register slots, and
// ONE body, svdd_seg_body.h, that both kernels compile: the token fetch, layer 1 through the image, the three LayerNorm passes, the
// accumulators starting at the bias, the 36 entries and relu(conv + b) + f are written once. A layout is compile-time constants only;
// what differs between the two is decided on them where the body needs it (SEG_LIVE / SEG_MINE / SEG_IROW ... in svdd_seg_body.h):
//   NC, NS, ROWS   the most own tiles of an item, the register slots, the image rows
//   PK             TIGHT: the slot that packs both halos
//   ORD            workgroup b takes entry b of the layer's size-ordered list; false: slot b of `items`
//   DIL            the layer's dilation
// The body is text that each kernel includes, not a function both call: as an inlined function (and with the layout as an object with
// methods) every one of the nine kernels came out with other instructions than before, as included text with none
// (profiles/backbone_shared_code.txt).
//
// SegAligned<NC, ORD, DIL> (backbone_seg_kernel): items of whole tiles, slots 0 .. NC + 1 = halo tile, own tiles, halo tile; image
// row i = sequence row 16 (t0 - 1) + i. ORD: svdd_backbone_incr2_f32's list; NC = 1 exists for that list only (3 image slots, one
// fragment set per entry, 4 workgroups per CU).
// DIL = 1 or 4 (svdd_backbone_incr3_f32): tap t reads image row + (t - 4) DIL, at most the 16 rows of one halo tile away. At dilation
// 4 backbone_kernel's schedule drops a (row tile, tap) pair whose inputs are all padding — with d = (t - 4) DIL, tile T is live iff
// max(0, -d) < 16 T + 16 and min(L, L - d) > 16 T; at L = 200 tile 0 drops tap -16, tile 12 taps +8, +12, +16 — and exactly those
// pairs issue no MFMA here (tapmask), so the accumulators see the same operations in the same order.
template <int NC_, bool ORD_, int DIL_>
struct SegAligned {
  static_assert(DIL_ == 1 || DIL_ == 4, "one halo tile per side holds taps of dilation <= 4");
  static constexpr int NC = NC_, NS = NC_ + 2, PK = NS, ROWS = 16 * NS, DIL = DIL_;
  static constexpr bool ORD = ORD_, TIGHT = false;
};

// SegTight (backbone_seg_tight_kernel): SegAligned<2, true, 1> for the TIGHT items of svdd_backbone_incr4_f32 (origin row |
// tiles << 8, any origin), with the halo packed: a dilation-1 item reads 4 rows beyond its tiles on each side, so the image is rows
// origin - 4 .. origin + 16 nown + 3 (40 rows for two tiles where the aligned layout holds 64) and the register arrays have THREE
// slots, not four: slots 0, 1 = the own tiles (image rows 4 + 16 s + 4 g + e), slot 2 = both halos — the lanes with g = 0 hold the
// left one (image rows 0 .. 3), those with g = 1 the right one (image rows 16 nown + 4 .. + 7), those with g = 2, 3 nothing (they
// neither load nor store; the VALU runs them along). A row's LayerNorm sums over the 16 lanes of one g and the four waves, so it is
// the same tree whichever slot holds the row. Output row j of tile c reads image rows 16 c + j + t, t = 0 .. 8.
struct SegTight {
  static constexpr int NC = 2, NS = NC + 1, PK = NC, ROWS = 16 * NC + 8, DIL = 1;
  static constexpr bool ORD = true, TIGHT = true;
};

// the two kernels: a layout each, and the occupancy its LDS image and register arrays allow
template <int NC_, bool ORD_ = false, int DIL_ = 1>
__global__ __launch_bounds__(256, NC_ == 4 ? 2 : NC_ == 1 ? 4 : 3) void backbone_seg_kernel(BackboneSegArgs a) {
  using LAY = SegAligned<NC_, ORD_, DIL_>;
#include "svdd_seg_body.h"
}
__global__ __launch_bounds__(256, 5) void backbone_seg_tight_kernel(BackboneSegArgs a) {
  using LAY = SegTight;
#include "svdd_seg_body.h"
}

// svdd_backbone_incr_seed_f32: the state a first = 1 forward leaves on n IDENTICAL rows, from one row's planes, logits and tokens (the
// prior of a decode is n all-MASK rows, and what the backbone makes of that row depends on the weights alone). A plain broadcast,
// grid-stride: rows < L of every carried plane as 16-byte vectors (the 1 MB source stays in L2), then the logits, then the tokens.
__global__ __launch_bounds__(256) void backbone_seed_kernel(const float4* __restrict__ row_planes, const float* __restrict__ row_logits,
                                                            const uint8_t* __restrict__ row_x, int n, int L, int depth,
                                                            float4* __restrict__ planes, float* __restrict__ out,
                                                            uint8_t* __restrict__ x_cur) {
  const int rowv = L * (BB_C / 4), planev = TW_ROWS * (BB_C / 4);       // vectors of a sequence's L rows / of a whole plane row
  const int tid = threadIdx.x;
  for (int pr = blockIdx.x; pr < depth * n; pr += gridDim.x) {         // pr = plane * n + row (depth * n < 2^31: the entry checks)
    const float4* src = row_planes + (size_t)(pr / n) * planev;
    float4* dst = planes + (size_t)pr * planev;
    for (int e = tid; e < rowv; e += 256) dst[e] = src[e];
  }
  for (int r = blockIdx.x; r < n; r += gridDim.x) {
    for (int e = tid; e < L * 5; e += 256) out[(size_t)r * (L * 5) + e] = row_logits[e];
    for (int e = tid; e < L; e += 256) x_cur[(size_t)r * L + e] = row_x[e];
  }
}

// ------------------------------------------- gradient of the backbone with respect to its one-hot input, ONE launch (round 5) ----
// The gradient-guidance baseline (DPS, reference diffusion_gosai.py:1321-1330 through models/dnaconv.py:212-247) needs
// d loss / d onehot(x_t) through the whole backbone; the weights are frozen. backbone_kernel<true, true> is the forward (the
// inference kernel's bits) that also leaves, per layer, x-hat, 1 / sigma and the ReLU decisions in its lane-private layout
// (BackboneSave); this kernel walks the layers in reverse with the SAME work split — wave (cg, rh) owns columns 32 cg .. + 32 of
// the row tiles rh + 2 r, the residual GRADIENT stream G lives in the registers the forward kept f in — so that every saved value
// comes back to the lane that wrote it in one coalesced load:
//     G1 = (dlogits W2) * relu'(final 1x1)                                    VALU, 5 MACs per element
//     G  = G1 W1                                                              1x1 conv with W1^T: the MFMA loop, taps = {4}
//     for i = nl - 1 .. 0:   dhn = conv9_dil_i^T (G * relu'_i)                the SAME implicit-GEMM loop on W_i with flipped taps and
//                                                                             swapped channel axes (packed by the host)
//                            G  += LayerNorm'(dhn ; xhat_i, rstd_i, gamma_i)   rstd (t - mean(t) - xhat mean(t xhat)), t = gamma dhn
//     dx[p][c] = sum_t sum_co W_first[co][c][t] (G * relu'_first)[p - (t - 4)][co]
// Tiles arrive in PROCESSING order: [4][128][32] of W1^T, then layer nl - 1, nl - 2, ... 0 as [4 chunks][9 taps][128][32].
struct BackboneGradArgs {
  const float* dlogits;    // [n][L][5]
  const float* tiles;      // see above
  const float* gamma;      // [nl][128], layer order
  const float* w2;         // [5][128]
  const float* table0;     // [9][5][128] = W_first[co][c][t] -> [t][c][co]
  float* dx;               // [n][L][5]
  int n, L, nl;
  int dil[BB_MAXL];        // layer order
};

__global__ __launch_bounds__(512, 2) void backbone_grad_kernel(BackboneGradArgs a, BackboneSave sv) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* img = smem + BB_AP;                              // rows -1 .. TW_ROWS ; [-1] and [TW_ROWS] stay zero
  float* Bs = smem + (TW_ROWS + 2) * BB_AP;               // [9][5][128]
  float* psum = Bs + 9 * 5 * BB_C;                        // [8][TW_ROWS]: partial sums of t (0..3) and of t xhat (4..7); first: dlogits
  float* rstat = psum + 8 * TW_ROWS;                      // [2][TW_ROWS]
  int* sdil = reinterpret_cast<int*>(rstat + 2 * TW_ROWS);  // [BB_MAXL + 1] dilation of processing step s (step 0 = the 1x1)
  int* sched = sdil + BB_MAXL + 1;                        // [(nl + 1) * 36]

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cg = w & 3, rh = w >> 2;
  const int j = lane & 15, g = lane >> 4;
  const int col0 = 32 * cg + j;
  const int L = a.L, nl = a.nl;
  const int tile_rows = L;
  const int64_t row0 = (int64_t)blockIdx.x * L;
  const int it_end = (nl + 1) * 36;
  constexpr int NR = 7;

  for (int e = tid; e < BB_AP; e += 512) { smem[e] = 0.0f; img[TW_ROWS * BB_AP + e] = 0.0f; }
  if (tid <= nl) sdil[tid] = tid == 0 ? 1 : a.dil[nl - tid];
  for (int e = tid; e < 9 * 5 * BB_C; e += 512) Bs[e] = a.table0[e];
  for (int e = tid; e < TW_ROWS * 5; e += 512) psum[e] = e < L * 5 ? a.dlogits[row0 * 5 + e] : 0.0f;
  __syncthreads();
  // Schedule: index k = (step*4 + chunk)*9 + tap ; the same word format as backbone_kernel's
  for (int k = tid; k < it_end; k += 512) {
    auto entry = [&](int kk) {
      const int step = kk / 36, t = kk % 9;
      if (step == 0) return t == 4 ? 0x1fff : 0;
      const int d = (t - 4) * sdil[step];
      const int lo = d < 0 ? -d : 0, hi = d > 0 ? L - d : L;
      if (lo >= hi) return 0;
      int m = 0;
      for (int r = 0; r < TW_RT; ++r) if (lo < 16 * r + 16 && hi > 16 * r) m |= 1 << r;
      return m;
    };
    const int m = entry(k);
    int nx = k + 1;
    while (nx < it_end && entry(nx) == 0) ++nx;
    sched[k] = m ? (m | ((k % 36) / 9) << 13 | (k % 9) << 15 | nx << 19) : 0;
  }

  // ---- G1 = (dlogits W2) * relu'(final 1x1) -> the image
  f32x4 G[NR][2], acc[NR][2];
  {
    const unsigned long long mk = sv.mask[((size_t)blockIdx.x * (nl + 2) + nl + 1) * 512 + tid];
    float w2a[5], w2b[5];
#pragma unroll
    for (int v = 0; v < 5; ++v) { w2a[v] = a.w2[v * BB_C + col0]; w2b[v] = a.w2[v * BB_C + col0 + 16]; }
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = 16 * (rh + 2 * r) + 4 * g + e;
        if (row < TW_ROWS) {
          float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
          for (int v = 0; v < 5; ++v) { const float dl = psum[row * 5 + v]; s0 += dl * w2a[v]; s1 += dl * w2b[v]; }
          img[row * BB_AP + col0] = ((mk >> ((r * 2) * 4 + e)) & 1ull) && row < tile_rows ? s0 : 0.0f;
          img[row * BB_AP + col0 + 16] = ((mk >> ((r * 2 + 1) * 4 + e)) & 1ull) && row < tile_rows ? s1 : 0.0f;
        }
      }
  }
  __syncthreads();                                        // sched and the image are visible

  const int img_lds = (int)(unsigned)(size_t)(const __attribute__((address_space(3))) float*)img;
  const int arow0 = img_lds + ((16 * rh + j) * BB_AP + 8 * g) * 4;
  const int a_lo = arow0 - (16 * rh + j + 1) * BB_AP * 4;
  const int a_hi = arow0 + (TW_ROWS - 16 * rh - j) * BB_AP * 4;

  const float* wsrc = a.tiles + col0 * CH + 8 * g;
  auto tile_of = [&](int k) { return k < 36 ? k / 9 : 4 + (k - 36); };
  int it = 0;
  while (it < it_end && sched[it] == 0) ++it;
  it = __builtin_amdgcn_readfirstlane(it);
  int en = __builtin_amdgcn_readfirstlane(sched[it]);
  float4 bA[4], bB[4];
  BB_WLOAD(bA, wsrc + (size_t)tile_of(it) * BB_C * CH)
  bB[0] = bA[0]; bB[1] = bA[1]; bB[2] = bA[2]; bB[3] = bA[3];

  for (int step = 0; step <= nl; ++step) {
    const int layer = nl - step;                          // step >= 1: the conv layer whose transpose this step applies
    if (step > 0) {
      // the image of this step: G * relu'(conv_layer), rows beyond the sequence zero
      const unsigned long long mk = sv.mask[((size_t)blockIdx.x * (nl + 2) + 1 + layer) * 512 + tid];
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * (rh + 2 * r) + 4 * g + e;
          if (row < TW_ROWS) {
            img[row * BB_AP + col0] = ((mk >> ((r * 2) * 4 + e)) & 1ull) && row < tile_rows ? G[r][0][e] : 0.0f;
            img[row * BB_AP + col0 + 16] = ((mk >> ((r * 2 + 1) * 4 + e)) & 1ull) && row < tile_rows ? G[r][1][e] : 0.0f;
          }
        }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) { acc[r][0] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; acc[r][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }
    const int dil = __builtin_amdgcn_readfirstlane(sdil[step]);
    const int layer_end = (step + 1) * 36;
    __syncthreads();                                      // the image is complete
    // the forward kernel's entry loop (B2_* at file scope)
    float4 ua[2], ub[2];
    if (it < layer_end) {
      B2_PARAMS(en, delta0, coff0, dbytes0)
      B2_ALOAD(0, ua, delta0, coff0, dbytes0)
      B2_ALOAD(1, ub, delta0, coff0, dbytes0)
    }
    bool odd = false;
    if (rh == 0) {
      while (it < layer_end) {
        B2_ENTRY(ua, ub, bA, bB)
        if (it >= layer_end) { odd = true; break; }
        B2_ENTRY(ub, ua, bB, bA)
      }
    } else {
      while (it < layer_end) {
        B2_ENTRY(ua, ub, bA, bB)
        if (it >= layer_end) { odd = true; break; }
        B2_ENTRY(ua, ub, bB, bA)
      }
    }
    if (odd) { bA[0] = bB[0]; bA[1] = bB[1]; bA[2] = bB[2]; bA[3] = bB[3]; }
    __syncthreads();                                      // every wave is done reading the image
    if (step == 0) {
#pragma unroll
      for (int r = 0; r < NR; ++r) { G[r][0] = acc[r][0]; G[r][1] = acc[r][1]; }
    } else {
      // LayerNorm backward: t = gamma dhn ; dh = rstd (t - mean(t) - xhat mean(t xhat)) ; both row sums in ONE exchange.
      // The saved x-hat comes back here, after the loop (56 coalesced loads in flight at once): held across the MFMA loop it
      // would not fit beside G and the accumulators (256 VGPRs at two waves per SIMD).
      float xh[NR][2][4];
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            xh[r][ct][e] = (16 * (rh + 2 * r) < TW_ROWS) ? sv.xhat[(((size_t)blockIdx.x * nl + layer) * 56 + (r * 2 + ct) * 4 + e) * 512 + tid] : 0.0f;
      const float gm0 = a.gamma[layer * BB_C + col0], gm1 = a.gamma[layer * BB_C + col0 + 16];
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * (rh + 2 * r) + 4 * g + e;
          const float t0 = acc[r][0][e] * gm0, t1 = acc[r][1][e] * gm1;
          acc[r][0][e] = t0; acc[r][1][e] = t1;
          const float s1 = group16_sum(t0 + t1);
          const float s2 = group16_sum(t0 * xh[r][0][e] + t1 * xh[r][1][e]);
          if (j == 0 && row < TW_ROWS) { psum[cg * TW_ROWS + row] = s1; psum[(4 + cg) * TW_ROWS + row] = s2; }
        }
      __syncthreads();
      if (tid < 2 * TW_ROWS) {
        const float* ps = psum + (tid < TW_ROWS ? 0 : 4 * TW_ROWS) + (tid < TW_ROWS ? tid : tid - TW_ROWS);
        rstat[tid] = ((ps[0] + ps[TW_ROWS]) + (ps[2 * TW_ROWS] + ps[3 * TW_ROWS])) * (1.0f / BB_C);
      }
      const float* rsd = sv.rstd + ((size_t)blockIdx.x * nl + layer) * TW_ROWS;
      __syncthreads();
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int rb = min(16 * (rh + 2 * r) + 4 * g, TW_ROWS - 4);
        const float4 m1 = *reinterpret_cast<const float4*>(rstat + rb);
        const float4 m2 = *reinterpret_cast<const float4*>(rstat + TW_ROWS + rb);
        const float4 rs = *reinterpret_cast<const float4*>(rsd + rb);
        const float m1v[4] = {m1.x, m1.y, m1.z, m1.w}, m2v[4] = {m2.x, m2.y, m2.z, m2.w}, rsv[4] = {rs.x, rs.y, rs.z, rs.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          G[r][0][e] += rsv[e] * (acc[r][0][e] - m1v[e] - xh[r][0][e] * m2v[e]);
          G[r][1][e] += rsv[e] * (acc[r][1][e] - m1v[e] - xh[r][1][e] * m2v[e]);
        }
      }
    }
  }
  // ---- the first layer's transpose: (G * relu'_first) -> image -> dx[p][c] = sum_t sum_co W_first[co][c][t] g0[p - (t - 4)][co]
  {
    const unsigned long long mk = sv.mask[(size_t)blockIdx.x * (nl + 2) * 512 + tid];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = 16 * (rh + 2 * r) + 4 * g + e;
        if (row < TW_ROWS) {
          img[row * BB_AP + col0] = ((mk >> ((r * 2) * 4 + e)) & 1ull) && row < tile_rows ? G[r][0][e] : 0.0f;
          img[row * BB_AP + col0 + 16] = ((mk >> ((r * 2 + 1) * 4 + e)) & 1ull) && row < tile_rows ? G[r][1][e] : 0.0f;
        }
      }
  }
  __syncthreads();
  for (int e = tid; e < L * 5; e += 512) {
    const int p = e / 5, c = e - 5 * p;
    float sm = 0.0f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int q = p - (t - 4);
      if (q < 0 || q >= L) continue;
      const float4* hr = reinterpret_cast<const float4*>(img + q * BB_AP);
      const float4* wv = reinterpret_cast<const float4*>(Bs + (t * 5 + c) * BB_C);
#pragma unroll 8
      for (int k = 0; k < BB_C / 4; ++k) {
        const float4 h4 = hr[k], w4 = wv[k];
        sm += h4.x * w4.x + h4.y * w4.y + h4.z * w4.z + h4.w * w4.w;
      }
    }
    a.dx[row0 * 5 + e] = sm;
  }
}

// ---------------------------------------------------- the same forward on SEVERAL workgroups per sequence (round 4) ----
// backbone_kernel takes ~2.1 ms per workgroup whatever the batch: 4 sequences (BASELINE.json configs[0]) used 4 of 256 CUs
// for as long as 256 sequences use all of them. Here R = 2 or 4 workgroups share one sequence (104 < L <= 208), split BY ROWS:
// workgroup q owns the row tiles {2 q, 2 q + 1} + 2 R r (wave (cg, rh): tiles rh + 2 q + 2 R r), all 128 channels of them —
// so the residual stream, the LayerNorm statistics (a row's 128 channels live in one workgroup), the first-layer lookup and
// both 1 x 1 convolutions stay workgroup-local, every accumulator sees the products of backbone_kernel in the same order
// (SAME BITS, tests/test_fused_gpu.py), and the only exchange is the LayerNorm'd image: a dilated tap reads rows up to 256
// away, so each workgroup publishes its 32-row blocks of hn to a global scratch image after the LayerNorm of a layer, the R
// workgroups meet at an agent-scope counter, and each copies the blocks it does not own into its LDS image (106 KB per
// sequence and layer through the L2: the members of a group are given workgroup ids 8 apart = the same XCD). The scratch
// image is double-buffered by layer parity (a fast workgroup may publish layer l + 1 while a slow one still reads layer l).
// All R workgroups of a group must be resident: the launcher only uses this kernel when n R <= CUs.
struct BackboneSplitWs { float* xchg; int* cnt; int* err; int groups; };

template <int R>
__global__ __launch_bounds__(512, 2) void backbone_split_kernel(BackboneArgs a, BackboneSplitWs ws) {
  constexpr int TS = 2 * R;                               // stride of a wave's row tiles
  constexpr int NR = (TW_RT + TS - 1) / TS;               // R = 2: 4 ; R = 4: 2
  static_assert(NR % 2 == 0, "the two A-fragment sets keep their roles from entry to entry");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* img = smem + BB_AP;
  float* Bs = smem + (TW_ROWS + 2) * BB_AP;
  float* psum = Bs + 9 * 5 * BB_C;
  float* rstat = psum + 8 * TW_ROWS;
  int* toks = reinterpret_cast<int*>(rstat + TW_ROWS);
  int* rpos = toks + TW_ROWS;
  int* sdil = rpos + TW_ROWS;
  int* sched = sdil + BB_MAXL + 1;

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cg = w & 3, rh = w >> 2;
  const int j = lane & 15, g = lane >> 4;
  const int col0 = 32 * cg + j;
  const int L = a.L;
  // workgroup -> (group = sequence, member q): the R members of a group sit 8 workgroup ids apart (one XCD, one L2)
  const int bid = blockIdx.x, kq = bid >> 3;
  const int q = kq % R, grp = (kq / R) * 8 + (bid & 7);
  if (grp >= a.n) return;                                 // (the whole group leaves together)
  const int t0 = rh + 2 * q;                              // this wave's row tiles: t0 + TS r
  const int tile_rows = L;
  const int64_t row0 = (int64_t)grp * L;
  const int nl = a.nl;
  const int it_end = (nl + 1) * 36;

  for (int e = tid; e < TW_ROWS; e += 512) {
    toks[e] = e < tile_rows ? (int)a.x[row0 + e] : -1;
    rpos[e] = e < tile_rows ? e : -(1 << 20);
  }
  for (int e = tid; e < BB_AP; e += 512) { smem[e] = 0.0f; img[TW_ROWS * BB_AP + e] = 0.0f; }
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < BB_MAXL; ++i) sdil[i] = a.dil[i];
    sdil[BB_MAXL] = 1;
  }
  for (int e = tid; e < 9 * 5 * BB_C; e += 512) Bs[e] = a.table0[e];
  __syncthreads();
  for (int k = tid; k < it_end; k += 512) {               // the schedule of backbone_kernel<true>
    auto entry = [&](int kk) {
      const int layer = kk / 36, t = kk % 9;
      if (layer >= nl) return t == 4 ? 0x1fff : 0;
      const int d = (t - 4) * sdil[layer];
      const int lo = d < 0 ? -d : 0, hi = d > 0 ? L - d : L;
      if (lo >= hi) return 0;
      int m = 0;
      for (int r = 0; r < TW_RT; ++r) if (lo < 16 * r + 16 && hi > 16 * r) m |= 1 << r;
      return m;
    };
    const int m = entry(k);
    int nx = k + 1;
    while (nx < it_end && entry(nx) == 0) ++nx;
    sched[k] = m ? (m | ((k % 36) / 9) << 13 | (k % 9) << 15 | nx << 19) : 0;
  }

  f32x4 f[NR][2], acc[NR][2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int col = col0 + 16 * ct;
    const float b0 = a.vec[col];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = 16 * (t0 + TS * r) + 4 * g + e;
        float v = b0;
        if (row < TW_ROWS) {
          const int pos = rpos[row];
#pragma unroll
          for (int t = 0; t < 9; ++t) {
            const int pp = pos + t - 4;
            const int tk = (pp >= 0 && pp < L) ? toks[row + t - 4] : -1;
            if (tk >= 0) v += Bs[(t * 5 + tk) * BB_C + col];
          }
        }
        f[r][ct][e] = row < tile_rows ? fmaxf(v, 0.0f) : 0.0f;
      }
  }
  __syncthreads();

  const int arow0 = ((16 * t0 + j) * BB_AP + 8 * g) * 4;
  const int a_lo = arow0 - (16 * t0 + j + 1) * BB_AP * 4;
  const int a_hi = arow0 + (TW_ROWS - 16 * t0 - j) * BB_AP * 4;
  const char* imgb = reinterpret_cast<const char*>(img);
  const float* wsrc = a.tiles + col0 * CH + 8 * g;
  auto tile_of = [&](int k) { return k < nl * 36 ? k : nl * 36 + (k - nl * 36) / 9; };
  int it = 0;
  while (it < it_end && sched[it] == 0) ++it;
  it = __builtin_amdgcn_readfirstlane(it);
  int en = __builtin_amdgcn_readfirstlane(sched[it]);
  float4 bn[4];
  BB_WLOAD(bn, wsrc + (size_t)tile_of(it) * BB_C * CH)
  float* const xg = ws.xchg + (size_t)grp * 2 * TW_ROWS * BB_C;      // this group's two scratch images
  int* const gcnt = ws.cnt + grp;

  for (int layer = 0; layer <= nl; ++layer) {
    const float* vl = a.vec + (size_t)(layer + 1) * 4 * BB_C;
    if (layer < nl) {
      const float tb0 = vl[BB_C + col0], tb1 = vl[BB_C + col0 + 16];
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * (t0 + TS * r) + 4 * g + e;
          const float sm = group16_sum((f[r][0][e] + tb0) + (f[r][1][e] + tb1));
          if (j == 0 && row < TW_ROWS) psum[cg * TW_ROWS + row] = sm;
        }
      __syncthreads();
      if (tid < TW_ROWS)
        rstat[tid] = ((psum[tid] + psum[TW_ROWS + tid]) + (psum[2 * TW_ROWS + tid] + psum[3 * TW_ROWS + tid])) * (1.0f / BB_C);
      __syncthreads();
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const float4 cur4 = *reinterpret_cast<const float4*>(rstat + min(16 * (t0 + TS * r) + 4 * g, TW_ROWS - 4));
        const float mean4[4] = {cur4.x, cur4.y, cur4.z, cur4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * (t0 + TS * r) + 4 * g + e;
          const float mean = mean4[e];
          const float d0 = f[r][0][e] + tb0 - mean, d1 = f[r][1][e] + tb1 - mean;
          acc[r][0][e] = d0; acc[r][1][e] = d1;
          const float sq = group16_sum(d0 * d0 + d1 * d1);
          if (j == 0 && row < TW_ROWS) psum[cg * TW_ROWS + row] = sq;
        }
      }
      __syncthreads();
      if (tid < TW_ROWS)
        rstat[tid] = rsqrtf(((psum[tid] + psum[TW_ROWS + tid]) + (psum[2 * TW_ROWS + tid] + psum[3 * TW_ROWS + tid])) *
                            (1.0f / BB_C) + 1e-5f);
      __syncthreads();
      const float gm0 = vl[2 * BB_C + col0], gm1 = vl[2 * BB_C + col0 + 16];
      const float bt0 = vl[3 * BB_C + col0], bt1 = vl[3 * BB_C + col0 + 16];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const float4 cur4 = *reinterpret_cast<const float4*>(rstat + min(16 * (t0 + TS * r) + 4 * g, TW_ROWS - 4));
        const float rs4[4] = {cur4.x, cur4.y, cur4.z, cur4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * (t0 + TS * r) + 4 * g + e;
          if (row < TW_ROWS) {
            const float rs = rs4[e];
            img[row * BB_AP + col0] = row < tile_rows ? acc[r][0][e] * rs * gm0 + bt0 : 0.0f;
            img[row * BB_AP + col0 + 16] = row < tile_rows ? acc[r][1][e] * rs * gm1 + bt1 : 0.0f;
          }
        }
      }
      // ---- exchange of the LayerNorm'd image: publish the 32-row blocks this workgroup owns (blocks q, q + R, ...), meet,
      //      fetch the others'. 32 float4 per row; one row per 32 lanes.
      __syncthreads();
      float* const xb = xg + (size_t)(layer & 1) * TW_ROWS * BB_C;
      // The scratch image is written and read with SYSTEM-SCOPE accesses (sc0 sc1: write-through to memory, reads past every
      // cache) and the counter with relaxed agent-scope atomics. The first version used ordinary stores / loads between
      // __threadfence()s: an agent-scope release / acquire on this part writes back and invalidates the XCD's whole L2 — the
      // 13 MB of weights every workgroup streams from it went with it, 25 us per layer (B = 64: slower than one workgroup per
      // sequence). Nothing but these 106 KB per layer needs to be coherent between the workgroups.
      for (int e = tid; e < NR * 32 * 32; e += 512) {
        const int c4 = e & 31, rr = e >> 5;
        const int row = 32 * (q + R * (rr >> 5)) + (rr & 31);
        if (row < TW_ROWS) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(img + row * BB_AP + 4 * c4);
          asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" :: "v"(xb + (size_t)row * BB_C + 4 * c4), "v"(v) : "memory");
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // this thread's blocks have reached memory
      __syncthreads();
      if (tid == 0) {
        __hip_atomic_fetch_add(gcnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int target = R * (layer + 1);
        int spins = 0;
        // (once a barrier of this launch has timed out the launch's results are void — svdd_backbone_split_status reports it, the
        //  samplers raise — and the remaining layers do not wait again)
        while (__hip_atomic_load(gcnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
          __builtin_amdgcn_s_sleep(1);
          if ((++spins & 0xFFF) == 0 && __hip_atomic_load(ws.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
          if (spins > (1 << 24)) { __hip_atomic_store(ws.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }  // a member is not resident: give up, never hang
        }
      }
      __syncthreads();
      // every foreign block of the image in ONE batch of loads per lane (14 slots of 512 lanes x 16 B cover the 208 x 512 B
      // image; the slots of the blocks this workgroup owns stay empty): one memory latency per layer, not one per four loads
      {
        f32x4 v[14];
        bool ok[14];
#define S_XLD(K)                                                                                             \
        { const int e_ = (K) * 512 + tid; const int row_ = e_ >> 5;                                          \
          ok[K] = row_ < TW_ROWS && ((row_ >> 5) % R) != q;                                                  \
          v[K] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};                                                              \
          if (ok[K]) asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=v"(v[K]) : "v"(xb + (size_t)row_ * BB_C + 4 * (e_ & 31)) : "memory"); }
        S_XLD(0) S_XLD(1) S_XLD(2) S_XLD(3) S_XLD(4) S_XLD(5) S_XLD(6) S_XLD(7) S_XLD(8) S_XLD(9) S_XLD(10) S_XLD(11) S_XLD(12) S_XLD(13)
#undef S_XLD
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]),
                     "+v"(v[8]), "+v"(v[9]), "+v"(v[10]), "+v"(v[11]), "+v"(v[12]), "+v"(v[13]) :: "memory");
#pragma unroll
        for (int k = 0; k < 14; ++k) {
          const int e_ = k * 512 + tid;
          if (ok[k]) *reinterpret_cast<f32x4*>(img + (e_ >> 5) * BB_AP + 4 * (e_ & 31)) = v[k];
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * (t0 + TS * r) + 4 * g + e;
          if (row < TW_ROWS) { img[row * BB_AP + col0] = f[r][0][e]; img[row * BB_AP + col0 + 16] = f[r][1][e]; }
        }
    }
    const float bl0 = vl[col0], bl1 = vl[col0 + 16];
#pragma unroll
    for (int r = 0; r < NR; ++r) { acc[r][0] = f32x4{bl0, bl0, bl0, bl0}; acc[r][1] = f32x4{bl1, bl1, bl1, bl1}; }
    const int dil = __builtin_amdgcn_readfirstlane(sdil[layer < nl ? layer : BB_MAXL]);
    const int layer_end = (layer + 1) * 36;
    __syncthreads();                                      // the image is complete
#define S_ALOAD(R_, V, COFF, DBYTES)                                                                         \
      { const int o_ = min(max(arow0 + (DBYTES) + (R_) * (16 * TS * BB_AP * 4), a_lo + (COFF)), a_hi + (COFF)); \
        const float4* ap_ = reinterpret_cast<const float4*>(imgb + o_);                                      \
        V[0] = ap_[0]; V[1] = ap_[1]; }
#define S_MM(R_, U)                                                                                          \
      __builtin_amdgcn_sched_barrier(0);                                                                     \
      __builtin_amdgcn_s_waitcnt(0xC07F | (2 << 8));      /* at least two LDS reads (the other set's) were issued after U's */ \
      BB_MM16(acc[R_], U, live & (1 << (TS * (R_))))                                                         \
      __builtin_amdgcn_sched_barrier(0);
#define S_PARAMS(EN, COFF, DBYTES)                                                                           \
      const int COFF = (((EN) >> 13) & 3) * (CH * 4);                                                        \
      const int DBYTES = ((((EN) >> 15) & 15) - 4) * dil * (BB_AP * 4) + COFF;
    float4 ua[2], ub[2];
    if (it < layer_end) {
      S_PARAMS(en, coff0, dbytes0)
      S_ALOAD(0, ua, coff0, dbytes0)
      S_ALOAD(1, ub, coff0, dbytes0)
    }
    while (it < layer_end) {
      const int nxt = en >> 19;
      const int en_next_v = sched[nxt < it_end ? nxt : it];
      BB_UNPACK(bn)
      if (nxt < it_end) BB_WLOAD(bn, wsrc + (size_t)tile_of(nxt) * BB_C * CH)
      S_PARAMS(en, coff, dbytes)
      const int live = (en & 0x1fff) >> t0;               // bit TS r = owned tile r (tiles >= 13 do not exist)
      S_MM(0, ua)
      const int en2 = __builtin_amdgcn_readfirstlane(en_next_v);
      S_PARAMS(en2, coff2, dbytes2)
      if constexpr (NR == 2) {
        S_ALOAD(0, ua, coff2, dbytes2)
        S_MM(1, ub)
        S_ALOAD(1, ub, coff2, dbytes2)
      } else {
        S_ALOAD(2, ua, coff, dbytes)
        S_MM(1, ub)
        S_ALOAD(3, ub, coff, dbytes)
        S_MM(2, ua)
        S_ALOAD(0, ua, coff2, dbytes2)
        S_MM(3, ub)
        S_ALOAD(1, ub, coff2, dbytes2)
      }
      it = nxt;
      en = en2;
    }
#undef S_PARAMS
#undef S_MM
#undef S_ALOAD
    __syncthreads();
    if (layer < nl) {
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
          for (int e = 0; e < 4; ++e) f[r][ct][e] = fmaxf(acc[r][ct][e], 0.0f) + f[r][ct][e];
    } else {
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * (t0 + TS * r) + 4 * g + e;
          if (row < TW_ROWS) {
            img[row * BB_AP + col0] = fmaxf(acc[r][0][e], 0.0f);
            img[row * BB_AP + col0 + 16] = fmaxf(acc[r][1][e], 0.0f);
          }
        }
    }
  }
  __syncthreads();
  // ---- last 1x1 conv 128 -> 5 on the rows this workgroup owns
  for (int e = tid; e < NR * 32 * 5; e += 512) {
    const int rr = e / 5, v = e - 5 * rr;
    const int row = 32 * (q + R * (rr >> 5)) + (rr & 31);
    if (row >= tile_rows) continue;
    const float* hr = img + row * BB_AP;
    const float* wv = a.w2 + v * BB_C;
    float sm = a.w2[5 * BB_C + v];
#pragma unroll 8
    for (int k = 0; k < BB_C; ++k) sm += hr[k] * wv[k];
    a.out[(row0 + row) * 5 + v] = sm;
  }
}

// ------------------------------------------------------- value-net tail: everything after the GRU in one pass ----
// score[n][t] = b_eff[t] + mean_l sum_c w_eff[c][t] * relu(b1[c] + sum_k W1[c][k] * LayerNorm(h_fwd + h_bwd)[n][l][k])
// (reference Enformer.py:1617 direction sum, :2010-2047 FeedForwardBlock LayerNorm -> Linear 64->128 -> ReLU ->
//  Linear 128->64, :2131-2173 ConvHead 1x1 conv + mean over length; the last two linear maps are collapsed and the
//  LayerNorm affine is folded into (W1, b1) by the host).
// Replaces epilogue_ln + 2 GEMMs + ReLU + mean: those moved 1.3 GB through HBM per value forward (n = 2560, L = 200);
// this reads the two GRU outputs once (262 MB) and writes n*T floats. One wave per sequence; 16-row tiles; the
// 64 -> 128 map runs on the exact-fp32 matrix cores with W1 held in registers as MFMA B operands; LayerNorm statistics
// are two-pass across the 4 lanes of a row. The next tile's rows are loaded RAW into registers under the current
// tile's MFMAs and only summed when their turn comes (summing at load time would park the wave on the loads).
template <int T>
__global__ __launch_bounds__(256, 2) void value_tail_kernel(const float* __restrict__ hf, const float* __restrict__ hb,
                                                            const float* __restrict__ w1pack, const float* __restrict__ b1,
                                                            const float* __restrict__ weff, const float* __restrict__ beff,
                                                            float* __restrict__ out, int n_alloc, int L,
                                                            const int* __restrict__ count) {
  // b1' and w_eff per output column, [j][8 ct | 8 ct x T]: read from LDS every tile (lgkmcnt, not the row prefetch's vmcnt) instead of
  // living in 8 + 8 T registers — with W1' (128), the accumulators (32) and two row sets the kernel sat at the 256-register limit and
  // spilled its lane offsets, reloading them from scratch every tile.
  __shared__ __attribute__((aligned(16))) float colv[16][8 + 8 * T];
  for (int e = threadIdx.x; e < 16 * (8 + 8 * T); e += 256) {
    const int jj = e / (8 + 8 * T), r = e - jj * (8 + 8 * T);
    colv[jj][r] = r < 8 ? b1[16 * r + jj] : weff[(16 * ((r - 8) / T) + jj) * T + (r - 8) % T];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int seq = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));   // wave-uniform: the row bases stay in SGPRs
  const int n = count ? *count : n_alloc;
  if (seq >= n) return;
  const int j = lane & 15, g = lane >> 4;
  // channel of this lane's value i (= MFMA k-step i): ch(i) = 16 (i / 4) + 4 g + (i % 4) — four 16-byte pieces that,
  // across the 4 lanes of a row, make each load instruction cover whole 64-byte segments
  float wb[128];                                           // wb[16 ct + s] = W1'[16 ct + j][ch(s)]
  {
    const float4* wp = reinterpret_cast<const float4*>(w1pack + (size_t)lane * 128);
#pragma unroll
    for (int i = 0; i < 32; ++i) { const float4 v = wp[i]; wb[4 * i] = v.x; wb[4 * i + 1] = v.y; wb[4 * i + 2] = v.z; wb[4 * i + 3] = v.w; }
  }
  // Round 6: the operands above are PINNED here (they must have arrived before the loop). Left pending, their loads share the
  // in-order vmcnt counter with the row prefetches, and the compiler's conservative waits inside the loop (s_waitcnt vmcnt(3..1) in
  // the middle of the MFMA block) drained each tile's prefetch a third of the way into the tile it was meant to fly under.
#pragma unroll
  for (int i = 0; i < 128; ++i) asm volatile("" : "+v"(wb[i]));
  float part[T];
#pragma unroll
  for (int t = 0; t < T; ++t) part[t] = 0.0f;
  const float* sf = hf + (size_t)seq * L * 64;             // scalar bases + a 32-bit lane offset (L * 64 floats < 2^31 bytes per sequence)
  const float* sb = hb + (size_t)seq * L * 64;
  const int ntiles = (L + 15) / 16;
  float4 xa[4], xb[4];
  auto load_rows = [&](int tile) {
    const int off = min(16 * tile + j, L - 1) * 64 + 4 * g;   // rows past the end re-read the last row; masked below
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xa[i] = *reinterpret_cast<const float4*>(sf + off + 16 * i);
      xb[i] = *reinterpret_cast<const float4*>(sb + off + 16 * i);
    }
  };
  load_rows(0);
  for (int tile = 0; tile < ntiles; ++tile) {
    float v[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[4 * i] = xa[i].x + xb[i].x; v[4 * i + 1] = xa[i].y + xb[i].y;
      v[4 * i + 2] = xa[i].z + xb[i].z; v[4 * i + 3] = xa[i].w + xb[i].w;
    }
    // the next tile's loads go into the registers the sums above just freed (hoisted above the sums, as the scheduler would, they
    // need a second set of 32 registers + 32 copies per tile, and that spilled the row pointers into scratch inside the loop)
    __builtin_amdgcn_sched_barrier(0);
    load_rows(min(tile + 1, ntiles - 1));                 // fly under the LayerNorm and the 128 MFMAs below (unconditional: a branch
    __builtin_amdgcn_sched_barrier(0);                    // here becomes a block of its own, placed BEFORE the sums; the last tile re-reads itself)
    // LayerNorm (no affine: folded into W1', b1') over the 64 channels of row 16 tile + j: 16 here, 48 in lanes j + 16 g'
    float sm = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) sm += v[i];
    sm += __shfl_xor(sm, 16, 64); sm += __shfl_xor(sm, 32, 64);
    const float mean = sm * (1.0f / 64.0f);
    float sq = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { v[i] -= mean; sq += v[i] * v[i]; }
    sq += __shfl_xor(sq, 16, 64); sq += __shfl_xor(sq, 32, 64);
    const float rstd = rsqrtf(sq * (1.0f / 64.0f) + 1e-5f);
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] *= rstd;
    int jj = j;
    asm volatile("" : "+v"(jj));                           // opaque per tile: the LDS reads stay in the loop (the INDEX, not the pointer:
    const float* cv = colv[jj];                            // a laundered pointer turns generic and its flat loads wait on vmcnt too)
    f32x4 acc[8];
#pragma unroll
    for (int ct = 0; ct < 8; ++ct) { const float b = cv[ct]; acc[ct] = f32x4{b, b, b, b}; }
#pragma unroll
    for (int sidx = 0; sidx < 16; ++sidx)
#pragma unroll
      for (int ct = 0; ct < 8; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[sidx], wb[16 * ct + sidx], acc[ct], 0, 0, 0);
    // C/D layout: reg rho -> row 4 g + rho, column 16 ct + j
    constexpr bool HOIST = T <= 3;                         // w_eff of this lane's columns: one LDS read per tile, not one per row
    float wl[HOIST ? 8 * T : 1];                           // (T = 4: 32 more registers would spill; read per row there)
    if constexpr (HOIST) {
#pragma unroll
      for (int i = 0; i < 8 * T; ++i) wl[i] = cv[8 + i];
    }
#pragma unroll
    for (int rho = 0; rho < 4; ++rho) {
      if (16 * tile + 4 * g + rho < L) {
#pragma unroll
        for (int ct = 0; ct < 8; ++ct) {
          const float z = fmaxf(acc[ct][rho], 0.0f);
#pragma unroll
          for (int t = 0; t < T; ++t) part[t] += z * (HOIST ? wl[ct * T + t] : cv[8 + ct * T + t]);
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const float tot = wave_sum(part[t]);
    if (lane == 0) out[(size_t)seq * T + t] = tot / (float)L + beff[t];
  }
}

}  // namespace

static int g_fixed_spt = 0;        // svdd_set_backbone_packing: 1 = always fill the 208-row tile (round-1 behaviour), -s = exactly
                                   // s sequences per tile (calibration of svdd_spt.h), 0 = choose (default)
extern "C" int svdd_set_backbone_packing(int full) { g_fixed_spt = full; return SVDD_OK; }
extern "C" int svdd_internal_fixed_spt() { return g_fixed_spt; }
extern "C" int svdd_internal_num_cus() {
  static int ncu = 0;
  if (!ncu) {
    hipDeviceProp_t prop;
    int dev = 0;
    ncu = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ? prop.multiProcessorCount : 256;
  }
  return ncu;
}

static int g_gru_mode = 0;         // 0 / 4: producer-consumer kernel (default) ; 1: one wave does both halves ; 2: both
                                   // directions per workgroup ; 3: mode 1 with an LDS reservation (experiments, A/B tests)
extern "C" int svdd_gru_set_mode(int mode) { g_gru_mode = mode; return SVDD_OK; }

extern "C" int svdd_gru_bidir_f32(const float* x, const float* wpack, const float* bpack, float* out, int n, int L,
                                  const int32_t* count, void* stream) {
  if (!x || !wpack || !bpack || !out || n <= 0 || L <= 0) return SVDD_E_ARG;
  SvddSpan span(SVDD_SLOT_GRU);
  // both directions per workgroup when that fills the chip evenly (<= 16 sequences per CU); else one direction each
  const int per_cu = (n + 255) / 256;
  const dim3 grid_dirs(2 * (unsigned)((n + TS - 1) / TS));   // one workgroup per (tile of TS sequences, direction)
  if (g_gru_mode == 0 || g_gru_mode == 4)            // default: producer / consumer waves (same bits as mode 1)
    return svdd_launch_timed(span.all(), gru_pc_kernel, grid_dirs, dim3(512), 0, stream, x, wpack, bpack, out, n, L, count);
  if (g_gru_mode == 2 && per_cu <= TS && n >= 256)   // measured slower (841 vs 758 us at n=2560, L=200): opt-in only
    return svdd_launch_timed(span.all(), gru_bidir_kernel<true>, dim3((unsigned)((n + per_cu - 1) / per_cu)), dim3(512), 0, stream, x,
                             wpack, bpack, out, n, L, per_cu, count);
  // (Reserving > 80 KB of dynamic LDS to force one workgroup per CU was measured: 2560 sequences = 320 units take
  //  749 us in two exclusive rounds against 678 us shared, and <= 256 units spread over the CUs by themselves: 367 us
  //  either way. Kept as mode 3 for the record.)
  const SvddLds pad = g_gru_mode == 3 ? svdd_lds_raised(84 * 1024) : SvddLds(0);
  return svdd_launch_timed(span.all(), gru_bidir_kernel<false>, grid_dirs, dim3(256), pad, stream, x, wpack, bpack, out, n, L, TS, count);
}

extern "C" int svdd_epilogue_ln_f32(const float* y, const float* bias, const float* f_prev, const float* tb,
                                    const float* gamma, const float* beta, float* f_out, float* hn, int64_t rows,
                                    int channels, int act, void* stream) {
  if (!y || (!f_out && !hn) || rows <= 0 || (hn && (!gamma || !beta)) || act < 0 || act > 2 ||
      (channels != 64 && channels != 128 && channels != 256))
    return SVDD_E_ARG;
  EpiArgs a{y, bias, f_prev, tb, gamma, beta, f_out, hn, rows, act};
  const int64_t nblocks = (rows + 3) / 4;
  const unsigned grid = (unsigned)(nblocks < 4096 ? nblocks : 4096);
  void (*kern)(EpiArgs);
  if (channels == 64) kern = epilogue_ln_kernel<1>;
  else if (channels == 128) kern = epilogue_ln_kernel<2>;
  else kern = epilogue_ln_kernel<4>;
  SvddSpan span(SVDD_SLOT_EPILOGUE_LN);
  return svdd_launch_timed(span.all(), kern, dim3(grid), dim3(256), 0, stream, a);
}

static int g_tower_ver = 0;        // svdd_set_tower_version: 0 = default (= 3), 1 = first generation, 2 / 3 = second generation
extern "C" int svdd_set_tower_version(int v) { g_tower_ver = v; return SVDD_OK; }   // with 2 / 1 column tiles per wave

static int g_conv_dynamic = 0;     // tests: force the dynamically scheduled kernel
extern "C" int svdd_conv1d_set_dynamic(int on) { g_conv_dynamic = on; return SVDD_OK; }

typedef void (*ConvKernel)(ConvArgs);
// the 128 -> 128 x 9 taps kernel compiled for (dilation, L), or nullptr where there is none
static ConvKernel conv128_static_kernel(int dilation, int L) {
  if (dilation == 1 && L == 200) return conv1d_cl_static_kernel<128, 128, 9, 1, 200>;
  if (dilation == 4 && L == 200) return conv1d_cl_static_kernel<128, 128, 9, 4, 200>;
  if (dilation == 16 && L == 200) return conv1d_cl_static_kernel<128, 128, 9, 16, 200>;
  if (dilation == 64 && L == 200) return conv1d_cl_static_kernel<128, 128, 9, 64, 200>;
  if (dilation == 1 && L == 50) return conv1d_cl_static_kernel<128, 128, 9, 1, 50>;
  if (dilation == 4 && L == 50) return conv1d_cl_static_kernel<128, 128, 9, 4, 50>;
  if (dilation == 16 && L == 50) return conv1d_cl_static_kernel<128, 128, 9, 16, 50>;
  if (dilation == 64 && L == 50) return conv1d_cl_static_kernel<128, 128, 9, 64, 50>;
  return nullptr;
}
static size_t conv_lds_bytes(int cout) { return sizeof(float) * ((size_t)(CONV_ROWS + 1) * CHP + 2 * (size_t)cout * CHP); }

extern "C" int svdd_conv1d_cl_f32(const float* x, const float* wpack, float* y, int n, int L, int cin, int cout,
                                  int taps, int dilation, const float* bias, const float* f_prev, int act,
                                  const float* tb, const float* gamma, const float* beta, float* hn, void* stream) {
  if (!x || !wpack || !y || n <= 0 || L <= 0 || L > CONV_ROWS || taps <= 0 || !(taps & 1) || dilation <= 0 ||
      act < -1 || act > 2 || (hn && (act < 0 || !gamma || !beta)))
    return SVDD_E_ARG;
  const bool dyn = g_conv_dynamic != 0;
  ConvKernel kern = nullptr;                                   // a statically scheduled kernel where one was compiled for the shape ...
  if (!dyn && cin == 128 && cout == 128 && taps == 9 && (L == 200 || L == 50)) kern = conv128_static_kernel(dilation, L);
  if (!kern && !dyn && cin == 64 && cout == 64 && taps == 5 && dilation == 1 && (L == 200 || L == 50))
    kern = L == 200 ? conv1d_cl_static_kernel<64, 64, 5, 1, 200> : conv1d_cl_static_kernel<64, 64, 5, 1, 50>;
  if (!kern) {                                                 // ... else the generic one
    if (act >= 0) return SVDD_E_ARG;                           // the generic kernel has no fused epilogue
    if (cin == 128 && cout == 128) kern = conv1d_cl_kernel<128, 128>;
    else if (cin == 64 && cout == 64) kern = conv1d_cl_kernel<64, 64>;
    else if (cin == 64 && cout == 128) kern = conv1d_cl_kernel<64, 128>;
    else if (cin == 128 && cout == 64) kern = conv1d_cl_kernel<128, 64>;
    else return SVDD_E_ARG;
  }
  const int spt = CONV_ROWS / L;                               // whole sequences per workgroup tile
  ConvArgs a{x, wpack, y, n, L, spt, taps, dilation, bias, f_prev, act, tb, gamma, beta, hn};
  SvddSpan span(SVDD_SLOT_CONV1D);
  return svdd_launch_timed(span.all(), kern, dim3((unsigned)((n + spt - 1) / spt)), dim3(256), svdd_lds_raised(conv_lds_bytes(cout)), stream, a);
}

// y = gate > 0 ? conv(x) + f_prev : 0 — one layer of the reward tower's BACKWARD pass (DPS): x = the gradient at this layer's
// pre-activation, wpack = the transposed / flipped taps, f_prev = the residual branch's gradient (NULL: none), gate = the forward
// activation of the layer BELOW (its ReLU decides where the gradient passes; NULL: no gating). 64 -> 64 x 5 taps, L = 200 / 50 only.
extern "C" int svdd_conv1d_cl_gated_f32(const float* x, const float* wpack, float* y, int n, int L, int cin, int cout, int taps,
                                        int dilation, const float* f_prev, const float* gate, void* stream) {
  if (!x || !wpack || !y || n <= 0 || cin != 64 || cout != 64 || taps != 5 || dilation != 1 || (L != 200 && L != 50)) return SVDD_E_ARG;
  const int spt = CONV_ROWS / L;
  ConvArgs a{x, wpack, y, n, L, spt, taps, dilation, nullptr, f_prev, gate ? 3 : 2, gate, nullptr, nullptr, nullptr};
  ConvKernel kern = L == 200 ? conv1d_cl_static_kernel<64, 64, 5, 1, 200> : conv1d_cl_static_kernel<64, 64, 5, 1, 50>;
  SvddSpan span(SVDD_SLOT_CONV1D);
  return svdd_launch_timed(span.all(), kern, dim3((unsigned)((n + spt - 1) / spt)), dim3(256), svdd_lds_raised(conv_lds_bytes(64)), stream, a);
}

// dynamic LDS of the second-generation tower (conv_tower2_kernel), whole sequences and windows
static size_t tower2_lds_bytes() { return sizeof(float) * ((size_t)(TW_ROWS + 2) * TW_AP + (size_t)(TW_ROWS + 16) * 4); }

extern "C" int svdd_conv_tower_f32(const float* onehot, const float* tiles, const float* bias, float* out, int n, int L,
                                   int nlayers, int residual_mask, const int32_t* count, void* stream) {
  if (!onehot || !tiles || !bias || !out || n <= 0 || L <= 0 || L > TW_ROWS || nlayers <= 0 || nlayers > TW_MAXL)
    return SVDD_E_ARG;
  const int spt = TW_ROWS / L;
  TowerArgs a{onehot, tiles, bias, out, n, L, spt, nlayers, residual_mask, count};
  SvddSpan span(SVDD_SLOT_CONV_TOWER);
  const dim3 grid((unsigned)((n + spt - 1) / spt));
  if (g_tower_ver != 1) {
    TowerWinArgs wa{a, nullptr, nullptr, 1, nullptr, nullptr};
    void (*kern)(TowerWinArgs);
    if (g_tower_ver == 2) kern = spt == 1 ? conv_tower2_kernel<true, false, 2> : conv_tower2_kernel<false, false, 2>;
    else kern = spt == 1 ? conv_tower2_kernel<true, false, 1> : conv_tower2_kernel<false, false, 1>;
    return svdd_launch_timed(span.all(), kern, grid, dim3(512), svdd_lds_raised(tower2_lds_bytes()), stream, wa);
  }
  const size_t lds = sizeof(float) * ((size_t)(TW_ROWS + 2) * TW_AP + (size_t)(TW_ROWS + 2) * 4);
  return svdd_launch_timed(span.all(), spt == 1 ? conv_tower_kernel<true> : conv_tower_kernel<false>, grid, dim3(512),
                           svdd_lds_raised(lds), stream, a);
}

// Scratch of backbone_split_kernel, owned by the caller (the library never allocates): `bytes` of device memory =
// groups * (2 * 208 * 128 floats) for the double-buffered LayerNorm images + groups + 1 ints (arrival counters, error flag).
// One workspace per process: launches that use it must not overlap (the engine issues its backbone forwards on one stream).
static BackboneSplitWs g_bb_ws = {nullptr, nullptr, nullptr, 0};
static int g_bb_split = 0;            // svdd_set_option(SVDD_OPT_BACKBONE_SPLIT): 0 auto, 1 off, 2 / 4 force R where it fits
extern "C" void svdd_internal_set_bb_split(int v) { g_bb_split = (v == 1 || v == 2 || v == 4) ? v : 0; }
extern "C" int svdd_backbone_set_workspace(void* ws, long long bytes) {
  const long long per = (long long)2 * TW_ROWS * BB_C * sizeof(float) + sizeof(int);
  if (!ws || bytes < per + (long long)sizeof(int)) { g_bb_ws = {nullptr, nullptr, nullptr, 0}; return ws ? SVDD_E_ARG : SVDD_OK; }
  const int groups = (int)((bytes - (long long)sizeof(int)) / per);
  g_bb_ws.xchg = reinterpret_cast<float*>(ws);
  g_bb_ws.cnt = reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + (size_t)groups * 2 * TW_ROWS * BB_C * sizeof(float));
  g_bb_ws.err = g_bb_ws.cnt + groups;
  g_bb_ws.groups = groups;
  return hipMemset(g_bb_ws.err, 0, sizeof(int)) == hipSuccess ? SVDD_OK : SVDD_E_LAUNCH;
}
// 0 = every group barrier of every split launch so far was met; 1 = one timed out (results of that launch are invalid). Synchronises.
extern "C" int svdd_backbone_split_status(int* err_out) {
  if (!err_out) return SVDD_E_ARG;
  *err_out = 0;
  if (!g_bb_ws.err) return SVDD_OK;
  // the split launches may sit on ANY stream (the caller passes its own): a blocking hipMemcpy orders only against the null stream
  // and blocking streams, so a launch on a non-blocking stream could still be running — and its time-out would surface one decode late
  if (hipDeviceSynchronize() != hipSuccess) return SVDD_E_LAUNCH;
  if (hipMemcpy(err_out, g_bb_ws.err, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return SVDD_E_LAUNCH;
  if (*err_out && hipMemset(g_bb_ws.err, 0, sizeof(int)) != hipSuccess) return SVDD_E_LAUNCH;   // reported once, then cleared
  return SVDD_OK;
}

// What every fp32 backbone entry sets the same way: the nets' tensors, the shape, `spt` sequences in every tile, the dilations; no
// device-side row count or index list, no carried planes (the entries that have them set them afterwards). false: a dilation <= 0.
static bool backbone_args(BackboneArgs& a, const uint8_t* x, const float* table0, const float* tiles, const float* vec, const float* w2,
                          float* out, int n, int L, int spt, int nlayers, const int* dilations) {
  if (!svdd_fill_dilations(a.dil, dilations, nlayers)) return false;
  a.x = x; a.table0 = table0; a.tiles = tiles; a.vec = vec; a.w2 = w2; a.out = out;
  a.n = n; a.L = L; a.spt = spt; a.nl = nlayers; a.count = nullptr; a.row_idx = nullptr; a.out_scatter = 0;
  a.auto_spt = 0; a.ncu = svdd_internal_num_cus(); a.plan = SvddTilePlan{spt, 0, spt};   // every tile full (one sequence per tile: never read)
  a.planes = nullptr; a.planes_P = 0;
  return true;
}
// Dynamic LDS of the one-launch backbone kernels: the image, the first layer's table, the LayerNorm partial sums, `row_stats` per-row
// arrays (3 in the forward kernels, 2 in backbone_grad_kernel), the dilations and the schedule of (nlayers + 1) x 36 weight tiles.
static size_t backbone_lds_bytes(int nlayers, int row_stats) {
  return sizeof(float) * ((size_t)(TW_ROWS + 2) * BB_AP + 9 * 5 * (size_t)BB_C + 8 * (size_t)TW_ROWS + (size_t)row_stats * TW_ROWS +
                          BB_MAXL + 1 + (size_t)(nlayers + 1) * 36);
}

// DPS: the forward that also saves what the gradient kernel needs, and the gradient kernel (one launch each way)
extern "C" int svdd_backbone_cnn_save_f32(const uint8_t* x, const float* table0, const float* tiles, const float* vec,
                                          const float* w2, float* out, int n, int L, int nlayers, const int* dilations,
                                          float* xhat, float* rstd, unsigned long long* mask, void* stream) {
  if (!x || !table0 || !tiles || !vec || !w2 || !out || !dilations || !xhat || !rstd || !mask || n <= 0 || L <= TW_ROWS / 2 ||
      L > TW_ROWS || nlayers <= 0 || nlayers > BB_MAXL)
    return SVDD_E_ARG;
  BackboneArgs a;
  if (!backbone_args(a, x, table0, tiles, vec, w2, out, n, L, 1, nlayers, dilations)) return SVDD_E_ARG;
  SvddSpan span(SVDD_SLOT_BACKBONE);
  return svdd_launch_timed(span.all(), backbone_kernel<true, true>, dim3((unsigned)n), dim3(512), svdd_lds_raised(backbone_lds_bytes(nlayers, 3)),
                           stream, a, BackboneSave{xhat, rstd, mask});
}

extern "C" int svdd_backbone_cnn_grad_f32(const float* dlogits, const float* tiles_bwd, const float* gamma, const float* w2,
                                          const float* table0, const float* xhat, const float* rstd, const unsigned long long* mask,
                                          float* dx, int n, int L, int nlayers, const int* dilations, void* stream) {
  if (!dlogits || !tiles_bwd || !gamma || !w2 || !table0 || !xhat || !rstd || !mask || !dx || !dilations || n <= 0 ||
      L <= TW_ROWS / 2 || L > TW_ROWS || nlayers <= 0 || nlayers > BB_MAXL)
    return SVDD_E_ARG;
  BackboneGradArgs a;
  if (!svdd_fill_dilations(a.dil, dilations, nlayers)) return SVDD_E_ARG;
  a.dlogits = dlogits; a.tiles = tiles_bwd; a.gamma = gamma; a.w2 = w2; a.table0 = table0; a.dx = dx;
  a.n = n; a.L = L; a.nl = nlayers;
  SvddSpan span(SVDD_SLOT_BACKBONE_GRAD);
  return svdd_launch_timed(span.all(), backbone_grad_kernel, dim3((unsigned)n), dim3(512), svdd_lds_raised(backbone_lds_bytes(nlayers, 2)),
                           stream, a, BackboneSave{const_cast<float*>(xhat), const_cast<float*>(rstd), const_cast<unsigned long long*>(mask)});
}

extern "C" int svdd_backbone_cnn_f32(const uint8_t* x, const float* table0, const float* tiles, const float* vec,
                                     const float* w2, float* out, int n, int L, int nlayers, const int* dilations,
                                     const int32_t* count, const int32_t* row_idx, int out_scatter, void* stream) {
  if (!x || !table0 || !tiles || !vec || !w2 || !out || !dilations || n <= 0 || L <= 0 || L > TW_ROWS ||
      nlayers <= 0 || nlayers > BB_MAXL)
    return SVDD_E_ARG;
  BackboneArgs a;
  if (!backbone_args(a, x, table0, tiles, vec, w2, out, n, L, TW_ROWS / L, nlayers, dilations)) return SVDD_E_ARG;
  a.count = count; a.row_idx = row_idx; a.out_scatter = out_scatter;
  unsigned nwg = (unsigned)((n + a.spt - 1) / a.spt);
  if (a.spt > 1 && g_fixed_spt <= 0) {                   // several sequences fit a tile: which tile takes how many (svdd_spt.h)
    if (g_fixed_spt < 0) { a.spt = -g_fixed_spt < a.spt ? -g_fixed_spt : a.spt; a.plan = SvddTilePlan{a.spt, 0, a.spt}; nwg = (unsigned)((n + a.spt - 1) / a.spt); }
    else if (count) { a.auto_spt = 1; nwg = (unsigned)n; }   // decided on the device from *count; grid for one sequence per tile
    else { a.plan = svdd_plan_tiles(n, L, a.ncu, 9); a.spt = a.plan.s2; nwg = (unsigned)svdd_plan_num_tiles(a.plan, n); }
  }
  const SvddLds lds = svdd_lds_raised(backbone_lds_bytes(nlayers, 3));
  SvddSpan span(SVDD_SLOT_BACKBONE);
  SvddEvents ev = span.all();
  // Small batches of one-sequence tiles: R = 2 / 4 workgroups per sequence (backbone_split_kernel; same bits). Needs the scratch
  // image of svdd_backbone_set_workspace, a row count known on the host (no device-side count / index list) and n R <= CUs
  // (every member of a group must be resident: they wait for each other).
  if (a.spt == 1 && !a.auto_spt && TW_ROWS / L == 1 && !count && !row_idx && g_bb_ws.xchg && g_bb_split != 1) {
    // ... and the TAIL ROUND of a batch that is not a multiple of the CU count (257 .. 384 sequences took two full rounds of
    // one-workgroup tiles): whole rounds on backbone_kernel, the remainder — when it is at most half a round — split.
    const int rem = n % a.ncu, n_main = n - rem;
    const int ns = n_main == 0 ? n : rem;                 // sequences that go to the split kernel
    int R = g_bb_split == 2 || g_bb_split == 4 ? g_bb_split : (4 * ns <= a.ncu ? 4 : 2 * ns <= a.ncu ? 2 : 1);
    if (ns > 0 && R > 1 && (int64_t)R * ns <= a.ncu && ns <= g_bb_ws.groups) {
      if (n_main > 0) {
        BackboneArgs am = a;
        am.n = n_main;
        if (svdd_launch_timed(span.first(), backbone_kernel<true>, dim3((unsigned)n_main), dim3(512), lds, stream, am, BackboneSave{}) != SVDD_OK)
          return SVDD_E_LAUNCH;
        a.x += (size_t)n_main * L; a.out += (size_t)n_main * L * 5; a.n = ns;
        ev = span.last();                                 // one timed span over both launches
      }
      if (hipMemsetAsync(g_bb_ws.cnt, 0, sizeof(int) * (size_t)ns, (hipStream_t)stream) != hipSuccess) return SVDD_E_LAUNCH;
      const dim3 sgrid((unsigned)(((ns + 7) / 8) * 8 * R));
      return svdd_launch_timed(ev, R == 2 ? backbone_split_kernel<2> : backbone_split_kernel<4>, sgrid, dim3(512), lds, stream, a, g_bb_ws);
    }
  }
  const bool spt1 = !a.auto_spt && a.plan.s2 == 1 && (a.plan.n1 == 0 || a.plan.s1 == 1);   // every tile holds one sequence
  return svdd_launch_timed(ev, spt1 ? backbone_kernel<true> : backbone_kernel<false>, dim3(nwg), dim3(512), lds, stream, a, BackboneSave{});
}

// Workgroups per CU of a padded segment launch: its dynamic-LDS request is raised until only g_incr_residency fit (0: no padding, as
// many as the kernel's own image and registers allow — 4 for items of <= 2 tiles, 6 for 1-tile items, 3 for <= 4, 5 for tight items).
constexpr int INCR_DEFAULT_RESIDENCY = 0;
constexpr size_t CU_LDS_BYTES = 160 * 1024;              // gfx950
static int g_incr_residency = INCR_DEFAULT_RESIDENCY;

extern "C" int svdd_backbone_incr_set_residency(int wg_per_cu) {
  if (wg_per_cu < 0 || wg_per_cu > 8) return SVDD_E_ARG;
  g_incr_residency = wg_per_cu;
  return SVDD_OK;
}

// Dynamic LDS of a segment workgroup whose image holds `rows` rows.
static size_t seg_lds_bytes(int rows, bool pad) {
  size_t bytes = sizeof(float) * ((size_t)rows * BB_AP + 5 * (size_t)rows + rows + 8);
  if (pad && g_incr_residency > 0) {                     // one request more than CU_LDS_BYTES / (r + 1): r + 1 workgroups no longer fit
    const size_t least = (CU_LDS_BYTES / (size_t)(g_incr_residency + 1) / 1024 + 1) * 1024;
    if (least > bytes) bytes = least;
  }
  return bytes;
}

// The four incremental entries (include/svdd_hip.h states each one's contract) are ONE host path and differ in data: the kind of
// work list, and the arguments an entry does not have (svdd_backbone_incr_f32 and incr2: depth = lead; all but incr4: parity 0).
//   INCR_SLOT     svdd_backbone_incr_f32: backbone_worklist_kernel, then backbone_seg_kernel<2 | 4> with one workgroup per (row, slot),
//                 empty slots included; max_item 2 or 4, any n, never padded.
//   INCR_ORDERED  incr2, incr3: + backbone_order_kernel (untimed), and the segment launches read its compact, size-ordered list:
//                 backbone_seg_kernel<1 | 2 | 4, true>; n <= 65536 (order packs row << 16 | item).
//   INCR_TIGHT    incr4: ONE list launch (backbone_list_kernel) instead of work list + order; the dilation-1 layers run TIGHT items
//                 (tiles that start at the first row a change reaches, not at a multiple of 16) on backbone_seg_tight_kernel, whose image
//                 holds the 4 halo rows per side instead of a halo tile; max_item 2. The carried tokens are a ping-pong pair, so the
//                 list launch never reads what it writes: `parity` names the buffer that holds them (0: x_prev, 1: x_prev2); a
//                 first == 0 call writes x into the other one.
// Planes 1 .. depth are carried: layers 1 .. lead (dilation 1) on the list kind's kernel, layers lead + 1 .. depth (dilation 4) on
// backbone_seg_kernel<.., true, 4> with aligned items, the tail (backbone_kernel<.., 2>) from plane `depth`. first: the whole forward,
// which also fills the planes; the tokens become the carried ones. Every refusal comes before the span and before any HIP call.
enum IncrList { INCR_SLOT, INCR_ORDERED, INCR_TIGHT };

struct IncrCall {
  const uint8_t* x; const float *table0, *tiles, *vec, *w2; float* out; int n, L, nlayers; const int* dilations; int lead;
  float* planes; uint8_t* x_prev; int32_t* items; unsigned long long* stat; int first, max_item;
  int32_t *order, *order_count; int depth; uint8_t* x_prev2; int parity; void* stream;
};

typedef void (*BackboneSegKernel)(BackboneSegArgs);
static BackboneSegKernel backbone_seg_choice(IncrList list, int mi, bool dilation4) {
  if (dilation4) return mi == 4 ? backbone_seg_kernel<4, true, 4> : mi == 2 ? backbone_seg_kernel<2, true, 4> : backbone_seg_kernel<1, true, 4>;
  if (list == INCR_TIGHT) return backbone_seg_tight_kernel;
  if (list == INCR_SLOT) return mi == 4 ? backbone_seg_kernel<4> : backbone_seg_kernel<2>;
  return mi == 4 ? backbone_seg_kernel<4, true> : mi == 2 ? backbone_seg_kernel<2, true> : backbone_seg_kernel<1, true>;
}

static int backbone_incr(IncrList list, const IncrCall& c) {
  const bool ordered = list != INCR_SLOT, tight = list == INCR_TIGHT;   // ordered: the segment launches read order / order_count
  const int n = c.n, L = c.L, mi = c.max_item, lead = c.lead, depth = c.depth;
  if (!c.x || !c.table0 || !c.tiles || !c.vec || !c.w2 || !c.out || !c.dilations || !c.planes || !c.x_prev || !c.items || n <= 0 ||
      L <= TW_ROWS / 2 || L > TW_ROWS || c.nlayers <= 0 || c.nlayers > BB_MAXL || lead < 2 || lead > c.nlayers || depth < lead ||
      depth > c.nlayers || !(mi == 2 || (mi == 4 && !tight) || (mi == 1 && list == INCR_ORDERED)) ||
      (ordered && (!c.order || !c.order_count || n > 65536)) ||
      (tight && (!c.x_prev2 || c.x_prev2 == c.x_prev || (c.parity != 0 && c.parity != 1))))
    return SVDD_E_ARG;
  for (int i = 0; i < depth; ++i) if (c.dilations[i] != (i < lead ? 1 : 4)) return SVDD_E_ARG;
  BackboneArgs a;
  if (!backbone_args(a, c.x, c.table0, c.tiles, c.vec, c.w2, c.out, n, L, 1, c.nlayers, c.dilations)) return SVDD_E_ARG;
  a.planes = c.planes; a.planes_P = depth;
  uint8_t* x_cur = c.parity ? c.x_prev2 : c.x_prev;      // the carried tokens
  uint8_t* x_next = c.parity ? c.x_prev : c.x_prev2;     // tight only: where this forward's tokens go
  const SvddLds lds = svdd_lds_raised(backbone_lds_bytes(c.nlayers, 3));
  SvddSpan span(SVDD_SLOT_BACKBONE);                      // ONE span per forward over all its launches
  if (c.first) {
    if (hipMemcpyAsync(x_cur, c.x, (size_t)n * L, hipMemcpyDeviceToDevice, (hipStream_t)c.stream) != hipSuccess) return SVDD_E_LAUNCH;
    return svdd_launch_timed(span.all(), backbone_kernel<true, false, 1>, dim3((unsigned)n), dim3(512), lds, c.stream, a, BackboneSave{});
  }
  const int slots = mi == 1 ? TW_RT : SEG_SLOTS;          // 13 one-tile items in a row that changed everywhere
  const BackboneReach reach = backbone_reach(c.dilations, depth, lead);
  int rc;
  if (tight) {
    rc = svdd_launch_timed(span.first(), backbone_list_kernel, dim3((unsigned)depth), dim3(256), 0, c.stream, c.x, (const uint8_t*)x_cur, x_next,
                           n, L, mi, c.items, c.order, c.order_count, c.stat, reach);
  } else {
    rc = svdd_launch_timed(span.first(), mi == 1 ? backbone_worklist_kernel<TW_RT> : backbone_worklist_kernel<SEG_SLOTS>,
                           dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c.stream, c.x, c.x_prev, n, L, depth, mi, c.items, c.stat, reach);
    if (rc == SVDD_OK && ordered)
      rc = svdd_launch(mi == 1 ? backbone_order_kernel<TW_RT> : backbone_order_kernel<SEG_SLOTS>, dim3((unsigned)depth), dim3(256), 0, c.stream,
                       c.items, n, c.order, c.order_count);
  }
  if (rc != SVDD_OK) return SVDD_E_LAUNCH;
  BackboneSegArgs sa{c.x, c.table0, c.tiles, c.vec, c.planes, c.items, n, L, 0, nullptr, nullptr, 0};
  if (ordered) { sa.order = c.order; sa.order_count = c.order_count; sa.order_stride = n * slots; }
  // [0]: the dilation-1 layers, [1]: the dilation-4 layers. An aligned item's image is its tiles and a halo tile per side.
  const BackboneSegKernel seg[2] = {backbone_seg_choice(list, mi, false), backbone_seg_choice(list, mi, true)};
  const size_t slds[2] = {seg_lds_bytes(tight ? 16 * mi + 8 : 16 * (mi + 2), ordered), seg_lds_bytes(16 * (mi + 2), ordered)};
  svdd_raise_lds_limit(seg[0], slds[0]);                  // once per kernel for the launches below
  if (depth > lead) svdd_raise_lds_limit(seg[1], slds[1]);
  const dim3 sgrid((unsigned)n * slots);
  for (int k = 1; k <= depth; ++k) {
    sa.layer = k;
    if (svdd_launch(seg[k > lead], sgrid, dim3(256), slds[k > lead], c.stream, sa) != SVDD_OK) return SVDD_E_LAUNCH;
  }
  return svdd_launch_timed(span.last(), backbone_kernel<true, false, 2>, dim3((unsigned)n), dim3(512), lds, c.stream, a, BackboneSave{});
}

extern "C" int svdd_backbone_incr_f32(const uint8_t* x, const float* table0, const float* tiles, const float* vec, const float* w2,
                                      float* out, int n, int L, int nlayers, const int* dilations, int lead, float* planes,
                                      uint8_t* x_prev, int32_t* items, unsigned long long* stat, int first, int max_item,
                                      void* stream) {
  return backbone_incr(INCR_SLOT, IncrCall{x, table0, tiles, vec, w2, out, n, L, nlayers, dilations, lead, planes, x_prev, items, stat, first,
                                           max_item, nullptr, nullptr, lead, nullptr, 0, stream});
}

extern "C" int svdd_backbone_incr2_f32(const uint8_t* x, const float* table0, const float* tiles, const float* vec, const float* w2,
                                       float* out, int n, int L, int nlayers, const int* dilations, int lead, float* planes,
                                       uint8_t* x_prev, int32_t* items, unsigned long long* stat, int first, int max_item,
                                       int32_t* order, int32_t* order_count, void* stream) {
  return backbone_incr(INCR_ORDERED, IncrCall{x, table0, tiles, vec, w2, out, n, L, nlayers, dilations, lead, planes, x_prev, items, stat, first,
                                              max_item, order, order_count, lead, nullptr, 0, stream});
}

extern "C" int svdd_backbone_incr3_f32(const uint8_t* x, const float* table0, const float* tiles, const float* vec, const float* w2,
                                       float* out, int n, int L, int nlayers, const int* dilations, int lead, float* planes,
                                       uint8_t* x_prev, int32_t* items, unsigned long long* stat, int first, int max_item,
                                       int32_t* order, int32_t* order_count, int depth, void* stream) {
  return backbone_incr(INCR_ORDERED, IncrCall{x, table0, tiles, vec, w2, out, n, L, nlayers, dilations, lead, planes, x_prev, items, stat, first,
                                              max_item, order, order_count, depth, nullptr, 0, stream});
}

extern "C" int svdd_backbone_incr4_f32(const uint8_t* x, const float* table0, const float* tiles, const float* vec, const float* w2,
                                       float* out, int n, int L, int nlayers, const int* dilations, int lead, float* planes,
                                       uint8_t* x_prev, int32_t* items, unsigned long long* stat, int first, int max_item,
                                       int32_t* order, int32_t* order_count, int depth, uint8_t* x_prev2, int parity,
                                       void* on_stream) {
  return backbone_incr(INCR_TIGHT, IncrCall{x, table0, tiles, vec, w2, out, n, L, nlayers, dilations, lead, planes, x_prev, items, stat, first,
                                            max_item, order, order_count, depth, x_prev2, parity, on_stream});
}

extern "C" int svdd_backbone_incr_seed_f32(const float* row_planes, const float* row_logits, const uint8_t* row_x, int n, int L,
                                           int depth, float* planes, float* out, uint8_t* x_prev, uint8_t* x_prev2, int parity,
                                           void* on_stream) {
  if (!row_planes || !row_logits || !row_x || !planes || !out || !x_prev || n <= 0 || L <= TW_ROWS / 2 || L > TW_ROWS || depth <= 0 ||
      depth > BB_MAXL || (parity != 0 && parity != 1) || (parity == 1 && !x_prev2) || x_prev2 == x_prev ||
      (long long)depth * n > 0x7fffffffLL || ((uintptr_t)row_planes | (uintptr_t)planes) % 16 != 0)
    return SVDD_E_ARG;
  const long long units = (long long)depth * n;           // one workgroup per (plane, row), grid-stride beyond 2^20 of them
  SvddSpan span(SVDD_SLOT_BACKBONE);
  return svdd_launch_timed(span.all(), backbone_seed_kernel, dim3((unsigned)(units < (1 << 20) ? units : (1 << 20))), dim3(256), 0, on_stream,
                           reinterpret_cast<const float4*>(row_planes), row_logits, row_x, n, L, depth, reinterpret_cast<float4*>(planes), out,
                           parity ? x_prev2 : x_prev);
}

typedef decltype(&value_tail_kernel<1>) ValueTailKernel;

extern "C" int svdd_value_tail_f32(const float* h_fwd, const float* h_bwd, const float* w1pack, const float* b1,
                                   const float* w_eff, const float* b_eff, float* out, int n, int L, int n_tasks,
                                   const int32_t* count, void* stream) {
  if (!h_fwd || !h_bwd || !w1pack || !b1 || !w_eff || !b_eff || !out || n <= 0 || L <= 0 || n_tasks < 1 || n_tasks > 4)
    return SVDD_E_ARG;
  ValueTailKernel kern;
  switch (n_tasks) {
    case 1: kern = value_tail_kernel<1>; break;
    case 2: kern = value_tail_kernel<2>; break;
    case 3: kern = value_tail_kernel<3>; break;
    default: kern = value_tail_kernel<4>; break;
  }
  SvddSpan span(SVDD_SLOT_VALUE_TAIL);
  return svdd_launch_timed(span.all(), kern, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, h_fwd, h_bwd, w1pack, b1, w_eff, b_eff, out,
                           n, L, count);
}

extern "C" int svdd_candidate_windows(const uint8_t* cand, const uint8_t* x, int B, int L, int M, int margin, int32_t* win,
                                      int32_t* flags, void* stream) {
  if (!cand || !x || !win || B <= 0 || L <= 0 || M <= 0 || margin < 0) return SVDD_E_ARG;
  const int n = B * M;
  return svdd_launch(candidate_windows_kernel<false>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, cand, x, n, L, M, margin, win, flags);
}

extern "C" int svdd_candidate_windows_tight(const uint8_t* cand, const uint8_t* x, int B, int L, int M, int margin, int32_t* win,
                                            int32_t* flags, void* on_stream) {
  if (!cand || !x || !win || B <= 0 || L <= 0 || M <= 0 || margin < 0 || margin > (1 << 20) ||
      (long long)B * M > 0x7fffffffLL)
    return SVDD_E_ARG;
  const int n = B * M;
  return svdd_launch(candidate_windows_kernel<true>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, on_stream, cand, x, n, L, M, margin, win, flags);
}

extern "C" int svdd_conv_tower_windows_f32(const float* onehot, const float* tiles, const float* bias, const int32_t* win,
                                           const float* parent_out, float* out, int n, int L, int M, int nlayers,
                                           int residual_mask, const int32_t* live_idx, const int32_t* count, void* stream) {
  if (!onehot || !tiles || !bias || !win || !parent_out || !out || n <= 0 || M <= 0 || (n % M && !live_idx) || L <= TW_ROWS / 2 ||
      L > TW_ROWS || nlayers != TP_BLOCKS)
    return SVDD_E_ARG;                                   // one sequence per tile; margins below assume the 5-layer tower
  // (with an index list, n is only the number of list entries this launch may take: a launch over PART of a compacted list)
  TowerWinArgs wa{TowerArgs{onehot, tiles, bias, out, n, L, 1, nlayers, residual_mask, nullptr}, win, parent_out, M, live_idx, count};
  void (*kern)(TowerWinArgs) = conv_tower_win_kernel;     // the first generation
  if (g_tower_ver != 1) kern = g_tower_ver == 2 ? conv_tower2_kernel<true, true, 2> : conv_tower2_kernel<true, true, 1>;
  SvddSpan span(SVDD_SLOT_CONV_TOWER);
  return svdd_launch_timed(span.all(), kern, dim3((unsigned)n), dim3(512), svdd_lds_raised(tower2_lds_bytes()), stream, wa);
}

extern "C" int svdd_candidate_parts(const uint8_t* cand, const uint8_t* x, int B, int L, int M, int reach, int gap, int32_t* parts,
                                    int32_t* nparts, int32_t* flags, int32_t* key, void* on_stream) {
  if (!cand || !x || !parts || B <= 0 || L <= 0 || M <= 0 || reach < 0 || reach > (1 << 20) || (long long)B * M > 0x7fffffffLL - 3 ||
      gap < 2 * (reach + 2 * TP_BLOCKS) + 16)
    return SVDD_E_ARG;                                   // a smaller gap would let two parts' computed tiles touch on the stem
  const int n = B * M;
  return svdd_launch(candidate_parts_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, on_stream, cand, x, n, L, M, reach, gap, parts,
                     nparts, flags, key);
}

extern "C" int svdd_conv_tower_parts_f32(const float* onehot, const float* tiles, const float* bias, const int32_t* parts,
                                         const float* parent_out, float* out, int n, int L, int M, int nlayers, int residual_mask,
                                         int reach, const int32_t* live_idx, const int32_t* count, void* on_stream) {
  if (!onehot || !tiles || !bias || !parts || !parent_out || !out || n <= 0 || M <= 0 || (n % M && !live_idx) || L <= TW_ROWS / 2 ||
      L > TW_ROWS || nlayers != TP_BLOCKS || reach != TP_REACH)
    return SVDD_E_ARG;                                   // one sequence per tile; the part rule is the 5-block tower's, and the parts must
                                                         // have been cut for this reach (a larger one here would make their tiles overlap)
  TowerPartArgs pa{TowerArgs{onehot, tiles, bias, out, n, L, 1, nlayers, residual_mask, nullptr}, parts, parent_out, M, reach, live_idx, count};
  SvddSpan span(SVDD_SLOT_CONV_TOWER);
  return svdd_launch_timed(span.all(), conv_tower_parts_kernel, dim3((unsigned)n), dim3(512), svdd_lds_raised(tower2_lds_bytes()), on_stream, pa);
}

// The value net on a compacted, size-ordered list of live candidates that may exceed one round of the GRU's units, as two parts sized
// on the device (count3 of svdd_compact_by_key with this `split`): A = the first count3[1] <= split entries, B = the count3[2] behind
// them (non-empty only when A is full, so the live rows are contiguous).
//     tower(B) -> [ GRU(B) || tower(A) ] in one launch (gru_tower_parts_kernel) -> GRU(A) -> tail(all count3[0] rows)
// B's GRU — a second round that would run with 3/4 of the chip idle — hides under A's tower. A launch whose part is empty leaves at
// its count check. Same kernels' bodies on the same rows as the one-part sequence: the same bits per candidate.
extern "C" int svdd_value_late_step_f32(const float* onehot, const float* tiles, const float* bias, const int32_t* parts,
                                        const float* parent_out, float* seq, int n, int L, int M, int nlayers, int residual_mask,
                                        int reach, const int32_t* live_idx, const int32_t* count3, int split, const float* wpack,
                                        const float* bpack, float* h, const float* w1pack, const float* b1, const float* w_eff,
                                        const float* b_eff, float* out, int n_tasks, void* on_stream) {
  if (!onehot || !tiles || !bias || !parts || !parent_out || !seq || !live_idx || !count3 || !wpack || !bpack || !h || !w1pack || !b1 ||
      !w_eff || !b_eff || !out || n <= 0 || M <= 0 || L <= TW_ROWS / 2 || L > TW_ROWS || nlayers != TP_BLOCKS || reach != TP_REACH ||
      split <= 0 || split >= n || n_tasks < 1 || n_tasks > 4)
    return SVDD_E_ARG;
  const size_t rowf = (size_t)L * TW_C;                   // floats of one row of seq and of one direction of h (TW_C = H = 64)
  const int nb = n - split;
  const unsigned units_a = 2 * (unsigned)((split + TS - 1) / TS), units_b = 2 * (unsigned)((nb + TS - 1) / TS);
  const SvddLds lds = svdd_lds_raised(tower2_lds_bytes());
  const TowerPartArgs tb{TowerArgs{onehot, tiles, bias, seq + split * rowf, nb, L, 1, nlayers, residual_mask, nullptr}, parts, parent_out, M,
                         reach, live_idx + split, count3 + 2};
  const TowerPartArgs ta{TowerArgs{onehot, tiles, bias, seq, split, L, 1, nlayers, residual_mask, nullptr}, parts, parent_out, M, reach,
                         live_idx, count3 + 1};
  const GruPartArgs gb{seq + split * rowf, wpack, bpack, h + split * rowf, n, L, count3 + 2};
  ValueTailKernel tail;
  switch (n_tasks) {
    case 1: tail = value_tail_kernel<1>; break;
    case 2: tail = value_tail_kernel<2>; break;
    case 3: tail = value_tail_kernel<3>; break;
    default: tail = value_tail_kernel<4>; break;
  }
  int rc;
  {
    SvddSpan span(SVDD_SLOT_CONV_TOWER);
    rc = svdd_launch_timed(span.all(), conv_tower_parts_kernel, dim3((unsigned)nb), dim3(512), lds, on_stream, tb);
  }
  if (rc != SVDD_OK) return rc;
  {
    SvddSpan span(SVDD_SLOT_GRU);                         // one span over the middle launch (A's tower included) and A's GRU
    rc = svdd_launch_timed(span.first(), gru_tower_parts_kernel, dim3(units_b + (unsigned)split), dim3(512), lds, on_stream, gb, ta, units_b);
    if (rc != SVDD_OK) return rc;
    rc = svdd_launch_timed(span.last(), gru_pc_kernel, dim3(units_a), dim3(512), 0, on_stream, (const float*)seq, wpack, bpack, h, n, L,
                           count3 + 1);
  }
  if (rc != SVDD_OK) return rc;
  SvddSpan span(SVDD_SLOT_VALUE_TAIL);
  return svdd_launch_timed(span.all(), tail, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, on_stream, (const float*)h,
                           (const float*)(h + (size_t)n * rowf), w1pack, b1, w_eff, b_eff, out, n, L, count3);
}
