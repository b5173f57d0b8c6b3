// svdd_motifs.hip — PWM motif scanning of 2-bit-packed sequences (not in the reference). Integer log-odds tables,
// int32 sums, integer atomics for the [M] totals only: no result depends on the launch shape or on how the caller cuts its rows
// into chunks.
//
//   svdd_motif_scan   a workgroup stages MS_TR packed rows and the tables of MS_MG motifs in LDS. All four waves work on one motif
//                     at a time, each on its own groups of MS_K rows: a lane owns one start position of each of the MS_K rows (a
//                     pass covers 64 starts), pulls its 32-token window out of three LDS words (16 lanes share a word: a
//                     broadcast) and walks the motif's columns. A column is one 16-byte LDS read at a wave-uniform address:
//                     {A|C, G|T} of the forward table and of the reverse-strand table (column w - 1 - i with the tokens
//                     complemented, built when the tables are staged), so both strands come from one pass over the tokens. The
//                     entry of a token is picked out of the two dwords by one v_perm_b32 (bytes 2t, 2t + 1 and the sign of byte
//                     2t + 1): no per-lane table gather. A row's windows for one motif live in one wave, so the per-row
//                     outputs need no atomics; they are collected in LDS and written MS_MG motifs of a row side by side. The
//                     totals cost one 64-bit atomic per wave and motif.
//   svdd_motif_reward the same scan (stage_tables, scan_row_group) folded into one fp32 score per row, for the SVDD-PM loop: a
//                     workgroup packs MR_TR u8 rows into LDS itself, under a device-side row count, and walks ALL motif groups for
//                     them; within a stage the (group of MS_K rows, motif) pairs are dealt to the four waves, a wave's lane 0
//                     leaves the pair's int64 terms in LDS and thread r adds row r's up: a row's sum is finished inside one
//                     workgroup, without atomics or a second pass.
#include "svdd_host.h"

namespace {

constexpr int MS_QB = 256;                  // threads per workgroup: 4 waves
constexpr int MS_TR = 64;                   // rows per workgroup
constexpr int MS_K = 8;                     // rows a wave scans together (a column's table read is shared by MS_K windows per lane)
constexpr int MS_MG = 8;                    // motifs per table stage
constexpr int MS_MAXL = 1024;
constexpr int MS_MAXW = 32;
constexpr int MS_MAXWS = MS_MAXL / 16 + 2;  // a row in LDS: its words and two zero words (a window reads three words)
constexpr uint32_t MS_BIAS = 1u << 20;      // |score| <= 32 * 32768 = 2^20: score + MS_BIAS lies in (0, 2^21)

// rows per workgroup of svdd_motif_reward (tools/motif_reward_time.py builds copies with other values; profiles/motif_reward_time.txt)
#ifndef SVDD_MOTIF_REWARD_ROWS
#define SVDD_MOTIF_REWARD_ROWS 8
#endif
constexpr int MR_TR = SVDD_MOTIF_REWARD_ROWS;
static_assert(MR_TR >= 1 && MR_TR <= MS_QB, "thread r of a workgroup finishes row r");

struct MotifArgs {
  const uint32_t* packed;
  const int16_t* pwm;
  const int32_t* width;
  const int32_t* threshold;
  int N, L, W, M, mgroups;
  unsigned long long* hits;
  unsigned long long* rows_hit;
  int32_t* row_hits;
  unsigned long long* row_best;
};

struct RewardArgs {
  const uint8_t* tok;
  const int32_t* count;
  const int16_t* pwm;
  const int32_t* width;
  const int32_t* threshold;
  const int32_t* hit_coef;
  const int32_t* hit_cap;
  const int32_t* margin_coef;
  const int32_t* margin_floor;
  const float* base;
  float unit;
  int n, L, W, M, mgroups;
  float* score;
  long long* term;
  int32_t* err;
};

// The int16 entry of token t (0..3) of a column held as lo = A | C << 16, hi = G | T << 16, as a 24-bit two's complement number
// (top byte zero). v_perm_b32 reads {hi, lo} as bytes 0..7; a selector byte 8 + t gives the sign bit of byte 2t + 1 replicated and
// 12 gives zero, so the selector is 0x0c080100 + t * 0x010202: bytes 2t, 2t + 1, the sign, zero. Sums of at most 32 entries stay
// inside 24 bits (|sum| <= 2^20): the low 24 bits of the running sum are exact and score24 sign-extends them once per window.
__device__ __forceinline__ uint32_t entry_selector(uint32_t window, int i) {
  return 0x0c080100u + ((window >> (2 * i)) & 3u) * 0x010202u;
}
__device__ __forceinline__ uint32_t column_entry(uint32_t lo, uint32_t hi, uint32_t sel) {
  return __builtin_amdgcn_perm(hi, lo, sel);
}
__device__ __forceinline__ int score24(uint32_t sum) {
  return (int)(sum << 8) >> 8;
}

// The in-kernel key of a window: (score + 2^20) << 11 | (2047 - (2 start + strand)), one u32 whose maximum is the highest score,
// then the lowest start, then forward before reverse. 0 = no window. Widened to the entry's i64 key on the way out.
__device__ __forceinline__ unsigned long long widen_key(uint32_t k) {
  if (k == 0) return 0ull;
  const int score = (int)(k >> 11) - (int)MS_BIAS;
  const uint32_t where = 2047u - (k & 2047u);                     // 2 start + strand
  return ((unsigned long long)((uint32_t)score ^ 0x80000000u) << 32) | (unsigned long long)(uint32_t)~where;
}

// Stage the tables of the motifs m0 .. m0 + nm - 1 (nm <= MS_MG): per column {fwd lo, fwd hi, rev lo, rev hi} in tab, the clamped
// widths and the thresholds. The caller synchronises before (the previous stage is read) and after.
__device__ __forceinline__ void stage_tables(const int16_t* pwm, const int32_t* width, const int32_t* threshold, int m0, int nm,
                                             uint32_t* tab, int* s_w, int* s_thr) {
  for (int t = threadIdx.x; t < nm * 64; t += MS_QB) {
    const int mi = t >> 6, j = t & 63, m = m0 + mi;
    const int w = min(max(width[m], 1), MS_MAXW);
    const int16_t* p = pwm + (long long)m * (MS_MAXW * 4) + 2 * j;
    const uint32_t v = (uint32_t)(uint16_t)p[0] | (uint32_t)(uint16_t)p[1] << 16;
    const int col = j >> 1, half = j & 1;
    if (col < w) {
      tab[(mi * MS_MAXW + col) * 4 + half] = v;
      // reverse strand: column w - 1 - col with the tokens complemented. {A|C, G|T} -> {T|G, C|A}
      tab[(mi * MS_MAXW + (w - 1 - col)) * 4 + 2 + (1 - half)] = v >> 16 | v << 16;
    }
    if (j == 0) {
      s_w[mi] = w;
      s_thr[mi] = threshold[m];
    }
  }
}

// One wave scans the MS_K rows rb .. rb + MS_K - 1 of the LDS tile `rows` (WS words a row, W of them tokens; rows past the tile's
// live ones are zero words) for one motif (col: its staged columns, width w, threshold thr; nw = L - w + 1 windows, <= 0: none).
// cnt[k]: the hits of row rb + k (wave-uniform); best[k]: this lane's highest in-kernel key of that row (0: none; BEST only).
template <bool BOTH, bool BEST>
__device__ __forceinline__ void scan_row_group(const uint32_t* rows, int WS, int W, int rb, int nw, int lane, const uint4* col, int w,
                                               int thr, uint32_t (&cnt)[MS_K], uint32_t (&best)[MS_K]) {
  const int npass = nw > 0 ? (nw + 63) >> 6 : 0;
#pragma unroll
  for (int k = 0; k < MS_K; ++k) {
    cnt[k] = best[k] = 0;
    asm volatile("" : "+v"(cnt[k]));                          // a vector register: MS_K wave-uniform counters would crowd the scalar file
  }
  for (int q = 0; q < npass; ++q) {
    const int p = q * 64 + lane;
    const bool valid = p < nw;
    const int wi = min(p >> 4, W - 1), sh = (p & 15) * 2;     // a valid start has p >> 4 < W; the others read in bounds
    uint32_t lo[MS_K], hi[MS_K];
    uint32_t af[MS_K], ar[MS_K];
#pragma unroll
    for (int k = 0; k < MS_K; ++k) {                          // rows past nrows are zero words
      const uint32_t* rw = rows + (rb + k) * WS + wi;
      const uint32_t w0 = rw[0], w1 = rw[1], w2 = rw[2];
      lo[k] = (uint32_t)(((unsigned long long)w1 << 32 | w0) >> sh);
      hi[k] = (uint32_t)(((unsigned long long)w2 << 32 | w1) >> sh);
      af[k] = ar[k] = 0;
    }
    const int n1 = min(w, 16);
    for (int i = 0; i < n1; ++i) {
      const uint4 c = col[i];
#pragma unroll
      for (int k = 0; k < MS_K; ++k) {
        const uint32_t sel = entry_selector(lo[k], i);
        af[k] += column_entry(c.x, c.y, sel);
        if (BOTH) ar[k] += column_entry(c.z, c.w, sel);
      }
    }
    for (int i = 16; i < w; ++i) {
      const uint4 c = col[i];
#pragma unroll
      for (int k = 0; k < MS_K; ++k) {
        const uint32_t sel = entry_selector(hi[k], i - 16);
        af[k] += column_entry(c.x, c.y, sel);
        if (BOTH) ar[k] += column_entry(c.z, c.w, sel);
      }
    }
    const uint32_t kc = (MS_BIAS << 11) + 2047u - 2u * (uint32_t)p;
#pragma unroll
    for (int k = 0; k < MS_K; ++k) {
      const int sf = score24(af[k]), sr = score24(ar[k]);
      cnt[k] += (uint32_t)__popcll(__ballot(valid && sf >= thr));
      if (BOTH) cnt[k] += (uint32_t)__popcll(__ballot(valid && sr >= thr));
      if (BEST) {
        uint32_t key = ((uint32_t)sf << 11) + kc;
        if (BOTH) key = max(key, ((uint32_t)sr << 11) + kc - 1u);
        best[k] = valid ? max(best[k], key) : best[k];
      }
    }
  }
}

// The wave's maximum of a lane's in-kernel key.
__device__ __forceinline__ uint32_t wave_max_key(uint32_t b) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) b = max(b, (uint32_t)__shfl_xor((int)b, s, 64));
  return b;
}

template <bool BOTH, bool BEST>
__global__ __launch_bounds__(MS_QB) void motif_scan_kernel(MotifArgs a) {
  __shared__ uint32_t rows[MS_TR * MS_MAXWS];
  __shared__ __attribute__((aligned(16))) uint32_t tab[MS_MG * MS_MAXW * 4];   // per column {fwd lo, fwd hi, rev lo, rev hi}
  __shared__ int s_w[MS_MG], s_thr[MS_MG];
  __shared__ uint32_t o_hits[MS_TR * MS_MG], o_best[MS_TR * MS_MG];

  const int WS = a.W + 2;
  const long long row0 = (long long)blockIdx.x * MS_TR;
  const int nrows = (int)min((long long)MS_TR, (long long)a.N - row0);
  for (int i = threadIdx.x; i < MS_TR * WS; i += MS_QB) {
    const int r = i / WS, c = i - r * WS;
    rows[i] = r < nrows && c < a.W ? a.packed[(row0 + r) * a.W + c] : 0u;
  }
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;

  for (int mg = blockIdx.y; mg < a.mgroups; mg += gridDim.y) {
    const int m0 = mg * MS_MG;
    const int nm = min(MS_MG, a.M - m0);
    __syncthreads();                                              // the previous stage's tables and outputs are read
    stage_tables(a.pwm, a.width, a.threshold, m0, nm, tab, s_w, s_thr);
    __syncthreads();

    for (int mi = 0; mi < nm; ++mi) {
      const int w = s_w[mi], thr = s_thr[mi];
      const int nw = a.L - w + 1;                                 // <= 0: no windows
      const uint4* col = reinterpret_cast<const uint4*>(tab) + mi * MS_MAXW;
      uint32_t tot_hits = 0, tot_rows = 0;
      for (int rb = wave * MS_K; rb < nrows; rb += 4 * MS_K) {
        uint32_t cnt[MS_K], best[MS_K];
        scan_row_group<BOTH, BEST>(rows, WS, a.W, rb, nw, lane, col, w, thr, cnt, best);
#pragma unroll
        for (int k = 0; k < MS_K; ++k) {
          if (rb + k < nrows) {                                     // wave-uniform
            tot_hits += cnt[k];
            tot_rows += cnt[k] != 0;
            uint32_t b = best[k];
            if (BEST) b = wave_max_key(b);
            if (lane == 0) {
              o_hits[(rb + k) * MS_MG + mi] = cnt[k];
              o_best[(rb + k) * MS_MG + mi] = b;
            }
          }
        }
      }
      if (lane == 0) {
        if (a.hits && tot_hits) atomicAdd(&a.hits[m0 + mi], (unsigned long long)tot_hits);
        if (a.rows_hit && tot_rows) atomicAdd(&a.rows_hit[m0 + mi], (unsigned long long)tot_rows);
      }
    }

    if (a.row_hits || a.row_best) {
      __syncthreads();
      for (int i = threadIdx.x; i < nrows * MS_MG; i += MS_QB) {
        const int r = i / MS_MG, mi = i - r * MS_MG;
        if (mi < nm) {
          const long long o = (row0 + r) * a.M + m0 + mi;
          if (a.row_hits) a.row_hits[o] = (int32_t)o_hits[i];
          if (BEST) a.row_best[o] = widen_key(o_best[i]);
        }
      }
    }
  }
}

// svdd_motif_reward: T(r) = sum_m [hit_coef_m min(hits_m, hit_cap_m) + margin_coef_m max(min(best_m - threshold_m, 0), -margin_floor_m)]
// in int64, then score[r] = base[r] + float(T) unit (two fp32 operations, one rounding each).
template <bool BOTH>
__global__ __launch_bounds__(MS_QB) void motif_reward_kernel(RewardArgs a) {
  constexpr int TRP = (MR_TR + MS_K - 1) / MS_K * MS_K;           // the tile in LDS: whole groups of MS_K rows
  __shared__ uint32_t rows[TRP * MS_MAXWS];
  __shared__ __attribute__((aligned(16))) uint32_t tab[MS_MG * MS_MAXW * 4];
  __shared__ int s_w[MS_MG], s_thr[MS_MG], s_hc[MS_MG], s_cap[MS_MG], s_mc[MS_MG], s_fl[MS_MG];
  __shared__ long long o_term[TRP * MS_MG];

  const int live = a.count ? min(max(a.count[0], 0), a.n) : a.n;  // rows >= count[0] are neither read nor written
  const long long row0 = (long long)blockIdx.x * MR_TR;
  if (row0 >= live) return;
  const int nrows = (int)min((long long)MR_TR, (long long)live - row0);
  const int WS = a.W + 2;
  bool bad = false;
  for (int i = threadIdx.x; i < TRP * WS; i += MS_QB) {           // pack the rows' tokens as svdd_pack_tokens does; the rest zero
    const int r = i / WS, c = i - r * WS;
    uint32_t v = 0;
    if (r < nrows && c < a.W) {
      const int l0 = 16 * c, nt = min(16, a.L - l0);
      const uint8_t* p = a.tok + (row0 + r) * a.L + l0;
      for (int j = 0; j < nt; ++j) {
        const uint32_t t = p[j];
        if (t > 3u) bad = true;
        else v |= t << (2 * j);
      }
    }
    rows[i] = v;
  }
  if (bad && a.err) a.err[0] = 1;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nrg = (nrows + MS_K - 1) / MS_K;
  long long T = 0;                                                // thread r < nrows: row r's term

  for (int mg = 0; mg < a.mgroups; ++mg) {
    const int m0 = mg * MS_MG;
    const int nm = min(MS_MG, a.M - m0);
    __syncthreads();                                              // the rows are packed; the previous stage's tables and terms are read
    stage_tables(a.pwm, a.width, a.threshold, m0, nm, tab, s_w, s_thr);
    if ((int)threadIdx.x < nm) {
      const int m = m0 + threadIdx.x;
      s_hc[threadIdx.x] = a.hit_coef[m];
      s_cap[threadIdx.x] = a.hit_cap[m];
      s_mc[threadIdx.x] = a.margin_coef[m];
      s_fl[threadIdx.x] = a.margin_floor[m];
    }
    __syncthreads();

    for (int item = wave; item < nrg * nm; item += MS_QB / 64) {   // (row group, motif) pairs, dealt to the waves
      const int mi = item / nrg, rb = (item - mi * nrg) * MS_K;
      const int w = s_w[mi], thr = s_thr[mi];
      const uint4* col = reinterpret_cast<const uint4*>(tab) + mi * MS_MAXW;
      uint32_t cnt[MS_K], best[MS_K];
      scan_row_group<BOTH, true>(rows, WS, a.W, rb, a.L - w + 1, lane, col, w, thr, cnt, best);
      const long long hc = s_hc[mi], cap = s_cap[mi], mc = s_mc[mi], fl = s_fl[mi];
#pragma unroll
      for (int k = 0; k < MS_K; ++k) {
        if (rb + k < nrows) {                                       // wave-uniform
          const uint32_t b = wave_max_key(best[k]);
          if (lane == 0) {
            long long margin = -fl;                                 // no window
            if (b) margin = max(min((long long)((int)(b >> 11) - (int)MS_BIAS) - thr, 0ll), -fl);
            o_term[(rb + k) * MS_MG + mi] = hc * min((long long)cnt[k], cap) + mc * margin;
          }
        }
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < nrows)
      for (int mi = 0; mi < nm; ++mi) T += o_term[threadIdx.x * MS_MG + mi];
  }

  if ((int)threadIdx.x < nrows) {
    const long long r = row0 + threadIdx.x;
    if (a.term) a.term[r] = T;
    if (a.score) a.score[r] = __fadd_rn(a.base ? a.base[r] : 0.0f, __fmul_rn((float)T, a.unit));
  }
}

}  // namespace

extern "C" {

int svdd_motif_scan(const uint32_t* packed, int N, int L, const int16_t* pwm, const int32_t* width, const int32_t* threshold, int M,
                    int both_strands, int64_t* hits, int64_t* rows_hit, int32_t* row_hits, int64_t* row_best, void* on_stream) {
  if (!packed || !pwm || !width || !threshold || N <= 0 || L <= 0 || L > MS_MAXL || M <= 0) return SVDD_E_ARG;
  if (!hits && !rows_hit && !row_hits && !row_best) return SVDD_E_ARG;
  const int mgroups = (M + MS_MG - 1) / MS_MG;
  const MotifArgs a{packed, pwm, width, threshold, N, L, (L + 15) / 16, M, mgroups, (unsigned long long*)hits,
                    (unsigned long long*)rows_hit, row_hits, (unsigned long long*)row_best};
  const dim3 grid((unsigned)(((long long)N + MS_TR - 1) / MS_TR),(unsigned)(mgroups < 65535 ? mgroups : 65535));
  void (*k)(MotifArgs) = both_strands ? (row_best ? motif_scan_kernel<true, true> : motif_scan_kernel<true, false>)
                                      : (row_best ? motif_scan_kernel<false, true> : motif_scan_kernel<false, false>);
  return svdd_launch(k, grid, dim3(MS_QB), 0, on_stream, a);
}

int svdd_motif_reward(const uint8_t* tok, int n, int L, const int32_t* count, const int16_t* pwm, const int32_t* width,
                      const int32_t* threshold, int M, int both_strands, const int32_t* hit_coef, const int32_t* hit_cap,
                      const int32_t* margin_coef, const int32_t* margin_floor, const float* base, float unit, float* score,
                      int64_t* term, int32_t* err, void* on_stream) {
  if (!tok || !pwm || !width || !threshold || !hit_coef || !hit_cap || !margin_coef || !margin_floor) return SVDD_E_ARG;
  if (n <= 0 || L <= 0 || L > MS_MAXL || M <= 0 || (!score && !term)) return SVDD_E_ARG;
  const RewardArgs a{tok, count, pwm, width, threshold, hit_coef, hit_cap, margin_coef, margin_floor, base, unit, n, L, (L + 15) / 16,
                     M, (M + MS_MG - 1) / MS_MG, score, (long long*)term, err};
  const dim3 grid((unsigned)(((long long)n + MR_TR - 1) / MR_TR));
  return svdd_launch(both_strands ? motif_reward_kernel<true> : motif_reward_kernel<false>, grid, dim3(MS_QB), 0, on_stream, a);
}

}  // extern "C"
