// svdd_quality.hip — sample-quality metrics of a decoded batch AS A SET: k-mer spectra (reference oracle.count_kmers,
// diffusion_gosai.py compare_kmer) and nearest-neighbour / pairwise Hamming distances on 2-bit-packed sequences (diversity and
// novelty: not in the reference). Everything here is integer arithmetic with integer atomics: no result depends on the launch
// shape or on how the caller cuts its rows into chunks.
//
//   svdd_kmer_counts   one workgroup takes a run of rows, counts their windows into a u32 histogram of 4^k bins in LDS and adds
//                      the non-zero bins to the caller's i64 counts with 64-bit atomics
//   svdd_pack_tokens   16 tokens per u32, one thread per word
//   svdd_hamming_nn    a thread keeps ONE query's W words in registers; a workgroup of 256 queries walks a segment of the
//                      database in tiles of HM_TILE rows staged in LDS. Every lane reads the same tile address (a broadcast: one
//                      LDS cycle per lane group, no bank conflict), so a pair costs W xor / fold / popcount steps and, with hist,
//                      one LDS atomic. The query's minimum is kept in registers (ascending rows, strictly smaller wins: the first
//                      row of a tie) and meets the other segments' in one 64-bit atomic min per query on the key
//                      (distance << 32 | database index).
//   svdd_edit_nn       the same skeleton for the Levenshtein distance: a thread keeps one query as four bit planes
//                      and runs the bit-vector recurrence on them as one multi-word integer, one step per database token; the
//                      token is wave-uniform, so the plane is chosen by a scalar branch.
//   svdd_within        svdd_hamming_nn's skeleton with a radius: which database rows are within it, as a bit matrix
//                      (the owning thread gathers 32 rows into a word: plain stores) and / or as the lowest such row; optionally
//                      the smaller of the distances to the query and to its reverse complement; the database's length may live
//                      on the device
//   svdd_greedy_pick   the serial walk of greedy selection over one block of rows, in one wave: the settled set lives in
//                      registers, only the rows that are picked load their row of the bit matrix
//   svdd_edit_within   svdd_edit_nn's skeleton with svdd_within's outputs: which database rows are within a Levenshtein
//                      radius, on one strand or on both; the second strand walks the staged row backwards with complemented
//                      tokens against the same planes
//   svdd_edit_pairs    row i against ONE database row each: one thread per pair, the plane chosen per lane
#include "svdd_host.h"

namespace {

constexpr int QB = 256;                     // threads per workgroup of all three kernels
constexpr int KM_MAXK = 6;
constexpr int KM_BINS = 1 << (2 * KM_MAXK); // 4096 bins, 16 KB
constexpr int HM_TILE = 64;                 // database rows per LDS tile
constexpr int HM_MAXL = 1024;               // 64 words per row: the register budget of a query

struct KmerArgs {
  const uint8_t* x;
  int N, L, k, rows_per_wg;
  unsigned long long* counts;
  unsigned long long* skipped;
};

// Rows [wg * rows_per_wg, ...) of x: window (r, i) -> bin sum_j x[r, i + j] 4^(k - 1 - j); a window with a token > 3 counts as
// skipped. rows_per_wg * (L - k + 1) < 2^32 (the host's bound), so no u32 bin wraps.
__global__ __launch_bounds__(QB) void kmer_counts_kernel(KmerArgs a) {
  __shared__ unsigned int h[KM_BINS];
  __shared__ unsigned int skip;
  const int nb = 1 << (2 * a.k);
  for (int i = threadIdx.x; i < nb; i += QB) h[i] = 0;
  if (threadIdx.x == 0) skip = 0;
  __syncthreads();
  const long long r0 = (long long)blockIdx.x * a.rows_per_wg;
  const long long rows = min((long long)a.rows_per_wg, (long long)a.N - r0);
  const int nw = a.L - a.k + 1;                                   // > 0: the host launches nothing otherwise
  const long long total = rows * nw;
  unsigned int my_skip = 0;
  for (long long w = threadIdx.x; w < total; w += QB) {
    const long long r = w / nw;
    const int i = (int)(w - r * nw);
    const uint8_t* p = a.x + (r0 + r) * a.L + i;
    unsigned int bin = 0, bad = 0;
    for (int j = 0; j < a.k; ++j) {
      const unsigned int t = p[j];
      bad |= t > 3u;
      bin = (bin << 2) | (t & 3u);
    }
    if (bad) ++my_skip;
    else atomicAdd(&h[bin], 1u);
  }
  if (my_skip) atomicAdd(&skip, my_skip);
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += QB)
    if (h[i]) atomicAdd(&a.counts[i], (unsigned long long)h[i]);
  if (threadIdx.x == 0 && a.skipped && skip) atomicAdd(a.skipped, (unsigned long long)skip);
}

struct PackArgs {
  const uint8_t* x;
  int N, L, W;
  uint32_t* packed;
  int32_t* err;
};

// one thread per packed word, grid-stride
__global__ __launch_bounds__(QB) void pack_tokens_kernel(PackArgs a) {
  const long long total = (long long)a.N * a.W;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * QB + threadIdx.x; i < total; i += (long long)gridDim.x * QB) {
    const long long r = i / a.W;
    const int w = (int)(i - r * a.W);
    const int l0 = 16 * w, n = min(16, a.L - l0);
    const uint8_t* p = a.x + r * a.L + l0;
    uint32_t v = 0;
    for (int j = 0; j < n; ++j) {
      const uint32_t t = p[j];
      if (t > 3u) bad = true;
      else v |= t << (2 * j);
    }
    a.packed[i] = v;
  }
  if (bad && a.err) a.err[0] = 1;
}

struct HammingArgs {
  const uint32_t* q;
  const uint32_t* db;
  int B, N, L, W;
  int q_base, db_base, exclude_diag, seg_rows;
  uint32_t last_mask;                       // the valid bits of a row's last word (the padding is never trusted)
  unsigned long long* nn_key;
  unsigned long long* hist;
};

__device__ __forceinline__ int diff_positions(uint32_t v) {       // positions (bit pairs) at which v = a ^ b is non-zero
  return __popc((v | (v >> 1)) & 0x55555555u);
}

// WT words of a row take part, WS is the row stride of the tile in LDS (a multiple of 4 where the row is read as uint4).
template <int WT, int WS>
__device__ __forceinline__ int row_distance(const uint32_t (&q)[WT], const uint32_t* row) {
  int d = 0;
  if constexpr (WS % 4 == 0) {
#pragma unroll
    for (int v = 0; v < WS / 4; ++v) {
      const uint4 t = reinterpret_cast<const uint4*>(row)[v];
      const uint32_t tt[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (4 * v + c < WT) d += diff_positions(q[4 * v + c] ^ tt[c]);
    }
  } else {
#pragma unroll
    for (int w = 0; w < WT; ++w) d += diff_positions(q[w] ^ row[w]);
  }
  return d;
}

// grid (ceil(B / QB), segments of seg_rows database rows). W <= WT; the words W .. WT - 1 are zero on both sides.
// A workgroup's u32 bins hold at most QB * seg_rows < 2^32 pairs (the host keeps seg_rows <= 2^22).
template <int WT, int WS>
__global__ __launch_bounds__(QB) void hamming_nn_kernel(HammingArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[HM_TILE * WS];
  __shared__ unsigned int h[HM_MAXL + 1];
  const bool want_hist = a.hist != nullptr;
  if (want_hist) {
    for (int i = threadIdx.x; i <= a.L; i += QB) h[i] = 0;
  }
  const int qi = blockIdx.x * QB + threadIdx.x;
  const bool live = qi < a.B;
  uint32_t q[WT];
#pragma unroll
  for (int w = 0; w < WT; ++w) q[w] = live && w < a.W ? a.q[(long long)qi * a.W + w] & (w == a.W - 1 ? a.last_mask : 0xFFFFFFFFu) : 0u;
  const int seg0 = (int)min((long long)blockIdx.y * a.seg_rows, (long long)a.N);
  const int seg1 = (int)min((long long)seg0 + a.seg_rows, (long long)a.N);
  // the database row this query must leave out: q_base + qi == db_base + j  <=>  j = q_base + qi - db_base
  const long long diag = a.exclude_diag ? (long long)a.q_base + qi - a.db_base : -1;
  unsigned int best_d = 0xFFFFFFFFu;
  int best_j = 0;
  for (int t0 = seg0; t0 < seg1; t0 += HM_TILE) {
    const int nr = min(HM_TILE, seg1 - t0);
    __syncthreads();                                            // the previous tile is read (and h is zeroed)
    for (int i = threadIdx.x; i < nr * WS; i += QB) {
      const int r = i / WS, w = i - r * WS;
      tile[i] = w < a.W ? a.db[(long long)(t0 + r) * a.W + w] & (w == a.W - 1 ? a.last_mask : 0xFFFFFFFFu) : 0u;
    }
    __syncthreads();
    if (live) {
#pragma unroll 2
      for (int r = 0; r < nr; ++r) {
        const int d = row_distance<WT, WS>(q, &tile[r * WS]);
        if ((long long)(t0 + r) != diag) {
          if (want_hist) atomicAdd(&h[d], 1u);
          if ((unsigned int)d < best_d) { best_d = (unsigned int)d; best_j = t0 + r; }
        }
      }
    }
  }
  if (live && a.nn_key && best_d != 0xFFFFFFFFu)
    atomicMin(&a.nn_key[qi], ((unsigned long long)best_d << 32) | (unsigned long long)(uint32_t)(a.db_base + best_j));
  if (want_hist) {
    __syncthreads();
    for (int i = threadIdx.x; i <= a.L; i += QB)
      if (h[i]) atomicAdd(&a.hist[i], (unsigned long long)h[i]);
  }
}

constexpr int ED_TILE = 64;                 // database rows per LDS tile of the edit-distance kernel
constexpr int ED_MAXW = HM_MAXL / 16;       // packed words of the longest database row

struct EditArgs {
  const uint32_t* q;
  const uint32_t* db;
  int B, N, Lq, Ld, Wq, Wd, cap;
  int q_base, db_base, exclude_diag, seg_rows;
  unsigned long long* nn_key;
  unsigned long long* hist;
};

// One database token against the whole query: Myers' / Hyyro's bit-vector step on ONE integer of 32 WT bits (word 0 lowest).
// eq: the positions of the query that hold this token. The only traffic between words is the carry of (eq & Pv) + Pv and the
// two one-bit left shifts. The query's LAST position is bit 31 of word WT - 1, so that is where the score bit is read.
template <int WT>
__device__ __forceinline__ void edit_column(const uint32_t (&eq)[WT], uint32_t (&Pv)[WT], uint32_t (&Mv)[WT], int& score) {
  uint32_t carry = 0, ph_in = 1, mh_in = 0;                       // Ph = (Ph << 1) | 1, Mh <<= 1
#pragma unroll
  for (int w = 0; w < WT; ++w) {
    const uint32_t e = eq[w], pv = Pv[w], mv = Mv[w];
    const uint32_t xv = e | mv;
    const uint32_t sum = __builtin_addc(e & pv, pv, carry, &carry);
    const uint32_t xh = (sum ^ pv) | e;
    const uint32_t ph = mv | ~(xh | pv);
    const uint32_t mh = pv & xh;
    const uint32_t phs = (ph << 1) | ph_in, mhs = (mh << 1) | mh_in;
    ph_in = ph >> 31;
    mh_in = mh >> 31;
    Pv[w] = mhs | ~(xv | phs);
    Mv[w] = phs & xv;
  }
  score += (int)ph_in - (int)mh_in;
}

// The table's value on the diagonal that ends in its last cell, `rest` columns before the end: the score (the last row) minus the
// vertical steps of the `rest` rows above it, which are the top `rest` bits of Pv (+1) and Mv (-1). Values never fall along a
// diagonal, so the final distance is at least this. rest >= the query's length: the mask takes every row, the value is the column
// number, which is no more than the difference of the lengths and so a bound as well. rest is wave-uniform: the masks are scalar.
template <int WT>
__device__ __forceinline__ int edit_diagonal(const uint32_t (&Pv)[WT], const uint32_t (&Mv)[WT], int score, int rest) {
  int up = 0, down = 0;
#pragma unroll
  for (int w = 0; w < WT; ++w) {
    const int lo = 32 * (WT - w) - rest;                            // the word's bits below this one are below the diagonal's row
    const uint32_t mask = lo <= 0 ? 0xFFFFFFFFu : lo >= 32 ? 0u : 0xFFFFFFFFu << lo;
    up += __popc(Pv[w] & mask);
    down += __popc(Mv[w] & mask);
  }
  return score - up + down;
}

// grid (ceil(B / QB), segments of seg_rows database rows). A thread owns one query of m = Lq <= 32 WT positions as four bit planes
// (one per token) placed at the TOP of the 32 WT bits: position i is bit off + i, off = 32 WT - m. The off bits below hold no
// plane bit and start with Pv = Mv = 0; such a bit keeps Pv = Mv = 0 for ever and hands Ph = 1, Mh = 0 and no carry upwards, which
// is what row 0 of the table hands to row 1 — so a shorter query needs no other code and the score bit never moves. The database
// token is read from the LDS tile by every lane at one address and made scalar, so the plane is chosen by a scalar branch.
// Every 16 columns a wave leaves the row if no lane can still use it: the diagonal's value (edit_diagonal) is a lower bound of the
// final distance, and a lane's limit is cap with hist and, without, min(cap, the distance of the key it read, the best it found).
// A workgroup's u32 bins hold at most QB * seg_rows < 2^32 pairs (the host keeps seg_rows <= 2^22).
template <int WT>
__global__ __launch_bounds__(QB) void edit_nn_kernel(EditArgs a) {
  __shared__ uint32_t tile[ED_TILE * ED_MAXW];
  __shared__ unsigned int h[HM_MAXL + 2];
  const bool want_hist = a.hist != nullptr;
  if (want_hist) {
    for (int i = threadIdx.x; i < a.cap + 2; i += QB) h[i] = 0;
  }
  const int qi = blockIdx.x * QB + threadIdx.x;
  const bool live = qi < a.B;
  const int m = a.Lq, off = 32 * WT - m;
  uint32_t eA[WT], eC[WT], eG[WT], eT[WT];
#pragma unroll
  for (int w = 0; w < WT; ++w) {
    uint32_t pa = 0, pc = 0, pg = 0, pt = 0;
    if (live && 32 * (w + 1) > off) {
      const uint32_t* row = a.q + (long long)qi * a.Wq;
      for (int b = max(0, off - 32 * w); b < 32; ++b) {
        const int i = 32 * w + b - off;                              // 0 <= i < m: the padding bits of the row are never read
        const uint32_t t = (row[i >> 4] >> (2 * (i & 15))) & 3u;
        const uint32_t bit = 1u << b;
        pa |= t == 0u ? bit : 0u;
        pc |= t == 1u ? bit : 0u;
        pg |= t == 2u ? bit : 0u;
        pt |= t == 3u ? bit : 0u;
      }
    }
    eA[w] = pa, eC[w] = pc, eG[w] = pg, eT[w] = pt;
  }
  const int seg0 = (int)min((long long)blockIdx.y * a.seg_rows, (long long)a.N);
  const int seg1 = (int)min((long long)seg0 + a.seg_rows, (long long)a.N);
  const long long diag = a.exclude_diag ? (long long)a.q_base + qi - a.db_base : -1;
  int limit = a.cap;                                               // the largest distance this lane can still use
  if (!want_hist && live) {
    const unsigned long long k = __atomic_load_n(&a.nn_key[qi], __ATOMIC_RELAXED);
    limit = (int)min((unsigned long long)a.cap, k >> 32);
  }
  unsigned int best_d = 0xFFFFFFFFu, beyond = 0;
  int best_j = 0;
  for (int t0 = seg0; t0 < seg1; t0 += ED_TILE) {
    const int nr = min(ED_TILE, seg1 - t0);
    __syncthreads();                                              // the previous tile is read (and h is zeroed)
    for (int i = threadIdx.x; i < nr * a.Wd; i += QB) tile[i] = a.db[(long long)t0 * a.Wd + i];
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
      const bool mine = live && (long long)(t0 + r) != diag;
      uint32_t Pv[WT], Mv[WT];
#pragma unroll
      for (int w = 0; w < WT; ++w) Pv[w] = eA[w] | eC[w] | eG[w] | eT[w], Mv[w] = 0u;
      int score = m;
      bool left = false;
      for (int j0 = 0; j0 < a.Ld; j0 += 16) {
        uint32_t word = __builtin_amdgcn_readfirstlane(tile[r * a.Wd + (j0 >> 4)]);
        const int nj = min(16, a.Ld - j0);
        for (int jj = 0; jj < nj; ++jj, word >>= 2) {
          switch (word & 3u) {
            case 0: edit_column<WT>(eA, Pv, Mv, score); break;
            case 1: edit_column<WT>(eC, Pv, Mv, score); break;
            case 2: edit_column<WT>(eG, Pv, Mv, score); break;
            default: edit_column<WT>(eT, Pv, Mv, score); break;
          }
        }
        const int rest = a.Ld - j0 - nj;                            // columns still to come
        if (rest > 0 && __all(!mine || edit_diagonal<WT>(Pv, Mv, score, rest) > limit)) { left = true; break; }
      }
      if (mine) {
        const unsigned int d = left ? 0xFFFFFFFFu : (unsigned int)score;
        if (d <= (unsigned int)a.cap) {
          if (want_hist) atomicAdd(&h[d], 1u);
          if (d < best_d && d <= (unsigned int)limit) {
            best_d = d, best_j = t0 + r;
            if (!want_hist) limit = (int)d;
          }
        } else {
          ++beyond;
        }
      }
    }
  }
  if (live && a.nn_key && best_d != 0xFFFFFFFFu)
    atomicMin(&a.nn_key[qi], ((unsigned long long)best_d << 32) | (unsigned long long)(uint32_t)(a.db_base + best_j));
  if (want_hist) {
    if (beyond) atomicAdd(&h[a.cap + 1], beyond);
    __syncthreads();
    for (int i = threadIdx.x; i < a.cap + 2; i += QB)
      if (h[i]) atomicAdd(&a.hist[i], (unsigned long long)h[i]);
  }
}

struct WithinArgs {
  const uint32_t* q;
  const uint32_t* q_rc;                      // the packed reverse complements of the queries, or NULL
  const uint32_t* db;
  const int32_t* db_count;                   // device: only the rows j < min(N, *db_count) exist; NULL: all N
  int B, N, W, radius, seg_rows, mask_words;
  uint32_t last_mask;
  int32_t* first;
  uint32_t* mask;
};

// grid (ceil(B / QB), segments of seg_rows database rows, seg_rows a multiple of HM_TILE). hamming_nn_kernel's skeleton with a
// threshold in place of the minimum: d = row_distance to the query, with RC the smaller of that and the distance to the query's
// reverse complement. A tile is two mask words: the owning thread gathers 32 database rows into a register and stores the word, so
// mask needs neither atomics nor zeroing; the words of its segment that no live tile covers (rows beyond the device count, and for
// the last segment everything up to mask_words) are stored as zeros. first: the lowest hit of the segment (ascending rows: the
// first one seen), one integer atomic min per query that has one.
template <int WT, int WS, bool RC>
__global__ __launch_bounds__(QB) void within_kernel(WithinArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[HM_TILE * WS];
  const int qi = blockIdx.x * QB + threadIdx.x;
  const bool live = qi < a.B;
  const int n = a.db_count ? max(0, min(a.N, *a.db_count)) : a.N;   // one address for the whole grid: a scalar load
  const long long seg_lo = (long long)blockIdx.y * a.seg_rows;     // < N: the host sizes the grid from N
  const bool last_seg = blockIdx.y == gridDim.y - 1;
  const int word_lo = (int)(seg_lo / 32);
  const int word_hi = last_seg ? a.mask_words : (int)((seg_lo + a.seg_rows) / 32);    // <= ceil(N / 32) <= mask_words otherwise
  uint32_t* mrow = a.mask && live ? a.mask + (long long)qi * a.mask_words : nullptr;
  const int seg0 = (int)min(seg_lo, (long long)n);
  const int seg1 = (int)min(seg_lo + a.seg_rows, (long long)n);
  if (seg0 >= seg1) {                                              // the segment starts at or beyond the device count
    if (mrow)
      for (int w = word_lo; w < word_hi; ++w) mrow[w] = 0u;
    return;
  }
  uint32_t q[WT], qr[RC ? WT : 1];
#pragma unroll
  for (int w = 0; w < WT; ++w) {
    const uint32_t keep = w == a.W - 1 ? a.last_mask : 0xFFFFFFFFu;
    q[w] = live && w < a.W ? a.q[(long long)qi * a.W + w] & keep : 0u;
    if constexpr (RC) qr[w] = live && w < a.W ? a.q_rc[(long long)qi * a.W + w] & keep : 0u;
  }
  int hit = INT32_MAX;
  int word = word_lo;                                              // the next mask word this thread stores
  for (int t0 = seg0; t0 < seg1; t0 += HM_TILE) {
    const int nr = min(HM_TILE, seg1 - t0);
    __syncthreads();                                              // the previous tile is read
    for (int i = threadIdx.x; i < nr * WS; i += QB) {
      const int r = i / WS, w = i - r * WS;
      tile[i] = w < a.W ? a.db[(long long)(t0 + r) * a.W + w] & (w == a.W - 1 ? a.last_mask : 0xFFFFFFFFu) : 0u;
    }
    __syncthreads();
    if (live) {
#pragma unroll
      for (int half = 0; half < HM_TILE / 32; ++half) {
        uint32_t bits = 0;
        const int r1 = min(32, nr - 32 * half);
#pragma unroll 2
        for (int r = 0; r < r1; ++r) {
          int d = row_distance<WT, WS>(q, &tile[(32 * half + r) * WS]);
          if constexpr (RC) d = min(d, row_distance<WT, WS>(qr, &tile[(32 * half + r) * WS]));
          if (d <= a.radius) {
            bits |= 1u << r;
            hit = min(hit, t0 + 32 * half + r);
          }
        }
        if (mrow && word < word_hi) mrow[word] = bits;
        ++word;
      }
    }
  }
  if (mrow)
    for (; word < word_hi; ++word) mrow[word] = 0u;
  if (live && a.first && hit != INT32_MAX) atomicMin(&a.first[qi], hit);
}

template <bool RC>
int launch_within(const WithinArgs& a, dim3 grid, void* on_stream) {
  SvddSpan span(SVDD_SLOT_WITHIN);
  const int W = a.W;
  void (*k)(WithinArgs) = W <= 1 ? within_kernel<1, 1, RC> : W <= 2 ? within_kernel<2, 2, RC> : W <= 4 ? within_kernel<4, 4, RC>
                        : W <= 8 ? within_kernel<8, 8, RC> : W <= 13 ? within_kernel<13, 16, RC> : W <= 16 ? within_kernel<16, 16, RC>
                        : W <= 32 ? within_kernel<32, 32, RC> : within_kernel<64, 64, RC>;
  return svdd_launch_timed(span.all(), k, grid, dim3(QB), 0, on_stream, a);
}

struct EditWithinArgs {
  const uint32_t* q;
  const uint32_t* db;
  const int32_t* db_count;                   // device: only the rows j < min(N, *db_count) exist; NULL: all N
  int B, N, L, W, radius, both, seg_rows, mask_words;
  int32_t* first;
  uint32_t* mask;
};

// One staged database row (W packed words in LDS, every lane at one address) against the lane's query planes: edit_nn_kernel's
// row walk with ONE limit for the whole wave. REV: the row is walked from its last token to its first and every token t is read
// as 3 - t, which is the walk over the row's reverse complement; lev(rc(q), row) = lev(q, rc(row)) (reversing both strings, and
// passing both through one bijection of the alphabet, leaves the distance as it is), so the second strand needs no second set of
// planes. At every packed word (16 columns) the wave leaves the row when the diagonal bound of every lane that still `need`s the
// row is beyond the limit -> true, and score means nothing; false: score is the distance. Nothing here differs between lanes but
// the planes: the token is scalar, the plane is chosen by a scalar branch, `rest` is scalar.
template <int WT, bool REV>
__device__ __forceinline__ bool edit_row_walk(const uint32_t (&eA)[WT], const uint32_t (&eC)[WT], const uint32_t (&eG)[WT],
                                              const uint32_t (&eT)[WT], const uint32_t* row, int L, int W, bool need, int limit,
                                              int& score) {
  uint32_t Pv[WT], Mv[WT];
#pragma unroll
  for (int w = 0; w < WT; ++w) Pv[w] = eA[w] | eC[w] | eG[w] | eT[w], Mv[w] = 0u;
  for (int c = 0; c < W; ++c) {
    const int w = REV ? W - 1 - c : c;
    uint32_t word = __builtin_amdgcn_readfirstlane(row[w]);
    const int nj = min(16, L - 16 * w);
    if (REV) word <<= 2 * (16 - nj);                                // the word's last token to the top; the padding bits fall out
    for (int jj = 0; jj < nj; ++jj) {
      const uint32_t t = REV ? 3u - (word >> 30) : word & 3u;
      word = REV ? word << 2 : word >> 2;
      switch (t) {
        case 0: edit_column<WT>(eA, Pv, Mv, score); break;
        case 1: edit_column<WT>(eC, Pv, Mv, score); break;
        case 2: edit_column<WT>(eG, Pv, Mv, score); break;
        default: edit_column<WT>(eT, Pv, Mv, score); break;
      }
    }
    const int rest = REV ? 16 * w : L - 16 * w - nj;                // columns still to come
    if (rest > 0 && __all(!need || edit_diagonal<WT>(Pv, Mv, score, rest) > limit)) return true;
  }
  return false;
}

// grid (ceil(B / QB), segments of seg_rows database rows, seg_rows a multiple of ED_TILE). edit_nn_kernel's skeleton (a thread owns
// one query as four bit planes at the top of 32 WT bits; 256 queries walk a segment in LDS tiles of 64 rows) with within_kernel's
// outputs: a tile is two mask words, the owning thread gathers 32 rows into a register and stores the word; the words of the
// segment that no live tile covers are stored as zeros; first takes one integer atomic min per query that has a hit. The limit of
// every lane is the radius. With both strands the row is walked a second time (edit_row_walk<REV>) only when a lane of the wave
// did not hit on the first.
template <int WT>
__global__ __launch_bounds__(QB) void edit_within_kernel(EditWithinArgs a) {
  __shared__ uint32_t tile[ED_TILE * ED_MAXW];
  const int qi = blockIdx.x * QB + threadIdx.x;
  const bool live = qi < a.B;
  const int n = a.db_count ? max(0, min(a.N, *a.db_count)) : a.N;   // one address for the whole grid: a scalar load
  const long long seg_lo = (long long)blockIdx.y * a.seg_rows;     // < N: the host sizes the grid from N
  const bool last_seg = blockIdx.y == gridDim.y - 1;
  const int word_lo = (int)(seg_lo / 32);
  const int word_hi = last_seg ? a.mask_words : (int)((seg_lo + a.seg_rows) / 32);    // <= ceil(N / 32) <= mask_words otherwise
  uint32_t* mrow = a.mask && live ? a.mask + (long long)qi * a.mask_words : nullptr;
  const int seg0 = (int)min(seg_lo, (long long)n);
  const int seg1 = (int)min(seg_lo + a.seg_rows, (long long)n);
  if (seg0 >= seg1) {                                              // the segment starts at or beyond the device count
    if (mrow)
      for (int w = word_lo; w < word_hi; ++w) mrow[w] = 0u;
    return;
  }
  const int m = a.L, off = 32 * WT - m;
  uint32_t eA[WT], eC[WT], eG[WT], eT[WT];
#pragma unroll
  for (int w = 0; w < WT; ++w) {
    uint32_t pa = 0, pc = 0, pg = 0, pt = 0;
    if (live && 32 * (w + 1) > off) {
      const uint32_t* row = a.q + (long long)qi * a.W;
      for (int b = max(0, off - 32 * w); b < 32; ++b) {
        const int i = 32 * w + b - off;                              // 0 <= i < m: the padding bits of the row are never read
        const uint32_t t = (row[i >> 4] >> (2 * (i & 15))) & 3u;
        const uint32_t bit = 1u << b;
        pa |= t == 0u ? bit : 0u;
        pc |= t == 1u ? bit : 0u;
        pg |= t == 2u ? bit : 0u;
        pt |= t == 3u ? bit : 0u;
      }
    }
    eA[w] = pa, eC[w] = pc, eG[w] = pg, eT[w] = pt;
  }
  int hit = INT32_MAX;
  int word = word_lo;                                              // the next mask word this thread stores
  for (int t0 = seg0; t0 < seg1; t0 += ED_TILE) {
    const int nr = min(ED_TILE, seg1 - t0);
    __syncthreads();                                              // the previous tile is read
    for (int i = threadIdx.x; i < nr * a.W; i += QB) tile[i] = a.db[(long long)t0 * a.W + i];
    __syncthreads();
    for (int half = 0; half < ED_TILE / 32; ++half) {
      uint32_t bits = 0;
      const int r1 = min(32, nr - 32 * half);
      for (int r = 0; r < r1; ++r) {
        const uint32_t* row = &tile[(32 * half + r) * a.W];
        int score = m;
        bool in = !edit_row_walk<WT, false>(eA, eC, eG, eT, row, a.L, a.W, live, a.radius, score) && score <= a.radius;
        if (a.both && __any(live && !in)) {
          score = m;
          in = in || (!edit_row_walk<WT, true>(eA, eC, eG, eT, row, a.L, a.W, live && !in, a.radius, score) && score <= a.radius);
        }
        if (live && in) {
          bits |= 1u << r;
          hit = min(hit, t0 + 32 * half + r);
        }
      }
      if (mrow && word < word_hi) mrow[word] = bits;
      ++word;
    }
  }
  if (mrow)
    for (; word < word_hi; ++word) mrow[word] = 0u;
  if (live && a.first && hit != INT32_MAX) atomicMin(&a.first[qi], hit);
}

struct EditPairsArgs {
  const uint32_t* q;
  const uint32_t* db;
  const int32_t* idx;
  int B, N, Lq, Ld, Wq, Wd, cap, both;
  int32_t* dist;
};

// One thread per pair (q_i, db[idx[i]]): the same planes and the same column step, but every lane has a database row of its own,
// so the plane is chosen per lane by selects and the row's words are read from global memory as they are needed. B pairs, not
// B N: this is not a hot path. The second strand as in edit_row_walk: the row backwards, every token t read as 3 - t.
template <int WT>
__global__ __launch_bounds__(64) void edit_pairs_kernel(EditPairsArgs a) {
  const int qi = blockIdx.x * 64 + threadIdx.x;
  if (qi >= a.B) return;
  const int j = a.idx[qi];
  if (j < 0 || j >= a.N) {
    a.dist[qi] = -1;
    return;
  }
  const int m = a.Lq, off = 32 * WT - m;
  const uint32_t* qrow = a.q + (long long)qi * a.Wq;
  const uint32_t* row = a.db + (long long)j * a.Wd;
  uint32_t eA[WT], eC[WT], eG[WT], eT[WT];
#pragma unroll
  for (int w = 0; w < WT; ++w) {
    uint32_t pa = 0, pc = 0, pg = 0, pt = 0;
    for (int b = max(0, off - 32 * w); b < 32; ++b) {
      const int i = 32 * w + b - off;                                // 0 <= i < m: the padding bits of the row are never read
      const uint32_t t = (qrow[i >> 4] >> (2 * (i & 15))) & 3u;
      const uint32_t bit = 1u << b;
      pa |= t == 0u ? bit : 0u;
      pc |= t == 1u ? bit : 0u;
      pg |= t == 2u ? bit : 0u;
      pt |= t == 3u ? bit : 0u;
    }
    eA[w] = pa, eC[w] = pc, eG[w] = pg, eT[w] = pt;
  }
  int best = INT32_MAX;
  for (int strand = 0; strand < (a.both ? 2 : 1); ++strand) {
    uint32_t Pv[WT], Mv[WT];
#pragma unroll
    for (int w = 0; w < WT; ++w) Pv[w] = eA[w] | eC[w] | eG[w] | eT[w], Mv[w] = 0u;
    int score = m;
    for (int c = 0; c < a.Ld; ++c) {
      const int l = strand ? a.Ld - 1 - c : c;
      uint32_t t = (row[l >> 4] >> (2 * (l & 15))) & 3u;
      if (strand) t = 3u - t;
      uint32_t eq[WT];
#pragma unroll
      for (int w = 0; w < WT; ++w) eq[w] = t == 0u ? eA[w] : t == 1u ? eC[w] : t == 2u ? eG[w] : eT[w];
      edit_column<WT>(eq, Pv, Mv, score);
    }
    best = min(best, score);
  }
  a.dist[qi] = best <= a.cap ? best : -1;
}

constexpr int GP_MAXT = 4096;              // rows of one greedy_pick block: 128 words of the suppressed set, two per lane
constexpr int GP_WAVE = 64;

struct PickArgs {
  const uint32_t* mask;
  const int32_t* first;
  const uint32_t* rows;
  int T, W, mask_words, base, k, cap;
  int32_t* count;
  uint32_t* reps;
  int32_t* picked_rank;
  int32_t* rep_pick;
};

__device__ __forceinline__ uint32_t lane_word(uint32_t s0, uint32_t s1, int w) {    // word w of the set, w wave-uniform
  return w < GP_WAVE ? __builtin_amdgcn_readlane(s0, w) : __builtin_amdgcn_readlane(s1, w - GP_WAVE);
}

// ONE wave. The set of rows that are settled (suppressed, picked, or represented by an earlier block's pick through `first`) is a
// bit set of T <= 4096 bits held in registers: lane l has words l and 64 + l. The walk reads the current word with a cross-lane
// read and visits only its zero bits, in order; everything it branches on is wave-uniform. A pick loads its own mask row (lane l
// the words l and 64 + l), ORs it in, and every lane writes the pick's number to the rows its words newly settle — the pick
// itself among them. Bits j <= i of the row change nothing: those rows are settled already. Rows settled later never load their
// mask row. When min(k, cap) picks exist the walk ends and the rows still open get -1.
__global__ __launch_bounds__(GP_WAVE) void greedy_pick_kernel(PickArgs a) {
  const int lane = threadIdx.x;
  int count = *a.count;
  if (count < 0 || count > a.cap) return;                          // a count the state cannot hold: nothing is written
  const int limit = min(a.k, a.cap);
  const int nw = (a.T + 31) / 32;
  // padding bits of the last word count as settled: never visited, never written
  auto valid = [&](int w) { return w >= nw ? 0u : w == nw - 1 && a.T % 32 ? (1u << (a.T % 32)) - 1u : 0xFFFFFFFFu; };
  uint32_t s0 = ~valid(lane), s1 = ~valid(GP_WAVE + lane);
  if (a.first) {
    for (int c = 0; 64 * c < a.T; ++c) {                           // 64 rows at a time, coalesced; the ballot is two words of the set
      const int i = 64 * c + lane;
      const int f = i < a.T ? a.first[i] : INT32_MAX;
      if (f != INT32_MAX) a.rep_pick[i] = f;
      const unsigned long long has = __ballot(f != INT32_MAX);
      const int w = 2 * c;
      if (lane == (w & 63)) (w < GP_WAVE ? s0 : s1) |= (uint32_t)has;
      if (lane == ((w + 1) & 63)) (w + 1 < GP_WAVE ? s0 : s1) |= (uint32_t)(has >> 32);
    }
  }
  bool full = false;
  for (int wi = 0; wi < nw && !full; ++wi) {
    uint32_t open = ~lane_word(s0, s1, wi);
    while (open) {
      if (count >= limit) { full = true; break; }
      const int b = __ffs(open) - 1, i = 32 * wi + b, p = count++;
      const uint32_t* mr = a.mask + (long long)i * a.mask_words;
      uint32_t m0 = lane < nw ? mr[lane] : 0u, m1 = GP_WAVE + lane < nw ? mr[GP_WAVE + lane] : 0u;
      if (lane == (wi & 63)) (wi < GP_WAVE ? m0 : m1) |= 1u << b;   // the pick settles itself, whatever the diagonal holds
      const uint32_t n0 = m0 & ~s0, n1 = m1 & ~s1;
      s0 |= n0, s1 |= n1;
      for (uint32_t v = n0; v; v &= v - 1) a.rep_pick[32 * lane + __ffs(v) - 1] = p;
      for (uint32_t v = n1; v; v &= v - 1) a.rep_pick[32 * (GP_WAVE + lane) + __ffs(v) - 1] = p;
      if (lane < a.W) a.reps[(long long)p * a.W + lane] = a.rows[(long long)i * a.W + lane];
      if (lane == 0) a.picked_rank[p] = a.base + i;
      open = ~lane_word(s0, s1, wi);
    }
  }
  for (uint32_t v = ~s0; v; v &= v - 1) a.rep_pick[32 * lane + __ffs(v) - 1] = -1;
  for (uint32_t v = ~s1; v; v &= v - 1) a.rep_pick[32 * (GP_WAVE + lane) + __ffs(v) - 1] = -1;
  if (lane == 0) *a.count = count;
}

}  // namespace

extern "C" {

int svdd_kmer_counts(const uint8_t* x, int N, int L, int k, int64_t* counts, int64_t* skipped, void* on_stream) {
  if (!x || !counts || N <= 0 || L <= 0 || k < 1 || k > KM_MAXK) return SVDD_E_ARG;
  if (k > L) return SVDD_OK;                                      // no windows: nothing is written
  // rows per workgroup: enough workgroups to fill the chip, few enough rows that rows * windows stays below 2^32
  const long long nw = L - k + 1;
  long long rows = ((long long)N + 2047) / 2048;
  const long long cap = 0xFFFFFFFFll / nw;                         // >= 1: nw < 2^31
  if (rows > cap) rows = cap;
  const long long wgs = ((long long)N + rows - 1) / rows;
  const KmerArgs a{x, N, L, k, (int)rows, (unsigned long long*)counts, (unsigned long long*)skipped};
  return svdd_launch(kmer_counts_kernel, dim3((unsigned)wgs), dim3(QB), 0, on_stream, a);
}

int svdd_pack_tokens(const uint8_t* x, int N, int L, uint32_t* packed, int32_t* err, void* on_stream) {
  if (!x || !packed || N <= 0 || L <= 0 || L > HM_MAXL) return SVDD_E_ARG;
  const int W = (L + 15) / 16;
  const long long blocks = ((long long)N * W + QB - 1) / QB;
  const PackArgs a{x, N, L, W, packed, err};
  return svdd_launch(pack_tokens_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(QB), 0, on_stream, a);
}

int svdd_hamming_nn(const uint32_t* q, const uint32_t* db, int B, int N, int L, int q_base, int db_base, int exclude_diag,
                    uint64_t* nn_key, int64_t* hist, void* on_stream) {
  if (!q || !db || (!nn_key && !hist) || B <= 0 || N <= 0 || L <= 0 || L > HM_MAXL || q_base < 0 || db_base < 0) return SVDD_E_ARG;
  if ((long long)db_base + N >= (long long)1 << 31 || (long long)q_base + B >= (long long)1 << 31) return SVDD_E_ARG;
  const int W = (L + 15) / 16;
  const unsigned gx = (unsigned)((B + QB - 1) / QB);
  // segments: about 1024 workgroups in all, whole tiles, at most 2^22 rows (QB * 2^22 pairs < 2^32 in a workgroup's u32 bins)
  const long long want = (1024 + gx - 1) / gx;
  long long seg = ((long long)N + want - 1) / want;
  seg = (seg + HM_TILE - 1) / HM_TILE * HM_TILE;
  if (seg > (1 << 22)) seg = 1 << 22;
  const unsigned gy = (unsigned)(((long long)N + seg - 1) / seg);
  const uint32_t last_mask = L % 16 ? (1u << (2 * (L % 16))) - 1u : 0xFFFFFFFFu;
  const HammingArgs a{q, db, B, N, L, W, q_base, db_base, exclude_diag, (int)seg, last_mask, (unsigned long long*)nn_key,
                      (unsigned long long*)hist};
  void (*k)(HammingArgs) = W <= 1 ? hamming_nn_kernel<1, 1> : W <= 2 ? hamming_nn_kernel<2, 2> : W <= 4 ? hamming_nn_kernel<4, 4>
                         : W <= 8 ? hamming_nn_kernel<8, 8> : W <= 13 ? hamming_nn_kernel<13, 16> : W <= 16 ? hamming_nn_kernel<16, 16>
                         : W <= 32 ? hamming_nn_kernel<32, 32> : hamming_nn_kernel<64, 64>;
  return svdd_launch(k, dim3(gx, gy), dim3(QB), 0, on_stream, a);
}

int svdd_edit_nn(const uint32_t* q, const uint32_t* db, int B, int N, int Lq, int Ld, int cap, int q_base, int db_base,
                 int exclude_diag, uint64_t* nn_key, int64_t* hist, void* on_stream) {
  if (!q || !db || (!nn_key && !hist) || B <= 0 || N <= 0 || Lq <= 0 || Ld <= 0 || Lq > HM_MAXL || Ld > HM_MAXL) return SVDD_E_ARG;
  if (cap < 0 || cap > (Lq > Ld ? Lq : Ld) || q_base < 0 || db_base < 0) return SVDD_E_ARG;
  if ((long long)db_base + N >= (long long)1 << 31 || (long long)q_base + B >= (long long)1 << 31) return SVDD_E_ARG;
  const unsigned gx = (unsigned)((B + QB - 1) / QB);
  // a pair costs Ld columns of ceil(Lq / 32) words, thousands of times a Hamming pair: about 4096 workgroups in all so that the
  // last ones to finish are short; whole tiles, at most 2^22 rows (QB * 2^22 pairs < 2^32 in a workgroup's u32 bins)
  const long long want = (4096 + gx - 1) / gx;
  long long seg = ((long long)N + want - 1) / want;
  seg = (seg + ED_TILE - 1) / ED_TILE * ED_TILE;
  if (seg > (1 << 22)) seg = 1 << 22;
  const unsigned gy = (unsigned)(((long long)N + seg - 1) / seg);
  const EditArgs a{q, db, B, N, Lq, Ld, (Lq + 15) / 16, (Ld + 15) / 16, cap, q_base, db_base, exclude_diag, (int)seg,
                   (unsigned long long*)nn_key, (unsigned long long*)hist};
  const int W = (Lq + 31) / 32;
  void (*k)(EditArgs) = W <= 1 ? edit_nn_kernel<1> : W <= 2 ? edit_nn_kernel<2> : W <= 4 ? edit_nn_kernel<4> : W <= 7 ? edit_nn_kernel<7>
                      : W <= 8 ? edit_nn_kernel<8> : W <= 16 ? edit_nn_kernel<16> : edit_nn_kernel<32>;
  return svdd_launch(k, dim3(gx, gy), dim3(QB), 0, on_stream, a);
}

int svdd_within(const uint32_t* q, const uint32_t* q_rc, const uint32_t* db, const int32_t* db_count, int B, int N, int L, int radius,
                int32_t* first, uint32_t* mask, int mask_words, void* on_stream) {
  if (!q || !db || (!first && !mask) || B <= 0 || N <= 0 || L <= 0 || L > HM_MAXL || radius < 0 || radius >= L) return SVDD_E_ARG;
  if (mask && (long long)mask_words * 32 < N) return SVDD_E_ARG;
  const int W = (L + 15) / 16;
  const unsigned gx = (unsigned)((B + QB - 1) / QB);
  // segments as svdd_hamming_nn's: about 1024 workgroups in all, whole tiles (so whole mask words), sized from N, the host's
  // upper bound of the device count
  const long long want = (1024 + gx - 1) / gx;
  long long seg = ((long long)N + want - 1) / want;
  seg = (seg + HM_TILE - 1) / HM_TILE * HM_TILE;
  if (seg > (1 << 22)) seg = 1 << 22;
  const unsigned gy = (unsigned)(((long long)N + seg - 1) / seg);
  const uint32_t last_mask = L % 16 ? (1u << (2 * (L % 16))) - 1u : 0xFFFFFFFFu;
  const WithinArgs a{q, q_rc, db, db_count, B, N, W, radius, (int)seg, mask ? mask_words : 0, last_mask, first, mask};
  return q_rc ? launch_within<true>(a, dim3(gx, gy), on_stream) : launch_within<false>(a, dim3(gx, gy), on_stream);
}

int svdd_edit_within(const uint32_t* q, const uint32_t* db, const int32_t* db_count, int B, int N, int L, int radius,
                     int both_strands, int32_t* first, uint32_t* mask, int mask_words, void* on_stream) {
  if (!q || !db || (!first && !mask) || B <= 0 || N <= 0 || L <= 0 || L > HM_MAXL || radius < 0 || radius >= L) return SVDD_E_ARG;
  if (mask && (long long)mask_words * 32 < N) return SVDD_E_ARG;
  const unsigned gx = (unsigned)((B + QB - 1) / QB);
  // segments as svdd_edit_nn's (a pair costs thousands of times a Hamming pair: about 4096 workgroups in all), whole tiles (so
  // whole mask words), sized from N, the host's upper bound of the device count
  const long long want = (4096 + gx - 1) / gx;
  long long seg = ((long long)N + want - 1) / want;
  seg = (seg + ED_TILE - 1) / ED_TILE * ED_TILE;
  const unsigned gy = (unsigned)(((long long)N + seg - 1) / seg);
  const EditWithinArgs a{q, db, db_count, B, N, L, (L + 15) / 16, radius, both_strands != 0, (int)seg, mask ? mask_words : 0, first, mask};
  const int W = (L + 31) / 32;
  void (*k)(EditWithinArgs) = W <= 1 ? edit_within_kernel<1> : W <= 2 ? edit_within_kernel<2> : W <= 4 ? edit_within_kernel<4>
                            : W <= 7 ? edit_within_kernel<7> : W <= 8 ? edit_within_kernel<8> : W <= 16 ? edit_within_kernel<16>
                            : edit_within_kernel<32>;
  SvddSpan span(SVDD_SLOT_EDIT_WITHIN);
  return svdd_launch_timed(span.all(), k, dim3(gx, gy), dim3(QB), 0, on_stream, a);
}

int svdd_edit_pairs(const uint32_t* q, const uint32_t* db, const int32_t* idx, int B, int N, int Lq, int Ld, int cap,
                    int both_strands, int32_t* dist, void* on_stream) {
  if (!q || !db || !idx || !dist || B <= 0 || N <= 0 || Lq <= 0 || Ld <= 0 || Lq > HM_MAXL || Ld > HM_MAXL) return SVDD_E_ARG;
  if (cap < 0 || cap > (Lq > Ld ? Lq : Ld)) return SVDD_E_ARG;
  const EditPairsArgs a{q, db, idx, B, N, Lq, Ld, (Lq + 15) / 16, (Ld + 15) / 16, cap, both_strands != 0, dist};
  const int W = (Lq + 31) / 32;
  void (*k)(EditPairsArgs) = W <= 1 ? edit_pairs_kernel<1> : W <= 2 ? edit_pairs_kernel<2> : W <= 4 ? edit_pairs_kernel<4>
                           : W <= 7 ? edit_pairs_kernel<7> : W <= 8 ? edit_pairs_kernel<8> : W <= 16 ? edit_pairs_kernel<16>
                           : edit_pairs_kernel<32>;
  return svdd_launch(k, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, on_stream, a);
}

int svdd_greedy_pick(const uint32_t* mask, int mask_words, const int32_t* first, const uint32_t* rows, int T, int L, int base, int k,
                     int32_t* count, uint32_t* reps, int32_t* picked_rank, int cap, int32_t* rep_pick, void* on_stream) {
  if (!mask || !rows || !count || !reps || !picked_rank || !rep_pick) return SVDD_E_ARG;
  if (T < 1 || T > GP_MAXT || L <= 0 || L > HM_MAXL || k < 1 || cap < 1 || (long long)mask_words * 32 < T) return SVDD_E_ARG;
  if (base < 0 || (long long)base + T >= (long long)1 << 31) return SVDD_E_ARG;
  SvddSpan span(SVDD_SLOT_GREEDY_PICK);
  const PickArgs a{mask, first, rows, T, (L + 15) / 16, mask_words, base, k, cap, count, reps, picked_rank, rep_pick};
  return svdd_launch_timed(span.all(), greedy_pick_kernel, dim3(1), dim3(GP_WAVE), 0, on_stream, a);
}

}  // extern "C"
