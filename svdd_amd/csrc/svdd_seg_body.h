// svdd_seg_body.h — NOT a header: the body of backbone_seg_kernel<NC, ORD, DIL> and of backbone_seg_tight_kernel, the two segment
// kernels of the incremental stem (svdd_nets.hip). Each kernel sets `using LAY = ...` (SegAligned<..> / SegTight, compile-time
// constants only) and includes this text between its braces; `a` is the kernel's BackboneSegArgs. It is included text and not an
// inlined function because only so do the nine kernels keep the instruction streams they had as two hand-copied bodies, and the
// project's contract is bit equality with backbone_kernel, checked by comparing disassembly (profiles/backbone_shared_code.txt).
// For the same reason a few quantities keep the SHAPE each kernel gave them — a sum's order (SEG_AT, SEG_OWN_ROW), a local against
// an expression at each use (nrows_t, SEG_NROWS), where the item's low byte is taken (t0) — where one spelling would do
// arithmetically: the compiler's schedule follows them. Every condition on TIGHT / DIL / NC folds at compile time.
//
// Slots: f[s] / acc[s] hold 4 rows x 2 columns per lane of slot s. Aligned: slots 0 .. NC + 1 = halo tile, own tiles, halo tile,
// image row i = sequence row 16 (t0 - 1) + i. Tight: slots 0 .. NC - 1 = the own tiles, slot PK = both 4-row halos packed (lanes
// g = 0: left, g = 1: right, g = 2, 3: nothing), image row i = sequence row origin - 4 + i.
  constexpr int NC = LAY::NC, NS = LAY::NS, PK = LAY::PK, ROWS = LAY::ROWS, DIL = LAY::DIL;
  constexpr bool TIGHT = LAY::TIGHT;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* img = smem;                                      // [ROWS][BB_AP] image row i = sequence row r0 + i
  float* psum = img + ROWS * BB_AP;                       // [4][ROWS]
  float* rstat = psum + 4 * ROWS;                         // [ROWS]
  int* toks = reinterpret_cast<int*>(rstat + ROWS);       // [ROWS + 8] tokens of sequence rows r0 - 4 ..   (layer 1)

  int item, seq;
  if (LAY::ORD) {
    if ((int)blockIdx.x >= a.order_count[a.layer - 1]) return;
    const unsigned ent = (unsigned)__builtin_amdgcn_readfirstlane(a.order[(size_t)(a.layer - 1) * a.order_stride + blockIdx.x]);
    item = (int)(ent & 0xFFFFu);
    seq = (int)(ent >> 16);
  } else {
    item = __builtin_amdgcn_readfirstlane(a.items[(size_t)(a.layer - 1) * a.n * SEG_SLOTS + blockIdx.x]);
    seq = blockIdx.x / SEG_SLOTS;
  }
  const int nown = min(item >> 8, NC);
  if (nown == 0) return;
  const int t0 = item & 255;                              // the item's first tile (TIGHT: the low byte is its origin ROW)
  const int tid = threadIdx.x, lane = tid & 63;
  const int cg = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, g = lane >> 4;
  const int col0 = 32 * cg + j;
  const int L = a.L;
  const int r0 = TIGHT ? (item & 255) - 4 : 16 * (t0 - 1);   // sequence row of image row 0
  const int nrows_t = 16 * nown + 8;                      // TIGHT: image rows the item uses
  const bool halo = g < 2;                                // TIGHT: this lane holds rows of the packed slot
  const int hrow = g == 1 ? 16 * nown + 4 : 0;            // ... from this image row on
  const size_t pl_stride = (size_t)a.n * TW_ROWS * BB_C;
  float* pl0 = a.planes + (size_t)seq * TW_ROWS * BB_C;
  const int cl = a.layer - 1;                             // the conv layer this launch runs
  // slot S holds rows of this item ; ... and this lane holds some of them ; the lane's first image row of slot S (it holds 4)
#define SEG_LIVE(S) (TIGHT ? ((S) < nown || (S) == PK) : ((S) <= nown + 1))
#define SEG_MINE(S) (!TIGHT || (S) < PK || halo)
#define SEG_IROW(S) (TIGHT ? ((S) < PK ? 4 + 16 * (S) + 4 * g : hrow) : 16 * (S) + 4 * g)
#define SEG_AT(BASE, S) (TIGHT ? (BASE) + SEG_IROW(S) : (BASE) + 16 * (S) + 4 * g)   /* BASE + SEG_IROW(S), summed in each kernel's own order */
#define SEG_OWN(C) (TIGHT ? (C) : (C) + 1)                /* the slot of own tile C */
#define SEG_OWN_ROW(C) (TIGHT ? r0 + 4 + 16 * (C) + 4 * g : r0 + 16 * ((C) + 1) + 4 * g)   /* SEG_AT(r0, SEG_OWN(C)), in each kernel's own order */
#define SEG_NROWS (TIGHT ? nrows_t : 16 * (nown + 2))   /* image rows the item uses */

  f32x4 f[NS][2], acc[NS][2];
  if (a.layer == 1) {
    for (int e = tid; e < (TIGHT ? SEG_NROWS : ROWS) + 8; e += 256) {
      const int p = r0 - 4 + e;
      toks[e] = (p >= 0 && p < L) ? (int)a.x[(size_t)seq * L + p] : -1;
    }
    __syncthreads();
    // f_0 of the item's rows goes through the (still unused) image: thread (ri, c) builds row ri, channel c with its nine table
    // reads issued together, at a clamped index and with no branch between them — four elements (36 reads) per wait, 32 (ri, c)
    // pairs per thread for a 2-tile item. (Built straight into the MFMA layout, every lane made 9 dependent, branch-guarded reads
    // for each of its 32 elements: 288 round trips to L2 in a row, 24 us per launch; batching them THERE costs 128 - 168 VGPRs and
    // scratch.) A wave shares the row, so the reads of a tap are 256 consecutive bytes and the tokens are wave-uniform. The sum is
    // backbone_kernel's: start b0, taps in order, a tap outside the sequence SKIPPED (a select, never an added 0.0f: -0.0 must
    // stay -0.0).
    {
      const int c = tid & (BB_C - 1);
      const float b0 = a.vec[c];
#pragma unroll 4
      for (int ri = tid >> 7; ri < SEG_NROWS; ri += 2) {
        int tk[9];
        float tv[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          tk[t] = toks[ri + t];                           // sequence row r0 + ri + t - 4 ; -1 outside the sequence
          tv[t] = a.table0[(unsigned)((t * 5 + max(tk[t], 0)) * BB_C + c)];
        }
        float v = b0;
#pragma unroll
        for (int t = 0; t < 9; ++t) v = tk[t] >= 0 ? v + tv[t] : v;
        const int row = r0 + ri;
        img[ri * BB_AP + c] = (row >= 0 && row < L) ? fmaxf(v, 0.0f) : 0.0f;
      }
    }
    __syncthreads();                                      // (the image is next written behind the LayerNorm barriers below)
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (!SEG_LIVE(s)) continue;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int e = 0; e < 4; ++e) f[s][ct][e] = SEG_MINE(s) ? img[(SEG_IROW(s) + e) * BB_AP + col0 + 16 * ct] : 0.0f;
    }
  } else {
    const float* src = pl0 + (size_t)(a.layer - 2) * pl_stride;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (!SEG_LIVE(s)) continue;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = SEG_AT(r0, s) + e;
          f[s][ct][e] = (SEG_MINE(s) && row >= 0 && row < L) ? src[row * BB_C + col0 + 16 * ct] : 0.0f;
        }
    }
  }

  // ---- LayerNorm(f + tb) of the item's tiles and its halo -> image (backbone_kernel's passes, row for row)
  const float* vl = a.vec + (size_t)(cl + 1) * 4 * BB_C;
  {
    const float tb0 = vl[BB_C + col0], tb1 = vl[BB_C + col0 + 16];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (!SEG_LIVE(s)) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float sm = group16_sum((f[s][0][e] + tb0) + (f[s][1][e] + tb1));
        if (j == 0 && SEG_MINE(s)) psum[SEG_AT(cg * ROWS, s) + e] = sm;
      }
    }
    __syncthreads();
    if (tid < SEG_NROWS)
      rstat[tid] = ((psum[tid] + psum[ROWS + tid]) + (psum[2 * ROWS + tid] + psum[3 * ROWS + tid])) * (1.0f / BB_C);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (!SEG_LIVE(s)) continue;
      const float4 cur4 = *reinterpret_cast<const float4*>(SEG_AT(rstat, s));
      const float mean4[4] = {cur4.x, cur4.y, cur4.z, cur4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float mean = mean4[e];
        const float d0 = f[s][0][e] + tb0 - mean, d1 = f[s][1][e] + tb1 - mean;
        acc[s][0][e] = d0; acc[s][1][e] = d1;
        const float sq = group16_sum(d0 * d0 + d1 * d1);
        if (j == 0 && SEG_MINE(s)) psum[SEG_AT(cg * ROWS, s) + e] = sq;
      }
    }
    __syncthreads();
    if (tid < SEG_NROWS)
      rstat[tid] = rsqrtf(((psum[tid] + psum[ROWS + tid]) + (psum[2 * ROWS + tid] + psum[3 * ROWS + tid])) * (1.0f / BB_C) + 1e-5f);
    __syncthreads();
    const float gm0 = vl[2 * BB_C + col0], gm1 = vl[2 * BB_C + col0 + 16];
    const float bt0 = vl[3 * BB_C + col0], bt1 = vl[3 * BB_C + col0 + 16];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (!SEG_LIVE(s)) continue;
      const float4 cur4 = *reinterpret_cast<const float4*>(SEG_AT(rstat, s));
      const float rs4[4] = {cur4.x, cur4.y, cur4.z, cur4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ri = SEG_IROW(s) + e, row = r0 + ri;
        const float rs = rs4[e];
        const bool in = row >= 0 && row < L;              // rows outside the sequence are the zero padding of the convolution
        if (SEG_MINE(s)) {
          img[ri * BB_AP + col0] = in ? acc[s][0][e] * rs * gm0 + bt0 : 0.0f;
          img[ri * BB_AP + col0 + 16] = in ? acc[s][1][e] * rs * gm1 + bt1 : 0.0f;
        }
      }
    }
  }

  // ---- the convolution of the own tiles: 36 (chunk, tap) entries, chunk outer
  const float bl0 = vl[col0], bl1 = vl[col0 + 16];
  f32x4 cacc[NC][2];
#pragma unroll
  for (int c = 0; c < NC; ++c) { cacc[c][0] = f32x4{bl0, bl0, bl0, bl0}; cacc[c][1] = f32x4{bl1, bl1, bl1, bl1}; }
  const int img_lds = (int)(unsigned)(size_t)(const __attribute__((address_space(3))) float*)img;
  const int arow0 = img_lds + ((TIGHT ? j : 16 + j) * BB_AP + 8 * g) * 4;   // LDS byte address of (output row j of own tile 0 at tap offset 0, col 8 g)
  const float* wsrc = a.tiles + (size_t)cl * 36 * BB_C * CH + col0 * CH + 8 * g;
  const int live = (1 << nown) - 1;
  int tapmask[NC];                                        // DIL > 1: bit t = tap t of own tile c is live in backbone_kernel's schedule (wave-uniform)
  if constexpr (!TIGHT)                                   // (the tight layout is dilation 1 only: it never had a mask)
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    int m = 0;
    if (DIL > 1 && c < nown) {
      const int T = t0 + c;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int d = (t - 4) * DIL;
        if (max(0, -d) < 16 * T + 16 && min(L, L - d) > 16 * T) m |= 1 << t;
      }
    }
    tapmask[c] = __builtin_amdgcn_readfirstlane(m);
  }
  float4 bA[4], bB[4];
  BB_WLOAD(bA, wsrc)
  bB[0] = bA[0]; bB[1] = bA[1]; bB[2] = bA[2]; bB[3] = bA[3];
  __syncthreads();                                        // the image is complete
#define SG_DBYTES(IT) ((TIGHT ? (IT) % 9 : (((IT) % 9) - 4) * DIL) * (BB_AP * 4) + ((IT) / 9) * (CH * 4))
#define SG_ALOAD(C, V, DBYTES) BB_ALOAD(V, arow0 + (DBYTES) + (C) * (16 * BB_AP * 4))
#define SG_MM(C, U)                                                                                          \
      __builtin_amdgcn_sched_barrier(0);                                                                     \
      __builtin_amdgcn_s_waitcnt(0xC07F | (2 << 8));      /* at most the two reads of the other fragment set in flight */ \
      BB_MM16(cacc[C], U, DIL == 1 ? (live & (1 << (C))) : (tapmask[C] >> (it % 9) & 1))                     \
      __builtin_amdgcn_sched_barrier(0);
  // one entry: the next entry's weight tile goes to the idle fragment set, the A fragments of its first two tiles are requested
  // under this entry's last MFMA groups (backbone_kernel's B2_ENTRY4 / B2_ENTRY2 without the schedule word)
#define SG_ENTRY(BC, BN, UC, UN)                                                                             \
    { const int nxt = it + 1 < 36 ? it + 1 : it;                                                             \
      BB_UNPACK(BC)                                                                                          \
      BB_WLOAD(BN, wsrc + (size_t)nxt * BB_C * CH)                                                           \
      const int dbytes = SG_DBYTES(it), dbytes2 = SG_DBYTES(nxt);                                            \
      if constexpr (NC == 4) {                                                                               \
        SG_MM(0, ua)                                                                                         \
        SG_ALOAD(2, ua, dbytes)                                                                              \
        SG_MM(1, ub)                                                                                         \
        SG_ALOAD(3, ub, dbytes)                                                                              \
        SG_MM(NC - 2, ua)                                                                                    \
        SG_ALOAD(0, ua, dbytes2)                                                                             \
        SG_MM(NC - 1, ub)                                                                                    \
        SG_ALOAD(1, ub, dbytes2)                                                                             \
      } else if constexpr (NC == 1) {                    /* one tile: the fragment sets alternate by entry */ \
        SG_ALOAD(0, UN, dbytes2)                                                                             \
        SG_MM(0, UC)                                                                                         \
      } else {                                                                                               \
        SG_MM(0, ua)                                                                                         \
        SG_ALOAD(0, ua, dbytes2)                                                                             \
        SG_MM(1, ub)                                                                                         \
        SG_ALOAD(1, ub, dbytes2)                                                                             \
      }                                                                                                      \
      ++it; }
  float4 ua[2], ub[2];
  SG_ALOAD(0, ua, SG_DBYTES(0))
  if constexpr (NC > 1) SG_ALOAD(1, ub, SG_DBYTES(0))
  for (int it = 0; it < 36;) {
    SG_ENTRY(bA, bB, ua, ub)
    SG_ENTRY(bB, bA, ub, ua)
  }
#undef SG_ENTRY
#undef SG_MM
#undef SG_ALOAD
#undef SG_DBYTES

  float* dst = pl0 + (size_t)cl * pl_stride;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (c >= nown) continue;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = SEG_OWN_ROW(c) + e;
        if (row < L) dst[row * BB_C + col0 + 16 * ct] = fmaxf(cacc[c][ct][e], 0.0f) + f[SEG_OWN(c)][ct][e];   // relu(conv + b) + f
      }
  }
#undef SEG_NROWS
#undef SEG_OWN_ROW
#undef SEG_OWN
#undef SEG_AT
#undef SEG_IROW
#undef SEG_MINE
#undef SEG_LIVE
