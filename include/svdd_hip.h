/*
 * svdd_hip.h — C ABI of libsvdd_hip.so, the MI355X (gfx950) implementation of the
 * SVDD per-step propose / score-select / resample hot path.
 *
 * The reference (masa-ue/SVDD) is pure Python and has no FFI layer; its boundary for
 * this path is the Python object protocol of `diffusion_gosai.Diffusion`. The entry
 * points below are what a binding for that path replaces, each citing the reference
 * lines whose tensor program it fuses (paths relative to the reference root).
 * INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *  - All pointers are DEVICE pointers unless marked "host". Caller owns every buffer;
 *    nothing is allocated, freed or synchronised inside. Launches go to `stream`
 *    (a hipStream_t passed as void*; NULL = the legacy default stream). Every entry
 *    point is capturable in a hipGraph.
 *  - Tokens are uint8: 0..3 = A,C,G,T; 4 = MASK (diffusion_gosai.py:85,94-95). The
 *    reference's int64 token tensors carry the same values; the Python host mirror
 *    converts at the API edge.
 *  - Return value: 0 on success, a negative SVDD_E_* code otherwise. Launch failures
 *    are reported as SVDD_E_LAUNCH (query hipGetLastError for detail).
 *  - Arithmetic is fp32 in the reference's operation order; exp/log are evaluated
 *    correctly rounded to fp32 (see DESIGN.md "Arithmetic contract").
 */
#ifndef SVDD_HIP_H
#define SVDD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVDD_VOCAB 5      /* A,C,G,T,MASK */
#define SVDD_MASK 4
#define SVDD_MAX_M 1024   /* candidates per sample supported by svdd_select */

enum {
  SVDD_OK = 0,
  SVDD_E_ARG = -1,      /* null pointer / non-positive size / M out of range */
  SVDD_E_LAUNCH = -2,   /* hipLaunchKernel failed */
  SVDD_E_NODEVICE = -3  /* no HIP device / wrong architecture */
};

/* Memory layout of the [B,L,5] tensors (logits, q_xs, logp, replay uniforms).
 * The reference's CNN backbone returns `feat.permute(0, 2, 1)` (models/dnaconv.py:201), a view of a
 * [B,5,L] buffer; log_p_x0, q_xs and rand_like(q_xs) inherit those strides and torch fills
 * rand_like in MEMORY order. A drop-in must therefore accept both images. */
enum {
  SVDD_LAYOUT_BLV = 0,  /* element (b,l,v) at (b*L + l)*5 + v   — contiguous [B,L,5] (e.g. DiT) */
  SVDD_LAYOUT_BVL = 1   /* element (b,l,v) at (b*5 + v)*L + l   — [B,5,L], the conv-native image */
};

/* Uniform source for the categorical draws. */
enum {
  SVDD_RNG_REPLAY = 0,  /* uniforms supplied by the caller (bit-exact replay of the
                           reference's torch-CPU mt19937 stream, diffusion_gosai.py:33) */
  SVDD_RNG_PHILOX = 1   /* counter-based Philox4x32-10 generated in-kernel; keyed by
                           (seed, step, global row, candidate, position) so output is
                           invariant to how rows are sharded over GPUs */
};

typedef struct svdd_rng {
  int32_t kind;            /* SVDD_RNG_REPLAY | SVDD_RNG_PHILOX */
  uint32_t step;           /* PHILOX: diffusion step index (0..S-1) */
  const float* uniforms;   /* REPLAY: M consecutive blocks of B*L*5 fp32 in [0,1), each laid out as
                              `uniforms_layout` — the order M rand_like(q_xs) calls consume, i.e. the
                              memory order of the REFERENCE backbone's output (BVL for its CNN) */
  uint64_t seed;           /* PHILOX: 64-bit key */
  uint64_t row_offset;     /* PHILOX: global index of this shard's row 0 ; REPLAY with uniforms_rows > 0: likewise */
  int32_t uniforms_layout; /* REPLAY: SVDD_LAYOUT_* of each uniforms block (independent of `layout`) */
  int32_t uniforms_rows;   /* REPLAY: 0 = each block holds B rows (this batch's own uniforms); > 0 = each block holds the uniforms of
                              a WHOLE batch of that many rows, of which this call's B rows start at `row_offset` — a rank of a
                              batch-sharded decode replays the global stream and reads its slice */
} svdd_rng_t;

/* Selection rule of svdd_select. */
enum {
  SVDD_SELECT_ARGMAX = 0,      /* reference behaviour: argmax(softmax(scores)) (diffusion_gosai.py:1220,1225) */
  SVDD_SELECT_MULTINOMIAL = 1  /* the commented-out torch.multinomial variant (:1223); PHILOX only */
};

/*
 * svdd_propose — replaces, per diffusion step:
 *   Diffusion._subs_parameterization               diffusion_gosai.py:286-304
 *   q_xs construction                               diffusion_gosai.py:1194-1196
 *   copy_flag                                       diffusion_gosai.py:1199
 *   M x _sample_categorical + copy-flag merge       diffusion_gosai.py:30-34, 1203
 *   M x transform_samples(...).float()              diffusion_gosai.py:1462-1470, 1208
 *
 *  logits  [B,L,5] fp32  raw backbone output in `layout` (NOT modified; the reference edits it in place)
 *  x       [B,L]   u8    current tokens x_t
 *  dm      = fl32(move_chance_t - move_chance_s),  mcs = move_chance_s   (:1184-1187)
 *  cand    [B,M,L] u8    out: the M proposals per sample
 *  onehot  [B*M,L,4] fp32 out: value-net input, row (b*M+m); MASK rows all-zero
 *  q_xs    [B,L,5] fp32  out in `layout`, may be NULL (only the per-step API returns it, :1228)
 */
int svdd_propose(const float* logits, const uint8_t* x, float dm, float mcs,
                 int B, int L, int M, int layout, const svdd_rng_t* rng,
                 uint8_t* cand, float* onehot, float* q_xs, void* stream);

/*
 * svdd_sample_categorical — M x (_sample_categorical(q) merged with copy_flag) + one-hot, for a caller-built
 * q (e.g. the DPS baseline's guided q_xs * exp(guidance), diffusion_gosai.py:1311-1318; :30-34).
 *  q [B,L,5] fp32 in `layout`, all entries >= 0; other arguments as svdd_propose.
 */
int svdd_sample_categorical(const float* q, const uint8_t* x, int B, int L, int M, int layout,
                            const svdd_rng_t* rng, uint8_t* cand, float* onehot, void* stream);

/*
 * svdd_classifier_propose — ABI 12. One step of classifier guidance (reference diffusion_gosai.py:1332-1360) after the value net's
 * input gradient, per position:
 *   q_xs = exp(log p(x0 | x_t)) (mct - mcs), q_xs[MASK] = mcs                 (SUBS as svdd_propose; :1348-1353)
 *   w    = q_xs + scale * cat(x_grad, 0)                                        (:1355-1357; SIGNED: w < 0 where the step lowers it)
 *   one _sample_categorical(w) draw, merged with copy_flag                      (:30-34, :1358-1359)
 * in fp32 with one rounding per operation: q = fl(exp(lp) * dm), w = fl(q + fl(scale * g)).
 *  logits      [B,L,5] fp32 raw backbone output in `layout`
 *  x           [B,L]   u8   current tokens x_t
 *  grad4       [B][L][4] fp32 x_grad = d mean(head(embedding(onehot(x_t)))) / d onehot (contiguous)
 *  rng         as svdd_propose with M = 1 (Philox: the same counters, so scale 0 draws what svdd_propose draws)
 *  x_next      [B][L] u8   out
 *  onehot_next [B][L][4] fp32 out, may be NULL: transform_samples(x_next) (MASK rows zero), the next step's value-net input
 *  q_xs        [B,L,5] fp32 out in `layout`, may be NULL: the UN-guided q_xs (the per-step API's third output)
 */
int svdd_classifier_propose(const float* logits, int layout, const uint8_t* x, const float* grad4, float dm, float mcs, float scale,
                            int B, int L, const svdd_rng_t* rng, uint8_t* x_next, float* onehot_next, float* q_xs, void* stream);

/*
 * ELBO scoring of clean sequences (ABI 13): the continuous-time SUBS loss of the reference's Diffusion with the gosai
 * configuration (T = 0, time_conditioning off, antithetic sampling, LogLinear noise), around ONE backbone forward of the
 * masked rows (svdd_backbone_cnn_f32 / _lp or the DiT, unchanged):
 *   svdd_elbo_mask replaces   _sample_t                                     diffusion_gosai.py:1660-1669
 *                             sigma, dsigma = noise(t); move_chance         :1725-1729, noise_schedule.py:126-145
 *                             q_xt                                          :738-749
 *   svdd_elbo_nll replaces    gather of log_p at x0, - log_p * dsigma / expm1(sigma)   :1745-1757
 *                             (and the per-row / per-sequence sums _loss and the nll metric take, :1759-1779, :50-71)
 * Row r = k n + b of a launch is draw k (0 <= k < K) of sequence b (0 <= b < n).
 *
 * svdd_elbo_mask — x0 [n, L] u8 (tokens 0..3) -> xt [n K, L] u8: MASK where u < move_chance of the row, else x0;
 *   nmasked [n K] i32 (may be NULL): masked positions per row.
 *   REPLAY (rng->uniforms, uniforms_rows == 0): uniforms = K blocks of n L fp32, block k in [b][l] order — the torch.rand(n, L)
 *     of q_xt in each of K consecutive _forward_pass_diffusion calls; move_chance_in [n K] = the rows' move_chance, computed by
 *     the caller with the reference's fp32 torch ops (a 1-ulp difference would flip mask decisions). t, move_chance, w must be NULL.
 *   PHILOX: move_chance_in must be NULL. Counter (word 0, 1, 2, 3) = (row_offset + b low, high, k << 16 | j, 3): stream word 3
 *     (0 = svdd_propose / svdd_classifier_propose, 2 = the multinomial select). Block j = 0 gives t: u = top 24 bits of word 0,
 *     e = (u / K + k / K) mod 1 — stratified over the sequence's OWN K draws, so results do not depend on how rows are sharded
 *     or chunked — t = (1 - eps) e + eps; block j >= 1 gives the mask uniforms of positions 4 (j - 1) .. 4 (j - 1) + 3 (words 0..3,
 *     top 24 bits). Written per row (each may be NULL): t, move_chance = (1 - eps) t, w = dsigma / expm1(sigma) = 1 / t (the
 *     LogLinear identities), each evaluated in fp64 and rounded once to fp32. rng->step is not used. eps in (0, 1).
 *   K <= 65535, L <= 262136.
 *
 * svdd_elbo_nll — logits [n K, L, 5] fp32 raw backbone output in `layout` (as svdd_subs_logp), xt [n K, L], x0 [n, L], w [n K]:
 *   nll      [n K, L] fp32 (may be NULL): -(log p at x0) * w at masked positions, log p = svdd_subs_logp's arithmetic, one fp32
 *            multiply; +0 at unmasked positions
 *   row_sum  [n K] fp64: sum over l of nll, accumulated in fp64 in position order
 *   seq_mean [n] fp64 (may be NULL): (sum over k of row_sum[k n + b], in draw order) / K
 *   err      device i32 (may be NULL, caller-zeroed): set to 1 if x0 holds a token > 3 (those rows' values are NaN). The library
 *            cannot refuse a device-side value without a synchronisation: the caller reads err after the stream and treats 1
 *            as SVDD_E_ARG.
 *   No result depends on the launch shape (one workgroup per sequence; fixed summation orders).
 */
int svdd_elbo_mask(const uint8_t* x0, int n, int L, int K, double eps, const svdd_rng_t* rng, const float* move_chance_in,
                   uint8_t* xt, float* t, float* move_chance, float* w, int32_t* nmasked, void* stream);
int svdd_elbo_nll(const float* logits, int layout, const uint8_t* xt, const uint8_t* x0, const float* w, int n, int L, int K,
                  float* nll, double* row_sum, double* seq_mean, int32_t* err, void* stream);

/*
 * Re-mask refinement and template-constrained design (ABI 16): the boundary between two guided decodes of the same rows, in
 * ONE launch and without a synchronisation. Per row b:
 *   accept   only when x_old, score_new and score_old are all given (x_keep and score_keep are then required): the row keeps its
 *            new version iff score_new[b] > score_old[b] — a NaN score_new and a tie keep the old row. Otherwise the new row is
 *            kept. x_keep [B, L] u8 = the kept row (may be NULL when nothing is judged), score_keep [B] f32 = its score (may be
 *            NULL; needs score_new), accepted [B] i32 (may be NULL) = 1 where the new row was kept.
 *            x_keep MAY BE x_old (a lane writes only the positions it has read), and score_keep may be score_old (the row's wave
 *            reads both scores before its one store); x_keep must not be x_new.
 *   re-mask  x_t[b, l] = MASK iff u[b, l] < move_chance and frozen[b, l] == 0, else x_keep[b, l]  (q_xt, diffusion_gosai.py:738-749,
 *            under a frozen mask). frozen [B, L] u8 or NULL (nothing frozen). A MASK token of the kept row stays MASK, frozen or
 *            not. nmasked [B] i32 (may be NULL) = MASK tokens of x_t[b], those included. x_t may be NULL: accept only (frozen
 *            and nmasked must then be NULL; rng is not read). x_t must be none of the other buffers, frozen none of the token buffers (SVDD_E_ARG).
 *   err      device i32 (may be NULL, caller-zeroed): set to 1 if the kept row holds a token > 4 (copied through as it is); read by
 *            the caller after the stream, as svdd_elbo_nll's.
 *  move_chance  ONE fp32 scalar in [0, 1], computed by the caller in both rng modes with the reference's fp32 torch ops
 *            (1 - exp(-sigma(t))): a 1-ulp difference flips masks.
 *  REPLAY    rng->uniforms = one block of B L fp32 in [b][l] order, the torch.rand(*x.shape) of q_xt; uniforms_rows must be 0.
 *  PHILOX    counter (word 0, 1, 2, 3) = (row_offset + b low, high, round << 16 | j, 1) with round = rng->step <= 65535: stream
 *            word 1 (0 = svdd_propose / svdd_classifier_propose, 2 = the multinomial select, 3 = ELBO). Block j gives the
 *            uniforms of positions 4 j .. 4 j + 3 (words 0..3, top 24 bits). L <= 262144.
 *  Rows of a multiple-of-4 length in 4-byte aligned buffers move as 32-bit words, any other shape byte by byte: same results.
 *  No result depends on the launch shape or on how rows are split over calls (one wave per row, keyed by the global row).
 *  The stream is an explicit argument (as svdd_backbone_incr*_f32).
 */
int svdd_refine_remask(const uint8_t* x_new, const uint8_t* x_old, const float* score_new, const float* score_old,
                       const uint8_t* frozen, float move_chance, int B, int L, const svdd_rng_t* rng, uint8_t* x_keep,
                       float* score_keep, int32_t* accepted, uint8_t* x_t, int32_t* nmasked, int32_t* err, void* on_stream);

/*
 * Value-function training data (ABI 17): the per-step boundary of a CD-Q rollout (reference Enformer.py:226-259 with
 * diffusion_gosai.py:839-853), in ONE launch and without a synchronisation. Per row b:
 *   continue  x_next[b, :] = cand[b, M - 1, :]: the reference continues from its LAST draw (`x = x0` after `for j in range(10)`,
 *             diffusion_gosai.py:845-851). cand [B, M, L] u8 (svdd_propose's), x_next [B, L] u8, not cand itself.
 *             onehot_next [B, L, 4] f32 (may be NULL) = transform_samples(x_next), MASK rows zero: written straight into the
 *             caller's training-input slab.
 *   reduce    target[b] from scores[b, 0 .. M - 1] (the value net on the M draws). scores [B, M] f32 and target [B] f32 are both
 *             given or both NULL (step 0 has no target: the reference skips time == 0, Enformer.py:233-234); not each other.
 *     SVDD_TARGET_MEAN        target[b] = fl(fl(...fl(fl(0 + s_0) + s_1)... + s_{M-1}) / fl(M)): a sequential fp32 sum in ascending m
 *                             and one fp32 division, bit for bit the reference's `case_sum = case_sum + v; case_sum / len(...)`
 *                             (Enformer.py:235-238). Not a tree reduction, not a multiplication by 1 / M. NaN and +-inf follow IEEE.
 *                             alpha is ignored.
 *     SVDD_TARGET_LOGMEANEXP  the soft backup alpha log mean exp(v / alpha) (no reference counterpart): mx = max_m s_m,
 *                             target[b] = mx + alpha * logf(sum_m expf((s_m - mx) / alpha) / M), the sum in ascending m, one rounding
 *                             per operation. A NaN score gives NaN, mx = +inf gives +inf, all scores -inf give -inf. alpha must be
 *                             finite and > 0.
 *  Rows of a multiple-of-4 length in aligned buffers (tokens 4 bytes, one-hot 16) move as 32-bit words, any other shape byte by
 *  byte: same results. No result depends on the launch shape (one wave per row). M <= SVDD_MAX_M.
 *  The stream is an explicit argument (as svdd_refine_remask).
 */
#define SVDD_TARGET_MEAN 0
#define SVDD_TARGET_LOGMEANEXP 1
int svdd_value_target(const float* scores, const uint8_t* cand, int B, int L, int M, int reduce, float alpha,
                      uint8_t* x_next, float* onehot_next, float* target, void* on_stream);

/*
 * In-silico mutagenesis and ISM-driven directed evolution (added under ABI 17: three new entries, nothing existing changed). The
 * boundary kernels around an unchanged value-net path (reference score.py ISM_predict, design.py:124-160 evolve(method="ism",
 * for_each=True)). Every entry takes its stream explicitly (as svdd_refine_remask).
 *
 * svdd_ism_mutants: the 3 P single-base mutants of every row. x [B, L] u8 (tokens 0..3), positions [P] i32 ascending (device),
 *   live [B] u8 or NULL. cand [B, 3P, L] u8; onehot [B * 3P, L, 4] f32 or NULL (the split-precision tower takes tokens).
 *   Mutant (b, j, k), row b * 3P + 3j + k, is row b with position positions[j] replaced by the k-th base of A, C, G, T that is NOT
 *   x[b, positions[j]], k = 0, 1, 2: the order of the reference's ISMDataset(..., drop_ref=True) (sequence, position, allele in
 *   ACGT order with the reference base skipped). A row with live[b] == 0 gets exact copies of its parent (svdd_candidate_windows
 *   flags those 0 and the compaction drops them). A parent token > 3 sets err[0] = 1 (err: caller-zeroed device word or NULL, read
 *   later) and is copied through unchanged (one-hot: a zero row); where it sits AT positions[j] the mutant is a copy. A position
 *   outside 0 .. L - 1 sets err[0] as well and gives copies: nothing is read or written out of bounds. cand must not be x.
 *   Rows of a multiple-of-4 length in aligned buffers (tokens 4 bytes, one-hot 16) move as 32-bit words, any other shape byte by
 *   byte: same results. One wave per mutant: no result depends on the launch shape. SVDD_E_ARG: B, L or P <= 0, a NULL x, positions
 *   or cand, cand == x, B * 3P * L >= 2^40.
 *
 * svdd_ism_fold: folds the scores of one chunk of positions (columns p0 .. p0 + Pc - 1 of positions [P]) into the ISM table and
 *   the per-row running best. scores: dense [B, 3 Pc] f32 in the order above when slot is NULL; with slot [B * 3 Pc] i32
 *   (svdd_compact_flags' map) the score of mutant i is scores[slot[i]], or parent_score[b] where slot[i] < 0 (an exact copy, not
 *   computed). parent_score [B] f32; x [B, L] u8 the parents (which base is the reference at each position).
 *   ism [B, P, 4] f32 or NULL: entry (b, p0 + j, a) = the score of the mutant carrying base a there, the entry of the parent's own
 *   base = parent_score[b] (a position whose parent token is > 3 or that is out of range: all four = parent_score[b], no pick).
 *   best_score [B] f32, best_pos [B] i32, best_allele [B] i32 (all three or none; ism or the three must be given): the running
 *   best over the chunks folded so far. The chunk with p0 == 0 starts it at (-inf, -1, -1); later chunks read what the earlier
 *   ones left, so chunks are folded in ascending p0 and the result does not depend on the chunking. A mutant replaces the running
 *   best only if its score is STRICTLY greater: the first mutant in (position, allele) order wins a tie (pandas idxmax), a NaN
 *   never wins, and neither does -inf. best_pos is the sequence position positions[j], best_allele the token 0..3. live [B] u8 or
 *   NULL: a row with live[b] == 0 offers no pick (its best stays (-inf, -1, -1)); its ism columns are still written.
 *   One wave per row, the wave's reduction is by comparison on (score, order index): no float atomics, no result depends on the
 *   launch shape. SVDD_E_ARG: B, L, P or Pc <= 0, p0 < 0, p0 + Pc > P, a NULL scores, parent_score, x or positions, neither
 *   output, a partial best triple, ism == scores.
 *
 * svdd_evolve_apply: one iteration's boundary of directed evolution, ONE launch of ONE workgroup (the per-row state score_cur /
 *   live is both an input of the batch-wide decision and an output of the launch: a second workgroup could read a row after its
 *   owner rewrote it; B rows of L bytes are a few microseconds for one workgroup). No grid-wide synchronisation, no float atomics.
 *   If stopped[0] != 0 at entry NOTHING is written. A row's pick is valid when the row is live (live NULL: every row) and
 *   0 <= best_pos < L, 0 <= best_allele <= 3.
 *     SVDD_EVOLVE_GLOBAL  the reference's rule (design.py:124-160, for_each=True): m = max of best_score over the rows with a valid
 *                         pick (by comparison; a NaN never wins). If m > best_so_far[0]: best_so_far[0] = m and EVERY row with a
 *                         valid pick takes it, whether or not that improves on the row's score_cur. Otherwise stopped[0] = 1 and
 *                         no row changes. live may be NULL and is never written.
 *     SVDD_EVOLVE_ROW     a row takes its pick only if best_score[b] > score_cur[b] (strictly; a NaN does not); otherwise
 *                         live[b] = 0 and the row never changes again. stopped[0] = 1 when no row took a pick. live is required.
 *   Taking a pick: x[b, best_pos] = best_allele in place, score_cur[b] = best_score[b]; then, if score_cur[b] > score_best[b]
 *   (strictly: the first occurrence of a row's highest score is kept), x_best[b, :] = x[b, :] and score_best[b] = score_cur[b].
 *   Trace (each NULL or [B]; written whenever the launch was not stopped at entry, also by the launch that sets stopped: the
 *   reference records the iteration before it breaks): tr_pos / tr_allele i32 = the pick (-1, -1 without a valid one), tr_score
 *   f32 = best_score[b] (score_cur[b] without a valid pick), tr_taken u8.
 *   x [B, L] u8, score_cur [B], best_so_far [1], stopped [1] i32, x_best [B, L] u8 (not x), score_best [B]: all required.
 *   SVDD_E_ARG: B or L <= 0, a stop mode other than the two, a NULL among the required pointers, ROW without live, x_best == x.
 */
#define SVDD_EVOLVE_GLOBAL 0
#define SVDD_EVOLVE_ROW 1
int svdd_ism_mutants(const uint8_t* x, const int32_t* positions, const uint8_t* live, int B, int L, int P, uint8_t* cand,
                     float* onehot, int32_t* err, void* on_stream);
int svdd_ism_fold(const float* scores, const int32_t* slot, const float* parent_score, const uint8_t* x, const int32_t* positions,
                  const uint8_t* live, int B, int L, int P, int p0, int Pc, float* ism, float* best_score, int32_t* best_pos,
                  int32_t* best_allele, void* on_stream);
int svdd_evolve_apply(const float* best_score, const int32_t* best_pos, const int32_t* best_allele, int B, int L, int stop,
                      uint8_t* x, float* score_cur, uint8_t* live, float* best_so_far, int32_t* stopped, uint8_t* x_best,
                      float* score_best, int32_t* tr_pos, int32_t* tr_allele, float* tr_score, uint8_t* tr_taken, void* on_stream);

/*
 * Pattern scanning and pattern-driven directed evolution (added under ABI 17: three new entries, nothing existing changed): the
 * three entries above with a pattern of 1 .. SVDD_PATTERN_MAX_WIDTH tokens written at a start position in place of one base
 * (reference design.py evolve(method="pattern", for_each=True); grelu's MotifScanDataset restated). A replacement, not
 * an insertion: the length stays L. Every entry takes its stream explicitly.
 *   patterns [K, SVDD_PATTERN_MAX_WIDTH] u8, 4-byte aligned: row k holds pattern k's widths[k] tokens 0..3, the rest is ignored.
 *   widths [K] i32, positions [P] i32 ascending start positions (both on the device).
 *
 * svdd_pattern_mutants: cand [B, P K, L] u8; onehot [B * P K, L, 4] f32 or NULL. Mutant (b, j, k), row (b P + j) K + k (the
 *   pattern index runs fastest), is row b with x[b, positions[j] : positions[j] + widths[k]] overwritten by pattern k. An exact
 *   copy of row b is written for a row with live[b] == 0 (live [B] u8 or NULL) and, with err[0] = 1 (err [1] i32 or NULL, zeroed
 *   by the caller, never cleared here), for a width outside 1..32, a window that leaves the row (positions[j] < 0 or positions[j] +
 *   widths[k] > L), a parent token > 3 ANYWHERE in row b and a pattern token > 3: nothing is read or written out of bounds.
 *   A mutant may equal its parent (the pattern is already there): svdd_candidate_windows / svdd_candidate_parts flag it 0.
 *   One wave per mutant; word accesses when L % 4 == 0 and x, cand (4) and onehot (16) are aligned, bytes otherwise, same result.
 *   SVDD_E_ARG: B, L, P or K <= 0, a NULL x, positions, patterns, widths or cand, cand == x, patterns not 4-byte aligned,
 *   P K > 2^30, B P K L >= 2^40.
 *
 * svdd_pattern_fold: folds the scores of one chunk of positions (columns p0 .. p0 + Pc - 1) into the table and the per-row
 *   running best. scores: dense [B, Pc K] f32 in the order above when slot is NULL; with slot [B * Pc K] i32 (svdd_compact_flags'
 *   map) the score of mutant i is scores[slot[i]], or parent_score[b] where slot[i] < 0 (an exact copy, not computed: the same
 *   bits as the parent's score). table [B, P, K] f32 or NULL. best_score [B] f32, best_pos [B] i32, best_pattern [B] i32 (all
 *   three or none; table or the three must be given): best_pos is the INDEX j into positions, best_pattern the index k. The rules
 *   are svdd_ism_fold's: the chunk with p0 == 0 starts at (-inf, -1, -1), chunks are folded in ascending p0, an entry replaces the
 *   running best only if STRICTLY greater (the first entry in (position, pattern) order wins a tie, the running best of the
 *   earlier chunks wins a tie, a NaN and -inf never win: a row whose every entry is NaN keeps (-1, -1)); a row with live[b] == 0
 *   offers no pick, its table columns are still written. One wave per row, reduced by comparison on (score, order index).
 *   SVDD_E_ARG: B, P, K or Pc <= 0, p0 < 0, p0 + Pc > P, P K > 2^30, a NULL scores or parent_score, neither output, a partial best
 *   triple, table == scores.
 *
 * svdd_pattern_apply: svdd_evolve_apply for a pick (best_pos = index into positions, best_pattern): ONE launch of ONE workgroup,
 *   both stop rules as there, nothing written if stopped[0] != 0 at entry. A row's pick is valid when the row is live (live NULL:
 *   every row), 0 <= best_pos < P, 0 <= best_pattern < K and the pattern's window lies inside the row. Taking a pick writes the
 *   pattern's widths[k] bytes into x[b] at positions[best_pos] (possibly the bytes already there: a no-op pick) and sets
 *   score_cur[b] = best_score[b]; then, if that is > score_best[b] (strictly), x_best[b, :] = x[b, :] and score_best[b] = it.
 *   Trace (each NULL or [B]): tr_pos i32 = the START POSITION positions[best_pos], tr_pattern i32 = best_pattern (-1, -1 without a
 *   valid pick), tr_score f32 = best_score[b] (score_cur[b] without a valid pick), tr_taken u8. Pattern tokens are not checked
 *   here: they are the patterns svdd_pattern_mutants accepted.
 *   SVDD_E_ARG: B, L, P or K <= 0, a stop mode other than the two, a NULL among the required pointers (everything but live and
 *   the trace), ROW without live, x_best == x, patterns not 4-byte aligned.
 */
#define SVDD_PATTERN_MAX_WIDTH 32
int svdd_pattern_mutants(const uint8_t* x, const int32_t* positions, const uint8_t* patterns, const int32_t* widths,
                         const uint8_t* live, int B, int L, int P, int K, uint8_t* cand, float* onehot, int32_t* err, void* on_stream);
int svdd_pattern_fold(const float* scores, const int32_t* slot, const float* parent_score, const uint8_t* live, int B, int P, int K,
                      int p0, int Pc, float* table, float* best_score, int32_t* best_pos, int32_t* best_pattern, void* on_stream);
int svdd_pattern_apply(const float* best_score, const int32_t* best_pos, const int32_t* best_pattern, const int32_t* positions,
                       const uint8_t* patterns, const int32_t* widths, int B, int L, int P, int K, int stop, uint8_t* x,
                       float* score_cur, uint8_t* live, float* best_so_far, int32_t* stopped, uint8_t* x_best, float* score_best,
                       int32_t* tr_pos, int32_t* tr_pattern, float* tr_score, uint8_t* tr_taken, void* on_stream);

/*
 * Gradient attributions (added under ABI 17: two new entries, nothing existing changed): gradient, input x gradient and integrated
 * gradients of a row's score (reference score.py get_attributions). The boundary kernels around an unchanged input-gradient pass.
 * A call's work is the B * S (row, step) pairs r = b * S + k in that order (S = 1 for the one-pass methods); a pass takes the
 * pairs r0 .. r0 + n_rows - 1 and may cut a row's steps. Both entries take their stream explicitly (as svdd_ism_*).
 *
 * svdd_attr_path: the interpolants of one pass. x [B, L] u8 (tokens 0..4; 4 = MASK: a zero one-hot row), baseline f32 [L, 4]
 *   (baseline_rows == 1), [B, L, 4] (baseline_rows == B) or NULL (zeros; baseline_rows ignored), alpha [S] f32 (device).
 *   out [n_rows + n_pad, L, 4] f32: row i < n_rows, pair r0 + i = (b, k), is base + alpha[k] * (onehot(x[b]) - base) evaluated as
 *   three separately rounded fp32 operations (sub, mul, add; no contraction): with baseline NULL and alpha[k] == 1 the exact
 *   one-hot. Rows n_rows .. n_rows + n_pad - 1 are copies of row 0 (a pass padded to a row count of the caller's choosing). A token
 *   > 4 sets err[0] = 1 (err: caller-zeroed device word or NULL, read later) and is treated as 4. One thread per position (16
 *   bytes: float4 where out and baseline are 16-byte aligned, scalars otherwise, same results), grid-stride: no result depends on
 *   the launch shape. SVDD_E_ARG: B, L, S or n_rows <= 0, n_pad < 0, r0 < 0, r0 + n_rows > B * S, a NULL x, alpha or out,
 *   baseline given with baseline_rows not 1 or B, (n_rows + n_pad) * L >= 2^40.
 *
 * svdd_attr_fold: folds one pass's gradients grad [>= n_rows, L, 4] f32 (svdd_attr_path's row order; rows beyond n_rows are not
 *   read) into acc [B, L, 4] f32. For every row b with pairs in the pass, in ascending k:
 *       acc[b, l, c] = acc[b, l, c] + weight[k] * (scale * grad[i, l, c])          (three separately rounded fp32 operations)
 *   A row's accumulator starts from 0 at its pair k == 0 (acc is not read there) and continues from acc otherwise: passes are
 *   folded in ascending r0, and the result does not depend on where they were cut. weight [S] f32 (device); scale: the factor that
 *   turns the pass's gradient into the row's (the row count of a pass that differentiated the mean over its rows). When the row's
 *   last pair k == S - 1 lies in the pass the row is finished, attr [B, 4, L] f32 (transposed):
 *     SVDD_ATTR_GRADIENT     attr[b, c, l] = acc[b, l, c]
 *     SVDD_ATTR_TIMES_INPUT  attr[b, c, l] = (onehot(x[b])[l, c] - base[l, c]) * acc[b, l, c]     (base as in svdd_attr_path)
 *   and, rowsum [B] f32 non-NULL, rowsum[b] = the sum of the row's 4 L attr values in a fixed order: lane j of the row's wave adds
 *   the positions l = j, j + 64, ... in ascending l, channels 0..3 inside a position, onto 0; then the 64 partial sums meet in an
 *   xor butterfly (offsets 32, 16, .. 1). No float atomics; one wave per row, rows are independent (a NaN stays in its row), no
 *   result depends on the launch shape. SVDD_E_ARG: B, L, S or n_rows <= 0, r0 < 0, r0 + n_rows > B * S, a mode other than the
 *   two, a NULL grad, weight, x, acc or attr, baseline given with baseline_rows not 1 or B, attr / acc / grad not pairwise distinct.
 */
#define SVDD_ATTR_GRADIENT 0
#define SVDD_ATTR_TIMES_INPUT 1
int svdd_attr_path(const uint8_t* x, const float* baseline, int baseline_rows, const float* alpha, int B, int L, int S, int r0,
                   int n_rows, int n_pad, float* out, int32_t* err, void* on_stream);
int svdd_attr_fold(const float* grad, float scale, const float* weight, const uint8_t* x, const float* baseline, int baseline_rows,
                   int B, int L, int S, int r0, int n_rows, int mode, float* acc, float* attr, float* rowsum, void* on_stream);

/*
 * Ledidi gradient-based sequence design (added under ABI 17: one new entry, nothing existing changed): editing of given sequences
 * through a Gumbel-softmax relaxation (reference design.py ledidi; the `ledidi` package's Ledidi.forward / fit_transform). The
 * boundary kernel around an unchanged scoring pass and an unchanged input-gradient pass. Designs are independent: design d of B
 * has S samples, weights w / AdamW moments m, v [B, L, 4] f32 (channels last), and best-so-far state. The stream is explicit.
 *
 * svdd_ledidi_step: ONE launch per iteration boundary and chunk of designs d0 .. d0 + nd - 1 (one workgroup per design, a thread
 *   owns a position; L > 256 strides). With grad given it closes iteration `iter` (losses, bookkeeping, update) and, sample != 0,
 *   draws the samples of iteration iter + 1; with grad NULL (the first launch) it only draws the samples of iteration `iter`.
 *   Arrays indexed by the design are whole-batch arrays ([B, ...], indexed by d); grad and xin belong to the chunk's pass (row
 *   (d - d0) * S + s). A design with stopped[d] != 0 at entry is left alone entirely: nothing of it is read or written.
 *
 *   losses (iteration iter; sc [B, S] f32 = the scores of tok, edits [B, S] i32 = what the sampling launch left):
 *     out = -((sum_s sc) / S), or with target [B] f32 non-NULL (sum_s (sc - target)^2) / S; the sum sequential in ascending s from 0
 *     inp = float(sum_s edits) / float(S)            total = out + l * inp                    (one rounding per operation)
 *   bookkeeping (the caller starts best_total / best_output from the same formula on S copies of the start score, with a
 *     correctly rounded division, so that an
 *     iteration without an edit ties with it): total < best_total[d] (strictly; a NaN never): best_total / best_output / best_input = total / out / inp,
 *     best_iter = iter, x_best[d] = tok[d] (all S rows, [B, S, L] u8), score_best[d] = sc[d] ([B, S]), wo[d] = 0. Otherwise
 *     wo[d] += 1 and, wo[d] == cfg->patience, stopped[d] = 1 and live[0] -= 1 (integer atomic; live: one device word the caller
 *     set to the number of live designs). trace_total / trace_out / trace_in [B] f32 (each may be NULL): this iteration's three.
 *   update (editable positions; editable [L] u8 or NULL = all), per position, for s ascending, c = 0..3:
 *     G_c   = coef_s * (scale * grad[s, c]) + pen_c       coef_s = -(1 / S), or with a target (2 (sc_s - target)) / S
 *             pen_c = +lam at the sample's base where it differs from x0's, -lam at x0's base there, 0 otherwise; lam = l / (2 S)
 *     dot   = ((y_0 G_0 + y_1 G_1) + y_2 G_2) + y_3 G_3                                        (y [B, S, L, 4]: the samples' softmax)
 *     gw_c  = gw_c + ((1 / tau) * y_c) * (G_c - dot)                                           (from 0)
 *     then AdamW: w = w * decay; m = m + w1 * (gw - m); v = v * beta2 + (w2 * gw) * gw;
 *                 w = w - (step_size * m) / (sqrt(v) / bc2_sqrt + adam_eps)
 *     with the host's float64 values rounded once: decay = 1 - lr wd, w1 = 1 - beta1, w2 = 1 - beta2, step_size = lr / (1 -
 *     beta1^(iter+1)), bc2_sqrt = sqrt(1 - beta2^(iter+1)). A design that stops in this launch still takes this update.
 *   sampling (iteration it = iter + 1, or iter with grad NULL; not for a design that stopped in this launch), per editable
 *     position j, sample s, channel c, u = the uniform:
 *     g = -log(1e-10 - log(u + 1e-10));  z = ((c == x0[j] ? la : lb) + w_c) + g;  zt = z / tau         (log: correctly rounded)
 *     tok[d, s, j] = the first argmax of zt; y_c = exp(zt_c - max) / (((e_0 + e_1) + e_2) + e_3)       (exp: correctly rounded)
 *     A frozen position copies x0[j] and writes no y. xin [nd S + n_pad, L, 4] f32: row (d - d0) S + s = onehot(tok[d, s]) (a
 *     token > 3: a zero row); the n_pad rows after the chunk's are copies of its row 0, written by design d0's workgroup (and, like
 *     that row, left alone once design d0 has stopped). edits[d, s] = positions with tok != x0.
 *     REPLAY: rng->uniforms [B, S, L, 4] f32, this iteration's uniforms of the WHOLE batch (indexed by d); uniforms_rows must be 0.
 *     PHILOX: counter (word 0, 1, 2, 3) = (row_offset + d low, high, it, s << 20 | j << 8 | 4): the iteration has a word of its own
 *       (32 bits), and word 3's low byte is the stream word 4 (0 = svdd_propose / svdd_classifier_propose, 1 = re-mask, 2 = the
 *       multinomial select, 3 = ELBO: their word 3 is 0..3 as a whole). The four words' top 24 bits are channels 0..3. The key is
 *       rng->seed. rng->step is not used. rng may be NULL when sample == 0.
 *   err: device i32 (may be NULL, caller-zeroed): set to 1 if x0 holds a token > 3 at a sampled position (no base gets la there).
 *   No float atomics; every float of a position is computed by one thread in a fixed order, the edit counts are integer sums:
 *   no result depends on the launch shape, on the chunking (d0, nd) or on the other designs.
 *   SVDD_E_ARG: B, nd <= 0, d0 < 0, d0 + nd > B, L outside 1..1024, S outside 1..64, n_pad < 0, iter < 0, a NULL x0, cfg, w, m, v,
 *   y, tok, xin or edits; tau not > 0; with grad: a NULL sc, best_*, x_best, score_best, wo, stopped or live; without: sample == 0;
 *   sample != 0 with a NULL rng, REPLAY without uniforms or with uniforms_rows != 0; grad, xin, y, w, m, v or the uniforms not
 *   16-byte aligned (a position's four channels move as one 16-byte access).
 */
typedef struct svdd_ledidi_cfg {
  float tau, l;                 /* softmax temperature; weight of the input loss */
  float la, lb;                 /* fp32(log(1 + eps)), fp32(log(eps)): the logits of x0's base and of the other three */
  float scale;                  /* turns the pass's gradient into the row's (the row count of a mean's gradient pass, else 1) */
  float decay, w1, beta2, w2, adam_eps, step_size, bc2_sqrt;   /* AdamW, as above (step_size and bc2_sqrt change per iteration) */
  int32_t patience;             /* early_stopping_iter */
} svdd_ledidi_cfg_t;
int svdd_ledidi_step(const uint8_t* x0, const uint8_t* editable, const float* grad, const float* sc, const float* target,
                     const svdd_ledidi_cfg_t* cfg, const svdd_rng_t* rng, int B, int L, int S, int d0, int nd, int n_pad, int iter,
                     int sample, float* w, float* m, float* v, float* y, uint8_t* tok, float* xin, int32_t* edits, float* best_total,
                     float* best_output, float* best_input, int32_t* best_iter, uint8_t* x_best, float* score_best, int32_t* wo,
                     int32_t* stopped, int32_t* live, float* trace_total, float* trace_out, float* trace_in, int32_t* err,
                     void* on_stream);

/*
 * Sample-quality metrics of a set of sequences (added under ABI 17: three new entries, nothing existing changed): k-mer spectra
 * (reference oracle.py count_kmers, diffusion_gosai.py compare_kmer) and Hamming distances on 2-bit-packed rows (nearest
 * neighbour and the histogram of all pairs: diversity and novelty, which the reference does not have). All three are integer
 * arithmetic with integer atomics only: no result depends on the launch shape or on how the caller cuts its rows into chunks.
 * Every entry takes its stream explicitly (as svdd_ism_* and svdd_attr_*).
 *
 * svdd_kmer_counts: x [N, L] u8. counts [4^k] i64 and skipped [1] i64 or NULL are ACCUMULATED INTO (the caller zeroes them), so
 *   a set can be fed in chunks of rows. The window of row r at i = 0 .. L - k has bin sum_j x[r, i + j] 4^(k - 1 - j): the
 *   lexicographic rank of its detokenised ACGT string. A window that holds a token > 3 (MASK included) is not counted and adds 1
 *   to skipped. k > L is valid: there are no windows and nothing is written. k = 1 .. 6 (4096 bins). A workgroup counts a run of
 *   rows into a u32 histogram in LDS and adds its non-zero bins with 64-bit integer atomics; it takes at most
 *   floor((2^32 - 1) / (L - k + 1)) rows, so no u32 bin can wrap. SVDD_E_ARG: N or L <= 0, k outside 1 .. 6, a NULL x or counts.
 *
 * svdd_pack_tokens: x [N, L] u8 (tokens 0..3) -> packed [N, W] u32, W = ceil(L / 16): position l sits in word l / 16 at bits
 *   2 (l mod 16), 2 (l mod 16) + 1; the padding bits of the last word are zero. A token > 3 sets err[0] = 1 (err: caller-zeroed
 *   device word or NULL, read later) and packs as 0. One thread per word, grid-stride. SVDD_E_ARG: N or L <= 0, L > 1024, a NULL
 *   x or packed.
 *
 * svdd_hamming_nn: q [B, W] and db [N, W] packed u32 (svdd_pack_tokens). For every pair (i, j), d = the number of positions at
 *   which the rows differ, per word popc((v | v >> 1) & 0x55555555) of v = q ^ db (the padding bits of the last word are masked
 *   out on both sides). With exclude_diag != 0 the pairs with q_base + i == db_base + j are left out of everything.
 *   nn_key [B] u64 or NULL, initialised by the caller to all ones: nn_key[i] = min(nn_key[i], (uint64(d) << 32) | uint32(db_base
 *   + j)) by 64-bit integer atomic min: the smallest distance and, among ties, the smallest database index (first wins); a query
 *   with no pair keeps its value. hist [L + 1] i64 or NULL, ACCUMULATED INTO: the number of pairs at each distance. Both are exact
 *   and independent of how the database (db_base) and the queries (q_base) are cut into calls. A thread keeps one query's W <= 64
 *   words in registers, a workgroup of 256 queries walks a segment of at most 2^22 database rows in tiles staged in LDS (every
 *   lane reads the same address: a broadcast) and counts into u32 bins in LDS (at most 256 * 2^22 < 2^32 pairs per workgroup).
 *   SVDD_E_ARG: B, N or L <= 0, L > 1024, a negative base, db_base + N or q_base + B >= 2^31, a NULL q or db, neither output.
 */
int svdd_kmer_counts(const uint8_t* x, int N, int L, int k, int64_t* counts, int64_t* skipped, void* on_stream);
int svdd_pack_tokens(const uint8_t* x, int N, int L, uint32_t* packed, int32_t* err, void* on_stream);
int svdd_hamming_nn(const uint32_t* q, const uint32_t* db, int B, int N, int L, int q_base, int db_base, int exclude_diag,
                    uint64_t* nn_key, int64_t* hist, void* on_stream);

/*
 * Edit-distance nearest neighbour (added under ABI 17: one new entry, nothing existing changed; not in the reference). A design
 * that is a training row shifted by a few bases is a copy, and its Hamming distance is that of an unrelated row.
 *
 * svdd_edit_nn: q [B, ceil(Lq / 16)] and db [N, ceil(Ld / 16)] packed u32 (svdd_pack_tokens; the padding bits are never read).
 *   Lq and Ld may differ, both 1 .. 1024. For every pair (i, j), d = the Levenshtein distance of the two rows: substitution,
 *   insertion and deletion cost 1 each, global (no free ends). cap = 0 .. max(Lq, Ld); a pair with d > cap is "beyond".
 *   exclude_diag, q_base and db_base as for svdd_hamming_nn. nn_key [B] u64 or NULL, started by the caller at all ones or at any
 *   earlier key: every pair with d <= cap does nn_key[i] = min(nn_key[i], (uint64(d) << 32) | uint32(db_base + j)) (the lowest
 *   database index among ties); pairs beyond never touch it, so an untouched key means "no neighbour within cap". hist [cap + 2]
 *   i64 or NULL, ACCUMULATED INTO: the pairs at each distance 0 .. cap, and in bin cap + 1 all pairs beyond. Exact integers,
 *   independent of the launch shape and of how queries and database are cut into calls. With hist NULL the kernel skips, or
 *   leaves part-way, a pair that cannot lower the key it read for that query (so a caller may seed nn_key with a cheap upper
 *   bound); the result is the same. With hist every pair lands in its exact bin. A thread keeps one query as four bit planes of
 *   ceil(Lq / 32) <= 32 words and runs Myers' bit-vector recurrence (Hyyro's edit-distance form) on them as one multi-word
 *   integer, one step per database token; a workgroup of 256 queries walks a segment of at most 2^22 database rows in tiles
 *   staged in LDS and counts into u32 bins in LDS. SVDD_E_ARG: B, N, Lq or Ld <= 0, Lq or Ld > 1024, cap outside 0 .. max(Lq, Ld),
 *   a negative base, db_base + N or q_base + B >= 2^31, a NULL q or db, neither output.
 */
int svdd_edit_nn(const uint32_t* q, const uint32_t* db, int B, int N, int Lq, int Ld, int cap, int q_base, int db_base,
                 int exclude_diag, uint64_t* nn_key, int64_t* hist, void* on_stream);

/*
 * Greedy selection under a minimum distance (added under ABI 17: two new entries, nothing existing changed; not in the
 * reference): the two device steps of "walk the rows from the best down, keep a row that is at least min_dist from every row kept".
 * Integer arithmetic only; every output is exact and independent of the launch shape. The stream is explicit (as svdd_edit_nn).
 *
 * svdd_within: q [B, W] and db [N, W] packed u32 (svdd_pack_tokens), W = ceil(L / 16); q_rc [B, W] or NULL: the packed reverse
 *   complements of the queries (row i of q_rc is rc(row i of q), rc(a)[l] = 3 - a[L - 1 - l]). d(i, j) = the Hamming distance of
 *   q_i and db_j (svdd_hamming_nn's; the padding bits of the last word are masked out on both sides) or, with q_rc, the smaller of
 *   that and the distance of q_rc_i and db_j. db_count: a device int32 or NULL; only the database rows j < n = min(N, *db_count)
 *   exist (a count below 0 reads as 0); NULL: n = N. radius = 0 .. L - 1; a pair is a hit when d <= radius.
 *   first [B] i32 or NULL, started by the caller at INT32_MAX or at any earlier value: first[i] = min(first[i], the lowest j < n
 *   that is a hit) by integer atomic min; a query without a hit keeps its value. mask [B, mask_words] u32 or NULL, mask_words >=
 *   ceil(N / 32): EVERY word of every row i < B is WRITTEN by a plain store (the caller need not zero it): bit j % 32 of word
 *   j / 32 is set iff j < n and (i, j) is a hit; all other bits, the words at and beyond ceil(N / 32) included, are zero. A
 *   thread keeps one query (and its reverse complement) in registers, a workgroup of 256 queries walks a segment of the database
 *   in tiles of 64 rows staged in LDS and the owning thread gathers 32 rows into one mask word. The grid is sized from N; a
 *   workgroup whose segment starts at or beyond n computes nothing (it stores its zero words of mask).
 *   SVDD_E_ARG: B, N or L <= 0, L > 1024, radius outside 0 .. L - 1, a NULL q or db, neither output, mask with mask_words <
 *   ceil(N / 32).
 *
 * svdd_greedy_pick: the serial walk over ONE block of T <= 4096 rows in rank order, in one launch of one wave. mask [T, mask_words]
 *   u32, mask_words >= ceil(T / 32): bit j of row i set = rows i and j of the block are closer than the minimum distance (svdd_within
 *   of the block against itself; only the bits j > i of row i matter, and only the first ceil(T / 32) words of a row are read).
 *   first [T] i32 or NULL: the number of the earliest pick of EARLIER blocks that row i is too close to, or INT32_MAX (svdd_within
 *   against reps). rows [T, W] packed u32, W = ceil(L / 16); base: the rank of the block's first row. State, read and advanced:
 *   count (device int32: the picks so far), reps [cap, W] u32 and picked_rank [cap] i32 (appended at index count). For i = 0 ..
 *   T - 1 in order: first[i] != INT32_MAX -> rep_pick[i] = first[i]; else a pick p of this block with bit i set in its mask row
 *   exists -> rep_pick[i] = the earliest such p; else *count < min(k, cap) -> the row is picked: p = (*count)++, reps[p] = rows[i],
 *   picked_rank[p] = base + i, rep_pick[i] = p; else rep_pick[i] = -1. rep_pick [T] i32 is WRITTEN in full; reps and picked_rank
 *   are written at the new picks' indices only, never at or beyond cap. A *count outside 0 .. cap when the kernel starts: nothing
 *   at all is written. The set of settled rows is held in registers (two words per lane); a row that is not picked never loads
 *   its mask row, and nothing the walk branches on differs between lanes.
 *   SVDD_E_ARG: T outside 1 .. 4096, L outside 1 .. 1024, k < 1, cap < 1, mask_words < ceil(T / 32), base < 0 or base + T >= 2^31,
 *   a NULL mask, rows, count, reps, picked_rank or rep_pick.
 */
int svdd_within(const uint32_t* q, const uint32_t* q_rc, const uint32_t* db, const int32_t* db_count, int B, int N, int L, int radius,
                int32_t* first, uint32_t* mask, int mask_words, void* on_stream);
int svdd_greedy_pick(const uint32_t* mask, int mask_words, const int32_t* first, const uint32_t* rows, int T, int L, int base, int k,
                     int32_t* count, uint32_t* reps, int32_t* picked_rank, int cap, int32_t* rep_pick, void* on_stream);

/*
 * Greedy selection under a minimum EDIT distance (added under ABI 17: two new entries, nothing existing changed; not in
 * the reference). A design and its copy shifted by one base are far apart by Hamming distance and one edit from each other twice
 * over; svdd_edit_within is the bit matrix svdd_greedy_pick needs by Levenshtein distance, svdd_edit_pairs the distance of chosen
 * pairs. Integer arithmetic only; every output is exact and independent of the launch shape. The stream is explicit.
 *
 * svdd_edit_within: q [B, W] and db [N, W] packed u32 (svdd_pack_tokens) of ONE length L = 1 .. 1024, W = ceil(L / 16); the padding
 *   bits of the last word are never read. d(i, j) = the Levenshtein distance of q_i and db_j (svdd_edit_nn's: substitution,
 *   insertion and deletion cost 1 each, global) or, with both_strands != 0, the smaller of that and the distance of rc(q_i) and
 *   db_j, rc(a)[l] = 3 - a[L - 1 - l]. The distance is unchanged when both rows are reversed and when both pass through one
 *   bijection of the alphabet, so lev(rc(q), db) = lev(q, rc(db)): the kernel walks the staged database row backwards with every
 *   token t read as 3 - t against the SAME four bit planes of the query, and only for the rows a lane of the wave did not hit on
 *   the first strand; the caller passes no reverse complements. db_count: a device int32 or NULL; only the database rows
 *   j < n = min(N, *db_count) exist (a count below 0 reads as 0); NULL: n = N. radius = 0 .. L - 1; a pair is a hit when
 *   d <= radius. first [B] i32 or NULL, started by the caller at INT32_MAX or at any earlier value: first[i] = min(first[i], the
 *   lowest j < n that is a hit) by integer atomic min; a query without a hit keeps its value. mask [B, mask_words] u32 or NULL,
 *   mask_words >= ceil(N / 32): EVERY word of every row i < B is WRITTEN by a plain store (the caller need not zero it): bit
 *   j % 32 of word j / 32 is set iff j < n and (i, j) is a hit; all other bits, the words at and beyond ceil(N / 32) and the
 *   words of segments beyond the device count included, are zero. A thread keeps one query as four bit planes of ceil(L / 32)
 *   <= 32 words (svdd_edit_nn's recurrence and its classes of 1, 2, 4, 7, 8, 16 and 32 words), a workgroup of 256 queries walks
 *   a segment of the database in tiles of 64 rows staged in LDS, and the owning thread gathers 32 rows into one mask word. Every
 *   16 columns a wave leaves a database row once the diagonal's lower bound exceeds the radius for all its lanes. The grid is
 *   sized from N; a workgroup whose segment starts at or beyond n computes nothing (it stores its zero words of mask).
 *   SVDD_E_ARG: B, N or L <= 0, L > 1024, radius outside 0 .. L - 1, a NULL q or db, neither output, mask with mask_words <
 *   ceil(N / 32).
 *
 * svdd_edit_pairs: q [B, ceil(Lq / 16)] and db [N, ceil(Ld / 16)] packed u32, Lq and Ld 1 .. 1024 (they may differ); idx [B] i32.
 *   dist [B] i32 is WRITTEN in full: dist[i] = the Levenshtein distance of q_i and db[idx[i]] (with both_strands != 0 the smaller
 *   of that and the distance of rc(q_i) and db[idx[i]]), or -1 where idx[i] < 0, where idx[i] >= N (no row is read) or where the
 *   distance exceeds cap = 0 .. max(Lq, Ld). One thread per pair, the plane chosen per lane: B pairs, not B N.
 *   SVDD_E_ARG: B, N, Lq or Ld <= 0, Lq or Ld > 1024, cap outside 0 .. max(Lq, Ld), a NULL q, db, idx or dist.
 */
int svdd_edit_within(const uint32_t* q, const uint32_t* db, const int32_t* db_count, int B, int N, int L, int radius,
                     int both_strands, int32_t* first, uint32_t* mask, int mask_words, void* on_stream);
int svdd_edit_pairs(const uint32_t* q, const uint32_t* db, const int32_t* idx, int B, int N, int Lq, int Ld, int cap,
                    int both_strands, int32_t* dist, void* on_stream);

/*
 * PWM motif scanning (added under ABI 17: one new entry, nothing existing changed; not in the reference). Integer log-odds tables,
 * int32 sums and integer atomics only: every result is exact and independent of the launch shape and of how the caller cuts its
 * rows into chunks. The stream is explicit (as svdd_kmer_counts).
 *
 * svdd_motif_scan: packed [N, W] u32, W = ceil(L / 16) (svdd_pack_tokens: finished rows, tokens 0..3; the padding bits are never
 *   read as tokens). pwm [M, 32, 4] i16 in A, C, G, T order, width [M] i32 (1 .. 32; clamped to that range, and a column at or
 *   beyond a motif's width never contributes), threshold [M] i32, all on the device. For row n, motif m of width w and every start
 *   p = 0 .. L - w:  forward S+ = sum_i pwm[m, i, x[p + i]];  reverse strand S- = sum_i pwm[m, w - 1 - i, 3 - x[p + i]]  (int32).
 *   A window is a hit on a strand when that strand's score is >= threshold[m]; the strands count separately (a palindromic site
 *   counts twice). both_strands = 0: only S+ exists.
 *   hits [M] i64 and rows_hit [M] i64 are ADDED to (64-bit integer atomics, one per wave and motif): the hits, and the rows with
 *   at least one hit. row_hits [N, M] i32 is WRITTEN: the row's hits. row_best [N, M] i64 is WRITTEN: the key of the row's best
 *   window, (uint64(uint32(score) ^ 0x80000000) << 32) | uint32(~(2 start + strand)) with strand 0 = forward, 1 = reverse: the
 *   largest key is the highest score, among equal scores the lowest start, at one start forward before reverse (the scheme of
 *   svdd_hamming_nn's key). L < w is valid: no windows, no hits, key 0 (score INT32_MIN, no start). Each of the four outputs may
 *   be NULL. A workgroup takes 64 rows and 8 motifs at a time; a row's windows for one motif are scanned by one wave, so the
 *   per-row outputs need no atomics.
 *   SVDD_E_ARG: N, L or M <= 0, L > 1024, a NULL packed / pwm / width / threshold, all four outputs NULL.
 */
int svdd_motif_scan(const uint32_t* packed, int N, int L, const int16_t* pwm, const int32_t* width, const int32_t* threshold, int M,
                    int both_strands, int64_t* hits, int64_t* rows_hit, int32_t* row_hits, int64_t* row_best, void* on_stream);

/*
 * The motif reward of SVDD-PM decoding (added under ABI 17: one new entry, nothing existing changed; not in the
 * reference): from u8 token rows to one fp32 score per row in one launch, under a device-side row count, so that it can stand
 * where a reward net stands in the posterior-mean loop. The stream is explicit (as svdd_motif_scan).
 *
 * svdd_motif_reward: tok [n, L] u8, finished rows; a token > 3 sets err[0] = 1 (err: caller-zeroed device word or NULL, read
 *   later) and is read as 0, as in svdd_pack_tokens. count: a device int32 or NULL; rows >= count[0] are neither read nor written
 *   (a count below 0 reads as 0, above n as n); NULL means all n rows. pwm / width / threshold and both_strands as svdd_motif_scan
 *   takes them. hit_coef, hit_cap (>= 0), margin_coef, margin_floor (>= 0): int32 [M] on the device. With hits_m and best_m of
 *   row r exactly as svdd_motif_scan defines them (the strands count separately; best_m the highest window score on either
 *   strand; L < w: no window),
 *     T(r) = sum_m [ hit_coef_m min(hits_m, hit_cap_m) + margin_coef_m max(min(best_m - threshold_m, 0), -margin_floor_m) ]
 *   in int64, the margin being -margin_floor_m where there is no window (the caller keeps the sum of |hit_coef_m| hit_cap_m +
 *   |margin_coef_m| margin_floor_m below 2^62). score [n] f32 or NULL: score[r] = __fadd_rn(base[r], __fmul_rn((float)T, unit));
 *   base [n] f32 or NULL (= 0); score may alias base. term [n] i64 or NULL receives T. Everything before the last two fp32
 *   operations is integer arithmetic: the result is exact and independent of the launch shape and of how rows are cut into calls.
 *   A workgroup packs its rows (8; measured against 32 and 64 in profiles/motif_reward_time.txt) into LDS itself and walks all
 *   motif groups for them, so a row's T is finished in one workgroup: no atomics, no second pass. A workgroup whose first row is
 *   >= count[0] exits at once.
 *   SVDD_E_ARG: n, L or M <= 0, L > 1024, a NULL tok, table or coefficient array, score and term both NULL.
 */
int svdd_motif_reward(const uint8_t* tok, int n, int L, const int32_t* count, const int16_t* pwm, const int32_t* width,
                      const int32_t* threshold, int M, int both_strands, const int32_t* hit_coef, const int32_t* hit_cap,
                      const int32_t* margin_coef, const int32_t* margin_floor, const float* base, float unit, float* score,
                      int64_t* term, int32_t* err, void* on_stream);

/*
 * svdd_select— replaces torch.stack(scores,1) -> softmax(dim=1) -> argmax(dim=1) ->
 * per-row Python gather + stack                     diffusion_gosai.py:1219-1227 (= :1451-1459)
 *
 *  scores [B,M] fp32 (row b, candidate m) ; cand [B,M,L] u8
 *  x_next [B,L] u8 out ; soft [B,M] fp32 out (softmax, may be NULL) ; idx [B] i32 out (may be NULL)
 *  (x_next == NULL with idx != NULL, M <= 64: the decision only, no row gather — round 6's measurement of what the gather costs)
 *  rng is read only for SVDD_SELECT_MULTINOMIAL (must be PHILOX).
 */
int svdd_select(const float* scores, const uint8_t* cand, int B, int L, int M, int mode,
                const svdd_rng_t* rng, uint8_t* x_next, float* soft, int32_t* idx,
                void* stream);

/*
 * svdd_x0hat — SVDD-PM / TDS posterior-mean candidate (Tweedie):
 *   forward()'s _subs_parameterization + argmax(dim=2) + one_hot + keep-unmasked merge +
 *   .float().transpose(1,2)                         diffusion_gosai.py:1415-1419,1430 ; :1263-1269
 *  logits [R,L,5] raw backbone output for tokens xt [R,L] ; out onehot_t [R,4,L] fp32 (may be NULL when x0hat is given) ;
 *  x0hat [R,L] u8 out (may be NULL).
 */
int svdd_x0hat(const float* logits, const uint8_t* xt, int R, int L, int layout,
               float* onehot_t, uint8_t* x0hat, void* stream);

/*
 * svdd_finalize — noise-removal step: forward() then logits[:,:,:-1].argmax(-1)
 *                                                   diffusion_gosai.py:1049-1060
 *  out_i64 [B,L] int64 (the API's LongTensor) and/or out_u8 [B,L]; either may be NULL.
 */
int svdd_finalize(const float* logits, const uint8_t* x, int B, int L, int layout,
                  int64_t* out_i64, uint8_t* out_u8, void* stream);

/*
 * svdd_transform_samples — tokens -> one-hot(4) with MASK rows zero
 *                                                   diffusion_gosai.py:1462-1470 ≡ Enformer.py:269-277
 *  transposed == 0: out [R,L,4] (value-net layout) ; != 0: out [R,4,L] (reward-model layout, Enformer.py:447)
 */
int svdd_transform_samples(const uint8_t* tok, int R, int L, int transposed, float* out,
                           void* stream);

/*
 * svdd_subs_logp — Diffusion.forward()'s SUBS re-parameterisation alone
 *                                                   diffusion_gosai.py:286-304
 *  logp [B,L,5] out. (Used by the per-step API mirror and the DPS baseline.)
 */
int svdd_subs_logp(const float* logits, const uint8_t* x, int B, int L, int layout, float* logp,
                   void* stream);

/*
 * Exact work-skipping. A candidate that unmasked nothing is a copy of its parent x_t
 * (diffusion_gosai.py:1203), and with time_conditioning off (:334-335) every net output for it equals the parent's; a
 * row whose selected candidate is such a copy keeps its logits. The helpers below let the engine run the nets only on
 * the LIVE candidates / rows without a host round trip: the compacted index list and its length stay in device memory
 * and the net kernels take the length as a device pointer (`count` arguments below).
 *
 * svdd_compact_flags — stable compaction of n flags (one workgroup): flags[i] != 0 -> live_idx[k] = i, slot[i] = k with
 *   k = number of live items before i; else slot[i] = -1; count[0] = number of live items. Both compactions write slot [n] fully,
 *   count[0], and live_idx at [0, count[0]) ONLY: the rest of live_idx keeps what it held.
 * svdd_compact_by_key — the same compaction ORDERED by key, largest first (stable inside a key; keys clamp to 15, key <= 0 = not
 *   live): live_idx lists the live items by descending key, slot[i] = position of item i in it or -1. With key = row tiles of a
 *   candidate's window (the flags svdd_candidate_windows writes) the windowed tower's long workgroups are dispatched first.
 *   split > 0: count must hold 3 ints; count[1] = min(count[0], split), count[2] = max(count[0] - split, 0) — the lengths of the
 *   list's two parts [0, split) and [split, ...), for callers that run the parts as separate launches (fused.py: the GRU's second round).
 *   count[1] and count[2] are written ONLY when split > 0: with split == 0 count may hold a single int.
 * svdd_gather_rows   — dst[i,:] = src[idx[i],:] for i < count[0] (count may be NULL = n); rows of row_bytes bytes; rows of dst at and
 *   beyond the count are left untouched. No alignment requirement: the copy unit (4, 2 or 1 bytes) is taken from
 *   row_bytes | src | dst, so every access is aligned to its unit.
 * svdd_advance_rows  — the selected candidate becomes the next parent: for every b, if slot[b*M + sel[b]] >= 0 then
 *   dst[b,:] = src[slot[...],:], else dst[b] is left untouched; rows of row_bytes, a multiple of 4, and src and dst aligned to
 *   4 bytes (anything else: SVDD_E_ARG). 16-byte units are used when row_bytes and both pointers allow, 4-byte units otherwise.
 * svdd_select_compact — svdd_select on compacted scores: candidate (b, m) has score scores[slot[b*M+m]] if its slot is
 *   >= 0, else parent_score[b]. Additionally writes sel_score[b] (the selected candidate's score = the NEXT step's
 *   parent score) and changed[b] (1 iff x_next[b] differs from x[b]). slot == NULL: exactly svdd_select.
 *   Bound on L (svdd_select too; M <= 64 with the row gather, i.e. x_next != NULL, unless SVDD_OPT_SELECT_ONE_ROW is 1): a wave copies
 *   the winning rows of its W rows in units of u = 8, 4, 2 or 1 bytes (the largest that divides L, the candidate row stride, cand
 *   and x_next), W = 64 / pow2(M) times 4 — times 1 below 2^21 (row, candidate) slots — capped at 64, and W * (L / u) must stay
 *   below 2^22 (SVDD_E_ARG otherwise): L < 65536 is always accepted.
 */
int svdd_compact_flags(const int32_t* flags, int n, int32_t* live_idx, int32_t* slot, int32_t* count, void* stream);
int svdd_compact_by_key(const int32_t* key, int n, int32_t* live_idx, int32_t* slot, int32_t* count, int split, void* stream);
int svdd_gather_rows(const void* src, const int32_t* idx, const int32_t* count, int n, int row_bytes, void* dst, void* stream);
int svdd_advance_rows(const void* src, const int32_t* slot, const int32_t* sel, int B, int M, int row_bytes, void* dst,
                      void* stream);
int svdd_select_compact(const float* scores, const int32_t* slot, const float* parent_score, const uint8_t* cand, int B,
                        int L, int M, int mode, const svdd_rng_t* rng, uint8_t* x_next, float* soft, int32_t* idx,
                        float* sel_score, int32_t* changed, void* stream);

/*
 * svdd_tds_resample — SMC/TDS baseline resampling step
 *   ratio = exp(fl32(1.0/alpha) * (num-den)); p = ratio/ratio.sum(); idx = np.random.choice(B,B,p=p);
 *   (alpha is the caller's Python float, i.e. a double: the reference rounds the double quotient 1.0/alpha to fp32 once)
 *   return sample[idx]                              diffusion_gosai.py:1280-1284
 *  reward_num, reward_den [B] fp32 ; sample [B,L] u8 ; u [B] fp64 uniforms in [0,1)
 *  (REPLAY of numpy's RandomState.random_sample, supplied by the host) ;
 *  out x_next [B,L] u8 ; idx [B] i32 (may be NULL) ; work [2*B] fp64 scratch (cdf + ratio).
 *  Two launches on `stream`: the CDF (one workgroup; the float64 cumsum is a serial chain by numpy's definition) and the
 *  searchsorted + row gather (whole chip). Any B; the pairwise sum's blocks run in parallel up to B = 131072.
 *  The row gather copies in units of 8, 4, 2 or 1 bytes taken from L | sample | x_next (no alignment requirement) and finds a
 *  unit's row by integer division; L < 2^25 (SVDD_E_ARG otherwise: a wave's 64 rows' units are counted in an int).
 */
int svdd_tds_resample(const float* reward_num, const float* reward_den, double alpha,
                      const uint8_t* sample, const double* u, int B, int L,
                      uint8_t* x_next, int32_t* idx, double* work, void* stream);

/*
 * svdd_mt19937_uniform_f32 — torch's CPU generator stream on the device (parity-mode RNG without host traffic)
 *   replaces torch.rand / rand_like on the global CPU generator: diffusion_gosai.py:33 (`torch.rand_like(categorical_probs)`),
 *   i.e. at::mt19937 (std::mt19937) + uniform_real_distribution<float>: out[i] = (y_i & 0xFFFFFF) * 2^-24, y_i the i-th
 *   tempered 32-bit output, strictly in sequence.
 *  state [625] u32 in device memory: the 624 state words + the index of the next output (624 = twist first, as
 *  torch.manual_seed leaves it); advanced in place by n outputs (any rotation of the word window is a valid state: the
 *  recurrence is shift-invariant; svdd_amd/ops.py converts from / to torch.get_rng_state()'s layout).
 *  out [n] fp32. One workgroup (the recurrence is serial): ~0.3 ns per output; launch it on a side stream a step ahead.
 */
int svdd_mt19937_uniform_f32(uint32_t* state, float* out, long long n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Net kernels — internals of the value network (reference Enformer.py), not of the sampler. They are
 * optional accelerations of PyTorch modules (svdd_amd/fused.py); the sampler API above never needs them.
 *
 * svdd_gru_bidir_f32 — bidirectional single-layer GRU, input = hidden = 64, fp32
 *   (reference Enformer.py:1595-1602 nn.GRU(64, 64, bidirectional=True, batch_first=True), gate order r,z,n).
 *   x [n,L,64] ; out [2,n,L,64] = per-direction hidden states (the caller sums them, Enformer.py:1617).
 *   wpack [2][4][64][96], bpack [2][4][64]: weights repacked per MFMA lane, see svdd_amd/fused.py:pack_gru.
 *   `count` arguments of the net kernels: device scalar with the number of VALID rows of a compacted batch (the tensors
 *   stay laid out for n rows); NULL = n. See "Exact work-skipping" above. */
int svdd_gru_bidir_f32(const float* x, const float* wpack, const float* bpack, float* out, int n, int L,
                       const int32_t* count, void* stream);

/* The same GRU with a backward pass to its INPUT (weights are frozen in every decode path) — for the gradient-guidance baseline
 * of BASELINE.json configs[4] (reference diffusion_gosai.py:1321-1330 compute_gradient_DPS differentiates the reward model, whose
 * trunk holds this GRU, Enformer.py:1595-1602, with respect to the one-hot input). csrc/svdd_gru_train.hip.
 * svdd_gru_bidir_train_f32: forward as svdd_gru_bidir_f32 (same bits; no compaction), also writing
 *   save [2 dirs][n][L][4][64] = r, z, n, W_hn h + b_hn per step.
 * svdd_gru_bidir_bwd_f32: grad_out [2][n][L][64] (gradient of the per-direction outputs), out / save of the forward call,
 *   wpack_bwd [2 dirs][4 waves][64 lanes][96] packed by svdd_amd.fused.pack_gru_bwd -> dx [2][n][L][64], each direction's
 *   contribution to d loss / d x (the caller adds the two). */
/* The element-wise half of a dilated-CNN backbone layer under autograd (reference models/dnaconv.py:212-247 CNNModel.forward2:
 * feat' = relu(conv(LayerNorm(feat + time_bias)) + b) + feat; differentiated with respect to its input by the DPS baseline,
 * diffusion_gosai.py:1321-1330). Rows [rows, channels] fp32 channels-last, channels in {64, 128, 256}; tb [rows / rows_per_seq,
 * channels] = the time bias per sequence. Weights are frozen: input gradients only.
 * svdd_bb_layer_fwd_f32: f_out = relu(y + bias) + f_prev, mask = (y + bias > 0) (y NULL: f_out = f_prev, nothing written), then
 *   hn = LayerNorm(f_out + tb) gamma + beta (gamma NULL: none).
 * svdd_bb_layer_bwd_f32: g_out = g_in + dLayerNorm(g_hn) at h = f_in + tb ; gt_out = g_out where mask_prev else 0 (both NULL: none). */
int svdd_bb_layer_fwd_f32(const float* y, const float* bias, const float* f_prev, const float* tb, const float* gamma,
                          const float* beta, float eps, float* f_out, uint8_t* mask, float* hn, int64_t rows, int rows_per_seq,
                          int channels, void* stream);
int svdd_bb_layer_bwd_f32(const float* g_hn, const float* f_in, const float* tb, const float* gamma, float eps, const float* g_in,
                          const uint8_t* mask_prev, float* g_out, float* gt_out, int64_t rows, int rows_per_seq, int channels,
                          void* stream);
int svdd_gru_bidir_train_f32(const float* x, const float* wpack, const float* bpack, float* out, float* save, int n, int L,
                             void* stream);
int svdd_gru_bidir_bwd_f32(const float* grad_out, const float* out, const float* save, const float* wpack_bwd, float* dx, int n,
                           int L, void* stream);
/* svdd_value_tail_f32 — everything of the ConvGRU value net after the GRU, in one pass over the two GRU outputs:
 *   out[n][t] = b_eff[t] + mean_l sum_c w_eff[c][t] * relu(b1'[c] + sum_k W1'[c][k] * norm(h_fwd + h_bwd)[n][l][k])
 *   norm = LayerNorm over the 64 channels WITHOUT affine (eps 1e-5); the caller folds the LayerNorm affine into the
 *   linear map: W1' = W1 diag(gamma), b1' = b1 + W1 beta
 *   (reference Enformer.py:1617 direction sum; :2010-2047 FeedForwardBlock; :2131-2173 ConvHead with pool "avg").
 *   h_fwd, h_bwd [n,L,64] ; w1pack [64 lanes][128]: lane (j = lane & 15, g = lane >> 4) holds
 *   W1'[16 ct + j][16 (s / 4) + 4 g + s % 4] at 16 ct + s (svdd_amd/fused.py:pack_tail) ; b1 = b1' [128] ;
 *   w_eff [128][n_tasks] = (W_head W_2)^T, b_eff [n_tasks] = W_head b_2 + b_head ; out [n][n_tasks] ; n_tasks <= 4.
 *   Summation order (what an fp32 restatement has to follow to carry this kernel's rounding error; tests/net_ref.py): the 64 -> 128
 *   chain of a row starts at b1' ; one wave per sequence, whose lane (j, g) adds w_eff[c][t] relu(.) of rows 16 tile + 4 g + rho
 *   (rho < 4) and columns c = 16 ct + j (ct < 8) to ONE fp32 accumulator in (tile, rho, ct) order — 32 ceil(L / 16) one-wide steps
 *   from zero, not one chain per row — then the 64 lanes are summed by an xor butterfly, divided by L, and b_eff is added. */
int svdd_value_tail_f32(const float* h_fwd, const float* h_bwd, const float* w1pack, const float* b1,
                        const float* w_eff, const float* b_eff, float* out, int n, int L, int n_tasks,
                        const int32_t* count, void* stream);
/* tests / experiments: 2 selects the both-directions-per-workgroup scheduling (balanced but measured slower), else default */
int svdd_gru_set_mode(int mode);

/* svdd_epilogue_ln_f32 — fused convolution epilogue (+ next layer's LayerNorm) on channels-last rows [rows, C],
 *   C in {64,128,256}: t = y + bias ; f_out = relu(t) + f_prev (act 0) | relu(t + f_prev) (act 1) | t + f_prev (act 2);
 *   hn = LayerNorm(f_out + tb) * gamma + beta (eps 1e-5).  bias, f_prev, tb may be NULL; hn NULL skips the norm;
 *   f_out NULL skips storing the pre-norm sum.
 *   Shapes: y, f_prev, f_out, hn [rows, C] ; bias, tb, gamma, beta [C] — tb is ONE time bias per channel, shared by every row (the
 *   sigma = 0 bias of inference; svdd_bb_layer_fwd_f32 is the entry with a time bias per sequence). tb is read only with hn.
 *   Replaces the bias/ReLU/residual/LayerNorm tensor ops between two convolutions of the dilated-CNN backbone
 *   (reference models/dnaconv.py:188-197) and of the value net's conv tower (Enformer.py:2269-2285). */
int svdd_epilogue_ln_f32(const float* y, const float* bias, const float* f_prev, const float* tb,
                         const float* gamma, const float* beta, float* f_out, float* hn, int64_t rows,
                         int channels, int act, void* stream);

/* svdd_conv1d_cl_f32 — dilated Conv1d with "same" zero padding on channels-last activations, fp32 on the
 *   exact-fp32 matrix cores, NO bias (the epilogue kernel adds it):
 *     y[n,l,co] = sum_{t,ci} x[n, l + (t - taps/2)*dilation, ci] * W[co,ci,t]
 *   x [n,L,cin], y [n,L,cout], cin/cout in {64,128}, taps odd, L <= 224.
 *   wpack [taps][cin/32][cout][32] = W[co][32c + k][t]   (svdd_amd/fused.py:pack_conv).
 *   Replaces the nn.Conv1d calls of reference models/dnaconv.py:151-156,196 and Enformer.py:2245-2253,2271. */
int svdd_conv1d_cl_f32(const float* x, const float* wpack, float* y, int n, int L, int cin, int cout,
                       int taps, int dilation, const float* bias, const float* f_prev, int act,
                       const float* tb, const float* gamma, const float* beta, float* hn, void* stream);
/*   fused epilogue (specialised shapes only: 128->128 x 9 taps x dilation {1,4,16,64}, 64->64 x 5 taps; L in {200,50}):
 *   act -1: y = conv ; 0: y = relu(conv + bias) + f_prev ; 1: y = relu(conv + bias + f_prev) ; 2: y = conv + bias + f_prev
 *   (bias, f_prev may be NULL); with hn != NULL additionally hn = LayerNorm(y + tb) * gamma + beta (eps 1e-5), the
 *   next layer's normalised input (tb may be NULL).  Other shapes take the generic kernel and require act = -1.
 *   Shapes: f_prev, hn [n,L,cout] like y ; bias, tb, gamma, beta [cout] — tb is ONE time bias per channel, shared by every row and
 *   sequence, as in svdd_epilogue_ln_f32. With act = -1 bias and f_prev are not read. */
/* tests only: != 0 forces the dynamically scheduled kernel instead of the per-(dilation,L) specialisations */
int svdd_conv1d_set_dynamic(int on);

/* svdd_conv_tower_f32 — the whole conv tower of the ConvGRU value net in one launch, activations resident in LDS:
 *   a0 = relu(conv15(onehot) + b0) ; a_{k+1} = relu(conv5(a_k) + b_k [+ a_k])  (k < nlayers, 64 channels, dilation 1)
 *   (reference Enformer.py:1634-1751: Stem + ConvBlocks "CDNRA"; eval-mode BatchNorm folded by the caller).
 *   onehot [n,L,4] ; tiles [2 + 10*nlayers][64][32] weight tiles in execution order (svdd_amd/fused.py:pack_tower) ;
 *   bias [1 + nlayers][64] ; out [n,L,64] ; residual_mask bit k = layer k adds its input ; L <= 208. */
int svdd_conv_tower_f32(const float* onehot, const float* tiles, const float* bias, float* out, int n, int L,
                        int nlayers, int residual_mask, const int32_t* count, void* stream);

/* tests / A-B: 1 = the backbone kernels always fill their 208-row tile with whole sequences (round-1 behaviour); 0 (default)
 * = when several sequences fit a tile (L <= 104) the number taken minimises rounds x tile cost, chosen on the host or, for a
 * device-side row count, by the workgroups themselves (csrc/svdd_spt.h). A row's logits do not depend on the choice. */
int svdd_set_backbone_packing(int full);

/* tests / A-B of the fp32 tower kernels (all produce the same bits): 1 = first generation (runtime tile predicates),
 * 2 / 3 = second generation (live-tile count as a template parameter) with two / one column tile per wave; 0 = default
 * (= 3, the fastest on whole sequences and on windows: profiles/r02_tower_ab.txt) */
int svdd_set_tower_version(int v);

/* svdd_candidate_windows + svdd_conv_tower_windows_f32 — the conv tower on the M candidates of every sample, sharing
 *   the work they have in common with their parent x_t (SVDD-MC scoring, reference diffusion_gosai.py:1203-1209: the
 *   candidates are copies of x_t with a few MASKs replaced). The tower's receptive field is +-17 rows, so a
 *   candidate's tower output differs from its parent's only near the replaced positions; only a row window around
 *   them is computed, the other rows are copied from the parent's output. Bit-identical to svdd_conv_tower_f32 on
 *   the candidates (tests/test_fused_gpu.py::test_tower_windows_equal_full_tower).
 *   svdd_candidate_windows: cand [B,M,L] u8, x [B,L] u8 -> win [B*M][2] = (w0, w1), multiples of 16 covering the
 *     positions where the candidate differs from its parent +- margin (27 for the 5-layer tower); (0, 0) if none:
 *     w0 = max(0, first - margin) rounded down, w1 = min(last + margin + 1, L) rounded up to a multiple of 16 (so w1 <= L rounded up).
 *   svdd_conv_tower_windows_f32: onehot [n = B*M, L, 4] (row b*M + m), win from above, parent_out [B, L, 64] =
 *     svdd_conv_tower_f32 of the parents' one-hot; out [n, L, 64]. 104 < L <= 208, nlayers = 5.
 *   flags [B*M] (may be NULL): the number of row tiles of the window ((w1 - w0) / 16 >= 1) if the candidate differs from its
 *     parent, 0 for an exact copy (input of svdd_compact_flags / key of svdd_compact_by_key). live_idx / count (may be NULL): process only the listed candidates; workgroup i handles
 *     candidate live_idx[i] and writes rows [i*L, (i+1)*L) of out (a compacted batch). */
int svdd_candidate_windows(const uint8_t* cand, const uint8_t* x, int B, int L, int M, int margin, int32_t* win,
                           int32_t* flags, void* stream);
int svdd_conv_tower_windows_f32(const float* onehot, const float* tiles, const float* bias, const int32_t* win,
                                const float* parent_out, float* out, int n, int L, int M, int nlayers,
                                int residual_mask, const int32_t* live_idx, const int32_t* count, void* stream);

/* svdd_candidate_windows_tight — svdd_candidate_windows with the window aligned at ONE end: same arguments, and
 *     w0 = max(0, first - margin),  w1 = w0 + 16 * ceil((min(L, last + margin + 1) - w0) / 16),  flags = (w1 - w0) / 16,
 *   (0, 0) and flag 0 for an exact copy. w0 is any row; w1 may pass L rounded up to 16, by less than a tile ((w1 - w0) / 16 <=
 *   ceil(L / 16)). For svdd_conv_tower_windows_f32 only, whose kernels address everything relative to w0 and need a multiple of 16
 *   of the LENGTH alone: any window that covers [first - margin, last + margin] gives the same rows inside its keep range, so the
 *   tower output equals the aligned windows' bit for bit (tests/test_tower_tight_windows_gpu.py), with 0.33 row tiles less per
 *   window over a decode (6.98 -> 6.65; a window that starts at row 0 was aligned already). The split-precision tower (svdd_conv_tower_windows_lp) takes aligned windows. The stream is the
 *   explicit last argument. SVDD_E_ARG: a NULL cand, x or win; B, L or M <= 0; margin < 0 or > 2^20; B * M >= 2^31. */
int svdd_candidate_windows_tight(const uint8_t* cand, const uint8_t* x, int B, int L, int M, int margin, int32_t* win,
                                 int32_t* flags, void* on_stream);

/* svdd_candidate_parts + svdd_conv_tower_parts_f32 — the windowed fp32 tower with PER-LAYER row ranges and separate parts for
 *   changes far apart: the same output as svdd_candidate_windows_tight + svdd_conv_tower_windows_f32, bit for bit
 *   (tests/test_tower_parts_gpu.py), on fewer row tiles. Layer k of the tower (0 = stem, 5 = last block) has to be right only on
 *   the changed positions +- (reach + 2 (5 - k)) rows, reach = 17 for this tower: 55, 51, ... 35 rows for one changed position,
 *   20 tile-layers where the one window takes 24 — and nothing between two neighbourhoods that are far apart.
 *   svdd_candidate_parts: the positions where a candidate differs from its parent, ascending, are cut into parts wherever two
 *     consecutive ones are >= gap apart; at most 3 parts, later ones are merged into the third. parts [B*M][3][2] = (first, last)
 *     changed position of each part, (-1, -1) where there is none; nparts [B*M] (may be NULL) their number; flags [B*M] (may be
 *     NULL) the candidate's tile-layers = sum over parts and the six layers of ceil(rows of [max(0, first - h), min(L, last + h + 1)) / 16),
 *     h = reach + 2 (5 - k); 0 for an exact copy. key [B*M] (may be NULL) = ceil(flags / 6), the average tiles per layer, 0 .. 13:
 *     what the compactions take in place of the window entries' flags (svdd_compact_flags: > 0 = live; svdd_compact_by_key tells only
 *     15 keys apart and tile-layers reach 78, so flags itself would lose the order) — fused.py hands its flags workspace to `key`.
 *     gap >= 2 (reach + 10) + 16 (70 for this tower), so that two parts' computed tiles never touch on any layer, each range being
 *     rounded up to whole tiles from its own first row; a gap above L gives one part always (per-layer ranges alone).
 *     SVDD_E_ARG: a NULL cand, x or parts; B, L or M <= 0; reach < 0 or > 2^20; a smaller gap; B * M > 2^31 - 4.
 *   svdd_conv_tower_parts_f32: svdd_conv_tower_windows_f32 with parts in place of win (same onehot, parent_out, out, live_idx,
 *     count and profile slot; one workgroup per listed candidate): every layer runs on the tiles that cover its range of every
 *     part, the rows [max(0, first - reach), min(L, last + reach + 1)) of each part come from this computation, all others are
 *     copied from the parent's output. 104 < L <= 208, nlayers = 5, reach = 17 (anything else: SVDD_E_ARG) — and the parts must have
 *     been cut by svdd_candidate_parts with that reach: its gap rule is what keeps two parts' tiles apart. One kernel generation
 *     (svdd_set_tower_version does not apply).
 *   Both take their stream as the explicit last argument. */
int svdd_candidate_parts(const uint8_t* cand, const uint8_t* x, int B, int L, int M, int reach, int gap, int32_t* parts,
                         int32_t* nparts, int32_t* flags, int32_t* key, void* on_stream);
int svdd_conv_tower_parts_f32(const float* onehot, const float* tiles, const float* bias, const int32_t* parts,
                              const float* parent_out, float* out, int n, int L, int M, int nlayers, int residual_mask,
                              int reach, const int32_t* live_idx, const int32_t* count, void* on_stream);
/* svdd_value_late_step_f32 — the fp32 value net (parts tower, GRU, tail) on a compacted, size-ordered list of live candidates that may
 *   exceed ONE round of the GRU's (16 sequences, direction) units on the chip's CUs, as two parts sized ON THE DEVICE:
 *   count3 [3] i32 = what svdd_compact_by_key wrote for this `split` (live entries, of them in the first part <= split, in the second);
 *   A = entries [0, count3[1]) of live_idx, B = entries [split, split + count3[2]) — B is non-empty only when A is full.
 *       tower(B) -> [ GRU(B) || tower(A) ] in ONE launch -> GRU(A) -> tail(rows 0 .. count3[0])
 *   The middle launch runs the GRU kernel's body in its leading workgroups and the parts tower's body in the others, so B's GRU — a
 *   second round with most of the chip idle — hides under A's tower. No host decision, no event, no second stream: a launch whose
 *   part is empty leaves at its count check. onehot, tiles, bias, parts, parent_out, M, nlayers, residual_mask, reach, live_idx: as
 *   svdd_conv_tower_parts_f32 over the n = B * M candidates; wpack, bpack: as svdd_gru_bidir_f32; w1pack, b1, w_eff, b_eff, n_tasks:
 *   as svdd_value_tail_f32. seq [n][L][64], h [2][n][L][64]: work buffers (row i = list entry i); out [n][n_tasks]: the scores of
 *   entries 0 .. count3[0], the SAME BITS as the three entries named above give for them; rows from count3[0] on are not written.
 *   0 < split < n. All four launches go to `on_stream`. */
int svdd_value_late_step_f32(const float* onehot, const float* tiles, const float* bias, const int32_t* parts,
                             const float* parent_out, float* seq, int n, int L, int M, int nlayers, int residual_mask, int reach,
                             const int32_t* live_idx, const int32_t* count3, int split, const float* wpack, const float* bpack,
                             float* h, const float* w1pack, const float* b1, const float* w_eff, const float* b_eff, float* out,
                             int n_tasks, void* on_stream);

/* svdd_backbone_cnn_f32 — the whole dilated-CNN masked-diffusion backbone at sigma = 0 in ONE launch
 *   (reference models/dnaconv.py:176-210 as called from diffusion_gosai.py:334-340): one-hot + 9-tap first conv,
 *   nlayers x [LayerNorm(f + tb_i) -> dilated 9-tap conv 128->128 -> ReLU -> + f], then the two 1x1 convs of
 *   final_conv. The residual stream stays in registers, the normalised activations in LDS; nothing but the tokens
 *   and the logits touches HBM.  hidden_dim = 128, alphabet 5, L <= 208, nlayers <= 32.
 *   x [n,L] u8 tokens ; table0 [9][5][128] = W_first[co][c][t] ; tiles [nlayers][4][9][128][32] = W_i[co][32c+k][t]
 *   followed by [4][128][32] = W_f1[co][32c+k] ; vec [nlayers+2][4][128]: row 0 = {b_first}, row 1+i = {b_i, tb_i,
 *   gamma_i, beta_i}, row nlayers+1 = {b_f1} ; w2 [5][128] then b2 [5] ; dilations: HOST int[nlayers] ;
 *   out [n,L,5] raw logits (layout BLV).  Packing: svdd_amd/fused.py:pack_backbone.
 *   Exact work-skipping: count (device scalar, NULL = n) limits the forward to the first count[0] compact rows; row_idx
 *   (NULL = identity) makes compact row r read the tokens of sequence row_idx[r] of x, and with out_scatter != 0 write
 *   its logits to row row_idx[r] of out (per-row logits cache: only the rows that changed are recomputed, in place)
 *   instead of row r (candidate compaction). A row's logits are the same bits wherever it is evaluated. */
int svdd_backbone_cnn_f32(const uint8_t* x, const float* table0, const float* tiles, const float* vec,
                          const float* w2, float* out, int n, int L, int nlayers, const int* dilations,
                          const int32_t* count, const int32_t* row_idx, int out_scatter, void* stream);
/* svdd_backbone_cnn_save_f32 + svdd_backbone_cnn_grad_f32 — the backbone's input gradient, one launch each way (the gradient-
 *   guidance baseline DPS: reference diffusion_gosai.py:1321-1330 differentiates reward(softmax(E[x0 | x_t])) with respect to
 *   onehot(x_t) through models/dnaconv.py:212-247; the weights are frozen). 104 < L <= 208 (one sequence per workgroup).
 *   svdd_backbone_cnn_save_f32: svdd_backbone_cnn_f32 on the tokens x (the SAME BITS in `out`) that also writes, in the kernel's
 *     lane-private layout, xhat [n][nlayers][56][512] f32 (LayerNorm'd value before the affine map), rstd [n][nlayers][208] f32
 *     and mask [n][nlayers + 2][512] u64 (ReLU decisions of the first layer, every conv layer and final_conv's first 1x1).
 *     Layout and extents: thread tid = 64 w + 16 g + j of the sequence's workgroup (w = wave, cg = w & 3, rh = w >> 2) owns rows
 *     16 (rh + 2 r) + 4 g + e (r < 7, e < 4) and channels 32 cg + j + 16 ct (ct < 2); slot s = (2 r + ct) 4 + e. xhat[..][s][tid] is
 *     written for every slot whose row is < 208 and for no other (r = 6 of the waves with rh = 1 is never written), bit s of
 *     mask[..][tid] is that element's decision (bits 56 .. 63 zero; every u64 is written), rstd[..][row] is written for all 208 rows
 *     of the tile. Rows >= L hold values of the zero padding, not of the sequence: svdd_backbone_cnn_grad_f32 reads them (they must
 *     be finite) but no bit of dx depends on them, nor on the mask bits of those rows (tests/test_backbone_grad_kernel_gpu.py).
 *   svdd_backbone_cnn_grad_f32: dlogits [n,L,5] = d loss / d `out` -> dx [n,L,5] = d loss / d onehot(x), through the transposed
 *     1x1 convs, 20 x [ReLU', transposed dilated conv (the same implicit GEMM on tiles_bwd), LayerNorm backward from xhat / rstd,
 *     residual] and the first conv's transpose. tiles_bwd: W_f1^T as [4][128][32], then layers nlayers-1 .. 0 as [4][9][128][32] of
 *     W'[ci][32c+k][t] = W[32c+k][ci][8-t] ; gamma [nlayers][128] ; w2, table0 as in svdd_backbone_cnn_f32.
 *     Packing: svdd_amd/fused.py:pack_backbone_grad. */
int svdd_backbone_cnn_save_f32(const uint8_t* x, const float* table0, const float* tiles, const float* vec, const float* w2,
                               float* out, int n, int L, int nlayers, const int* dilations, float* xhat, float* rstd,
                               unsigned long long* mask, void* stream);
int svdd_backbone_cnn_grad_f32(const float* dlogits, const float* tiles_bwd, const float* gamma, const float* w2,
                               const float* table0, const float* xhat, const float* rstd, const unsigned long long* mask,
                               float* dx, int n, int L, int nlayers, const int* dilations, void* stream);
/* svdd_backbone_incr_f32 — svdd_backbone_cnn_f32 (the SAME BITS in `out`) for a decode that forwards the same n sequences step
 *   after step with few tokens changed in between: the residual stream behind the leading run of `lead` dilation-1 conv layers
 *   (lead >= 2, dilations[0 .. lead) all 1; 104 < L <= 208) is carried in caller-owned device memory and only the 16-row tiles
 *   inside the reach of a changed token are recomputed. x, table0, tiles, vec, w2, out, dilations: as svdd_backbone_cnn_f32.
 *   planes [lead][n][208][128] f32: plane k - 1 = the stream after conv layer k - 1 (rows >= L are never written) ;
 *   x_prev [n][L] u8: the tokens the planes belong to ; items [lead][n][7] i32: the step's work list, first tile | tiles << 8 per
 *   run of adjacent tiles inside p +- (4 + 4 k) of a changed position p for plane k, runs cut to max_item (2 or 4) tiles, 0 = empty
 *   slot (all 7 slots of every row are rewritten each step) ; stat (may be NULL): device u64, += the tile-layers the step marked.
 *   first != 0: the whole forward in one launch, which also fills planes and x_prev (the first step of a decode, or any step
 *   after the planes went stale). first == 0: compares x with x_prev (and updates it), one launch per leading layer over the
 *   items (each reads plane k - 1 of its tiles and one halo tile per side, writes plane k of its tiles and nothing else), then
 *   the layers lead .. nlayers - 1 and final_conv from plane `lead` in one launch for every row. All launches go to the hipStream_t `on_stream`
 *   (passed by the caller like any other argument: svdd_amd/_lib.call does not add it for this entry), none waits for another workgroup; the profile slot (6) records one span per call. */
int svdd_backbone_incr_f32(const uint8_t* x, const float* table0, const float* tiles, const float* vec, const float* w2,
                           float* out, int n, int L, int nlayers, const int* dilations, int lead, float* planes,
                           uint8_t* x_prev, int32_t* items, unsigned long long* stat, int first, int max_item, void* on_stream);
/* svdd_backbone_incr2_f32 (ABI 15) — svdd_backbone_incr_f32 with the segment launches dealt from a compact, size-ordered list, so
 *   that the dispatcher balances the CUs: the items of most tiles come first and every empty workgroup comes after the work.
 *   Arguments, results, planes, x_prev, stat and `first` as svdd_backbone_incr_f32. max_item is 1, 2 or 4. With S = 7 slots per
 *   (layer, row) for max_item 2 and 4, and S = 13 for max_item 1 (a row that changed everywhere has 13 one-tile items):
 *   items [lead][n][S] i32: written exactly as svdd_backbone_incr_f32 writes it (every slot rewritten each step, 0 = empty) ;
 *   order [lead][n * S] i32, order_count [lead] i32 (caller-owned, n <= 65536): order_count[k] = the non-empty items of layer k + 1,
 *   order[k][0 .. order_count[k]) = one entry row << 16 | item (item = first tile | tiles << 8) per non-empty item, SORTED BY TILE
 *   COUNT, largest first. The build is deterministic — inside a size class the entries are in (row, slot) order — but callers may
 *   rely only on the sort by size and on the multiset of entries; entries at and beyond order_count[k] are unspecified. Workgroup
 *   b of layer k's launch (grid n * S) takes order[k][b] and returns at once if b >= order_count[k]. first != 0 writes neither list.
 *   svdd_backbone_incr_set_residency(r): the most segment workgroups resident per CU from the next call on — the launch's LDS
 *   request is padded until only r fit (1 .. 8 ; 0 = no padding: what the kernel's own image and registers allow, 4 workgroups
 *   for max_item 2, 6 for max_item 1, 3 for max_item 4). Process-wide, like svdd_set_option; not a per-call argument. */
int svdd_backbone_incr2_f32(const uint8_t* x, const float* table0, const float* tiles, const float* vec, const float* w2,
                            float* out, int n, int L, int nlayers, const int* dilations, int lead, float* planes,
                            uint8_t* x_prev, int32_t* items, unsigned long long* stat, int first, int max_item,
                            int32_t* order, int32_t* order_count, void* on_stream);
/* svdd_backbone_incr3_f32 — svdd_backbone_incr2_f32 with the carried planes extended through the dilation-4 layers that follow the
 *   `lead` dilation-1 layers: planes 1 .. depth are carried, lead <= depth <= nlayers, dilations[0 .. lead) all 1 and
 *   dilations[lead .. depth) all 4 (anything else: SVDD_E_ARG; depth == lead is svdd_backbone_incr2_f32's forward). A changed
 *   position p has reached p +- (4 + sum_{i<k} 4 dilations[i]) in plane k: 8 .. 36 behind eight dilation-1 layers, 52, 68, 84, 100
 *   behind four dilation-4 layers. planes [depth][n][208][128], items [depth][n][S], order [depth][n * S], order_count [depth] ;
 *   stat (may be NULL): TWO device u64, stat[0] += the marked tile-layers of planes 1 .. lead, stat[1] += those of the deeper
 *   planes. first != 0 fills all `depth` planes; first == 0: work list, order, one segment launch per carried layer (the dilation-4
 *   layers skip exactly the (row tile, tap) pairs the one-launch kernel's schedule skips), then layers depth .. nlayers - 1 and
 *   final_conv from plane `depth`. Everything else — bits of `out`, x_prev, max_item, the lists, on_stream, the profile span,
 *   svdd_backbone_incr_set_residency — as svdd_backbone_incr2_f32. */
int svdd_backbone_incr3_f32(const uint8_t* x, const float* table0, const float* tiles, const float* vec, const float* w2,
                            float* out, int n, int L, int nlayers, const int* dilations, int lead, float* planes,
                            uint8_t* x_prev, int32_t* items, unsigned long long* stat, int first, int max_item,
                            int32_t* order, int32_t* order_count, int depth, void* on_stream);
/* svdd_backbone_incr4_f32 — svdd_backbone_incr3_f32 (the SAME BITS in `out` and in every plane) with less work in the stem.
 *   max_item is 2 (anything else: SVDD_E_ARG); S = 7 slots per (layer, row). Arguments as svdd_backbone_incr3_f32, and:
 *   x_prev2 [n][L] u8, parity: the carried tokens are a ping-pong pair. parity (0 or 1) names the buffer that holds the tokens the
 *   planes belong to, 0 = x_prev, 1 = x_prev2. first != 0 writes x into THAT buffer; first == 0 reads it and writes x into the other
 *   one, so the next call passes parity ^ 1. (The list is built in ONE launch, one workgroup per carried layer, each reading the
 *   tokens for itself: no workgroup reads what another writes.)
 *   items of layers 1 .. lead are TIGHT: entry = origin row | tiles << 8 (origin 0 .. L - 1, any value; tiles >= 1, so the word is
 *   never 0 for an item). Per (layer k, row): the rows within 4 + 4 k of a changed position form maximal runs [a, b]; a run is covered
 *   by 16-row tiles at a, a + 16, .. ; a tile that reaches the next run's first row takes that run into the same cover; tiles are
 *   disjoint, at most 13, and runs of adjacent tiles (origins 16 apart) are cut to max_item. If that needs more than 7 items (four
 *   3-tile runs cut 2 + 1 each need 8) the (layer, row) takes svdd_backbone_incr3_f32's aligned tiles, as origins 16 T. The segment
 *   launch of such a layer reads rows origin - 4 .. origin + 16 tiles + 3 of plane k - 1 and writes rows origin .. + 16 tiles - 1
 *   (< L) of plane k. items of layers lead + 1 .. depth: as svdd_backbone_incr3_f32 (first tile | tiles << 8).
 *   order / order_count: svdd_backbone_incr2_f32's contract over these items. stat[0] += the tiles cut for layers 1 .. lead (tight
 *   ones, or aligned where the fallback fired), stat[1] += those of the deeper layers. */
int svdd_backbone_incr4_f32(const uint8_t* x, const float* table0, const float* tiles, const float* vec, const float* w2,
                            float* out, int n, int L, int nlayers, const int* dilations, int lead, float* planes,
                            uint8_t* x_prev, int32_t* items, unsigned long long* stat, int first, int max_item,
                            int32_t* order, int32_t* order_count, int depth, uint8_t* x_prev2, int parity, void* on_stream);
/* svdd_backbone_incr_seed_f32 — the state a first != 0 call of the entries above leaves on n IDENTICAL rows, broadcast from ONE row's
 *   state in one launch (the prior of a decode is n all-MASK rows; what the backbone makes of that row depends on the weights alone,
 *   so a caller computes it once with a first != 0 call at n = 1 and keeps it while the weights stand).
 *   row_planes [depth][1][208][128] f32, row_logits [L][5] f32, row_x [L] u8: planes, `out` and carried tokens of that one-row call.
 *   Writes rows < L of every row of planes [depth][n][208][128] (rows >= L are never written), out [n][L][5], and the n token rows of
 *   the buffer `parity` names (0 = x_prev, 1 = x_prev2; x_prev2 may be NULL with parity 0: the entries without the pair) — the same
 *   bits as the first != 0 forward of n copies of row_x; like that forward it writes neither the other token buffer nor a list nor
 *   stat, and the next call passes the same parity. 104 < L <= 208, 1 <= depth <= 32, row_planes and planes 16-byte aligned. The
 *   launch goes to `on_stream` (passed by the caller, as for the entries above); profile slot 6 records it as one span. */
int svdd_backbone_incr_seed_f32(const float* row_planes, const float* row_logits, const uint8_t* row_x, int n, int L, int depth,
                                float* planes, float* out, uint8_t* x_prev, uint8_t* x_prev2, int parity, void* on_stream);
int svdd_backbone_incr_set_residency(int wg_per_cu);
/* svdd_backbone_set_workspace — caller-owned scratch for the small-batch form of svdd_backbone_cnn_f32 (several workgroups per
 * sequence exchange the LayerNorm'd image of every layer through it): ws = device memory of `bytes` >= n_max * (2 * 208 * 128 * 4
 * + 4) + 4 bytes for batches of up to n_max sequences (n_max = 128 covers every case the split is used for); NULL: none (one
 * workgroup per sequence at every batch size). Launches that use it must not overlap. svdd_backbone_split_status: *err = 1 if a
 * group barrier ever timed out (never in a correct launch: the launcher only splits when every workgroup is resident). */
int svdd_backbone_set_workspace(void* ws, long long bytes);
int svdd_backbone_split_status(int* err);

/* ------------------------------------------------------------------------------------------------
 * Split-precision net kernels (svdd_amd/csrc/svdd_lp_*.hip) — the same functions as the *_f32 net kernels above
 * with the matrix products on the 16-bit matrix cores (fp32 accumulate). An explicit opt-in of the caller
 * (Diffusion.precision); the exact-fp32 kernels remain the default and the parity reference.
 *   SVDD_PREC_F16X3 / BF16X3: fp32 operands split hi + lo on the fly, a*b = ahi*bhi + ahi*blo + alo*bhi (3 MFMAs):
 *     f16x3 is fp32-class (a 22-bit operand: 1.5e-7 of sum|a b| at K = 1152 vs 1.8e-7 for the fp32 MFMA chain); bf16x3 is NOT — its
 *     operand keeps 16 bits (5.3e-7 of sum|a b| per product, backbone logits 4.5e-5 from an fp64 forward: 10 x fp32's 4.5e-6);
 *   SVDD_PREC_F16 / BF16: one pass on the 16-bit roundings of the operands (~3e-5 / ~3e-4 of sum|a b|).
 * Everything that is not a matrix product stays fp32. */
enum { SVDD_PREC_F32 = 0, SVDD_PREC_F16X3 = 1, SVDD_PREC_BF16X3 = 2, SVDD_PREC_F16 = 3, SVDD_PREC_BF16 = 4 };

/* svdd_backbone_cnn_lp — svdd_backbone_cnn_f32 on the 16-bit matrix cores. x, table0, vec, w2, out, dilations as
 *   there. tiles: [nlayers*36 + 4] weight tiles in the order (layer, chunk, tap) then the 4 chunks of W_f1, each
 *   [4 cg][64 lanes][2 ct][P][8] 16-bit values, P = 2 (hi, lo) for the x3 modes and 1 otherwise: lane (j = lane & 15,
 *   g = lane >> 4) of column group cg holds s_w * W[32 cg + 2 j + ct][32 c + 8 g + e][t], e = 0..7.
 *   lscale [nlayers + 1][2] = {sa, 1 / (sa * s_w)}: power-of-two scales of the activations / weights of each stage
 *   (1 for bf16).  Packing: svdd_amd/fused.py:pack_backbone_lp. */
int svdd_backbone_cnn_lp(const uint8_t* x, const float* table0, const void* tiles, const float* vec,
                         const float* lscale, const float* w2, float* out, int n, int L, int nlayers,
                         const int* dilations, int prec, const int32_t* count, const int32_t* row_idx, int out_scatter,
                         void* stream);

/* svdd_conv_tower_lp / svdd_conv_tower_windows_lp — svdd_conv_tower_f32 / svdd_conv_tower_windows_f32 on the 16-bit
 *   matrix cores. The input is the TOKEN tensor (u8, 4 = MASK -> zero one-hot row; reference transform_samples,
 *   diffusion_gosai.py:1462-1470), not the fp32 one-hot: tok [n,L] (windows: the candidates [B,M,L] flattened).
 *   tiles: [2 + 10*nlayers] weight tiles in execution order (stem chunks 0,1 with k = 4*tap + channel, then per layer,
 *   per 32-channel chunk, per tap), each [2 cp][64 lanes][2 ct][P][8] 16-bit: lane (j, g) of column pair cp holds
 *   s_w * W[32 cp + 2 j + ct][8 g + e]; inv [1 + nlayers] = 1 / s_w of each stage; bias as in the fp32 kernel.
 *   out (and parent_out): [n, L, P, 64] 16-bit planes — per row the hi halves of the 64 channels, then (x3 modes) the
 *   lo halves: the form svdd_gru_bidir_lp consumes directly (value = hi + lo).
 *   windows: live_idx [count] (may be NULL = identity) lists the candidates to process, `count` (device scalar, may be
 *   NULL = n) how many — workgroup i handles candidate live_idx[i] and writes rows [i*L, (i+1)*L) of `out`, so a
 *   compacted batch needs no host round trip (exact work-skipping). Packing: svdd_amd/fused.py:pack_tower_lp. */
int svdd_conv_tower_lp(const uint8_t* tok, const void* tiles, const float* bias, const float* inv, void* out,
                       int n, int L, int nlayers, int residual_mask, const int32_t* count, int prec, void* stream);
int svdd_conv_tower_windows_lp(const uint8_t* cand, const void* tiles, const float* bias, const float* inv,
                               const int32_t* win, const void* parent_out, void* out, int n, int L, int M,
                               int nlayers, int residual_mask, const int32_t* live_idx, const int32_t* count,
                               int prec, void* stream);

/* svdd_gru_bidir_lp — svdd_gru_bidir_f32 on the 16-bit matrix cores. wpack [2 dirs][4 waves][64 lanes][6][2][P][8]
 *   16-bit: lane (j, g) of wave w holds s_w * W_m[16 w + j][32 c + 8 g + e] for m = ir, hr, iz, hz, in, hn and chunk
 *   c = 0, 1; bpack as in the fp32 kernel; inv [2] = 1 / s_w per direction. `count` (device scalar, may be NULL = n):
 *   number of valid sequences. The input is EITHER x [n,L,64] fp32 (split into hi / lo by the kernel) OR x16
 *   [n,L,P,64] 16-bit planes (hi, lo) as the split-precision tower writes them (then x is ignored).
 *   Packing: svdd_amd/fused.py:pack_gru_lp. */
int svdd_gru_bidir_lp(const float* x, const void* x16, const void* wpack, const float* bpack, const float* inv,
                      float* out, int n, int L, const int32_t* count, int prec, void* stream);

/* svdd_value_tail_lp — svdd_value_tail_f32 with the 64 -> 128 map on the 16-bit matrix cores. w1pack [64 lanes][8 ct][2 c]
 *   [P][8] 16-bit: s_w * W1'[16 ct + j][32 c + 8 g + e]; inv = 1 / s_w; the rest as in the fp32 kernel. `count` as above.
 *   Packing: svdd_amd/fused.py:pack_tail_lp. */
int svdd_value_tail_lp(const float* h_fwd, const float* h_bwd, const void* w1pack, const float* b1,
                       const float* w_eff, const float* b_eff, float inv, float* out, int n, int L, int n_tasks,
                       const int32_t* count, int prec, void* stream);

/* Process-wide options (host). SVDD_OPT_FORCE_EXACT != 0 makes svdd_propose evaluate every draw in the
 * exact (fp64, correctly rounded) arithmetic instead of the filtered fast path — same results, used
 * to A/B the filter. */
enum { SVDD_OPT_FORCE_EXACT = 0,
       SVDD_OPT_MSPLIT = 1 /* tuning: waves per 64-position tile in svdd_propose, 0 = auto */,
       SVDD_OPT_SELECT_ONE_ROW = 2 /* A/B: 1 = svdd_select as one wave per row for every M (default 0: several rows per wave for M <= 64,
                                      4 row groups per wave from 2^21 (row, candidate) slots on); 2 / 3 = force 4 / 1 row groups per wave */,
       SVDD_OPT_BACKBONE_LP_VERSION = 3 /* A/B: 1 = svdd_backbone_cnn_lp runs the round-2 kernel for every shape; 2 (default) = the
                                            transposed-accumulator kernel where one sequence fills a tile (104 < L <= 208);
                                            21 / 22 (= 2) / 23: that kernel with one / two / three waves per SIMD (same bits) */,
       SVDD_OPT_TRUNK_GEMM_VERSION = 4 /* A/B: svdd_trunk_gemm kernel: 1 = 128 x 128 tiles everywhere, 2 (default) = 256 x 256 LDS-DMA
                                           tiles from 128 tiles up, 3 = 256 x 256 everywhere (13 .. 16: timing experiments with
                                           wrong results: no epilogue / one K block / no DMA / no fragment reads); 40 / 41 / 42: the
                                           LDS-DMA kernel's tile height by cost (default) / 256 rows / 192 rows; 51 .. 54: how many
                                           chains of GEMMs share the chip (the cost model prices a launch against CUs / that) */,
       SVDD_OPT_CAND_ROW_STRIDE = 5 /* layout experiment (round 4): bytes between two candidate rows of `cand` as svdd_select /
                                        svdd_select_compact read it (0 = L, the default): rows padded to whole 128-byte lines. The library cannot
                                        check the caller's padding: a non-zero value is refused (SVDD_E_ARG) unless the process has
                                        SVDD_EXPERIMENTS set in its environment */,
       SVDD_OPT_TRUNK_PLANES_F32 = 6 /* the svdd_trunk_* entry points take ONE fp32 operand plane (the *_hi pointers are float*, the
                                         *_lo pointers NULL) and svdd_trunk_gemm multiplies on v_mfma_f32_16x16x4_f32: the Enformer-shaped
                                         trunk at the reference's precision (weights packed by fused_trunk.pack_gemm_weight_f32) */,
       SVDD_OPT_SELECT_BATCHES = 8 /* A/B (round 6): batches of row groups a wave of a SATURATED svdd_select launch (>= 2^21 (row, candidate)
                                      slots, M = 10 / 20) takes: 0 / 1 = one (default), 2 / 4 = the next batch decided under the row
                                      gathers of the one before — measured slower, kept for the record */,
       SVDD_OPT_BACKBONE_SPLIT = 7 /* svdd_backbone_cnn_f32 on several workgroups per sequence (small batches; same bits): 0 = automatic
                                       (4 workgroups per sequence while 4 n <= CUs, 2 while 2 n <= CUs; needs
                                       svdd_backbone_set_workspace), 1 = never, 2 / 4 = that many wherever n R <= CUs */ };
int svdd_set_option(int key, int value);

/* Soak / profiling aid: while `device_counters2` (two zero-initialised uint64 on the device) is non-NULL, every
 * svdd_propose / svdd_sample_categorical launch adds {draws at masked positions, draws the exact-arithmetic filter
 * could not decide on the fast path} to it. NULL switches the counting off. */
int svdd_k1_stats(unsigned long long* device_counters2);

/* Per-launch kernel timing (host). While enabled, svdd_propose (kernel 0), svdd_select (1), svdd_conv1d_cl_f32 (2),
 * svdd_gru_bidir_f32 (3), svdd_epilogue_ln_f32 (4), svdd_conv_tower_f32 (5), svdd_backbone_cnn_f32 / _save_f32 / svdd_backbone_incr_f32 (6; the latter as one span over its launches), svdd_value_tail_f32 (7), svdd_tds_resample (8), svdd_mt19937_uniform_f32 (9), svdd_backbone_cnn_grad_f32 (10), svdd_gru_bidir_train[2]_f32 (11) and svdd_gru_bidir_bwd[2]_f32 (12; the *2 forms as one span over their two launches) are dispatched (the reward net's DPS kernels share slots: svdd_reward_stem*_f32 5, svdd_reward_tail_grad_f32 7, svdd_conv1d_cl_gated_f32 2)
 * with HIP start/stop events bound to the dispatch on its launch stream
 * (hipExtLaunchKernelGGL); svdd_profile_collect waits for the recorded launches, returns the summed
 * hipEventElapsedTime and their count, and clears the record. Not for use during graph capture. */
int svdd_profile_enable(int on);
int svdd_profile_collect(int kernel, double* total_ms, int* launches);

/* Self-test of the fast-math error bounds the K1 filter relies on (host; synchronous; allocates).
 * out3[0] = max relative error of the fast Gumbel-norm g over ALL 2^24 possible uniforms,
 * out3[1] = max relative error of the fast exp over 2^24 points of [-80,0],
 * out3[2] = max relative error of the fast log over 2^24 points of (1,4]. */
int svdd_selftest_fastmath(double* out3);

/* Library / device probe (host). Returns SVDD_OK and fills arch (e.g. "gfx950") and CU count. */
int svdd_device_info(char* arch, int arch_len, int* num_cu);

/* ABI version of this header: bumped on any signature change. */
int svdd_abi_version(void);
#define SVDD_ABI_VERSION 17

/*
 * Enformer-shaped value trunk (BASELINE.json configs[3]; reference decode.py:78-80, Enformer.py:1271-1334 trunk, :1807-1884
 * conv tower, :1887-2007 transformer tower, :2176-2292 ConvBlock "NACDR") on the 16-bit matrix cores, split precision
 * bf16x3 (a_lo != NULL) or one-pass bf16 (a_lo == NULL). csrc/svdd_trunk.hip. Activations are channels-last rows
 * [n * rows_per_seq, C]; for the k = 5 convolutions rows_per_seq = L + 2 (two zero rows behind every sequence, two guard rows in
 * front of the first), so that a tap is a row shift of a plain GEMM. count (may be NULL): device scalar, number of live sequences of a compacted batch.
 *
 * svdd_trunk_gemm        out[M, N] = act(sum_{t < T} A[rows + t - T/2, Cin] W_t[Cin, N] + bias) (+ resid), fp32 [M, ldo].
 *                        a_hi / a_lo: bf16 operand planes [>= M + 128 + T rows, lda] with T/2 readable rows before row 0;
 *                        lda % 8 == 0 (fp32 planes: lda % 4 == 0) and ldo % 4 == 0: rows are moved in 16-byte pieces;
 *                        w: bf16 weight fragments packed by svdd_amd.fused_trunk.pack_gemm_weight ; N % 128 == 0, Cin % 32 == 0,
 *                        T odd ; act 0 none, 1 relu, 2 x * sigmoid(1.702 x).
 *                        Fused second output (out_hi != NULL; out may then be NULL): the operand planes of the NEXT GEMM,
 *                        post_act(post_scale[c] y + post_shift[c]) -> (out_hi, out_lo) [M, N] (scale / shift NULL: identity), zero in
 *                        the last `pad` rows of every sequence (row stride N, whatever ldo is) — what svdd_trunk_act_split would write from `out`. The
 *                        output planes must not be the input planes. Two kernels behind it (SVDD_OPT_TRUNK_GEMM_VERSION).
 * svdd_trunk_act_split   x fp32 [rows, C] -> act(scale[c] x + shift[c]) (scale / shift NULL: identity) -> planes hi (lo may be
 *                        NULL) ; the last `pad` rows of every sequence are written as zeros.
 * svdd_trunk_layernorm_split   LayerNorm(x[row, :C]) gamma + beta -> planes (C % 8 == 0, C <= 4096).
 * svdd_trunk_attn_pool   softmax-weighted pooling over position pairs: x, logits fp32 [n, L + 2, C] -> out [n, ceil(L/2) + 2, C]
 *                        (may be NULL) and / or the next GEMM's operand planes post_act(post_scale o + post_shift), pad rows zeroed.
 * svdd_trunk_attn_small  relative-position attention on T <= 4 tokens per sequence (what the conv tower leaves of L <= 512): qkv fp32
 *                        [n T, heads (2 dk + dv)] = [q | k | v], rel_k [heads, 2 T - 1, dk] (positional keys), content / pos bias
 *                        [heads, dk] -> softmax(((q s + cb) k^T + shift((q s + pb) rel_k^T))) v as (hi, lo) planes [n T, heads dv].
 * svdd_trunk_stem_unfold tokens [n, L] u8 -> hi plane [n (L + 2), 64]: channel 4 t + token of position l + t - 7 (t < 15) set to 1.
 *
 * First level shared between a candidate and its parent (exact; the SVDD-MC step of reference diffusion_gosai.py:1203-1209 scores
 * M candidates that differ from x_t at a few positions, and the stem, the 1 x 1 block and the pooling of the first level are
 * functions of a 15-token window): only the rows of up to `slots` (<= 4) even-aligned windows per candidate go through the
 * level's GEMMs, as compact rows without pads; the rest of the level's output planes are copies of the parent's.
 * The next levels go the same way while their lengths are even: level d + 1 can differ in rows [w0/2 - 2, w1/2 + 2) (k = 5
 * convolution); a level d >= 1 works on compact segments of window + 2 rows of context on each side.
 * svdd_trunk_windows         candidate c (cand [n, L] u8, L <= 256) vs row parent_idx[c] / div of parent [., L]: for the `depth`
 *                            shared levels (L % 2^(depth - 1) == 0: only the last may have an odd length) and window slot j: w0[(d n + c) slots + j], wlen[.] = the even-aligned
 *                            windows of level d in ascending order (level 0: one per position that differs, +- halo, windows that
 *                            touch merged, the last slot takes what is left; deeper: windows within 4 rows merged; wlen 0: unused
 *                            slot, and for c >= count), seg[.] = its compact rows (wlen, + 4 context rows for d >= 1).
 *                            Every one of the depth x n x slots entries of the three tables is written: the used slots come first, an
 *                            unused slot has w0 = wlen = seg = 0, and so has every slot of a candidate c >= count. Two windows of a
 *                            level >= 1 are MORE than 4 rows apart, so their segments (window + 2 context rows on each side) never
 *                            overlap; level-0 windows do not touch. The window rows of a candidate and level add up to <= its length.
 * svdd_trunk_stem_unfold_win the stem operand of the window rows: the r-th window row of candidate c at compact row off[c slots] + r
 *                            (off = exclusive prefix sum of seg over [n slots]).
 * svdd_trunk_attn_pool_win   x, logits fp32 (compact rows of a level of length L; the segment of slot s starts at off[s], its window
 *                            in_halo rows further) -> the next GEMM's operand planes: pooled window rows where a window covers the
 *                            pair, else the row of the parent's planes [., L/2 + 2, C] (zeros outside the sequence). v0 == NULL:
 *                            whole sequences [n, L/2 + 2, C], pad rows zero; else the compact segments of the next level: rows
 *                            v0[s] - 2 .. v0[s] + vlen[s] + 1 at off2[s] (an even L only). Of x / logits only window rows are ever read:
 *                            never a segment's context rows, never a row between two segments. Candidates c >= count write nothing.
 */
int svdd_trunk_gemm(const void* a_hi, const void* a_lo, const void* w, const float* bias, const float* resid, float* out,
                    int M, int N, int Cin, int T, int lda, int ldo, int act, const int32_t* count, int rows_per_seq,
                    void* out_hi, void* out_lo, const float* post_scale, const float* post_shift, int post_act, int pad,
                    void* stream);
int svdd_trunk_act_split(const float* x, const float* scale, const float* shift, int act, int64_t rows, int C,
                         int rows_per_seq, int pad, void* hi, void* lo, const int32_t* count, void* stream);
int svdd_trunk_layernorm_split(const float* x, const float* gamma, const float* beta, float eps, int64_t rows, int C,
                               void* hi, void* lo, const int32_t* count, int rows_per_seq, void* stream);
int svdd_trunk_attn_pool(const float* x, const float* logits, int n, int L, int C, float* out, const int32_t* count,
                         void* out_hi, void* out_lo, const float* post_scale, const float* post_shift, int post_act, void* stream);
int svdd_trunk_attn_small(const float* qkv, const float* rel_k, const float* content_bias, const float* pos_bias, int n, int T,
                          int heads, int dk, int dv, void* hi, void* lo, const int32_t* count, void* stream);
int svdd_trunk_stem_unfold(const uint8_t* tok, int n, int L, void* hi, const int32_t* count, void* stream);
int svdd_trunk_windows(const uint8_t* cand, const uint8_t* parent, const int32_t* parent_idx, int div, int n, int L, int halo,
                       int depth, int slots, const int32_t* count, int32_t* w0, int32_t* wlen, int32_t* seg, void* stream);
int svdd_trunk_stem_unfold_win(const uint8_t* tok, int n, int L, int slots, const int32_t* w0, const int32_t* wlen,
                               const int32_t* off, void* hi, const int32_t* count, void* stream);
int svdd_trunk_attn_pool_win(const float* x, const float* logits, int n, int L, int C, int in_halo, int slots, const int32_t* w0,
                             const int32_t* wlen, const int32_t* off, const int32_t* parent_idx, int div, const void* parent_hi,
                             const void* parent_lo, const int32_t* count, void* out_hi, void* out_lo, const float* post_scale,
                             const float* post_shift, int post_act, const int32_t* v0, const int32_t* vlen, const int32_t* off2,
                             void* stream);

/* --------------------------------------------------------------------------------------------------------------------------
 * DPS (gradient guidance, BASELINE configs[4]) without autograd — ABI 11. The reference's step (diffusion_gosai.py:1286-1330):
 *   x_grad = d mean(reward(softmax(E)[:, 0:4])) / d onehot(x_t),  E = keep onehot(x_t) + (1 - keep) log p(x0 | x_t)      (:1321-1330)
 *   q_xs   = exp(log p) (mct - mcs), q_xs[MASK] = mcs, times exp(scale (x_grad - x_grad[MASK]))                        (:1306-1314)
 * Per-position pieces (logits = the one-launch backbone's raw output [B][L][5] contiguous, x = tokens u8 [B][L]):
 *   svdd_dps_probs       -> probs4 [B][L][4] = softmax(E)[..., 0:4], the reward net's input
 *   svdd_dps_probs_bwd   dprobs4 [B][L][4] -> dlogits [B][L][5] (input of svdd_backbone_cnn_grad_f32; zero at unmasked positions) and
 *                        direct [B][L][5] = keep dE (the term through `keep * x_onehot`; zero at masked positions)
 *   svdd_dps_guided_q    grad_backbone + grad_direct = x_grad -> the guided q_xs [B][L][5]
 * The reward net's gradient pass (ConvGRUTrunk + ConvHead, Enformer.py:1411-1426, 2166-2173; eval-mode BatchNorm folded):
 *   svdd_reward_stem_f32 / _bwd_f32   the 4 -> 64 x 15-tap stem on REAL-valued rows x [n][L][4] (w as [15][4][64]): relu(conv + b) /
 *                                     its transpose applied to the gradient at the stem's pre-activation
 *   svdd_conv1d_cl_f32 (act = 1)      a tower layer forwards: relu(conv + b + f_prev)
 *   svdd_conv1d_cl_gated_f32          a tower layer backwards: gate > 0 ? conv^T(g) + f_prev : 0 (wpack = flipped, transposed taps)
 *   svdd_gru_bidir_train_f32 / _bwd_f32   the GRU (above)
 *   svdd_reward_tail_grad_f32         h_fwd, h_bwd [n][L][64] -> d mean_n(mean_l(score)) / d (h_fwd + h_bwd), written to g_fwd AND g_bwd
 *                                     (w1 [128][64], b1 [128]: dense1; gamma / beta [64]: its LayerNorm; w_eff [128]: dense2 and the
 *                                     head collapsed, task 0)
 *   svdd_sum_gate_f32                 g = f > 0 ? a + b : 0 over `count` floats (count % 4 == 0)
 * All: caller-owned device buffers, launched on `stream`, no allocation, no synchronisation. */
int svdd_dps_probs(const float* logits, const uint8_t* x, int B, int L, float* probs4, void* stream);
int svdd_dps_probs_bwd(const float* logits, const uint8_t* x, const float* dprobs4, int B, int L, float* dlogits, float* direct,
                       void* stream);
int svdd_dps_guided_q(const float* logits, const uint8_t* x, const float* grad_backbone, const float* grad_direct, float dm, float mcs,
                      float scale, int B, int L, float* q, void* stream);
int svdd_reward_stem_f32(const float* x, const float* w, const float* b, float* out, int n, int L, int taps, void* stream);
int svdd_reward_stem_bwd_f32(const float* g, const float* w, float* dx, int n, int L, int taps, void* stream);
int svdd_conv1d_cl_gated_f32(const float* x, const float* wpack, float* y, int n, int L, int cin, int cout, int taps, int dilation,
                             const float* f_prev, const float* gate, void* stream);
int svdd_reward_tail_grad_f32(const float* h_fwd, const float* h_bwd, const float* w1, const float* b1, const float* gamma,
                              const float* beta, const float* w_eff, float eps, int n, int L, float* g_fwd, float* g_bwd, void* stream);
int svdd_sum_gate_f32(const float* a, const float* b, const float* f, float* g, int64_t count, void* stream);
/* The GRU pair with the non-recurrent halves off the serial chain (at the DPS batch the chains are latency: 32 workgroups, 200 dependent
 * steps). Same results as svdd_gru_bidir_train_f32 (out / save: same bits) and as dx_fwd + dx_bwd of svdd_gru_bidir_bwd_f32 (to rounding:
 * the two directions accumulate in one chain):
 *   svdd_gru_bidir_train2_f32: gi = caller scratch [2][n L][192] fp32 (receives b + W_i x of every step: one launch on the whole chip),
 *                              then the chain with W_h h only; out [2][n][L][64], save [2][n][L][4][64] as above.
 *                              A row of gi is [r | z | n] x 64 with every bias outside the r-product folded in:
 *                              b_ir + b_hr + W_ir x | b_iz + b_hz + W_iz x | b_in + W_in x (b_hn stays with W_hn h, save plane 3).
 *   svdd_gru_bidir_bwd2_f32:   da = caller scratch [2][n L][192] (receives the gate derivatives: a row is [da_r | da_z | da_n] x 64 of
 *                              one (sequence, step), rows in (n, L) order for both directions; every row is written), then
 *                              g [n][L][64] = gate > 0 ? da_fwd W_i,fwd + da_bwd W_i,bwd : 0 (gate [n][L][64] or NULL: no gate).
 * Aliasing: f_prev of svdd_conv1d_cl_gated_f32 may be x itself (same bits as a separate copy); gi and da may be one buffer across the
 * two calls; every output is otherwise a buffer of its own. A shut gate (gate <= 0, either zero included) stores +0.0. */
int svdd_gru_bidir_train2_f32(const float* x, const float* wpack, const float* bpack, float* gi, float* out, float* save, int n, int L,
                              void* stream);
int svdd_gru_bidir_bwd2_f32(const float* grad_out, const float* out, const float* save, const float* wpack_bwd, float* da, const float* gate,
                            float* g, int n, int L, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVDD_HIP_H */
