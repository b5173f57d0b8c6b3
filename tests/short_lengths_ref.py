"""What tests/test_short_lengths_cpu.py and tests/test_short_lengths_gpu.py share: the lengths and the forced sequences-per-tile
values at which the kernels that put SEVERAL sequences into one 208-row workgroup tile (L <= 104) are pinned, the schedule rule of
the interleaved backbone kernel, and csrc/svdd_spt.h restated in numpy. Nothing here touches a device.

backbone_kernel<false> interleaves the s sequences of a tile position-major: the tile behaves like ONE sequence of R = s L rows
whose dilations are multiplied by s. What the kernel distinguishes is therefore a function of (L, s): nt = ceil(R / 16) row tiles
(entry bodies of 2 / 4 / 7 slots at nt <= 4 / <= 8 / more, nro = the slots a wave half owns, other for odd nt), R mod 16 (padding rows
in the last row tile), which taps are dead (k dil >= L) and which (row tile, tap) pairs are alive for a single row. A forced s = 1
(and every host-side plan of one sequence per tile) runs the one-sequence form backbone_kernel<true>, where nt, body and nro are
constants: it is the reference the other packings are held to, not a case of the shared-tile kernel. The kernel meets tiles of ONE
sequence (il = 1, nt = ceil(L / 16) <= 7) where the workgroups plan from a device-side count of at most one round of rows
(small_count / small_spt) and in the remainder of a two-size plan. shared_pairs() = the forced s > 1 and that launch reaches every
class; tests/test_short_lengths_cpu.py proves it, so a later edit of the list cannot lose one unnoticed."""
import numpy as np

from tests.lengths_ref import DIL

TILE_ROWS = 208                                             # TW_ROWS: a backbone / tower workgroup tile
CONV_TILE_ROWS = 224                                        # conv1d_cl_kernel's tile
DILS = tuple(sorted(set(DIL)))                              # 1, 4, 16, 64
SHORT_LENS = [1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 15, 16, 17, 20, 23, 26, 27, 29, 30, 32, 33, 34, 35, 37, 41, 42, 43, 48, 49, 50, 52, 53, 63,
              64, 65, 69, 70, 80, 81, 96, 97, 103, 104]
DEAD_TAP_THRESHOLDS = (1, 2, 3, 4, 8, 12, 16, 32, 48, 64)   # k dil <= 104 for k = 1 .. 4 and the dilations 1, 4, 16, 64
SMAX_CHANGES = (104, 69, 70, 52, 53, 41, 42, 34, 35, 29, 30, 26, 27)
TWO_SIZE_LENS = (104, 69, 33)                               # 208 // L = 2, 3, 6
TOWER_MASK_LENS = (104, 50, 33)
# the generic convolution's tile holds 224 rows: the lengths of SHORT_LENS on either side of a change of 224 // L or of a dead-tap
# threshold, 112 | 113 (two sequences per tile | one), and — SHORT_LENS follows the 208-row tile — 28 (eight per tile) and both sides of
# 44 | 45, 56 | 57, 74 | 75 (five | four, four | three, three | two)
CONV_LENS = [L for L in SHORT_LENS if CONV_TILE_ROWS // L != CONV_TILE_ROWS // (L + 1) or (L > 1 and CONV_TILE_ROWS // (L - 1) != CONV_TILE_ROWS // L)
             or L in DEAD_TAP_THRESHOLDS or L - 1 in DEAD_TAP_THRESHOLDS] + [112, 113] + [28, 44, 45, 56, 57, 74, 75]


def packs(L):
    """The forced sequences-per-tile values of length L: 1, 2, 3, 4, smax - 1, smax inside [1, smax], smax = 208 // L."""
    smax = TILE_ROWS // L
    return sorted({s for s in (1, 2, 3, 4, smax - 1, smax) if 1 <= s <= smax})


def pairs(lens=None):
    return [(L, s) for L in (SHORT_LENS if lens is None else lens) for s in packs(L)]


def batch_sizes(s):
    """n of the forced-s launches: two full tiles and a tile with one sequence; for s >= 3 also a last tile that lacks exactly one."""
    return [2 * s + 1] + ([2 * s - 1] if s >= 3 else [])


# ------------------------------------------------------------------------------------------------------------- the schedule
def row_tiles(L, s):
    return (s * L + 15) // 16


def live_rows(L, s, T, tap, dil):
    """Rows of row tile T that tap `tap` of a dilation-dil layer maps inside the tile of s interleaved sequences (the schedule's
    lo / hi with d = (t - 4) dil s in tile rows)."""
    R, d = s * L, (tap - 4) * dil * s
    lo, hi = (-d if d < 0 else 0), (R - d if d > 0 else R)
    if lo >= hi:
        return 0
    return max(0, min(hi, 16 * T + 16) - max(lo, 16 * T))


def one_row_pairs(L, s, dil):
    """[(row tile, tap)] that backbone_kernel<false>'s schedule keeps for exactly one row at s sequences of length L per tile."""
    return [(T, t) for T in range(TILE_ROWS // 16) for t in range(9) if live_rows(L, s, T, t, dil) == 1]


def one_row_sides(L, s, dil):
    """{(side, tap distance)} of the one-row pairs: "hi" = the tap's LAST live row is the first row of its row tile (hi = 16 T + 1),
    "lo" = a negative tap's FIRST live row is the last row of its row tile (lo = 16 T + 15)."""
    R, out = s * L, set()
    for T, t in one_row_pairs(L, s, dil):
        d = (t - 4) * dil * s
        lo, hi = (-d if d < 0 else 0), (R - d if d > 0 else R)
        if hi == 16 * T + 1:
            out.add(("hi", abs(t - 4)))
        if lo == 16 * T + 15:
            out.add(("lo", abs(t - 4)))
    return out


def live_distances(dil, lmax=104):
    """Tap distances k = |t - 4| of a dilation-dil layer that are alive at some L <= lmax (k dil < L)."""
    return [k for k in range(5) if k * dil < lmax]


def entry_body(nt):
    return 2 if nt <= 4 else 4 if nt <= 8 else 7


def owned_slots(nt, rh):
    """nro: the row tiles rh, rh + 2, .. < nt of wave half rh."""
    return len(range(rh, nt, 2))


# -------------------------------------------------------------------------------------------- csrc/svdd_spt.h, restated
def tile_cost(rt, fixed_half):
    return 2 * rt + (6 if fixed_half == 9 and 4 < rt <= 8 else fixed_half)


def choose_spt(n, L, ncu, fixed_half):
    s = np.arange(TILE_ROWS // L, 0, -1, dtype=np.int64)                    # ties: the fuller tile
    tiles = (n + s - 1) // s
    rt = (s * L + 15) // 16
    cost = ((tiles + ncu - 1) // ncu) * (2 * rt + np.where((fixed_half == 9) & (rt > 4) & (rt <= 8), 6, fixed_half))
    return int(s[np.argmin(cost)])                                          # argmin: the first of equal costs


def _single_cost(n, s, L, ncu, fixed_half):
    tiles = (n + s - 1) // s
    return ((tiles + ncu - 1) // ncu) * tile_cost((s * L + 15) // 16, fixed_half)


def plan_tiles(n, L, ncu, fixed_half):
    """-> (s1, n1, s2): tiles 0 .. n1 - 1 take s1 sequences each, the tiles after them s2."""
    smax = TILE_ROWS // L
    best = (smax, 0, choose_spt(n, L, ncu, fixed_half))
    best_cost = _single_cost(n, best[2], L, ncu, fixed_half)
    for s1 in range(smax, 0, -1):
        c1 = tile_cost((s1 * L + 15) // 16, fixed_half)
        per_round = s1 * ncu
        for k in range(1, n // per_round + 1):
            r = n - k * per_round
            if r == 0:
                if k * c1 < best_cost:
                    best_cost, best = k * c1, (s1, k * ncu, s1)
                continue
            for s2 in range(smax, 0, -1):
                cost = k * c1 + _single_cost(r, s2, L, ncu, fixed_half)
                if cost < best_cost:
                    best_cost, best = cost, (s1, k * ncu, s2)
    return best


def plan_num_tiles(plan, n):
    s1, n1, s2 = plan
    rest = n - n1 * s1
    return n1 + ((rest + s2 - 1) // s2 if rest > 0 else 0)


def plan_tile(plan, t):
    """(first sequence, sequences) of tile t."""
    s1, n1, s2 = plan
    return (t * s1, s1) if t < n1 else (n1 * s1 + (t - n1) * s2, s2)


def two_size_batch(L, ncu, fixed_half=9, limit=4096):
    """The smallest n whose plan mixes two tile sizes (n1 > 0, s1 != s2) with a ragged last tile if there is one below `limit`,
    else the smallest that mixes two sizes; None if there is none."""
    first = None
    for n in range(ncu + 1, limit):
        s1, n1, s2 = plan_tiles(n, L, ncu, fixed_half)
        if n1 > 0 and s1 != s2:
            first = n if first is None else first
            if (n - n1 * s1) % s2:
                return n
    return first


def ragged_count(L, ncu, fixed_half=9):
    """The smallest live-row count k > ncu at which the plan's last tile takes more than one sequence and is ragged, and the always-full
    packing's last tile is ragged too; None if there is none near ncu."""
    smax = TILE_ROWS // L
    for k in range(ncu + 1, ncu + 200):
        s1, n1, s2 = plan_tiles(k, L, ncu, fixed_half)
        rest = k - n1 * s1
        if rest > 0 and s2 > 1 and rest % s2 and k % smax:
            return k
    return None


def small_count(L, ncu):
    """A device-side row count of at most ncu rows: what a work-skipping launch with few live rows hands the kernel."""
    return min(2 * (TILE_ROWS // L), ncu - 1)


def small_spt(L, ncu, fixed_half=9):
    """The sequences per tile the workgroups plan for small_count(L, ncu) rows. Any k <= ncu is one round whatever the tile size, so
    the cheapest tile wins, ties to the fuller: ONE sequence per tile from L = 9 up (nt = ceil(L / 16) <= 7, il = 1), the most that fit
    one row tile below. Such a launch runs backbone_kernel<false>; svdd_set_backbone_packing(-1) and a host-side plan of one sequence
    per tile run the one-sequence form backbone_kernel<true> instead, whose nt, entry body and owned slots are constants."""
    s1, n1, s2 = plan_tiles(small_count(L, ncu), L, ncu, fixed_half)
    assert n1 == 0
    return s2


def shared_pairs(ncu=256, lens=None):
    """The (L, s) at which tests/test_short_lengths_gpu.py runs backbone_kernel<false>: the forced packings s > 1 and the tile size
    of the small device-side count."""
    lens = SHORT_LENS if lens is None else lens
    return sorted({(L, s) for L, s in pairs(lens) if s > 1} | {(L, small_spt(L, ncu)) for L in lens})
