"""No GPU: conditions on the INPUTS of tests/test_short_lengths_gpu.py — that SHORT_LENS with packs() (tests/short_lengths_ref.py)
reaches every class the shared-tile kernels (L <= 104, several sequences per 208-row workgroup tile) distinguish — and the numpy
restatement of csrc/svdd_spt.h held to the header itself, compiled on the host. Only the (L, s) that really run backbone_kernel<false>
count (short_lengths_ref.shared_pairs): the forced packings s > 1, and the tile size the workgroups plan from a small device-side
count (one sequence per tile from L = 9 up). A forced s = 1 runs the one-sequence form and counts for nothing here.
  * nt = ceil(s L / 16) takes every value 1 .. 13: the 2-, 4- and 7-slot entry bodies on both sides of their limits and both
    parities of nt (nro of the two wave halves differs for odd nt);
  * s L mod 16 takes every residue, 0 (no padding row in the last row tile) and 1 (one live row) among them;
  * for each dilation of config.dna_config() and each tap distance that can be alive at L <= 104 some (L, s) has a (row tile, tap)
    pair that the schedule keeps for exactly ONE row;
  * both sides of every dead-tap threshold (L = k dil: the tap is dead; L = k dil + 1: alive for one position);
  * both sides of the changes of 208 // L from 1 | 2 down to 7 | 8 sequences per tile.
Each test names the lengths that carry a class alone (`sole`): removing one of them from SHORT_LENS makes that test fail."""
import os
import subprocess

import numpy as np

from tests import short_lengths_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCU = 256                                                   # the classes are proved for the MI355X's plan; test_the_small_count_plan: 64 and 304 too


def _carriers(key, lens=None):
    """{class: the lengths of SHORT_LENS that reach it} for key(L, s) -> an iterable of classes."""
    out = {}
    for L, s in S.shared_pairs(NCU, lens):
        for c in key(L, s):
            out.setdefault(c, set()).add(L)
    return out


def test_the_lengths_and_packings():
    assert len(S.SHORT_LENS) == len(set(S.SHORT_LENS)) == 43 and S.SHORT_LENS == sorted(S.SHORT_LENS)
    assert all(1 <= L <= 104 for L in S.SHORT_LENS) and {3, 12} <= set(S.SHORT_LENS)
    assert S.packs(104) == [1, 2] and S.packs(50) == [1, 2, 3, 4] and S.packs(33) == [1, 2, 3, 4, 5, 6] and S.packs(1) == [1, 2, 3, 4, 207, 208]
    assert S.packs(69) == [1, 2, 3] and S.packs(70) == [1, 2]
    for L, s in S.pairs():
        assert 1 <= s <= 208 // L and s * L <= S.TILE_ROWS
        assert S.batch_sizes(s) == ([2 * s + 1, 2 * s - 1] if s >= 3 else [2 * s + 1])
    assert len(S.pairs()) == sum(len(S.packs(L)) for L in S.SHORT_LENS) >= 184
    assert S.DILS == (1, 4, 16, 64)
    from svdd_amd import backbone, config
    assert tuple(d for d in backbone.DILATIONS for _ in range(config.dna_config().model.num_cnn_stacks)) == tuple(S.DIL)


def test_every_row_tile_count_and_entry_body():
    by = _carriers(lambda L, s: [S.row_tiles(L, s)])
    assert sorted(by) == list(range(1, 14)), sorted(by)
    assert {S.entry_body(nt) for nt in by} == {2, 4, 7}
    assert [S.entry_body(nt) for nt in (4, 5, 8, 9)] == [2, 4, 4, 7]                 # both sides of both limits are among 1 .. 13
    for nt in by:                                                                   # nro: the wave halves own ceil / floor of nt / 2
        assert (S.owned_slots(nt, 0), S.owned_slots(nt, 1)) == ((nt + 1) // 2, nt // 2) and S.owned_slots(nt, 0) <= 7
    assert any(S.owned_slots(nt, 0) != S.owned_slots(nt, 1) for nt in by) and any(S.owned_slots(nt, 0) == S.owned_slots(nt, 1) for nt in by)


def test_every_residue_of_the_tile_rows():
    by = _carriers(lambda L, s: [s * L % 16])
    assert sorted(by) == list(range(16)), sorted(by)
    assert by[0] and by[1]                                                          # no padding row | one live row in the last row tile
    # ... at every entry body
    for body in (2, 4, 7):
        got = {s * L % 16 for L, s in S.shared_pairs(NCU) if S.entry_body(S.row_tiles(L, s)) == body}
        assert {0, 1} <= got, (body, sorted(got))


def _one_row_classes(L, s):
    """(dilation, tap distance) with a one-row (row tile, tap) pair at (L, s)."""
    return {(dil, abs(t - 4)) for dil in S.DILS for _, t in S.one_row_pairs(L, s, dil)}


def test_every_dilation_and_tap_distance_has_a_one_row_pair():
    want = {(dil, k) for dil in S.DILS for k in S.live_distances(dil)}
    assert want == {(1, k) for k in range(5)} | {(4, k) for k in range(5)} | {(16, k) for k in range(5)} | {(64, 0), (64, 1)}
    by = _carriers(_one_row_classes)
    assert set(by) == want, sorted(want - set(by))
    for (dil, k), lens in by.items():
        assert all(k * dil < L for L in lens)                                       # only a live tap can have one
    # both sides: the tap's last live row first in its row tile (hi = 16 T + 1), and a negative tap's first live row last in its
    # row tile (lo = 16 T + 15 = s k dil: dilation 1 and odd s k only — 4, 16 and 64 times anything is even)
    sides = _carriers(lambda L, s: {(side, dil) for dil in S.DILS for side, _ in S.one_row_sides(L, s, dil)})
    assert set(sides) == {("hi", dil) for dil in S.DILS} | {("lo", 1)}, sorted(sides)
    assert S.one_row_sides(13, 15, 1) >= {("lo", 1)} and S.one_row_sides(30, 5, 1) >= {("lo", 3)}
    # the rule itself at hand-checked cases: one sequence of 33 rows: tile 2 holds row 32 alone, every tap that does not point past
    # the end keeps it; tap + 1 of dilation 16 ends at row 33 - 16 = 17 = the first row of tile 1
    assert S.one_row_pairs(33, 1, 1) == [(2, t) for t in range(5)] and (1, 5) in S.one_row_pairs(33, 1, 16)
    assert S.live_rows(33, 1, 2, 5, 1) == 0 and S.live_rows(33, 1, 1, 5, 16) == 1 and S.live_rows(33, 1, 0, 3, 16) == 0
    # four sequences of 50: d = 4 (t - 4) dil; tap + 1 of dilation 4 ends at 200 - 16 = 184 = 11 x 16 + 8: no such pair
    assert S.live_rows(50, 4, 11, 5, 4) == 8 and not S.one_row_pairs(50, 4, 4) and not S.one_row_pairs(50, 4, 64)
    # what the suite ran the interleaved kernel on before (full tiles at L = 104, 50, 33, 9): one such pair, dilation 1, distance 2
    old = {L: sorted(_one_row_classes(L, 208 // L)) for L in (104, 50, 33, 9)}
    assert {k: v for k, v in old.items() if v} == {9: [(1, 2)]}, old


def test_the_small_count_plan_and_what_only_single_sequence_tiles_carry():
    """The forced s = 1 launches run the one-sequence form, so they count for nothing above. Without the launch on a small device-side
    count these classes would be lost: one live row in the last row tile of a 2-slot tile, and the one-row pairs of (dilation 16,
    distance 3 and 4) and (dilation 64, distance 1). (Dilation 64, distance 1 is alive from L = 65 up, where only one sequence fits
    a tile: no forced packing s > 1 can carry it.)"""
    for ncu in (64, 256, 304):
        for L in S.SHORT_LENS:
            k = S.small_count(L, ncu)
            assert 2 <= k <= ncu and k <= 2 * (208 // L)
            s = S.small_spt(L, ncu)
            assert s == (1 if L >= 9 else 16 // L), (L, ncu, s)                     # one row tile's worth below L = 9
            assert S.small_spt(L, ncu) == S.small_spt(L, NCU)
    def classes(ps):
        out = set()
        for L, s in ps:
            out |= {("one row",) + c for c in _one_row_classes(L, s)}
            if s * L % 16 < 2:
                out.add(("body, residue", S.entry_body(S.row_tiles(L, s)), s * L % 16))
            out |= {("nt", S.row_tiles(L, s)), ("residue", s * L % 16)}
        return out
    forced = [(L, s) for L, s in S.pairs() if s > 1]
    assert classes(S.shared_pairs(NCU)) - classes(forced) == {("body, residue", 2, 1), ("one row", 16, 3), ("one row", 16, 4), ("one row", 64, 1)}
    assert classes(S.shared_pairs(NCU)) == classes(S.pairs())
    single = [(L, 1) for L in S.SHORT_LENS if L >= 9]
    assert {S.entry_body(S.row_tiles(L, 1)) for L, _ in single} == {2, 4} and max(S.row_tiles(L, 1) for L, _ in single) == 7


def test_both_sides_of_every_dead_tap_threshold():
    assert sorted({k * dil for dil in S.DILS for k in range(1, 5) if k * dil <= 104}) == list(S.DEAD_TAP_THRESHOLDS)
    for kd in S.DEAD_TAP_THRESHOLDS:
        assert kd in S.SHORT_LENS and kd + 1 in S.SHORT_LENS, kd
        for dil in S.DILS:
            if kd % dil == 0 and 1 <= kd // dil <= 4:
                t = 4 + kd // dil
                for s in S.packs(kd):
                    assert not any(S.live_rows(kd, s, T, t, dil) or S.live_rows(kd, s, T, 8 - t, dil) for T in range(13))
                for s in S.packs(kd + 1):                                           # alive for one position: s rows of the tile
                    assert sum(S.live_rows(kd + 1, s, T, t, dil) for T in range(13)) == s
                    assert sum(S.live_rows(kd + 1, s, T, 8 - t, dil) for T in range(13)) == s


def test_both_sides_of_the_changes_of_sequences_per_tile():
    assert set(S.SMAX_CHANGES) <= set(S.SHORT_LENS)
    assert [208 // L for L in (104, 69, 70, 52, 53, 41, 42, 34, 35, 29, 30, 26, 27)] == [2, 3, 2, 4, 3, 5, 4, 6, 5, 7, 6, 8, 7]
    assert {208 // L for L in S.SHORT_LENS} >= set(range(2, 9))
    assert set(S.TWO_SIZE_LENS) <= set(S.SHORT_LENS) and len({208 // L for L in S.TWO_SIZE_LENS}) == 3
    assert set(S.TOWER_MASK_LENS) <= set(S.SHORT_LENS)


def test_the_generic_convolution_lengths():
    assert {112, 113} <= set(S.CONV_LENS) and set(S.CONV_LENS) - {112, 113, 28, 44, 45, 56, 57, 74, 75} <= set(S.SHORT_LENS)
    assert all(kd in S.CONV_LENS and kd + 1 in S.CONV_LENS for kd in S.DEAD_TAP_THRESHOLDS)
    assert {224 // L for L in S.CONV_LENS} >= set(range(1, 10))
    assert {44, 45, 56, 57, 74, 75} <= set(S.CONV_LENS)                              # 5 | 4, 4 | 3, 3 | 2 sequences per 224-row tile
    assert len(S.CONV_LENS) == len(set(S.CONV_LENS))


def test_a_length_that_carries_a_class_alone_cannot_be_removed():
    """Removing a sole carrier loses its class: the checks above are not vacuous. 43 is the only length with one live row in the
    last row tile of a 7-slot tile (3 x 43 = 129); every sole carrier found is tried."""
    keys = {"nt": lambda L, s: [S.row_tiles(L, s)], "residue": lambda L, s: [s * L % 16], "one row": _one_row_classes,
            "body, residue 0 | 1": lambda L, s: [(S.entry_body(S.row_tiles(L, s)), s * L % 16)] if s * L % 16 < 2 else []}
    sole = {}
    for name, key in keys.items():
        for c, lens in _carriers(key).items():
            if len(lens) == 1:
                sole.setdefault(next(iter(lens)), []).append((name, c))
    for L, classes in sole.items():
        rest = [x for x in S.SHORT_LENS if x != L]
        for name, c in classes:
            assert c not in _carriers(keys[name], rest), (L, name, c)
    # the thresholds and the changes of 208 // L name their lengths outright
    named = {kd + e for kd in S.DEAD_TAP_THRESHOLDS for e in (0, 1)} | set(S.SMAX_CHANGES)
    assert named <= set(S.SHORT_LENS) and {3, 12} <= named
    assert (7, 1) in [c for _, c in sole.get(43, [])], sole
    print("sole carriers:", {L: v for L, v in sorted(sole.items())})


_PLAN_CPP = r'''
#define __host__
#define __device__
#include <cstdio>
#include <cstdlib>
#include "svdd_spt.h"
int main(int argc, char** argv) {
  for (int i = 1; i + 3 < argc; i += 4) {
    const int n = std::atoi(argv[i]), L = std::atoi(argv[i + 1]), ncu = std::atoi(argv[i + 2]), fixed = std::atoi(argv[i + 3]);
    const SvddTilePlan p = svdd_plan_tiles(n, L, ncu, fixed);
    const int tiles = svdd_plan_num_tiles(p, n);
    int s0, ns;
    svdd_plan_tile(p, tiles - 1, s0, ns);
    std::printf("%d %d %d %d %d %d %d\n", svdd_choose_spt(n, L, ncu, fixed), p.s1, p.n1, p.s2, tiles, s0, ns);
  }
  return 0;
}'''


def test_numpy_tile_plan_is_the_header(tmp_path):
    """svdd_choose_spt / svdd_plan_tiles / svdd_plan_num_tiles / svdd_plan_tile of csrc/svdd_spt.h against their restatement, over
    (n, L, ncu, fixed_half): every length of the two-size GPU cases and more, CU counts 8, 64, 256 and 304, the fixed parts of
    the fp32 kernel and of the lp modes."""
    src, exe = tmp_path / "plan.cpp", tmp_path / "plan"
    src.write_text(_PLAN_CPP)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "svdd_amd", "csrc"), "-o", str(exe), str(src)])
    ns = sorted(set(list(range(1, 40)) + list(range(250, 270)) + list(range(500, 1300, 37)) + [1100, 1408, 1650, 2560, 3001]))
    grid = [(n, L, ncu, fixed) for L in (1, 9, 26, 33, 50, 52, 69, 70, 104) for ncu in (8, 64, 256, 304) for fixed in (9, 58, 90) for n in ns]
    got = []
    for i in range(0, len(grid), 2000):                                             # (the command line has a length limit)
        args = [str(v) for case in grid[i:i + 2000] for v in case]
        got += [tuple(map(int, ln.split())) for ln in subprocess.run([str(exe)] + args, capture_output=True, text=True, check=True).stdout.splitlines()]
    assert len(got) == len(grid)
    mixed = 0
    for case, g in zip(grid, got):
        n = case[0]
        plan = S.plan_tiles(*case)
        tiles = S.plan_num_tiles(plan, n)
        want = (S.choose_spt(*case),) + plan + (tiles,) + S.plan_tile(plan, tiles - 1)
        assert g == want, (case, g, want)
        mixed += plan[1] > 0 and plan[0] != plan[2]
    assert mixed > 100
    # the GPU file's two-size cases exist at the CU counts of the devices the kernels run on
    for ncu in (256, 304, 64):
        for L in S.TWO_SIZE_LENS:
            n = S.two_size_batch(L, ncu)
            s1, n1, s2 = S.plan_tiles(n, L, ncu, 9)
            assert n1 > 0 and s1 != s2 and n1 % ncu == 0, (L, ncu, n)
    assert np.all([S.choose_spt(n, 50, 256, 9) >= 1 for n in (1, 256, 1408)])
