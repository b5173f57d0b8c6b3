"""No GPU: conditions on the INPUTS of tests/test_lengths_gpu.py, checked on the numpy / torch references alone — that the lengths
and the change and candidate sets built from them (tests/lengths_ref.py) really reach the cases the GPU file is there for.
  * LENS holds every residue mod 16;
  * for each of the dilations 1, 4, 16 and 64 some length of LENS has a (row tile, tap) pair that backbone_kernel's schedule keeps
    for exactly ONE row, and some length has a tile of padding only inside the 208-row planes; which residues can have such a pair;
  * at every length the stem's change sets produce a tight item whose last tile holds exactly one row < L, one that ends exactly at
    L - 1 and one that starts at row 0, and (where L = 1 mod 16) an aligned item of the deeper layers whose last tile holds one row;
  * the tight work list (tests/incr4_ref.py), the part rule (tests/test_tower_parts_cpu.py) and the window formulas
    (tests/test_tight_windows_cpu.py) keep their own invariants at every length: cover of the reach, disjoint tiles, at most 7
    items; disjoint part tiles whose layers cover what the next layer reads; windows that cover lo - 27 .. hi + 27 in <= 13 tiles;
  * the tower's candidate sets put a kept range's end exactly on L - 1 and one row before it, and hold the 69 / 70 part boundary;
    the pair sweeps hold every separation once."""
import numpy as np

from tests import incr3_ref as R3
from tests import incr4_ref as R4
from tests import lengths_ref as G
from tests.test_backbone_incr4_cpu import _check_row
from tests.test_tight_windows_cpu import aligned_windows, first_last, tight_windows
from tests.test_tower_parts_cpu import _check_geometry, part_ranges, part_rule, tile_layers

REACH = R3.reach(G.DIL, 12)


def test_lens_hold_every_residue():
    assert sorted({L % 16 for L in G.LENS}) == list(range(16))
    assert all(104 < L <= 208 for L in G.LENS + G.SWEEP_LENS) and len(set(G.LENS)) == len(G.LENS) == 24
    assert {112, 113} <= set(G.LENS)


def test_every_dilation_has_a_one_row_pair_and_a_padding_tile():
    residues = {1: {1, 2, 3, 4, 5}, 4: {1, 5, 9, 13}, 16: {1}, 64: {1}}
    for dil, want in residues.items():
        got = {L % 16 for L in range(105, 209) if G.one_row_pairs(L, dil)}
        assert got == want, (dil, sorted(got))
        hit = [L for L in G.LENS if G.one_row_pairs(L, dil)]
        assert hit and {L % 16 for L in hit} == want, (dil, hit)               # every residue that can have such a pair has one
        for L in hit:
            for T, t in G.one_row_pairs(L, dil):
                d = max(0, (t - 4) * dil)                                       # the pair's one row is the tap's LAST live row:
                assert (L - d) % 16 == 1 and 16 * T + 1 == L - d                # L - d for a positive tap, L itself for the others
        assert all(t > 4 for L in hit if L % 16 != 1 for _, t in G.one_row_pairs(L, dil))
        assert any(G.padding_tiles(L) for L in G.LENS)
    assert G.padding_tiles(112) == list(range(7, 13)) and G.padding_tiles(192) == [12] and not G.padding_tiles(207)
    # the lengths the suite ran the one-sequence forms at before (residues 9, 8, 0, 11) reach one pair of this kind: dilation 4, tap + 2
    old = {(L, dil): G.one_row_pairs(L, dil) for L in (105, 128, 187, 200, 208) for dil in (1, 4, 16, 64)}
    assert {k: v for k, v in old.items() if v} == {(105, 4): [(6, 6)]}
    # where the last tile holds at most four rows the one-launch kernel drops (last tile, tap + d) at dilation 1
    for L in G.LENS:
        last = (L - 1) // 16
        assert (len(R3.live_taps(L, last, 1)) < 9) == (1 <= L % 16 <= 4), L


def _tight_items(L):
    """[(origin, tiles)] of every (forward, dilation-1 layer, row) of the stem's change sets; the aligned items [(tile, tiles)] too."""
    states = [s.numpy() for s in G.stem_states(L)]
    tight, aligned = [], []
    for prev, new in zip(states, states[1:]):
        items, tiles, fb = R4.expected_items(prev, new, L, G.DIL, G.LEAD, 12)
        assert not items[:, 0].any()                                            # row 0 never changes
        for k in range(12):
            for e in items[k].reshape(-1).tolist():
                if e:
                    (tight if k < G.LEAD else aligned).append((e & 255, e >> 8))
    return tight, aligned


def test_stem_change_sets_reach_the_edges_at_every_length():
    for L in G.LENS + G.SWEEP_LENS:
        ch = G.stem_changes(L)
        assert all(not f[0] for f in ch) and [0, L - 1] in ch[0] and list(range(L)) in ch[1]
        assert all(0 <= p < L for f in ch for r in f for p in r)
        tight, aligned = _tight_items(L)
        assert any(o + 16 * (n - 1) == L - 1 for o, n in tight), (L, "no tight item whose last tile holds exactly one row < L")
        assert any(o + 16 * n == L for o, n in tight), (L, "no tight item that ends exactly at L - 1")
        assert any(o == 0 for o, _ in tight) and any(t == 0 for t, _ in aligned), (L, "no item at row 0")
        assert any(16 * (t + n) >= L for t, n in aligned), (L, "no deep item on the last tile")
        assert all(o < L for o, _ in tight) and all(16 * t < L for t, _ in aligned)


def test_work_list_invariants_at_every_length():
    for L in G.LENS:
        for f in G.stem_changes(L):
            for changed in f:
                for rc in REACH[:G.LEAD]:
                    _check_row(sorted(changed), L, rc)
        for p in (0, 7, 8, 9, L - 10, L - 9, L - 8, L - 1):                     # single positions next to both ends
            for rc in REACH[:G.LEAD]:
                tiles, _, fb = _check_row([p], L, rc)
                assert not fb and tiles == -(-(min(L - 1, p + rc) - max(0, p - rc) + 1) // 16)
        for sets in (G.sweep_single(L)[0][::7], G.sweep_pairs(L)[0]):
            for changed in sets:
                _check_row(sorted(changed), L, REACH[0])
                _check_row(sorted(changed), L, REACH[G.LEAD - 1])
    for L in G.SWEEP_LENS:
        pairs = G.sweep_pairs(L)[0]
        assert sorted(b - a for a, b in pairs) == list(range(1, L)) and len(G.sweep_single(L)[0]) == L


def test_tower_candidate_sets_at_every_length():
    for L in G.LENS:
        cand, x = (t.numpy() for t in G.tower_case(L))
        M = cand.shape[1]
        lo, hi = first_last(cand, x)
        live = hi >= 0
        assert (~live).sum() == 3 and M == 15
        wt, wa = tight_windows(lo, hi, L), aligned_windows(lo, hi, L)
        assert (wt[~live] == 0).all() and (wa[~live] == 0).all()
        need0, need1 = np.maximum(0, lo - G.MARGIN), np.minimum(L, hi + G.MARGIN + 1)
        for w in (wt, wa):
            assert (w[live, 0] <= need0[live]).all() and (w[live, 1] >= need1[live]).all()          # covers
            assert ((w[live, 1] - w[live, 0]) % 16 == 0).all() and ((w[live, 1] - w[live, 0]) // 16 <= (L + 15) // 16).all()
        assert (wt[live, 0] == need0[live]).all() and (wa % 16 == 0).all() and (wa[:, 1] <= (L + 15) // 16 * 16).all()
        # a window whose kept range [.., w1 - 10) ends exactly at the last changed row's reach (hi + 17): the tight window of a lone
        # change away from both ends is 55 rows, so w1 - 10 = hi + 18 never happens there; at the sequence end the kept range ends at
        # L, and L - 18 is the last position that reaches row L - 1
        one = [m for m in range(M) if lo[m] == hi[m] >= 0]
        assert {int(hi[m]) + 17 for m in one} >= {L - 2, L - 1, L}
        for gap in (G.GAP, L + 1):
            parts, nparts = part_rule(cand, x, gap)
            _check_geometry(parts, L)
            assert nparts.max() == (2 if gap == G.GAP else 1) and ((nparts > 0) == live).all()
            t = tile_layers(parts, L)
            assert (t <= 6 * (wt[:, 1] - wt[:, 0]) // 16).all() and ((t == 0) == ~live).all()
        parts, nparts = part_rule(cand, x, G.GAP)
        assert nparts[:M].tolist() == [0] + [1] * 12 + [2, 1]                       # 69 apart: one part; 70 apart: two
        assert parts[13].tolist() == [[L - 71, L - 71], [L - 1, L - 1], [-1, -1]] and parts[12, 0].tolist() == [L - 70, L - 1]
        for a, b in ((L - 18, L - 18), (L - 1, L - 1), (0, 0)):
            rng = part_ranges(a, b, L)
            assert rng[5] == (max(0, a - 17), min(L, b + 18)) and all(0 <= s < e <= L for s, e in rng)
    for L in G.SWEEP_LENS:
        pairs = G.tower_sweep_pairs(L)
        cand, x = (t.numpy() for t in G.tower_case(L, pairs, B=1))
        parts, nparts = part_rule(cand, x, G.GAP)
        _check_geometry(parts, L)
        sep = np.array([b - a for a, b in pairs])
        assert ((nparts == 2) == (sep >= G.GAP)).all() and {69, 70} <= set(sep.tolist())
