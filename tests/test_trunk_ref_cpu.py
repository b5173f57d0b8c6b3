"""No GPU: the restatements of tests/trunk_ref.py that the GPU tests of the shared-level window kernels compare against
(windows_ref, reach_ref) are themselves proved here — windows_ref against the brute-force dependency cone reach_ref, and that
cone against the float64 EnformerConvTower, which is what ties the integer tables to the network."""
import numpy as np
import pytest
import torch

from svdd_amd.enformer_value import EnformerConvTower
from tests import trunk_ref as R


def _check_windows(w0, wlen, seg, edits, L, halo, depth, slots, live):
    n = len(edits)
    for c in range(n):
        if c >= live:
            assert not w0[:, c].any() and not wlen[:, c].any() and not seg[:, c].any()
            continue
        reach = R.reach_ref(edits[c], L, halo, depth)
        Lc = L
        for d in range(depth):
            used = [(int(w0[d, c, j]), int(wlen[d, c, j])) for j in range(slots) if wlen[d, c, j] > 0]
            k = len(used)                                       # used slots come first, unused ones are all zero
            assert not wlen[d, c, k:].any() and not w0[d, c, k:].any() and not seg[d, c, k:].any()
            assert (wlen[d, c, :k] > 0).all() and k <= slots
            assert (seg[d, c, :k] == wlen[d, c, :k] + (4 if d else 0)).all()
            covered = set()
            for j, (a, ln) in enumerate(used):
                b = a + ln
                assert a % 2 == 0 and (b % 2 == 0 or b == Lc) and 0 <= a < b <= Lc            # even-aligned, inside the level
                if j:
                    prev_end = used[j - 1][0] + used[j - 1][1]
                    assert a > prev_end + (4 if d else 0), (d, c, used)   # level 0: not touching; deeper: more than 4 rows apart
                covered |= set(range(a, b))
            assert reach[d] <= covered, (L, halo, depth, slots, c, d, sorted(reach[d] - covered))
            assert bool(edits[c]) == bool(used)
            assert sum(ln for _, ln in used) <= Lc <= L
            Lc = (Lc + 1) // 2


@pytest.mark.parametrize("case", R.WINDOW_CASES, ids=R.window_case_id)
def test_windows_ref_covers_the_cone_on_the_gpu_case_table(case):
    """The tables the GPU tests hold the kernels to: at every level the windows cover every row the changed tokens can reach,
    are even-aligned, ascending, inside the level, apart (level 0: not touching; deeper: more than 4 rows, so segments with
    their context never overlap), at most `slots`, at most L rows in all; c >= count and unused slots are zero. Every edit kind
    of the table occurs."""
    L, depth, slots, halo, count, perm = case
    cand, parent, pidx, div, edits = R.window_case_tokens(case)
    for c, ps in enumerate(edits):                              # the tokens really differ at the scripted positions, and only there
        assert sorted(np.nonzero(cand[c] != parent[pidx[c] // div])[0].tolist()) == ps
    w0, wlen, seg = R.windows_ref(cand, parent, pidx, div, L, halo, depth, slots, count)
    assert w0.dtype == np.int32 and w0.shape == (depth, R.WIN_N, slots)
    _check_windows(w0, wlen, seg, edits, L, halo, depth, slots, R.WIN_N if count is None else count)
    assert (parent[3] == R.MASK).all() and edits[0] == [] and edits[10] == list(range(L))


def test_case_table_holds_every_edit_kind():
    """L = 200, halo 7: the scripted pairs are what their names say (touching / not, level-1 windows 4 / 6 rows apart)."""
    e = R.window_case_edits(200, 7, 4)
    assert e[:5] == [[], [0], [199], [0, 199], [100, 101]]
    l0 = lambda k: [R._level0(p, 200, 7) for p in e[k]]           # noqa: E731
    l1 = lambda k: [R._level1(p, 200, 7) for p in e[k]]           # noqa: E731
    assert l0(5)[1][0] == l0(5)[0][1] and l0(6)[1][0] == l0(6)[0][1] + 2
    assert l1(7)[1][0] == l1(7)[0][1] + 4 and l1(8)[1][0] == l1(8)[0][1] + 6
    assert len(e[9]) > 4 and len(e) == R.WIN_N
    cand, parent, pidx, div, edits = R.window_case_tokens((200, 2, 4, 7, None, False))
    w0, wlen, _ = R.windows_ref(cand, parent, pidx, div, 200, 7, 2, 4)
    used = lambda d, c: int((wlen[d, c] > 0).sum())              # noqa: E731
    assert (used(0, 5), used(0, 6)) == (1, 2) and (used(0, 7), used(1, 7)) == (2, 1) and (used(0, 8), used(1, 8)) == (2, 2)
    assert used(0, 9) == 4 and wlen[0, 10, 0] == 200


def test_windows_ref_covers_the_cone_on_random_cases():
    """Random lengths 2 .. 256, depths 1 - 4 (as the evenness of L allows), 1 - 4 slots, halo 0 .. 9, 0 .. 12 changed positions."""
    rng = np.random.default_rng(5)
    for _ in range(400):
        depth = int(rng.integers(1, 5))
        L = int(rng.integers(2, 257))
        L -= L % (1 << (depth - 1))
        if L < 2:
            continue
        slots, halo = int(rng.integers(1, 5)), int(rng.choice([7, 7, 0, 1, 2, 3, 9]))
        n = 4
        parent = rng.integers(0, 5, size=(2, L)).astype(np.uint8)
        pidx = np.array([0, 3, 2, 1], dtype=np.int32)
        cand = parent[pidx // 2].copy()
        edits = []
        for c in range(n):
            k = int(rng.integers(0, 13)) if c else 0
            ps = sorted({int(p) for p in rng.integers(0, L, size=k)})
            if rng.random() < 0.3 and ps:                       # clustered: positions next to each other
                ps = sorted({min(L - 1, ps[0] + int(q)) for q in rng.integers(0, 40, size=k)})
            for p in ps:
                cand[c, p] = (cand[c, p] + 1 + p % 4) % 5
            edits.append(ps)
        count = None if rng.random() < 0.7 else int(rng.integers(0, n + 1))
        w0, wlen, seg = R.windows_ref(cand, parent, pidx, 2, L, halo, depth, slots, count)
        _check_windows(w0, wlen, seg, edits, L, halo, depth, slots, n if count is None else count)


def test_reach_ref_is_the_cone_of_the_float64_tower():
    """EnformerConvTower in float64 (3 levels, 128 - 256 channels, weights as trunk_ref.randomise draws them), a parent and
    candidates that differ at scripted positions: at every level the rows of the block output (what the pooling reads) outside
    reach_ref(., halo 7) are bit-equal to the parent's, and for single interior edits the outermost rows of the cone at levels
    0, 1 and 2 DO differ — the cone is the module's, 7 and 2 are not generous. L = 64 (even levels) and L = 37 (odd levels)."""
    torch.manual_seed(0)
    tower = EnformerConvTower(3, 256).double().eval()
    R.randomise_tower(tower, 4)
    rows = []
    for blk in tower.blocks:
        blk[1].pool.register_forward_pre_hook(lambda m, inp: rows.append(inp[0].detach().transpose(1, 2)))   # [n, Lc, C]
    g = torch.Generator(device="cpu").manual_seed(9)
    tight = set()
    for L, edits in ((64, [[], [30], [0], [63], [0, 63], [20, 21], [5, 40], [33], list(range(0, 64, 7))]),
                     (37, [[], [18], [0], [36], [17, 30]])):
        par = torch.randint(0, 5, (L,), generator=g)
        tok = par.repeat(1 + len(edits), 1)
        for c, ps in enumerate(edits):
            for p in ps:
                tok[1 + c, p] = (tok[1 + c, p] + 1 + p % 3) % 5
        x = torch.nn.functional.one_hot(tok, 5)[:, :, :4].double().transpose(1, 2).contiguous()      # MASK: no channel
        rows.clear()
        with torch.no_grad():
            for i in range(x.shape[0]):                         # one sequence per call: every sequence then goes through the same
                tower(x[i:i + 1])                               # arithmetic (a batch is cut into vector / remainder pieces by position)
        assert len(rows) == 3 * x.shape[0]
        rows[:] = [torch.cat(rows[d::3]) for d in range(3)]
        for c, ps in enumerate(edits):
            changed = torch.nonzero(tok[1 + c] != par).flatten().tolist()
            assert changed == ps
            reach = R.reach_ref(ps, L, 7, 3)
            for d in range(3):
                y, yp = rows[d][1 + c], rows[d][0]
                differ = {i for i in range(y.shape[0]) if not torch.equal(y[i], yp[i])}
                assert differ <= reach[d], (L, c, d, sorted(differ - reach[d]))
                if len(ps) == 1 and 16 <= ps[0] < L - 16:       # an interior edit: the cone's outermost rows are reached
                    assert min(differ) == min(reach[d]) and max(differ) == max(reach[d]), (L, c, d)
                    inside = 0 < min(reach[d]) and max(reach[d]) < y.shape[0] - 1
                    assert inside or d == 2                     # (levels 0 and 1: the cone's ends are not the sequence's)
                    tight.add((L, d, inside))
    assert {(64, 0, True), (64, 1, True), (64, 2, True), (37, 0, True), (37, 1, True)} <= tight
