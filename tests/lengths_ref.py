"""What tests/test_lengths_cpu.py and tests/test_lengths_gpu.py share: the lengths at which the kernels that put ONE sequence into
one workgroup (104 < L <= 208) are pinned, and the inputs that are built from L — the change sets of the incremental stem and the
candidate sets of the windowed tower. Nothing here touches a device.

LENS holds every residue of L mod 16 (105 .. 120), whole tiles of padding inside the 208-row planes (112, 128, 144, 192), one live
row in the last tile (113, 129, 177, 193) and lengths next to a tile end (199, 207). A (row tile, tap) pair of a 9-tap convolution
of dilation d is alive for exactly ONE row where L - max(0, t - 4) d = 1 (mod 16): dilations 16 and 64 only at L = 1 (mod 16),
dilation 4 at residues 1, 5, 9, 13, dilation 1 at residues 1 .. 5 (one_row_pairs; at residue 1 it is the last tile with every tap
that does not point past the end)."""
import numpy as np
import torch

from tests import incr3_ref as R3

LENS = list(range(105, 121)) + [128, 129, 144, 177, 192, 193, 199, 207]
SWEEP_LENS = [105, 113, 192, 200, 208]
DIL = (1,) * 8 + (4,) * 4 + (16,) * 4 + (64,) * 4          # the backbone's dilations (config.dna_config)
LEAD, MASK, ROWS = 8, 4, 5
MARGIN, GAP = 27, 70                                        # fused.TOWER_WINDOW_MARGIN, fused.TOWER_PART_GAP


# ------------------------------------------------------------------------------------------------------------- the schedule
def live_rows(L, T, tap, dil):
    """Rows of tile T that tap `tap` of a dilation-dil convolution maps inside a sequence of length L (the schedule's lo / hi)."""
    d = (tap - 4) * dil
    lo, hi = max(0, -d), min(L, L - d)
    return max(0, min(hi, 16 * T + 16) - max(lo, 16 * T))


def one_row_pairs(L, dil):
    """[(tile, tap)] that backbone_kernel's schedule keeps at length L for exactly one row."""
    return [(T, t) for T in range(R3.TILES) for t in R3.live_taps(L, T, dil) if live_rows(L, T, t, dil) == 1]


def padding_tiles(L):
    """Tiles of the 208-row planes that hold no row of the sequence."""
    return [T for T in range(R3.TILES) if 16 * T >= L]


# ----------------------------------------------------------------------------------------------------- the stem's change sets
def stem_changes(L):
    """Per incremental forward, per row: the positions that change. Row 0 never changes; position L - 9 is the one whose reach in
    plane 1 (8 rows) ends exactly at L - 1 — its tight cover is the tiles at L - 17 and at L - 1, the last of which holds ONE row of
    the sequence —, L - 10 lies a row further in; 39 has (p - 8) % 16 == 15; (40, 57) are 17 apart (their runs join), (40, 73) 33
    apart (they do not); L - 24 gives the 2-tile item [L - 32, L - 1] that ends exactly at the last row."""
    assert (39 - 8) % 16 == 15
    return [[[], [0, L - 1], [L - 9], [39], [40, 57]],
            [[], list(range(L)), [L - 10], [40, 73], [L - 24]],
            [[], [L // 2], [0], [L - 1], [3, 90, 91]]]


def stem_states(L, changes=None, rows=ROWS):
    """tokens [1 + forwards][rows][L] u8 (CPU): state 0 belongs to the full forward, state t follows the t-th change set."""
    changes = stem_changes(L) if changes is None else changes
    g = torch.Generator().manual_seed(4100 + L)
    x = torch.randint(0, 4, (rows, L), generator=g, dtype=torch.int64)
    x[torch.rand(rows, L, generator=g) < 0.5] = MASK
    states = [x.clone()]
    for t, sets in enumerate(changes):
        for r, pos in enumerate(sets):
            x[r, pos] = (x[r, pos] + 1 + t) % 5                     # a real change: never the token that is there
        states.append(x.clone())
    return [s.to(torch.uint8) for s in states]


def sweep_single(L):
    """Row r changes position r only: [L][1]."""
    return [[[r] for r in range(L)]]


def sweep_pairs(L):
    """Row r changes positions c and c + r + 1, c = (7 r) % (L - r - 1): every separation 1 .. L - 1 once: [L - 1][2]."""
    out = []
    for r in range(L - 1):
        c = (7 * r) % (L - r - 1)
        assert 0 <= c < c + r + 1 < L
        out.append([c, c + r + 1])
    return [out]


def item_rows(items, lead, rows=ROWS):
    """bool [D][rows][208]: the rows of plane k that the items of layer k may write (tight items below `lead`: origin row | tiles
    << 8; aligned items: first tile | tiles << 8; lead = 0: every layer aligned)."""
    D = items.shape[0]
    m = torch.zeros(D, rows, 208 + 16 * 2, dtype=torch.bool)
    for k in range(D):
        for r in range(rows):
            for e in items[k, r].tolist():
                if e:
                    o = (e & 255) if k < lead else 16 * (e & 255)
                    m[k, r, o:o + 16 * (e >> 8)] = True
    return m[:, :, :208]


# ------------------------------------------------------------------------------------------------- the tower's candidate sets
def tower_changes(L):
    """The changed positions of each candidate of one parent: no change; single changes at both sequence ends, around the window
    margin (27) from the front and from the back, and at the reach (17) from the back (L - 18 is the last position whose last
    reached row is L - 1); pairs 69 apart (one part) and 70 apart (two) that end at L - 1; every position."""
    return [[], [0], [26], [27], [28], [L - 29], [L - 28], [L - 27], [L - 19], [L - 18], [L - 17], [L - 1],
            [L - 70, L - 1], [L - 71, L - 1], list(range(L))]


def tower_case(L, changes=None, B=3):
    """(cand [B, M, L] u8, x [B, L] u8) on the CPU: every parent gets the whole candidate set, with its own replaced tokens."""
    changes = tower_changes(L) if changes is None else changes
    M = len(changes)
    g = torch.Generator().manual_seed(7100 + L)
    x = torch.randint(0, 4, (B, L), generator=g, dtype=torch.uint8)
    x[torch.rand(B, L, generator=g) < 0.5] = MASK
    cand = x[:, None, :].repeat(1, M, 1)
    for b in range(B):
        for m, pos in enumerate(changes):
            for p in pos:
                cand[b, m, p] = (int(x[b, p]) + 1 + (b + m + p) % 3) % 4 if x[b, p] < 4 else (m + b + p) % 4   # a real change
    assert all(int((cand[b, m] != x[b]).sum()) == len(changes[m]) for b in range(B) for m in range(M))
    return cand.contiguous(), x.contiguous()


def tower_sweep_single(L):
    return [[m] for m in range(L)]


def tower_sweep_pairs(L):
    return sweep_pairs(L)[0]


def window_rows(win, L):
    """bool [n][L]: rows inside each candidate's window (w0, w1)."""
    r = np.arange(L)[None, :]
    win = np.asarray(win)
    return (r >= win[:, :1]) & (r < win[:, 1:2])
