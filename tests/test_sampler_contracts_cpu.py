"""The row index of svdd_select's row gather, restated in numpy float32 (no GPU).

select_rows_kernel copies the winning rows of a wave's RG rows in units of u bytes, U = L / u units per row, unit i of the wave
belonging to row i / U. It computes that quotient as min((int)(((float)i + 0.5f) * (1.0f / (float)U)), RG - 1) for i < RG U, and
the host (svdd_select_compact) refuses a launch with RG U >= 2^22. This file holds the expression to integer division over all
the host admits: i and U convert to fp32 exactly (< 2^24), i + 0.5 is exact (< 2^23), so the restatement below is the kernel's
arithmetic operation for operation (one rounding in the reciprocal, one in the product, truncation)."""
import numpy as np
import pytest

LIMIT = 1 << 22                                     # the host's bound: RG * U < LIMIT
ROW_COUNTS = [1, 2, 4, 8, 16, 32, 64]               # RG = R * (64 / pow2(M)), R = min(1 | 4, pow2(M)): the powers of two up to 64


def row_index(i, U, RG):
    """The kernel's expression on int64 arrays i, U (broadcastable) -> int64."""
    i, U = np.broadcast_arrays(np.asarray(i, np.int64), np.asarray(U, np.int64))
    inv_u = (np.float32(1.0) / U.astype(np.float32)).astype(np.float32)
    q = ((i.astype(np.float32) + np.float32(0.5)).astype(np.float32) * inv_u).astype(np.float32)
    return np.minimum(q.astype(np.int64), RG - 1)


def boundary_mismatch(RG, U):
    """U int64 [n] -> bool [n]: the restatement differs from min(i // U, RG - 1) at a row boundary, i = q U - 1 or q U, q = 1 .. RG
    (i = RG U is one past the wave's last unit: the kernel masks it off, and the clamp gives RG - 1 there as well)."""
    U = np.asarray(U, np.int64)[:, None]
    q = np.arange(1, RG + 1, dtype=np.int64)[None, :]
    bad = np.zeros(U.shape[0], bool)
    for i in (q * U - 1, q * U):
        bad |= (row_index(i, U, RG) != np.minimum(i // U, RG - 1)).any(axis=1)
    return bad


@pytest.mark.parametrize("RG", ROW_COUNTS)
def test_row_index_equals_integer_division_at_every_row_boundary_the_host_admits(RG):
    """Every U from 1 to the largest with RG U < 2^22. The expression is monotone in i (fp32 multiplication by a positive number and
    truncation both are), so agreeing on both sides of every boundary is agreeing everywhere; the next test does not rely on that."""
    u_max = (LIMIT - 1) // RG
    for u0 in range(1, u_max + 1, 1 << 16):
        U = np.arange(u0, min(u0 + (1 << 16), u_max + 1), dtype=np.int64)
        bad = boundary_mismatch(RG, U)
        assert not bad.any(), (RG, int(U[bad][0]))


@pytest.mark.parametrize("RG", ROW_COUNTS)
def test_row_index_equals_integer_division_for_every_unit_of_short_rows(RG):
    """Exhaustive over i in [0, RG U) for U < 600 (every L the project runs: U = 25 at L = 200)."""
    for U in range(1, 600):
        i = np.arange(RG * U, dtype=np.int64)
        assert np.array_equal(row_index(i, U, RG), i // U), (RG, U)


def test_the_bound_is_needed_and_has_room():
    """Without the host's bound the expression does go wrong inside what the entry point used to accept: for RG = 64 it agrees with
    integer division up to U = 103203 and first disagrees at U = 103204 — beyond the 65535 the bound admits for 64 rows."""
    U = np.arange(1, 103205, dtype=np.int64)
    bad = boundary_mismatch(64, U)
    assert not bad[:-1].any() and bad[-1]
    assert (LIMIT - 1) // 64 == 65535 < 103203
