"""Recorded Levenshtein tables of the raw-kernel tests of tests/test_select_edit_gpu.py: the outputs of tests/edit_ref.py's plain
Wagner-Fischer table (edit_matrix) at the sizes where it takes minutes, so that the GPU tests need not recompute them on every run.

    python tests/golden/make_golden_select_edit.py            # about five minutes of numpy, no GPU, nothing but this repository

Everything is generated from seeds by tests/select_edit_ref.py; tests/test_select_edit_cpu.py checks that the recorded inputs are
what the generators give today and recomputes the cheapest tables. g41_select_edit.npz holds arrays only:

  xq_<L>_<si>  [B, L] u8, xdb_<L>_<si> [N, L] u8   select_edit_ref.kernel_rows(L, si) for L >= 64
  d0_<L>_<si>  [B, N] i16                          edit_matrix(xq, xdb)
  d1_<L>_<si>  [B, N] i16                          the smaller of that and edit_matrix(revcomp(xq), xdb)
  seg_xq [260, 16] u8, seg_xdb_sha1                select_edit_ref.segment_rows(): the queries and the SHA-1 of the 20,000 database rows
  seg_hit_i, seg_hit_j  i32                        the pairs of them within 2 edits (edit_matrix in database chunks)
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import select_edit_ref as E  # noqa: E402


def main():
    out = {}
    for L in (L for L in E.KERNEL_LS if L >= E.GOLDEN_MIN_L):
        for si in range(len(E.kernel_sizes(L))):
            xq, xdb = E.kernel_rows(L, si)
            out[f"xq_{L}_{si}"], out[f"xdb_{L}_{si}"] = xq, xdb
            for rc in (False, True):
                out[f"d{int(rc)}_{L}_{si}"] = E.distance_matrix(xq, xdb, rc).astype(np.int16)
            print(L, si, xq.shape, xdb.shape, flush=True)
    xq, xdb = E.segment_rows()
    i, j = np.nonzero(E.segment_hits(xq, xdb))
    out.update(seg_xq=xq, seg_xdb_sha1=np.str_(hashlib.sha1(xdb.tobytes()).hexdigest()), seg_hit_i=i.astype(np.int32),
               seg_hit_j=j.astype(np.int32))
    print("segments:", len(i), "hits", flush=True)
    np.savez_compressed(E.GOLDEN, **out)
    print("wrote", E.GOLDEN, os.path.getsize(E.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
