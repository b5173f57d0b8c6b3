"""Golden vectors of the sample-quality metrics, recorded by RUNNING THE REFERENCE'S OWN FUNCTIONS on CPU.

Run in the build container only (needs the reference and scipy; imported through tests/golden/_ref_import.py):

    python tests/golden/make_golden_quality.py

_ref_import.install_stubs() registers an inert `oracle` module (the reference's oracle.py loads gReLU, pandas and W&B at import).
This script removes that entry in its own process, adds inert stubs for what oracle.py imports beyond the shared ones
(grelu.data.preprocess, grelu.data.dataset, pandas if it is not installed) and loads the reference's oracle.py by path, so that
`oracle.count_kmers` and `oracle.get_wasserstein_dist` are the reference's own; `Diffusion.compare_kmer` is called unbound on the
reference's class. No reference text is copied. g40_quality.npz holds arrays only:

  a200, b200      [64, 200] u8   two seeded token sets (torch.randint)
  a50, b50        [16, 50] u8    two small ones
  s1, s2          [48, 60] u8    a skewed pair over the two-letter alphabet {A, G}: 56 of the 64 3-mers are absent from BOTH, so the
                                 union rule matters: Pearson over all 64 bins gives another r (asserted below)
  kmers_<set>     [64] i64       oracle.count_kmers(detokenised set, k=3) as a vector in the lexicographic order of the ACGT strings
  r_<x>_<y>       f64            Diffusion.compare_kmer(None, kmers_x, kmers_y, n_x, n_y) for the three pairs
  r_all64_s1_s2   f64            scipy pearsonr of the skewed pair over ALL 64 bins (what a wrong restatement gives)
  scores_a [300], scores_b [170] f64, ws_scores: scipy.stats.wasserstein_distance of the two (unequal sizes)
  emb_a, emb_b    [256, 8] f64,  frechet: oracle.get_wasserstein_dist of the two (scipy sqrtm)
"""
import importlib.util
import itertools
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402

ALPHABET = "ACGT"


def load_reference():
    """-> (the reference's oracle module, its Diffusion class)."""
    _ref_import.install_stubs()
    del sys.modules["oracle"]
    grelu = sys.modules["grelu"]
    grelu.data = _ref_import._mod("grelu.data")
    grelu.data.preprocess = _ref_import._mod("grelu.data.preprocess")
    grelu.data.dataset = _ref_import._mod("grelu.data.dataset")
    try:
        import pandas  # noqa: F401
    except ImportError:
        _ref_import._mod("pandas")
    if _ref_import.REF not in sys.path:
        sys.path.insert(0, _ref_import.REF)
    spec = importlib.util.spec_from_file_location("oracle", os.path.join(_ref_import.REF, "oracle.py"))
    oracle = importlib.util.module_from_spec(spec)
    sys.modules["oracle"] = oracle
    spec.loader.exec_module(oracle)
    import diffusion_gosai
    assert diffusion_gosai.oracle is oracle
    return oracle, diffusion_gosai.Diffusion


def detok(x):
    return ["".join(ALPHABET[t] for t in row) for row in x]


def as_vector(d, k=3):
    names = ["".join(p) for p in itertools.product(ALPHABET, repeat=k)]
    assert set(d) <= set(names)
    return np.array([d.get(n, 0) for n in names], np.int64)


def main():
    from scipy.stats import pearsonr, wasserstein_distance
    oracle, Diffusion = load_reference()
    g = torch.Generator().manual_seed(4040)
    sets = {"a200": torch.randint(0, 4, (64, 200), generator=g), "b200": torch.randint(0, 4, (64, 200), generator=g),
            "a50": torch.randint(0, 4, (16, 50), generator=g), "b50": torch.randint(0, 4, (16, 50), generator=g)}
    # the skewed pair: two letters (A = 0, G = 2), with different letter frequencies on the two sides
    sets["s1"] = 2 * (torch.rand(48, 60, generator=g) < 0.3).long()
    sets["s2"] = 2 * (torch.rand(48, 60, generator=g) < 0.6).long()
    out = {name: x.numpy().astype(np.uint8) for name, x in sets.items()}
    dicts = {name: oracle.count_kmers(detok(x), k=3) for name, x in out.items()}
    for name, d in dicts.items():
        out["kmers_" + name] = as_vector(d)
        assert out["kmers_" + name].sum() == out[name].shape[0] * (out[name].shape[1] - 2)
    for x, y in (("a200", "b200"), ("a50", "b50"), ("s1", "s2")):
        out[f"r_{x}_{y}"] = np.float64(Diffusion.compare_kmer(None, dicts[x], dicts[y], out[x].shape[0], out[y].shape[0]))
        print(f"compare_kmer {x} {y}: {out[f'r_{x}_{y}']!r}")
    k1, k2 = out["kmers_s1"], out["kmers_s2"]
    absent = int(((k1 == 0) & (k2 == 0)).sum())
    out["r_all64_s1_s2"] = np.float64(pearsonr(k2.astype(np.float64), k1.astype(np.float64))[0])
    print(f"skewed pair: {absent} 3-mers absent from both; r over the union {out['r_s1_s2']!r}, over all 64 bins {out['r_all64_s1_s2']!r}")
    assert absent == 56 and abs(out["r_all64_s1_s2"] - out["r_s1_s2"]) > 1e-3      # the union rule matters on this pair
    rng = np.random.default_rng(4041)
    out["scores_a"], out["scores_b"] = rng.normal(0.3, 1.0, 300), rng.normal(-0.2, 1.7, 170)
    out["ws_scores"] = np.float64(wasserstein_distance(out["scores_a"], out["scores_b"]))
    mix = rng.normal(size=(8, 8))
    out["emb_a"], out["emb_b"] = rng.normal(size=(256, 8)), rng.normal(size=(256, 8)) @ mix * 0.7 + 0.25
    out["frechet"] = np.float64(oracle.get_wasserstein_dist(out["emb_a"], out["emb_b"]))
    print(f"wasserstein {out['ws_scores']!r} frechet {out['frechet']!r}")
    path = os.path.join(HERE, "g40_quality.npz")
    np.savez_compressed(path, **out)
    print(f"g40_quality.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
