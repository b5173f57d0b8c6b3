"""Motif content of a set of sequences: which known transcription-factor motifs a decoded batch contains, and whether
its motif usage looks like a reference set's. Not in the reference.

  MotifSet / load_meme      integer log-odds PWMs and exact p-value thresholds from position-frequency matrices (numpy float64 on
                            the host; MEME "minimal" text, the format JASPAR and HOCOMOCO are distributed in; no file is shipped)
  scan_counts / scan_rows   the scan on the device (svdd_pack_tokens + svdd_motif_scan): exact integers, independent of the chunking
  motif_frequencies / motif_corr
                            per-motif frequencies and their Spearman / Pearson correlation with a reference set
  spearmanr / pearsonr      host-level float64, average ranks for ties
  MotifReward / GuidedReward
                            decoding TOWARDS (or away from) motifs: a per-row integer motif term, one svdd_motif_reward
                            launch from u8 tokens to fp32 scores, and the wrapper the SVDD-PM sampler takes as its reward model

Token inputs are [N, L] integer tensors of finished sequences (tokens 0..3, L <= 1024), as in svdd_amd.quality. The kernel has no
CPU fallback."""
import os
import re

import numpy as np
import torch

from . import ops
from .quality import _checked, _chunk_rows, _on_device
from .tokens import INDEX_TO_DNA

DNA_ALPHABET = "".join(INDEX_TO_DNA[i] for i in range(4))       # "ACGT": the token order of the tables
MAX_WIDTH = ops.MOTIF_MAX_W
SCAN_CHUNK_ROWS = 1 << 18                # rows per pack + scan (any value gives the same integers)
_I16 = np.iinfo(np.int16)


# ------------------------------------------------------------------------------------------------- host-side tables ----
def _background(background):
    bg = np.asarray(background, np.float64).reshape(-1)
    if bg.size != 4 or not np.all(np.isfinite(bg)) or np.any(bg <= 0) or abs(float(bg.sum()) - 1.0) > 1e-9:
        raise ValueError(f"background = {background!r}: expected four positive numbers (A, C, G, T) that sum to 1 within 1e-9")
    return bg


def score_distribution(pwm, bg):
    """The exact distribution of the integer score of a random w-mer under the i.i.d. background: (lowest score, mass float64
    [max - min + 1]). One pass over the columns, in column order; within a column A, C, G, T in turn."""
    dist, low = np.ones(1, np.float64), 0
    for col in np.asarray(pwm, np.int64):
        lo, hi = int(col.min()), int(col.max())
        new = np.zeros(dist.size + hi - lo, np.float64)
        for t in range(4):
            o = int(col[t]) - lo
            new[o:o + dist.size] += dist * bg[t]
        dist, low = new, low + lo
    return low, dist


def pvalue_threshold(pwm, bg, pvalue):
    """The smallest attainable score t (non-zero mass) with P(S >= t) <= pvalue; max_score + 1 if there is none."""
    low, dist = score_distribution(pwm, bg)
    tail = np.cumsum(dist[::-1])[::-1]
    ok = np.nonzero((dist > 0) & (tail <= pvalue))[0]
    return low + int(ok[0]) if ok.size else low + dist.size


class MotifSet:
    """M motifs as integer log-odds tables: names, width i32 [M] (1 .. 32), pwm i16 [M, 32, 4] in A, C, G, T order (columns at or
    beyond a motif's width are never read), threshold i32 [M], max_score / min_score i32 [M]. Build one with from_pfms or
    load_meme."""

    def __init__(self, names, width, pwm, threshold):
        self.names = [str(n) for n in names]
        self.width = np.ascontiguousarray(width, np.int32)
        self.pwm = np.ascontiguousarray(pwm, np.int16)
        self.threshold = np.ascontiguousarray(threshold, np.int32)
        M = len(self.names)
        if M == 0 or self.width.shape != (M,) or self.pwm.shape != (M, MAX_WIDTH, 4) or self.threshold.shape != (M,):
            raise ValueError(f"a MotifSet needs M >= 1 names, width [M], pwm [M, {MAX_WIDTH}, 4] and threshold [M], got {M} names, "
                             f"{self.width.shape}, {self.pwm.shape}, {self.threshold.shape}")
        for name, w in zip(self.names, self.width):
            if not 1 <= int(w) <= MAX_WIDTH:
                raise ValueError(f"motif {name}: width {int(w)} outside 1 .. {MAX_WIDTH}")
        live = np.arange(MAX_WIDTH)[None, :, None] < self.width[:, None, None]
        p = self.pwm.astype(np.int64)
        self.max_score = np.where(live, p, 0).max(2).sum(1).astype(np.int32)
        self.min_score = np.where(live, p, 0).min(2).sum(1).astype(np.int32)
        self._dev = {}

    def __len__(self):
        return len(self.names)

    @property
    def reachable(self):
        """bool [M]: the motif's threshold can be met at all (False: it never hits; a motif of width w cannot reach a p-value
        below 4^-w under the uniform background)."""
        return self.threshold.astype(np.int64) <= self.max_score

    def to_device(self, device="cuda"):
        """-> ops.MotifTables on `device` (kept for the next call)."""
        if not torch.cuda.is_available():
            raise ops.SvddError("motifs: the scan runs on the GPU (the SVDD hot path has no CPU fallback)")
        device = torch.device(device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._dev:
            self._dev[device] = ops.MotifTables(*(torch.from_numpy(a).to(device) for a in (self.pwm, self.width, self.threshold)))
        return self._dev[device]

    @classmethod
    def from_pfms(cls, pfms, names=None, nsites=None, background=(0.25,) * 4, pseudocount=0.1, scale=100, pvalue=1e-4,
                  thresholds=None):
        """pfms: M position-frequency (or count) matrices [w, 4] in A, C, G, T order. Every column is normalised to sum 1; with
        nsites (a number or one per motif, default 20) p = (f nsites + pseudocount bg) / (nsites + pseudocount) and the entry is
        rint(log2(p / bg) scale). The threshold of a motif is the smallest attainable score whose tail probability under the
        i.i.d. background is <= pvalue (exact, by dynamic programming), or max_score + 1 if there is none (see reachable);
        thresholds = M ints gives them instead."""
        pfms = list(pfms)
        M = len(pfms)
        names = [f"motif_{i}" for i in range(M)] if names is None else [str(n) for n in names]
        if M == 0 or len(names) != M:
            raise ValueError(f"{M} matrices and {len(names)} names: expected the same number, at least one")
        bg = _background(background)
        if not np.isfinite(scale) or scale <= 0:
            raise ValueError(f"scale = {scale!r}: expected a positive number")
        if not np.isfinite(pseudocount) or pseudocount < 0:
            raise ValueError(f"pseudocount = {pseudocount!r}: expected a number >= 0")
        if thresholds is None and not 0.0 < pvalue < 1.0:
            raise ValueError(f"pvalue = {pvalue!r}: expected a number in (0, 1)")
        ns = np.full(M, 20.0) if nsites is None else np.broadcast_to(np.asarray(nsites, np.float64), (M,))
        if thresholds is not None:
            thresholds = list(thresholds)
            if len(thresholds) != M or any(isinstance(t, bool) or not isinstance(t, (int, np.integer)) for t in thresholds):
                raise ValueError(f"thresholds: expected {M} ints, one per motif")
        width, pwm, thr = np.zeros(M, np.int32), np.zeros((M, MAX_WIDTH, 4), np.int16), np.zeros(M, np.int32)
        for m, (name, f) in enumerate(zip(names, pfms)):
            f = np.asarray(f, np.float64)
            if f.ndim != 2 or f.shape[1] != 4:
                raise ValueError(f"motif {name}: expected a [w, 4] matrix, got {f.shape}")
            w = f.shape[0]
            if not 1 <= w <= MAX_WIDTH:
                raise ValueError(f"motif {name}: width {w} outside 1 .. {MAX_WIDTH}")
            if not np.all(np.isfinite(f)) or np.any(f < 0):
                raise ValueError(f"motif {name}: a negative or non-finite entry")
            s = f.sum(1, keepdims=True)
            if np.any(s <= 0):
                raise ValueError(f"motif {name}: column {int(np.nonzero(s[:, 0] <= 0)[0][0])} sums to zero")
            if not np.isfinite(ns[m]) or ns[m] <= 0:
                raise ValueError(f"motif {name}: nsites = {ns[m]!r}: expected a positive number")
            p = (f / s * ns[m] + pseudocount * bg) / (ns[m] + pseudocount)
            with np.errstate(divide="ignore"):
                e = np.rint(np.log2(p / bg) * scale)
            if not np.all(np.isfinite(e)) or e.min() < _I16.min or e.max() > _I16.max:
                raise ValueError(f"motif {name}: an entry outside int16 ({e.min()} .. {e.max()}); lower scale or raise pseudocount")
            width[m], pwm[m, :w] = w, e.astype(np.int16)
            thr[m] = int(thresholds[m]) if thresholds is not None else pvalue_threshold(pwm[m, :w], bg, pvalue)
        return cls(names, width, pwm, thr)


_NUM = r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?"
_HEADER = re.compile(r"letter-probability matrix:(.*)", re.I)


def load_meme(path_or_text, **from_pfms_kwargs):
    """A MotifSet from MEME "minimal" text (a path, or the text itself): `MOTIF <id> [name]` lines, `letter-probability matrix:
    alength= 4 w= W nsites= N` headers followed by rows of four numbers, an optional `Background letter frequencies` block (used
    unless background= is given; renormalised, since such files round to three digits). A missing nsites means 20; nsites= overrides
    the file's. The rows are read to the end of their block (a blank line, the next MOTIF or URL line, the end of the text): where
    they disagree with w= the rows count; a row that is not four numbers raises with its line number."""
    text = str(path_or_text)
    if "\n" not in text and not text.lstrip().startswith("MEME"):
        with open(os.fspath(path_or_text)) as f:
            text = f.read()
    lines = text.splitlines()
    names, pfms, nsites, file_bg = [], [], [], None
    current, i = None, 0
    while i < len(lines):
        line = lines[i].strip()
        i += 1
        if line.upper().startswith("ALPHABET"):
            letters = line.split("=", 1)[1].strip() if "=" in line else ""
            if letters.upper() != DNA_ALPHABET:
                raise ValueError(f"line {i}: alphabet {letters!r}: only {DNA_ALPHABET} is supported")
        elif line.lower().startswith("background letter frequencies"):
            vals = []
            while i < len(lines) and len(vals) < 8 and lines[i].strip() and not lines[i].strip().startswith("MOTIF"):
                vals += lines[i].split()
                i += 1
            if len(vals) != 8 or "".join(vals[0::2]).upper() != DNA_ALPHABET or not all(re.fullmatch(_NUM, v) for v in vals[1::2]):
                raise ValueError(f"line {i}: a background block must read `A p C p G p T p`, got {' '.join(vals)!r}")
            file_bg = np.array([float(v) for v in vals[1::2]])
            if np.any(file_bg <= 0) or abs(file_bg.sum() - 1.0) > 1e-2:
                raise ValueError(f"line {i}: background frequencies {file_bg.tolist()} are not positive numbers that sum to 1")
            file_bg = file_bg / file_bg.sum()
        elif line.startswith("MOTIF"):
            parts = line.split()
            if len(parts) < 2:
                raise ValueError(f"line {i}: a MOTIF line without an identifier")
            current = parts[1]
        elif _HEADER.match(line):
            if current is None:
                raise ValueError(f"line {i}: a letter-probability matrix before any MOTIF line")
            fields = dict(re.findall(r"(\w+)=\s*(\S+)", _HEADER.match(line).group(1)))
            if "alength" in fields and fields["alength"] != "4":
                raise ValueError(f"line {i}: motif {current}: alength= {fields['alength']}: only 4 (A, C, G, T) is supported")
            rows = []
            while i < len(lines):
                row = lines[i].strip()
                if not row or row.startswith("MOTIF") or row.startswith("URL"):
                    break
                cells = row.split()
                if len(cells) != 4 or not all(re.fullmatch(_NUM, c) for c in cells):
                    raise ValueError(f"line {i + 1}: motif {current}: expected a row of four numbers, got {row!r}")
                rows.append([float(c) for c in cells])
                i += 1
            if not rows:
                raise ValueError(f"line {i}: motif {current}: a matrix without rows")
            names.append(current)
            pfms.append(np.array(rows, np.float64))
            nsites.append(float(fields["nsites"]) if "nsites" in fields and float(fields["nsites"]) > 0 else 20.0)
            current = None
    if not pfms:
        raise ValueError("no motif found: expected MEME text with MOTIF lines and letter-probability matrices")
    kw = {k: v for k, v in from_pfms_kwargs.items() if v is not None}     # the caller's values win over the file's
    kw.setdefault("names", names)
    kw.setdefault("nsites", nsites)
    if file_bg is not None:
        kw.setdefault("background", file_bg)
    return MotifSet.from_pfms(pfms, **kw)


# ----------------------------------------------------------------------------------------------- correlations (host) ----
def _vec(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, np.float64).reshape(-1)


def _pair_of_vectors(a, b):
    a, b = _vec(a), _vec(b)
    if a.size != b.size:
        raise ValueError(f"a and b must have one length, got {a.size} and {b.size}")
    return a, b


def rank_average(a):
    """Ranks 1 .. n of a float64 vector; equal values share the mean of their ranks."""
    a = _vec(a)
    order = np.argsort(a, kind="stable")
    s = a[order]
    first = np.concatenate([[True], s[1:] != s[:-1]])
    start = np.nonzero(first)[0]
    end = np.concatenate([start[1:], [a.size]])
    group = np.cumsum(first) - 1
    ranks = np.empty(a.size, np.float64)
    ranks[order] = ((start + 1 + end) / 2.0)[group]
    return ranks


def pearsonr(a, b):
    """Pearson r in float64; NaN when a side has fewer than 2 entries or no variance."""
    a, b = _pair_of_vectors(a, b)
    if a.size < 2:
        return float("nan")
    a, b = a - a.mean(), b - b.mean()
    den = float(np.sqrt((a * a).sum() * (b * b).sum()))
    return float((a * b).sum()) / den if den > 0 else float("nan")


def spearmanr(a, b):
    """Spearman's rank correlation: Pearson r of the average ranks. NaN as pearsonr."""
    a, b = _pair_of_vectors(a, b)
    if a.size < 2:
        return float("nan")
    return pearsonr(rank_average(a), rank_average(b))


# ------------------------------------------------------------------------------------------------------- the scan ----
def _strands(strands):
    if strands not in ("both", "forward"):
        raise ValueError(f"strands = {strands!r}: expected 'both' or 'forward'")
    return strands == "both"


def _mset(mset):
    if not isinstance(mset, MotifSet):
        raise ValueError(f"mset must be a MotifSet (MotifSet.from_pfms, load_meme), got {type(mset).__name__}")
    return mset


def _scan_args(x, mset, strands, chunk_rows):
    both, rows = _strands(strands), _chunk_rows(chunk_rows, SCAN_CHUNK_ROWS)
    _mset(mset)
    x = _checked(x, "x", 3)
    if x.shape[1] > ops.PACK_MAX_L:
        raise ValueError(f"L = {x.shape[1]} > {ops.PACK_MAX_L}")
    x = _on_device(x, "x")
    return x, mset.to_device(x.device), both, rows


def scan_counts(x, mset, strands="both", chunk_rows=None):
    """-> {"hits": i64 [M], "rows_hit": i64 [M], "rows": N} on the device: per motif the windows at or above its threshold (the
    strands count separately) and the rows with at least one. chunk_rows: rows per pack + scan (every value gives the same
    integers)."""
    x, tables, both, rows = _scan_args(x, mset, strands, chunk_rows)
    N, L = x.shape
    hits = torch.zeros(len(mset), dtype=torch.int64, device=x.device)
    rows_hit = torch.zeros_like(hits)
    err = torch.zeros(1, dtype=torch.int32, device=x.device)
    for r0 in range(0, N, rows):
        ops.motif_scan(ops.pack_tokens(x[r0:r0 + rows], err=err), L, tables, both, hits=hits, rows_hit=rows_hit)
    ops.check_pack_err(err)
    return {"hits": hits, "rows_hit": rows_hit, "rows": N}


def scan_rows(x, mset, strands="both", chunk_rows=None):
    """-> (row_hits i32 [N, M], best_score i32 [N, M], best_start i32 [N, M], best_strand i8 [N, M]) on the device: a row's hits of
    every motif and its best window (highest score; then the lowest start; then forward, strand 0, before reverse, strand 1).
    L < width: no window, (0, INT32_MIN, -1, -1)."""
    x, tables, both, rows = _scan_args(x, mset, strands, chunk_rows)
    N, L = x.shape
    row_hits = torch.empty((N, len(mset)), dtype=torch.int32, device=x.device)
    row_best = torch.empty((N, len(mset)), dtype=torch.int64, device=x.device)
    err = torch.zeros(1, dtype=torch.int32, device=x.device)
    for r0 in range(0, N, rows):
        ops.motif_scan(ops.pack_tokens(x[r0:r0 + rows], err=err), L, tables, both, row_hits=row_hits[r0:r0 + rows],
                       row_best=row_best[r0:r0 + rows])
    ops.check_pack_err(err)
    return (row_hits,) + ops.motif_best_decode(row_best)


def consensus_patterns(mset, names=None):
    """-> a list of uint8 token arrays, one per motif of `names` (None: every motif, in the set's order): the highest log-odds base
    of each of the motif's `width` columns, the lowest base among equal entries. A consensus scores the motif's max_score on the
    forward strand, so Diffusion.evolve_patterns(x, consensus_patterns(mset, ["HNF1A"]), ...) implants sites scan_rows finds.
    No device."""
    _mset(mset)
    if names is None:
        idx = range(len(mset))
    else:
        if isinstance(names, str):
            names = [names]
        missing = [n for n in names if n not in mset.names]
        if missing:
            raise ValueError(f"consensus_patterns: no motif named {missing} in the set")
        idx = [mset.names.index(n) for n in names]
    return [mset.pwm[m, :int(mset.width[m])].argmax(1).astype(np.uint8) for m in idx]      # argmax: the first among equals


def _per(per):
    if per not in ("row", "site"):
        raise ValueError(f"per = {per!r}: expected 'row' or 'site'")
    return "rows_hit" if per == "row" else "hits"


def motif_frequencies(x, mset, per="row", strands="both"):
    """float64 [M] on the host: per = "row": the share of rows with at least one hit of the motif; "site": hits per row."""
    key = _per(per)
    c = scan_counts(x, mset, strands)
    return c[key].cpu().numpy().astype(np.float64) / c["rows"]


def _ref_frequencies(ref, mset, per, strands, name="ref"):
    """ref: tokens [N', L'] or a ready frequency vector [M] -> float64 [M]."""
    if getattr(ref, "ndim", 0) == 1:
        f = _vec(ref)
        if f.size != len(mset) or (isinstance(ref, torch.Tensor) and not ref.dtype.is_floating_point) \
                or (isinstance(ref, np.ndarray) and ref.dtype.kind != "f"):
            raise ValueError(f"{name}: a frequency vector must hold M = {len(mset)} floats, got {tuple(ref.shape)} {ref.dtype}")
        return f
    return motif_frequencies(ref, mset, per, strands)


_CORR = {"spearman": spearmanr, "pearson": pearsonr}


def motif_corr(x, ref, mset, method="spearman", per="row", strands="both"):
    """Correlation over all M motifs of the motif frequencies of x and of ref (tokens [N', L'] or a ready frequency vector [M]).
    NaN when M < 2 or a side has no variance."""
    if method not in _CORR:
        raise ValueError(f"method = {method!r}: expected 'spearman' or 'pearson'")
    _per(per), _strands(strands), _mset(mset)
    return _CORR[method](motif_frequencies(x, mset, per, strands), _ref_frequencies(ref, mset, per, strands))


def motif_report(x, mset, refs=None):
    """The flat dict of BaseModel.evaluate_motifs: motif_spearman_<name> for every set of refs {name: tokens or frequencies [M]}
    (per row, both strands), motifs_per_row_mean (hits per design) and motifs_reachable."""
    c = scan_counts(x, _mset(mset))
    freq = c["rows_hit"].cpu().numpy().astype(np.float64) / c["rows"]
    out = {f"motif_spearman_{name}": spearmanr(freq, _ref_frequencies(ref, mset, "row", "both", name)) for name, ref in (refs or {}).items()}
    out["motifs_per_row_mean"] = int(c["hits"].sum()) / c["rows"]
    out["motifs_reachable"] = int(mset.reachable.sum())
    return out


# ------------------------------------------------------------------------------------- motif-guided decoding (4m) ----
REWARD_CHUNK_ROWS = 1 << 18              # rows per svdd_motif_reward launch of MotifReward.term (any value gives the same bits)
_I32 = np.iinfo(np.int32)
TERM_BOUND = 1 << 62                     # the host keeps sum_m (|hit_coef| hit_cap + |margin_coef| margin_floor) below it: T fits int64


def _per_motif(value, mset, name, default, missing):
    """None -> default; a number -> that number for every motif; [M] values; a {motif name: value} dict (the other motifs get
    `missing`) -> float64 / int64 [M] as `default` is."""
    M = len(mset)
    default = np.asarray(default)
    if value is None:
        return default.copy()
    if isinstance(value, dict):
        unknown = [k for k in value if k not in mset.names]
        if unknown:
            raise ValueError(f"{name}: no motif named {unknown[0]!r} (the set has {', '.join(mset.names[:8])}{' ...' if M > 8 else ''})")
        rest = np.broadcast_to(missing, (M,))
        value = [value.get(n, rest[m]) for m, n in enumerate(mset.names)]
    a = np.asarray(value)
    if a.dtype.kind not in "iuf" or a.ndim > 1 or (a.ndim == 1 and a.size != M):
        raise ValueError(f"{name}: expected a number, M = {M} numbers or a {{name: value}} dict, got {value!r}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{name}: a non-finite value")
    if default.dtype.kind == "i":
        if a.dtype.kind == "f" and np.any(a != np.rint(a)):
            raise ValueError(f"{name}: expected integers, got {value!r}")
        if np.any(a < 0) or np.any(a > _I32.max):
            raise ValueError(f"{name}: expected values in 0 .. {_I32.max}, got {value!r}")
    return np.broadcast_to(a, (M,)).astype(default.dtype)


class MotifReward:
    """A motif objective for SVDD-PM decoding: per finished row the integer term of svdd_motif_reward
        T = sum_m [hit_coef_m min(hits_m, hit_cap_m) + margin_coef_m max(min(best_m - threshold_m, 0), -margin_floor_m)]
    times `unit`. hit_weight / margin_weight: per motif a float (a number, M numbers, or a {name: value} dict whose unnamed motifs
    get 0; None = all 0), quantised to hit_coef / margin_coef = round(weight / unit) int32. A hit weight is the reward of one hit,
    up to hit_cap of them (negative: a penalty); a margin weight is the reward per score unit by which the row's best window
    falls short of the threshold (0 once a window reaches it), cut off at margin_floor score units (default: the threshold minus
    the motif's lowest reachable score, i.e. never cut off). hit_cap / margin_floor: a number, M numbers or a dict (unnamed
    motifs keep the default)."""

    def __init__(self, mset, hit_weight=None, margin_weight=None, hit_cap=1, margin_floor=None, unit=2 ** -10, strands="both"):
        self.mset = _mset(mset)
        self.both = _strands(strands)
        self.strands = strands
        if isinstance(unit, bool) or not isinstance(unit, (int, float)) or not 0.0 < float(unit) < float("inf"):
            raise ValueError(f"unit = {unit!r}: expected a positive finite number")
        self.unit = float(np.float32(unit))
        if self.unit != float(unit):                                 # (an underflow to 0 included)
            raise ValueError(f"unit = {unit!r}: expected a number fp32 holds exactly (a power of two, say)")
        M = len(mset)
        zeros = np.zeros(M, np.float64)
        self.hit_coef = self._quantise(_per_motif(hit_weight, mset, "hit_weight", zeros, 0.0), "hit_weight")
        self.margin_coef = self._quantise(_per_motif(margin_weight, mset, "margin_weight", zeros, 0.0), "margin_weight")
        self.hit_cap = _per_motif(hit_cap, mset, "hit_cap", np.ones(M, np.int64), 1).astype(np.int32)
        floor = np.maximum(mset.threshold.astype(np.int64) - mset.min_score.astype(np.int64), 0)
        if np.any(floor > _I32.max):
            raise ValueError("margin_floor: a threshold lies more than 2^31 - 1 above its motif's lowest score")
        self.margin_floor = _per_motif(margin_floor, mset, "margin_floor", floor, floor).astype(np.int32)
        self.bound = sum(abs(int(h)) * int(c) + abs(int(g)) * int(f)
                         for h, c, g, f in zip(self.hit_coef, self.hit_cap, self.margin_coef, self.margin_floor))
        if self.bound >= TERM_BOUND:
            raise ValueError(f"the term can reach {self.bound} >= 2^62 in magnitude: lower the weights, hit_cap or margin_floor, or raise unit")
        self._dev = {}

    def _quantise(self, w, name):
        q = np.rint(w / self.unit)
        if np.any(np.abs(q) > _I32.max):
            raise ValueError(f"{name}: round(weight / unit) leaves int32 ({q[np.argmax(np.abs(q))]:.0f}); raise unit or lower the weight")
        return q.astype(np.int32)

    def __len__(self):
        return len(self.mset)

    def to_device(self, device="cuda"):
        """-> (ops.MotifTables, ops.MotifCoefs) on `device` (kept for the next call)."""
        tables = self.mset.to_device(device)
        device = tables.width.device
        if device not in self._dev:
            self._dev[device] = ops.MotifCoefs(*(torch.from_numpy(a).to(device)
                                                 for a in (self.hit_coef, self.hit_cap, self.margin_coef, self.margin_floor)))
        return tables, self._dev[device]

    def term_tokens(self, tok, count=None, base=None, out=None):
        """tok u8 [n, L] on the device (finished rows) -> fp32 [n]: base + T unit (base fp32 [n] or None = 0; out may be base). count:
        int32 device tensor [1], the rows beyond count[0] are neither read nor written. One launch, nothing crosses to the host."""
        if not isinstance(tok, torch.Tensor) or not tok.is_cuda:
            raise ops.SvddError("tok must be a GPU tensor (the SVDD hot path has no CPU fallback)")
        tables, coefs = self.to_device(tok.device)
        return ops.motif_reward(tok, tables, coefs, self.unit, count=count, base=base, out=out, both_strands=self.both)[0]

    def term(self, x, chunk_rows=None, return_int=False):
        """Any [N, L] token array (tokens 0..3, L <= 1024) -> T unit as fp32 [N] on the device, in chunks of chunk_rows rows (every
        value gives the same bits). return_int: (that, T int64 [N])."""
        rows = _chunk_rows(chunk_rows, REWARD_CHUNK_ROWS)
        x = _checked(x, "x", 3)
        if x.shape[1] > ops.PACK_MAX_L:
            raise ValueError(f"L = {x.shape[1]} > {ops.PACK_MAX_L}")
        x = _on_device(x, "x")
        tables, coefs = self.to_device(x.device)
        N = x.shape[0]
        out = torch.empty(N, dtype=torch.float32, device=x.device)
        T = torch.empty(N, dtype=torch.int64, device=x.device) if return_int else None
        err = torch.zeros(1, dtype=torch.int32, device=x.device)
        for r0 in range(0, N, rows):
            ops.motif_reward(x[r0:r0 + rows], tables, coefs, self.unit, out=out[r0:r0 + rows], term=None if T is None else T[r0:r0 + rows],
                             err=err, both_strands=self.both)
        ops.check_pack_err(err)
        return (out, T) if return_int else out


class GuidedReward:
    """reward_model (or None: base 0, a pure motif objective that needs no trained net) plus a MotifReward's term on task 0: what
    the samplers take as `reward_model` (Diffusion.controlled_sample_tweedie, controlled_sample_TDS). It has reward values, no
    gradient: the gradient samplers refuse it."""

    def __init__(self, reward_model, motif_reward):
        if not isinstance(motif_reward, MotifReward):
            raise ValueError(f"motif_reward must be a MotifReward, got {type(motif_reward).__name__}")
        if reward_model is not None and not callable(reward_model):
            raise ValueError(f"reward_model must be a reward model (a callable) or None, got {type(reward_model).__name__}")
        if isinstance(reward_model, GuidedReward):
            raise ValueError("reward_model is a GuidedReward already: give one MotifReward with all the weights")
        self.reward_model = reward_model
        self.motif_reward = motif_reward

    def __call__(self, onehot):
        """onehot fp32 [n, 4, L] (the reward models' layout) or [n, L, 4] -> [n, n_tasks, 1]; a zero (MASK) row raises."""
        if not isinstance(onehot, torch.Tensor) or onehot.dim() != 3 or 4 not in onehot.shape[1:]:
            raise ValueError(f"onehot must be a [n, 4, L] or [n, L, 4] tensor, got {tuple(getattr(onehot, 'shape', ()))}")
        if not onehot.is_cuda:
            raise ops.SvddError("onehot must be a GPU tensor (the SVDD hot path has no CPU fallback)")
        rows = onehot if onehot.shape[1] == 4 else onehot.transpose(1, 2)          # [n, 4, L]
        if bool((rows.sum(1) == 0).any()):
            raise ValueError("a row of onehot is zero (MASK): the motif term is defined for finished sequences (tokens 0..3)")
        term = self.motif_reward.term_tokens(rows.argmax(1).to(torch.uint8).contiguous())
        if self.reward_model is None:
            return term.view(-1, 1, 1)
        out = self.reward_model(onehot).float().clone()
        out[:, 0, 0] += term
        return out

    def forward_tokens(self, tok, count=None):
        """tok u8 [n, L] on the device -> [n, n_tasks, 1]; count as MotifReward.term_tokens (rows beyond it are undefined)."""
        n = tok.shape[0]
        if self.reward_model is None:
            return self.motif_reward.term_tokens(tok, count=count).view(n, 1, 1)
        if not hasattr(self.reward_model, "forward_tokens"):
            if count is not None:
                raise ops.SvddError("a compacted batch (count) needs a reward net with forward_tokens (the fused kernels)")
            return self(ops.transform_samples(tok, transposed=True))
        out = self.reward_model.forward_tokens(tok, count=count).float()
        if out.numel() == n and out.is_contiguous():
            flat = out.view(n)
            self.motif_reward.term_tokens(tok, count=count, base=flat, out=flat)
            return out.view(n, 1, 1)
        out = out.reshape(n, -1, 1).clone()
        out[:, 0, 0] = self.motif_reward.term_tokens(tok, count=count, base=out[:, 0, 0].contiguous())
        return out
