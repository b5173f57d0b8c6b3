"""-m gpu: the write contracts of the sampler core and of the row movers of exact work-skipping (svdd_kernels.hip).

tests/test_kernels_gpu.py and the primitives of tests/test_skip_gpu.py pin the VALUES of these kernels to the CPU oracle, on plain
torch.empty outputs: a store past the last row lands in the allocator's rounding, an element left unwritten reads back as whatever
was there, an optional output written although another one was passed goes unseen. Here every entry is called through the C ABI
with every output in a sentinel-filled buffer between two guards (tests/kernel_harness.py), twice:
  * both guards of every output intact; exactly the elements the header's contract names written (a NULL-able output that is not
    passed is not needed; one that is passed is fully written); the two launches bit-identical;
  * the values equal to the same references at the same bars as in tests/test_kernels_gpu.py / test_skip_gpu.py /
    test_classifier_gpu.py: tokens, indices, one-hots, counts, lists and the classifier step's q exact; q_xs, logp, soft within 1 ulp;
    the DPS pieces at the np.allclose bars of test_dps_kernels_vs_oracle;
at the smallest shapes that cross each boundary: below / at / above one 256-thread block and one 64-lane wave, the copy units 8, 4,
2 and 1 of the row gathers — reached through L AND through misaligned base pointers —, ragged last waves, both launch forms of
svdd_select, both copy paths of svdd_advance_rows, the 227-lane generations of the mt19937 kernel.
Every case prints one line: `CASE <entry> <shape and form> [<output> err <e> bar <b>]`."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import svdd_oracle as orc
from svdd_amd import _lib, ops
from tests.kernel_harness import DEV, GUARD, _Buf
from tests.test_classifier_cpu import guided_step

pytestmark = pytest.mark.gpu

U8, I32, I64, F64 = torch.uint8, torch.int32, torch.int64, torch.float64
GUARDS_ONLY = "guards only"                         # a scratch buffer: nothing is said about which of its elements are written


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    arch, _ = _lib.device_info()
    assert arch.startswith("gfx950"), arch


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ulp_diff(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max()) if a.size else 0


def case(entry, what, *errs):
    print(f"CASE {entry} {what}" + "".join(f" [{n} err {e} bar {b}]" for n, e, b in errs))


def run(name, entry, args_of, outs, written=None, init=None, call=_lib.call):
    """The steps of kernel_harness._twice with named, optional outputs. outs: {key: None (pass NULL) | numel | (numel, dtype[,
    offset])}; args_of(p), p[key] = the output's pointer or None -> the arguments of _lib.call(entry, ...). written[key]: True (the
    default: fully written) | False (untouched) | a bool tensor (exactly its True elements) | GUARDS_ONLY. init(bufs): fill in / out
    buffers. Two launches on fresh buffers, bit-identical. -> the first launch's {key: _Buf}. (call: the self-check's stand-in.)"""
    runs = []
    for _ in range(2):
        bufs = {k: (_Buf(*s) if isinstance(s, tuple) else _Buf(s)) for k, s in outs.items() if s is not None}
        if init is not None:
            init(bufs)
        call(entry, *args_of({k: (bufs[k].ptr if k in bufs else None) for k in outs}))
        torch.cuda.synchronize()
        for k, b in bufs.items():
            w = True if written is None else written.get(k, True)
            if isinstance(w, torch.Tensor):
                b.assert_written_where(f"{name} {k}", w)
            elif w is GUARDS_ONLY:
                b.untouched()
            elif w:
                b.assert_written(f"{name} {k}")
            else:
                b.assert_untouched(f"{name} {k}")
        runs.append(bufs)
    for k in runs[0]:
        assert torch.equal(runs[0][k].bits(), runs[1][k].bits()), f"{name} {k}: two launches differ"
    return runs[0]


def rand_case(rng, B, L, frac_unmasked=0.5, scale=2.0):
    """logits logical [B, L, 5], x u8 [B, L] with masked AND unmasked positions wherever there is room for both."""
    logits = (rng.standard_normal((B, L, 5)) * scale).astype(np.float32)
    x = np.where(rng.random((B, L)) < frac_unmasked, rng.integers(0, 4, (B, L)), 4).astype(np.uint8)
    x.flat[0] = 4
    if x.size > 1:
        x.flat[-1] = 1
    logits[0, : min(L, 4)] = 0.0                                    # exact ties between categories
    return logits, x


def in_layout(a, layout):
    """logical [.., L, 5] -> the array whose memory is the layout's image ([.., L, 5] or [.., 5, L])."""
    return np.ascontiguousarray(a if layout == orc.BLV else np.swapaxes(a, -1, -2))


def philox_u(seed, row_offset, step, B, L, M=1):
    u = np.empty((M, B, L, 5), np.float32)
    for m in range(M):
        for b in range(B):
            for l in range(L):
                u[m, b, l] = orc.philox_uniform5(seed, (row_offset + b) * L + l, step, m)
    return u


# ------------------------------------------------------------------------------------------ the method checks itself
def test_harness_assertions_raise_on_each_kind_of_violation():
    """No project kernel runs here: torch stores play the kernel that breaks its contract, on every kind of buffer this file uses
    (fp32 words, bytes at an offset, the words of int64 / fp64 values)."""
    for mk in (lambda: _Buf(8), lambda: _Buf(8, U8, 3), lambda: _Buf(8, I64), lambda: _Buf(8, F64)):
        b = mk()
        b.bits()[:] = 0
        b.assert_written("all written")
        b.raw[b.lo + 8] = 0                                 # the first guard word behind the body
        with pytest.raises(AssertionError, match="guard overwritten"):
            b.assert_written("a store past the end")
        b = mk()
        b.bits()[:] = 0
        b.raw[b.lo - 1] = 0                                         # the last guard word in front of it
        with pytest.raises(AssertionError, match="guard overwritten"):
            b.assert_written("a store in front of element 0")
        b = mk()
        b.bits()[:7] = 0                                    # the last element keeps the sentinel
        with pytest.raises(AssertionError, match="1 of 8 elements were never written"):
            b.assert_written("last element left out")
        mask = torch.arange(8) < 4
        with pytest.raises(AssertionError, match="elements were written that the contract says are not"):
            b.assert_written_where("three extra elements", mask)
        b = mk()
        b.bits()[:3] = 0
        with pytest.raises(AssertionError, match="1 of 4 elements the contract names were never written"):
            b.assert_written_where("one element short", mask)
        with pytest.raises(AssertionError, match="written although the contract says it is not"):
            b.assert_untouched("an optional output nobody passed")
        b = mk()
        b.assert_untouched("fresh")
        b.assert_written_where("nothing named, nothing written", torch.zeros(8, dtype=torch.bool))
    b = _Buf(8, U8, 3)
    assert b.ptr % 16 == 3 and b.ptr == b.raw.data_ptr() + GUARD + 3
    b = _Buf(2 * 5, I64)                                            # five int64 values = ten words
    b.body()[:] = torch.arange(5, device=DEV)
    assert b.body().dtype == I64 and b.cpu().tolist() == [0, 1, 2, 3, 4] and not bool(b.untouched().any())
    # run() itself, with torch stores in place of the launch: two launches that differ, an output left short, a store past a body
    nth = []

    def differs(name, ptr):
        nth.append(name)
        bufs_seen[-1]["o"].bits()[:] = len(nth)

    bufs_seen = []
    with pytest.raises(AssertionError, match="two launches differ"):
        run("self-check", "none", lambda p: (p["o"],), {"o": 4}, init=bufs_seen.append, call=differs)
    with pytest.raises(AssertionError, match="never written"):
        run("self-check", "none", lambda p: (p["o"],), {"o": 4}, call=lambda name, ptr: None)

    def overruns(name, ptr):
        b = bufs_seen[-1]["o"]
        b.raw[b.lo:b.lo + 5] = 0

    with pytest.raises(AssertionError, match="guard overwritten"):
        run("self-check", "none", lambda p: (p["o"],), {"o": 4}, init=bufs_seen.append, call=overruns)


# ------------------------------------------------------------------------------------------ K1: propose / sample_categorical
PROPOSE_SHAPES = [(1, 1, 1), (1, 7, 1), (3, 50, 5), (5, 64, 4), (2, 129, 13), (3, 77, 70)]
DM, MCS = np.float32(0.0078), np.float32(0.61)


def _propose_once(tag, lg_d, x_d, B, L, M, layout, r, want_q, ref):
    rs = r.c_struct(layout)
    outs = {"cand": (B * M * L, U8), "onehot": B * M * L * 4, "q_xs": B * L * 5 if want_q else None}
    got = run(tag, "svdd_propose", lambda p: (lg_d, x_d, float(DM), float(MCS), B, L, M, layout, ctypes.byref(rs), p["cand"],
                                              p["onehot"], p["q_xs"]), outs)
    c_ref, oh_ref, q_ref = ref
    assert np.array_equal(got["cand"].cpu(B, M, L).numpy(), c_ref), tag
    assert np.array_equal(got["onehot"].cpu(B * M, L, 4).numpy(), oh_ref), tag
    errs = ()
    if want_q:
        d = ulp_diff(got["q_xs"].cpu().numpy(), q_ref.reshape(-1))  # both in the layout's memory order
        errs = (("q_xs", f"{d} ulp", "1 ulp"),)
        case("svdd_propose", tag, *errs)
        assert d <= 1, tag
    else:
        case("svdd_propose", tag)
    return got


@pytest.mark.parametrize("B,L,M", PROPOSE_SHAPES)
@pytest.mark.parametrize("layout", [orc.BLV, orc.BVL])
def test_propose_writes_cand_and_onehot_everywhere_and_q_only_when_asked(B, L, M, layout):
    rng = np.random.default_rng(100 + B * L + M)
    logits, x = rand_case(rng, B, L)
    lg_np = in_layout(logits, layout)
    uni = in_layout(rng.random((M, B, L, 5), dtype=np.float32), layout)
    uni.flat[:3] = [0.0, (2 ** 24 - 1) / 2 ** 24, 2.0 ** -24]       # extremes of the 24-bit grid
    lg_d, x_d, uni_d = dev(lg_np), dev(x), dev(uni)
    for kind in ("replay", "philox"):
        if kind == "replay":
            r, ref = ops.Rng(uniforms=uni_d), orc.propose(lg_np, x, DM, MCS, M, uniforms=uni, layout=layout)
        else:
            r = ops.Rng(seed=2 ** 63 + 5, row_offset=1000, step=77)
            ref = orc.propose(lg_np, x, DM, MCS, M, seed=2 ** 63 + 5, row_offset=1000, step=77, layout=layout)
        for want_q in (False, True):
            _propose_once(f"B={B} L={L} M={M} layout={layout} {kind} q_xs={'given' if want_q else 'NULL'}", lg_d, x_d, B, L, M,
                          layout, r, want_q, ref)


@pytest.mark.parametrize("B,L,M", PROPOSE_SHAPES)
@pytest.mark.parametrize("layout", [orc.BLV, orc.BVL])
def test_sample_categorical_writes_cand_and_onehot_everywhere(B, L, M, layout):
    rng = np.random.default_rng(200 + B * L + M)
    _, x = rand_case(rng, B, L)
    q = (rng.random((B, L, 5)) * 0.01).astype(np.float32)
    q[..., 4] = 0.5
    q[0, :, :4] = 0.0                                               # zeros: ties at 0 among the losers
    q_np = in_layout(q, layout)
    seed, off, step = 3, 7, 1
    q_d, x_d = dev(q_np), dev(x)
    for kind in ("replay", "philox"):
        u = rng.random((M, B, L, 5), dtype=np.float32) if kind == "replay" else philox_u(seed, off, step, B, L, M)
        u_np = in_layout(u, layout)
        u_d = dev(u_np)
        r = ops.Rng(uniforms=u_d) if kind == "replay" else ops.Rng(seed=seed, row_offset=off, step=step)
        rs = r.c_struct(layout)
        c_ref = orc.sample_categorical_merged(q_np, x, u_np, layout=layout)
        tag = f"B={B} L={L} M={M} layout={layout} {kind}"
        got = run(tag, "svdd_sample_categorical", lambda p: (q_d, x_d, B, L, M, layout, ctypes.byref(rs), p["cand"], p["onehot"]),
                  {"cand": (B * M * L, U8), "onehot": B * M * L * 4})
        assert np.array_equal(got["cand"].cpu(B, M, L).numpy(), c_ref), tag
        assert np.array_equal(got["onehot"].cpu(B * M, L, 4).numpy(), orc.transform_samples(c_ref.reshape(B * M, L))), tag
        case("svdd_sample_categorical", tag)


@pytest.mark.parametrize("layout", [orc.BLV, orc.BVL])
def test_propose_sharded_replay_equals_its_rows_of_the_whole_batch(layout):
    """uniforms_rows = 8, row_offset = 4, B = 3: rows 4..6 of the 8-row call, output for output."""
    rng = np.random.default_rng(8)
    R, B, off, L, M = 8, 3, 4, 50, 5
    logits, x = rand_case(rng, R, L)
    lg_np = in_layout(logits, layout)
    uni = in_layout(rng.random((M, R, L, 5), dtype=np.float32), layout)
    uni_d = dev(uni)
    ref = orc.propose(lg_np, x, DM, MCS, M, uniforms=uni, layout=layout)
    whole = _propose_once(f"B={R} L={L} M={M} layout={layout} replay whole batch", dev(lg_np), dev(x), R, L, M, layout,
                          ops.Rng(uniforms=uni_d), True, ref)
    part_ref = (ref[0][off:off + B], ref[1][off * M:(off + B) * M], ref[2][off:off + B])
    part = _propose_once(f"B={B} L={L} M={M} layout={layout} replay uniforms_rows={R} row_offset={off}", dev(lg_np[off:off + B]),
                         dev(x[off:off + B]), B, L, M, layout, ops.Rng(uniforms=uni_d, uniforms_rows=R, row_offset=off), True, part_ref)
    assert torch.equal(part["cand"].body(), whole["cand"].body()[off * M * L:(off + B) * M * L])
    assert torch.equal(part["onehot"].bits(), whole["onehot"].bits()[off * M * L * 4:(off + B) * M * L * 4])
    assert torch.equal(part["q_xs"].bits(), whole["q_xs"].bits()[off * L * 5:(off + B) * L * 5])


@pytest.mark.parametrize("msplit", [3])
def test_propose_forced_candidate_split_keeps_the_contract(msplit):
    """M = 70 (more than one pass of the 64-row token table) with the candidates of a tile dealt to 3 waves instead of the host's
    choice: every (candidate, position) still written once, same tokens."""
    B, L, M, layout = 3, 77, 70, orc.BLV
    rng = np.random.default_rng(M)
    logits, x = rand_case(rng, B, L, frac_unmasked=0.4)
    uni = rng.random((M, B, L, 5), dtype=np.float32)
    uni_d = dev(uni)
    ref_r = orc.propose(logits, x, DM, MCS, M, uniforms=uni)
    ref_p = orc.propose(logits, x, DM, MCS, M, seed=11, row_offset=5, step=9)
    prev = _lib.set_option(_lib.OPT_MSPLIT, msplit)
    try:
        _propose_once(f"B={B} L={L} M={M} msplit={msplit} replay q_xs=given", dev(logits), dev(x), B, L, M, layout,
                      ops.Rng(uniforms=uni_d), True, ref_r)
        _propose_once(f"B={B} L={L} M={M} msplit={msplit} philox q_xs=NULL", dev(logits), dev(x), B, L, M, layout,
                      ops.Rng(seed=11, row_offset=5, step=9), False, ref_p)
    finally:
        _lib.set_option(_lib.OPT_MSPLIT, prev)


# ------------------------------------------------------------------------------------------ classifier guidance
@pytest.mark.parametrize("B,L", [(1, 7), (3, 129)])
@pytest.mark.parametrize("layout", [orc.BLV, orc.BVL])
@pytest.mark.parametrize("kind", ["replay", "philox"])
def test_classifier_propose_optional_outputs(B, L, layout, kind):
    rng = np.random.default_rng(5 + B + L + layout)
    dm, mcs, scale, seed, step, off = 0.0078125, 0.61, 3.0, 12345, 17, 5
    logits, x = rand_case(rng, B, L, frac_unmasked=0.4)
    grad = (rng.standard_normal((B, L, 4)) * 0.01).astype(np.float32)      # scale * g >> q: many negative weights
    u = rng.random((B, L, 5), dtype=np.float32) if kind == "replay" else philox_u(seed, off, step, B, L)[0]
    u_d = dev(in_layout(u, layout))
    r = ops.Rng(uniforms=u_d) if kind == "replay" else ops.Rng(seed=seed, row_offset=off, step=step)
    rs = r.c_struct(layout)
    lg_d, x_d, g_d = dev(in_layout(logits, layout)), dev(x), dev(grad)
    want_x, want_q, _ = guided_step(logits, x, grad, dm, mcs, scale, u)
    for want_oh in (False, True):
        for want_q_out in (False, True):
            tag = f"B={B} L={L} layout={layout} {kind} onehot_next={'given' if want_oh else 'NULL'} q_xs={'given' if want_q_out else 'NULL'}"
            got = run(tag, "svdd_classifier_propose",
                      lambda p: (lg_d, layout, x_d, g_d, dm, mcs, scale, B, L, ctypes.byref(rs), p["x_next"], p["onehot"], p["q_xs"]),
                      {"x_next": (B * L, U8), "onehot": B * L * 4 if want_oh else None, "q_xs": B * L * 5 if want_q_out else None})
            assert np.array_equal(got["x_next"].cpu(B, L).numpy(), want_x), tag
            if want_oh:
                assert np.array_equal(got["onehot"].cpu(B, L, 4).numpy(), orc.transform_samples(want_x)), tag
            if want_q_out:                                          # exact, as in tests/test_classifier_gpu.py
                assert np.array_equal(got["q_xs"].cpu().numpy(), in_layout(want_q, layout).reshape(-1)), tag
                case("svdd_classifier_propose", tag, ("q_xs", f"{ulp_diff(got['q_xs'].cpu().numpy(), in_layout(want_q, layout).reshape(-1))} ulp", "0 ulp"))
            else:
                case("svdd_classifier_propose", tag)


# ------------------------------------------------------------------------------------------ K2: select / select_compact
SELECT_SHAPES = [(1, 1, 200), (5, 3, 7), (67, 10, 200), (67, 20, 36), (37, 64, 50), (5, 65, 200), (261, 10, 50)]
SELECT_FORMS = {1: "one row per wave", 3: "one row group per wave", 2: "four row groups per wave"}
SEL_RNG = dict(seed=11, row_offset=5, step=9)


def _select_scores(rng, B, M):
    s = (rng.standard_normal((B, M)) * 0.3).astype(np.float32)
    if B > 1:
        s[1] = 0.25                                                 # all tied -> first index
    if B > 2 and M > 2:
        s[2, M - 1] = s[2, 1] = s[2].max() + 1.0                    # exact tie -> lower index
    if B > 3:
        s[3] = np.float32(0.1) + (rng.integers(0, 3, M) * 2.0 ** -27).astype(np.float32)      # ulp near-ties: the exact path
    if B > 4:
        s[4] *= 100.0
    s[B - 1] = (rng.standard_normal(M) * 1e-7).astype(np.float32) + np.float32(0.01)          # near-uniform, in the ragged last wave
    return s


def _select_args(sc_d, cand_ptr, B, L, M, mode, rs):
    return lambda p: (sc_d, cand_ptr, B, L, M, mode, ctypes.byref(rs), p["x_next"], p["soft"], p["idx"])


@pytest.mark.parametrize("B,M,L", SELECT_SHAPES)
@pytest.mark.parametrize("one_row", [1, 3, 2])
def test_select_optional_outputs_in_every_launch_form(B, M, L, one_row):
    rng = np.random.default_rng(1000 * M + L + B)
    scores, cand = _select_scores(rng, B, M), rng.integers(0, 5, (B, M, L)).astype(np.uint8)
    sc_d, cand_d = dev(scores), dev(cand)
    rs = ops.Rng(**SEL_RNG).c_struct()
    prev = _lib.set_option(_lib.OPT_SELECT_ONE_ROW, one_row)
    try:
        for mode in (ops.SELECT_ARGMAX, ops.SELECT_MULTINOMIAL):
            x_ref, soft_ref, idx_ref = orc.select(scores, cand, mode=mode, **SEL_RNG)
            forms = [(True, True, True), (True, False, True), (True, True, False), (True, False, False)]
            if M <= 64 and one_row != 1:
                forms += [(False, False, True), (False, True, True)]        # the decision only: x_next NULL with idx
            for want_x, want_soft, want_idx in forms:
                tag = (f"B={B} M={M} L={L} {SELECT_FORMS[one_row]} mode={mode} x_next={'given' if want_x else 'NULL'} "
                       f"soft={'given' if want_soft else 'NULL'} idx={'given' if want_idx else 'NULL'}")
                got = run(tag, "svdd_select", _select_args(sc_d, cand_d, B, L, M, mode, rs),
                          {"x_next": (B * L, U8) if want_x else None, "soft": B * M if want_soft else None,
                           "idx": (B, I32) if want_idx else None})
                if want_x:
                    assert np.array_equal(got["x_next"].cpu(B, L).numpy(), x_ref), tag
                if want_idx:
                    assert np.array_equal(got["idx"].cpu().numpy(), idx_ref), tag
                if want_soft:
                    d = ulp_diff(got["soft"].cpu(B, M).numpy(), soft_ref)
                    case("svdd_select", tag, ("soft", f"{d} ulp", "1 ulp"))
                    assert d <= 1, tag
                else:
                    case("svdd_select", tag)
    finally:
        _lib.set_option(_lib.OPT_SELECT_ONE_ROW, prev)


@pytest.mark.parametrize("B,M,L", SELECT_SHAPES)
@pytest.mark.parametrize("one_row", [1, 3, 2])
def test_select_compact_writes_every_row_and_reads_no_score_beyond_count(B, M, L, one_row):
    """The compacted form: a slot map with one row of copies only (all -1), NaN in `scores` beyond the live count; x_next, idx,
    sel_score and changed against the dense restatement of test_select_compact_equals_select_on_dense_scores, here with the oracle
    as the dense select."""
    rng = np.random.default_rng(77 * M + L + B)
    cand = rng.integers(0, 5, (B, M, L)).astype(np.uint8)
    flags = (rng.random((B, M)) < 0.7)
    flags[B // 2] = False                                           # a row whose candidates are all copies of the parent
    live = np.flatnonzero(flags.reshape(-1))
    k = live.size
    slot = np.full(B * M, -1, np.int32)
    slot[live] = np.arange(k, dtype=np.int32)
    sc = np.full(B * M, np.nan, np.float32)                         # beyond count: must never be read
    sc[:k] = _select_scores(rng, B, M).reshape(-1)[:k]
    parent = (rng.standard_normal(B) * 0.3).astype(np.float32)
    dense = np.where(slot >= 0, sc[np.maximum(slot, 0)], np.repeat(parent, M)).reshape(B, M).astype(np.float32)
    sc_d, slot_d, par_d, cand_d = dev(sc), dev(slot), dev(parent), dev(cand)
    rs = ops.Rng(**SEL_RNG).c_struct()
    prev = _lib.set_option(_lib.OPT_SELECT_ONE_ROW, one_row)
    try:
        for mode in (ops.SELECT_ARGMAX, ops.SELECT_MULTINOMIAL):
            x_ref, soft_ref, idx_ref = orc.select(dense, cand, mode=mode, **SEL_RNG)
            for want_soft, want_idx, want_rest in [(False, True, True), (True, True, True), (False, False, True), (True, True, False)]:
                tag = (f"B={B} M={M} L={L} {SELECT_FORMS[one_row]} mode={mode} live={k} soft={'given' if want_soft else 'NULL'} "
                       f"idx={'given' if want_idx else 'NULL'} sel_score/changed={'given' if want_rest else 'NULL'}")
                got = run(tag, "svdd_select_compact",
                          lambda p: (sc_d, slot_d, par_d, cand_d, B, L, M, mode, ctypes.byref(rs), p["x_next"], p["soft"], p["idx"],
                                     p["sel_score"], p["changed"]),
                          {"x_next": (B * L, U8), "soft": B * M if want_soft else None, "idx": (B, I32) if want_idx else None,
                           "sel_score": B if want_rest else None, "changed": (B, I32) if want_rest else None})
                assert np.array_equal(got["x_next"].cpu(B, L).numpy(), x_ref), tag
                if want_idx:
                    assert np.array_equal(got["idx"].cpu().numpy(), idx_ref), tag
                if want_rest:
                    assert np.array_equal(got["sel_score"].cpu().numpy(), dense[np.arange(B), idx_ref]), tag
                    assert np.array_equal(got["changed"].cpu().numpy() != 0, flags[np.arange(B), idx_ref]), tag
                    assert set(got["changed"].cpu().tolist()) <= {0, 1}
                if want_soft:
                    d = ulp_diff(got["soft"].cpu(B, M).numpy(), soft_ref)
                    case("svdd_select_compact", tag, ("soft", f"{d} ulp", "1 ulp"))
                    assert d <= 1, tag
                else:
                    case("svdd_select_compact", tag)
    finally:
        _lib.set_option(_lib.OPT_SELECT_ONE_ROW, prev)


@pytest.mark.parametrize("one_row", [1, 3, 2])
def test_select_takes_its_copy_unit_from_the_pointers(one_row):
    """L = 200 divides by 8; cand or x_next 4, 2, 1 bytes off an aligned address leaves a 4-, 2-, 1-byte unit. Both select kernels
    derive the unit from L | row stride | cand | x_next, so every access stays aligned to its unit; tokens and indices are the
    aligned call's, and the misaligned x_next keeps its guards to the byte."""
    B, M, L = 67, 10, 200
    rng = np.random.default_rng(5)
    scores, cand = _select_scores(rng, B, M), rng.integers(0, 5, (B, M, L)).astype(np.uint8)
    sc_d = dev(scores)
    room = torch.zeros(B * M * L + 16, dtype=U8, device=DEV)
    assert room.data_ptr() % 16 == 0
    rs = ops.Rng(**SEL_RNG).c_struct()
    x_ref, _, idx_ref = orc.select(scores, cand)
    prev = _lib.set_option(_lib.OPT_SELECT_ONE_ROW, one_row)
    try:
        for off_c, off_x in [(0, 0), (1, 0), (2, 0), (4, 0), (0, 1), (0, 2), (0, 4), (4, 2)]:
            room.zero_()
            view = room[off_c:off_c + B * M * L]
            view.copy_(dev(cand).reshape(-1))
            tag = f"B={B} M={M} L={L} {SELECT_FORMS[one_row]} cand+{off_c} x_next+{off_x}"
            got = run(tag, "svdd_select", _select_args(sc_d, view.data_ptr(), B, L, M, ops.SELECT_ARGMAX, rs),
                      {"x_next": (B * L, U8, off_x), "soft": None, "idx": (B, I32)})
            assert got["x_next"].ptr % 8 == off_x and view.data_ptr() % 8 == off_c
            assert np.array_equal(got["x_next"].cpu(B, L).numpy(), x_ref), tag
            assert np.array_equal(got["idx"].cpu().numpy(), idx_ref), tag
            case("svdd_select", tag)
    finally:
        _lib.set_option(_lib.OPT_SELECT_ONE_ROW, prev)


def test_select_row_gather_at_the_largest_row_the_host_admits():
    """M = 1: a wave owns 64 rows and the gather's unit index runs up to 64 L / 8. L = 8 * 65535 is the longest row whose index
    stays below the 2^22 the float reciprocal is exact for (tests/test_sampler_contracts_cpu.py): 64 full rows and one ragged
    wave, every byte of x_next the candidate's, guards intact. Eight bytes more are refused."""
    B, M, L = 65, 1, 8 * 65535
    g = torch.Generator(device=DEV).manual_seed(1)
    cand = torch.randint(0, 5, (B, M, L), device=DEV, dtype=U8, generator=g)
    scores = torch.zeros(B, M, device=DEV)
    got = run(f"B={B} M={M} L={L}", "svdd_select", lambda p: (scores, cand, B, L, M, ops.SELECT_ARGMAX, None, p["x_next"], None, p["idx"]),
              {"x_next": (B * L, U8), "idx": (B, I32)})
    assert torch.equal(got["x_next"].body(), cand.reshape(-1))
    assert not bool(got["idx"].body().any())
    case("svdd_select", f"B={B} M={M} L={L} units per wave {64 * L // 8} < 2^22")
    out = torch.empty(B * (L + 8), dtype=U8, device=DEV)
    with pytest.raises(_lib.SvddError, match="svdd_select: invalid argument"):
        _lib.call("svdd_select", scores, torch.empty(B * (L + 8), dtype=U8, device=DEV), B, L + 8, M, ops.SELECT_ARGMAX, None, out, None, None)


# ------------------------------------------------------------------------------------------ the per-position kernels
POS_SHAPES = [(1, 1), (1, 7), (3, 85), (1, 256), (1, 257), (9, 200)]     # below, at and above one 256-thread block
DPS_BARS = {"probs4": (2e-6, 1e-7), "dlogits": (1e-5, 1e-9), "direct": (1e-5, 1e-9), "q": (2e-6, 1e-12)}   # test_dps_kernels_vs_oracle's


def _allclose_err(got, ref, rtol, atol):
    """-> (max of |got - ref| / (atol + rtol |ref|): <= 1 is np.allclose, max |got - ref|)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    d = np.abs(got - ref)
    return float((d / (atol + rtol * np.abs(ref))).max()), float(d.max())


@pytest.mark.parametrize("R,L", POS_SHAPES)
@pytest.mark.parametrize("layout", [orc.BLV, orc.BVL])
def test_pointwise_kernels_each_optional_output_alone_and_together(R, L, layout):
    rng = np.random.default_rng(21 + R * L)
    logits, x = rand_case(rng, R, L)
    logits[0, : min(L, 8), :4] = 1.5                                # ties among the 4 real tokens
    lg_np = in_layout(logits, layout)
    lg_d, x_d = dev(lg_np), dev(x)
    shape = f"R={R} L={L} layout={layout}"
    oh_ref, xh_ref = orc.x0hat(lg_np, x, layout=layout)
    for want_oh, want_tok in [(True, False), (False, True), (True, True)]:
        tag = f"{shape} onehot_t={'given' if want_oh else 'NULL'} x0hat={'given' if want_tok else 'NULL'}"
        got = run(tag, "svdd_x0hat", lambda p: (lg_d, x_d, R, L, layout, p["onehot_t"], p["x0hat"]),
                  {"onehot_t": R * 4 * L if want_oh else None, "x0hat": (R * L, U8) if want_tok else None})
        if want_oh:
            assert np.array_equal(got["onehot_t"].cpu(R, 4, L).numpy(), oh_ref), tag
        if want_tok:
            assert np.array_equal(got["x0hat"].cpu(R, L).numpy(), xh_ref), tag
        case("svdd_x0hat", tag)
    fin_ref = orc.finalize(lg_np, x, layout=layout)
    for want_64, want_8 in [(True, False), (False, True), (True, True)]:
        tag = f"{shape} out_i64={'given' if want_64 else 'NULL'} out_u8={'given' if want_8 else 'NULL'}"
        got = run(tag, "svdd_finalize", lambda p: (lg_d, x_d, R, L, layout, p["out_i64"], p["out_u8"]),
                  {"out_i64": (2 * R * L, I64) if want_64 else None, "out_u8": (R * L, U8) if want_8 else None})
        if want_64:
            assert np.array_equal(got["out_i64"].cpu(R, L).numpy(), fin_ref), tag
        if want_8:
            assert np.array_equal(got["out_u8"].cpu(R, L).numpy(), fin_ref.astype(np.uint8)), tag
        case("svdd_finalize", tag)
    got = run(shape, "svdd_subs_logp", lambda p: (lg_d, x_d, R, L, layout, p["logp"]), {"logp": R * L * 5})
    d = ulp_diff(got["logp"].cpu().numpy(), orc.subs_logp(lg_np, x, layout=layout).reshape(-1))
    case("svdd_subs_logp", shape, ("logp", f"{d} ulp", "1 ulp"))
    assert d <= 1
    if layout == orc.BLV:                                           # the entries without a layout parameter: once
        for tr in (0, 1):
            tag = f"R={R} L={L} transposed={tr}"
            got = run(tag, "svdd_transform_samples", lambda p: (x_d, R, L, tr, p["out"]), {"out": R * L * 4})
            assert np.array_equal(got["out"].cpu(*((R, 4, L) if tr else (R, L, 4))).numpy(), orc.transform_samples(x, transposed=bool(tr))), tag
            case("svdd_transform_samples", tag)
        shape = f"B={R} L={L}"
        got = run(shape, "svdd_dps_probs", lambda p: (lg_d, x_d, R, L, p["probs4"]), {"probs4": R * L * 4})
        e, a = _allclose_err(got["probs4"].cpu(R, L, 4).numpy(), orc.dps_probs(logits, x), *DPS_BARS["probs4"])
        case("svdd_dps_probs", shape, ("probs4", f"{a:.2e} = {e:.3f} of it", "rtol 2e-6 atol 1e-7"))
        assert e <= 1.0
        dp = (rng.standard_normal((R, L, 4)) * 1e-3).astype(np.float32)
        dp_d = dev(dp)
        got = run(shape, "svdd_dps_probs_bwd", lambda p: (lg_d, x_d, dp_d, R, L, p["dlogits"], p["direct"]),
                  {"dlogits": R * L * 5, "direct": R * L * 5})
        wl, wr = orc.dps_probs_bwd(logits, x, dp)
        gl, gr = got["dlogits"].cpu(R, L, 5).numpy(), got["direct"].cpu(R, L, 5).numpy()
        (el, al), (er, ar) = _allclose_err(gl, wl, *DPS_BARS["dlogits"]), _allclose_err(gr, wr, *DPS_BARS["direct"])
        case("svdd_dps_probs_bwd", shape, ("dlogits", f"{al:.2e} = {el:.3f} of it", "rtol 1e-5 atol 1e-9"),
             ("direct", f"{ar:.2e} = {er:.3f} of it", "rtol 1e-5 atol 1e-9"))
        assert el <= 1.0 and er <= 1.0
        assert not gl[x != 4].any() and not gr[x == 4].any()        # each position feeds exactly one of the two paths, the other gets zeros
        ga, gb = ((rng.standard_normal((R, L, 5)) * 1e-4).astype(np.float32) for _ in range(2))
        ga_d, gb_d = dev(ga), dev(gb)
        for scale in (0.0, 300.0):
            tag = f"{shape} scale={scale}"
            got = run(tag, "svdd_dps_guided_q", lambda p: (lg_d, x_d, ga_d, gb_d, 0.0078, 0.31, scale, R, L, p["q"]), {"q": R * L * 5})
            e, a = _allclose_err(got["q"].cpu(R, L, 5).numpy(), orc.dps_guided_q(logits, x, ga + gb, 0.0078, 0.31, scale), *DPS_BARS["q"])
            case("svdd_dps_guided_q", tag, ("q", f"{a:.2e} = {e:.3f} of it", "rtol 2e-6 atol 1e-12"))
            assert e <= 1.0


# ------------------------------------------------------------------------------------------ K4: TDS resampling
def _tds_inputs(B, L):
    rng = np.random.default_rng(B)
    num, den = rng.standard_normal(B).astype(np.float32), rng.standard_normal(B).astype(np.float32)
    sample = rng.integers(0, 5, (B, L)).astype(np.uint8)
    u = rng.random(B)
    u[0] = 0.0
    return num, den, sample, u


@pytest.mark.parametrize("B,L", [(1, 200), (63, 50), (65, 7), (130, 36), (257, 200)])
def test_tds_resample_outputs_and_scratch_stay_inside_their_buffers(B, L):
    num, den, sample, u = _tds_inputs(B, L)
    x_ref, idx_ref, _, _ = orc.tds_resample(num, den, 0.5, sample, u)
    num_d, den_d, u_d = dev(num), dev(den), dev(u)
    room = torch.zeros(B * L + 16, dtype=U8, device=DEV)
    offsets = [(0, 0)] + ([(1, 0), (2, 0), (4, 0), (0, 1), (0, 2), (0, 4)] if L == 200 else [])
    for off_s, off_x in offsets:
        room.zero_()
        view = room[off_s:off_s + B * L]
        view.copy_(dev(sample).reshape(-1))
        for want_idx in (True, False):
            tag = f"B={B} L={L} sample+{off_s} x_next+{off_x} idx={'given' if want_idx else 'NULL'}"
            got = run(tag, "svdd_tds_resample",
                      lambda p: (num_d, den_d, 0.5, view.data_ptr(), u_d, B, L, p["x_next"], p["idx"], p["work"]),
                      {"x_next": (B * L, U8, off_x), "idx": (B, I32) if want_idx else None, "work": (2 * 2 * B, F64)},
                      written={"work": GUARDS_ONLY})
            assert np.array_equal(got["x_next"].cpu(B, L).numpy(), x_ref), tag
            if want_idx:
                assert np.array_equal(got["idx"].cpu().numpy(), idx_ref), tag
            case("svdd_tds_resample", tag)


# ------------------------------------------------------------------------------------------ the compactions
COMPACT_N = [1, 63, 64, 1023, 1024, 1025, 2560]


@pytest.mark.parametrize("n", COMPACT_N)
@pytest.mark.parametrize("p", [0.0, 0.3, 1.0])
def test_compact_flags_writes_the_list_up_to_count_only(n, p):
    g = torch.Generator(device=DEV).manual_seed(n)
    flags = (torch.rand(n, device=DEV, generator=g) < p).to(I32) * 7
    ref = torch.nonzero(flags).flatten().to(I32)
    k = ref.numel()
    got = run(f"n={n} p={p}", "svdd_compact_flags", lambda q: (flags, n, q["live_idx"], q["slot"], q["count"]),
              {"live_idx": (n, I32), "slot": (n, I32), "count": (1, I32)}, written={"live_idx": torch.arange(n) < k})
    assert got["count"].cpu().tolist() == [k]
    assert torch.equal(got["live_idx"].body()[:k], ref)
    exp_slot = torch.full((n,), -1, dtype=I32, device=DEV)
    exp_slot[ref.long()] = torch.arange(k, dtype=I32, device=DEV)
    assert torch.equal(got["slot"].body(), exp_slot)
    case("svdd_compact_flags", f"n={n} density={p} live={k}")


@pytest.mark.parametrize("n", COMPACT_N)
@pytest.mark.parametrize("p", [0.0, 0.3, 1.0])
def test_compact_by_key_list_and_the_lengths_of_its_two_parts(n, p):
    g = torch.Generator(device=DEV).manual_seed(n + 1)
    key = torch.randint(1, 21, (n,), device=DEV, generator=g, dtype=I32)              # keys above 15 clamp to 15
    key = torch.where(torch.rand(n, device=DEV, generator=g) < p, key, torch.zeros_like(key))
    if n > 3:
        key[1] = -2                                                                    # negative = not live
    kc = key.clamp(0, 15)
    live = torch.nonzero(kc).flatten()
    ref = live[torch.sort(kc[live], descending=True, stable=True).indices].to(I32)
    k = ref.numel()
    exp_slot = torch.full((n,), -1, dtype=I32, device=DEV)
    exp_slot[ref.long()] = torch.arange(k, dtype=I32, device=DEV)
    for split in sorted({0, 1, k, k + 1, n + 5}):
        got = run(f"n={n} p={p} split={split}", "svdd_compact_by_key", lambda q: (key, n, q["live_idx"], q["slot"], q["count"], split),
                  {"live_idx": (n, I32), "slot": (n, I32), "count": (3, I32)},
                  written={"live_idx": torch.arange(n) < k, "count": torch.tensor([True, split > 0, split > 0])})
        count = got["count"].cpu().tolist()
        assert count[0] == k
        if split > 0:
            assert count[1:] == [min(k, split), max(k - split, 0)], (count, split)
        assert torch.equal(got["live_idx"].body()[:k], ref)
        assert torch.equal(got["slot"].body(), exp_slot)
        case("svdd_compact_by_key", f"n={n} density={p} live={k} split={split} count={count[:3 if split else 1]}")


# ------------------------------------------------------------------------------------------ the row movers
def _rows(rng, n, row_bytes):
    return rng.integers(0, 160, (n, row_bytes)).astype(np.uint8)    # any byte but the sentinel: a copied row never looks untouched


@pytest.mark.parametrize("row_bytes", [1, 2, 6, 200, 1000, 1024])
def test_gather_rows_stops_at_the_count(row_bytes):
    rng = np.random.default_rng(row_bytes)
    n, n_src, k = 37, 50, 11
    src, idx = _rows(rng, n_src, row_bytes), rng.integers(0, n_src, n).astype(np.int32)
    idx_d = dev(idx)
    room = torch.zeros(n_src * row_bytes + 16, dtype=U8, device=DEV)
    offsets = [(0, 0)] + ([(1, 0), (2, 0), (0, 1), (0, 2), (2, 1)] if row_bytes == 200 else [])
    for off_s, off_d in offsets:
        room.zero_()
        view = room[off_s:off_s + n_src * row_bytes]
        view.copy_(dev(src).reshape(-1))
        for count in (None, 0, k, n):
            rows = n if count is None else count
            cnt_d = None if count is None else torch.tensor([count], dtype=I32, device=DEV)
            tag = f"n={n} row_bytes={row_bytes} count={'NULL' if count is None else count} src+{off_s} dst+{off_d}"
            got = run(tag, "svdd_gather_rows", lambda p: (view.data_ptr(), idx_d, cnt_d, n, row_bytes, p["dst"]),
                      {"dst": (n * row_bytes, U8, off_d)}, written={"dst": (torch.arange(n) < rows).repeat_interleave(row_bytes)})
            assert np.array_equal(got["dst"].cpu(n, row_bytes).numpy()[:rows], src[idx[:rows]]), tag
            case("svdd_gather_rows", tag)


@pytest.mark.parametrize("row_bytes", [4, 20, 1000, 1024, 4112])
@pytest.mark.parametrize("B", [1, 37])
def test_advance_rows_moves_live_winners_and_nothing_else(row_bytes, B):
    """16-byte units where the row size allows (1024; 4112 = 257 units: more than one pass of the 256 threads), 4-byte units
    otherwise; a row whose winner is a copy of its parent (slot -1) keeps every byte."""
    rng = np.random.default_rng(row_bytes + B)
    M, n_src = 5, 23
    src = _rows(rng, n_src, row_bytes)
    src_d = dev(src)
    sel = rng.integers(0, M, B).astype(np.int32)
    slot = np.where(rng.random(B * M) < 0.4, -1, rng.integers(0, n_src, B * M)).astype(np.int32)
    won = np.arange(B) * M + sel
    slot[won[0]] = 3                                                # at least one row moves
    if B > 1:
        slot[won[1]] = -1                                           # and one stays
    sel_d = dev(sel)
    for name, sl in (("mixed", slot), ("every slot -1", np.full(B * M, -1, np.int32))):
        sl_d = dev(sl)
        moved = sl[won] >= 0
        tag = f"B={B} M={M} row_bytes={row_bytes} slots={name} moved={int(moved.sum())}"
        got = run(tag, "svdd_advance_rows", lambda p: (src_d, sl_d, sel_d, B, M, row_bytes, p["dst"]), {"dst": (B * row_bytes, U8)},
                  written={"dst": torch.from_numpy(moved).repeat_interleave(row_bytes)})
        out = got["dst"].cpu(B, row_bytes).numpy()
        assert np.array_equal(out[moved], src[sl[won][moved]]), tag
        case("svdd_advance_rows", tag)


# ------------------------------------------------------------------------------------------ K8: mt19937
@pytest.mark.parametrize("n", [1, 226, 227, 228, 623, 624, 625, 2053, 10007])
@pytest.mark.parametrize("drawn", [0, 1010])
def test_mt19937_writes_n_outputs_and_625_state_words(n, drawn):
    from tests.test_kernels_gpu import _mt_device_state
    state0, m = _mt_device_state(44, drawn)
    want, want_next = m.torch_rand(n), m.torch_rand(5)

    def load(bufs):
        bufs["state"].bits().copy_(state0)

    tag = f"n={n} state after {drawn} draws"
    got = run(tag, "svdd_mt19937_uniform_f32", lambda p: (p["state"], p["out"], n), {"state": (625, I32), "out": n},
              written={"state": GUARDS_ONLY}, init=load)
    assert np.array_equal(got["out"].cpu().numpy(), want), tag
    assert 1 <= int(got["state"].body()[624]) <= 624
    after = got["state"].bits().clone()
    nxt = run(tag + " then 5", "svdd_mt19937_uniform_f32", lambda p: (got["state"].ptr, p["out"], 5), {"out": 5},
              init=lambda bufs: got["state"].bits().copy_(after))
    assert np.array_equal(nxt["out"].cpu().numpy(), want_next), tag     # the state left behind continues the stream
    got["state"].untouched()                                            # (guards, again, after the second pair of launches)
    case("svdd_mt19937_uniform_f32", tag)


@pytest.mark.parametrize("drawn", [0, 1010])
def test_mt19937_n_zero_writes_nothing(drawn):
    from tests.test_kernels_gpu import _mt_device_state
    state0, _ = _mt_device_state(44, drawn)
    got = run(f"n=0 state after {drawn} draws", "svdd_mt19937_uniform_f32", lambda p: (p["state"], p["out"], 0),
              {"state": (625, I32), "out": 4}, written={"state": GUARDS_ONLY, "out": False},
              init=lambda bufs: bufs["state"].bits().copy_(state0))
    assert torch.equal(got["state"].bits(), state0)
    case("svdd_mt19937_uniform_f32", f"n=0 state after {drawn} draws")
