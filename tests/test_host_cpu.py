"""CPU-side checks (no GPU): the C-ABI library loads and exports what include/svdd_hip.h declares,
the host mirror exposes the reference's sampler API, the schedule table equals the reference's, the
product path refuses to run without a GPU, and the multi-process sharding/gather logic (gloo, 2 ranks)."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from svdd_amd import _lib
    _lib.build()
    hdr = open(os.path.join(ROOT, "include", "svdd_hip.h")).read()
    declared = set(re.findall(r"^int (svdd_\w+)\(", hdr, flags=re.M))
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.svdd_abi_version() == _lib.ABI_VERSION
    # the code object is gfx950
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/clang-offload-bundler", "--list", "--type=o", f"--input={_lib.SO_PATH}"],
                         capture_output=True, text=True)
    if out.returncode == 0 and out.stdout.strip():
        assert "gfx950" in out.stdout


def _header_without_comments():
    hdr = open(os.path.join(ROOT, "include", "svdd_hip.h")).read()
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))


def _header_class(param):
    """A C parameter declaration -> "ptr" | "f32" | "f64" | "i32" | "i64"."""
    param = " ".join(param.split())
    if "*" in param or "hipStream_t" in param:
        return "ptr"
    ctype = param.rsplit(" ", 1)[0].replace("const ", "").strip()            # drop the parameter's name
    return {"float": "f32", "double": "f64", "int": "i32", "int32_t": "i32", "uint32_t": "i32", "long long": "i64",
            "int64_t": "i64"}[ctype]


def _table_class(t):
    """An entry of _lib.SIGNATURES -> the same classes."""
    if t is ctypes.c_float:
        return "f32"
    if t is ctypes.c_double:
        return "f64"
    if issubclass(t, (ctypes.c_void_p, ctypes.c_char_p, ctypes._Pointer)):
        return "ptr"
    assert issubclass(t, ctypes._SimpleCData) and t._type_ in "ilqIL", t   # an integer type: classed by its size
    return {4: "i32", 8: "i64"}[ctypes.sizeof(t)]


def _signature_mismatches(signatures):
    """Every difference between a name -> parameter types table and the `int svdd_*(...);` prototypes of include/svdd_hip.h."""
    from svdd_amd import _lib
    protos = re.findall(r"\bint\s+(svdd_\w+)\s*\(([^)]*)\)\s*;", _header_without_comments())
    assert len(protos) >= 68 and len(set(n for n, _ in protos)) == len(protos)
    bad = [f"{n}: not in the {'table' if n not in signatures else 'header'}" for n in set(signatures) ^ set(n for n, _ in protos)]
    for name, params in protos:
        if name not in signatures:
            continue
        params = [] if params.strip() in ("", "void") else [p.strip() for p in params.split(",")]
        sig = signatures[name]
        if len(sig) != len(params):
            bad.append(f"{name}: {len(params)} parameters in the header, {len(sig)} in the table")
            continue
        for i, (p, t) in enumerate(zip(params, sig)):
            if _header_class(p) != _table_class(t):
                bad.append(f"{name}: parameter {i} `{p}` is {_header_class(p)} in the header, {_table_class(t)} in the table")
            is_stream = i == len(params) - 1 and p.split()[-1].lstrip("*") == "stream"
            if is_stream != (t is _lib.STREAM):
                bad.append(f"{name}: parameter {i} `{p}`: the table {'marks' if not is_stream else 'does not mark'} it as the stream")
    return bad


def test_signature_table_equals_the_header():
    """_lib.SIGNATURES (the argtypes of every export, and which functions _lib.call hands the current stream) against the prototypes
    of include/svdd_hip.h: the same functions, per function the same number of parameters, per parameter the same class (pointer,
    float, double, 32-bit, 64-bit integer), and the stream marked exactly where the last parameter is `stream`."""
    from svdd_amd import _lib
    assert _lib.EXPORTS == tuple(_lib.SIGNATURES)
    assert _signature_mismatches(_lib.SIGNATURES) == []
    assert sum(1 for s in _lib.SIGNATURES.values() if s and s[-1] is _lib.STREAM) == 55
    # the check bites: a 32-bit entry widened, an entry dropped, a stream mark lost
    sig = dict(_lib.SIGNATURES)
    g = list(sig["svdd_gather_rows"])
    assert g[3] is _lib.i32
    g[3] = _lib.i64
    sig["svdd_gather_rows"] = tuple(g)
    assert any("svdd_gather_rows: parameter 3" in m for m in _signature_mismatches(sig))
    sig = dict(_lib.SIGNATURES)
    sig["svdd_select"] = sig["svdd_select"][:-2] + (_lib.STREAM,)
    assert any("svdd_select: 11 parameters in the header, 10" in m for m in _signature_mismatches(sig))
    sig = dict(_lib.SIGNATURES)
    del sig["svdd_elbo_nll"]
    assert any("svdd_elbo_nll: not in the table" in m for m in _signature_mismatches(sig))
    sig = dict(_lib.SIGNATURES)
    sig["svdd_x0hat"] = sig["svdd_x0hat"][:-1] + (_lib.vp,)
    assert any("svdd_x0hat: parameter 7" in m and "stream" in m for m in _signature_mismatches(sig))
    # lib() sets the argtypes from the table (the stream as a plain pointer)
    L = _lib.lib()
    for name, s in _lib.SIGNATURES.items():
        assert list(getattr(L, name).argtypes) == [ctypes.c_void_p if t is _lib.STREAM else t for t in s], name
        assert getattr(L, name).restype is ctypes.c_int


def test_option_constants_equal_the_header_enum():
    """_lib.OPT_* against the SVDD_OPT_* enum of include/svdd_hip.h: the same names with the same values, both ways."""
    from svdd_amd import _lib
    declared = {n: int(v) for n, v in re.findall(r"\bSVDD_(OPT_\w+)\s*=\s*(-?\d+)", _header_without_comments())}
    bound = {n: v for n, v in vars(_lib).items() if n.startswith("OPT_")}
    assert len(declared) == 9 and sorted(declared.values()) == list(range(9))
    assert bound == declared


def test_call_door_checks_before_it_launches():
    """_lib.call refuses, without a GPU: a name the library does not have, a wrong number of arguments (the stream is never the
    caller's to pass), and a tensor where the function takes a number (it must not be read as an address)."""
    from svdd_amd import _lib
    with pytest.raises(_lib.SvddError, match="svdd_compact_flag "):
        _lib.call("svdd_compact_flag", None, 0, None, None, None)
    with pytest.raises(TypeError, match="svdd_compact_flags takes 5 arguments"):
        _lib.call("svdd_compact_flags", None, 0, None, None, None, None)
    with pytest.raises(TypeError, match="svdd_compact_flags: argument 1 is a number"):
        _lib.call("svdd_compact_flags", None, torch.tensor(16), None, None, None)
    with pytest.raises(TypeError, match="svdd_value_tail_lp: argument 6 is a number"):
        _lib.call("svdd_value_tail_lp", None, None, None, None, None, None, torch.tensor(0.5), None, 1, 1, 1, None, 1)
    # a function without a stream goes through the same door: its return code is checked under its own name
    with pytest.raises(_lib.SvddError, match="svdd_set_option: invalid argument"):
        _lib.call("svdd_set_option", 99, 0)


def test_every_entry_refuses_nulls_before_it_touches_the_device():
    """Every export that takes a device pointer (`vp` in _lib.SIGNATURES) and more than two parameters, called with zeros and NULLs
    — a NULL rng and a NULL stream included — returns E_ARG, in this process on a machine without a GPU: the validation comes
    before the profile span and before any HIP call (an entry that reached either would answer E_LAUNCH / E_NODEVICE, or take the
    process down). Table-driven, so an entry added later is held to the same order. The two host-side queries with pointer
    parameters (svdd_device_info, svdd_profile_collect) take no device pointer and are not launches."""
    from svdd_amd import _lib
    L = _lib.lib()
    zero = {_lib.i32: 0, _lib.i64: 0, _lib.f32: 0.0, _lib.f64: 0.0}
    entries = [name for name, sig in _lib.SIGNATURES.items() if len(sig) > 2 and _lib.vp in sig]
    assert len(entries) >= 56 and "svdd_backbone_incr_f32" in entries and "svdd_elbo_nll" in entries
    wrong = {}
    for name in entries:
        rc = getattr(L, name)(*[zero.get(t) for t in _lib.SIGNATURES[name]])     # every pointer type -> None = NULL
        if rc != _lib.E_ARG:
            wrong[name] = rc
    assert not wrong, wrong


def test_argument_validation_without_gpu():
    """Entry points reject bad arguments before touching the device."""
    from svdd_amd import _lib
    L = _lib.lib()
    rs = _lib.SvddRng(_lib.RNG_PHILOX, 0, None, 0, 0, 0, 0)
    assert L.svdd_propose(None, None, 0.0, 0.0, 1, 1, 1, 0, ctypes.byref(rs), None, None, None, None) == _lib.E_ARG
    assert L.svdd_select(None, None, 1, 1, 1, 0, None, None, None, None, None) == _lib.E_ARG
    assert L.svdd_finalize(None, None, 1, 1, 0, None, None, None) == _lib.E_ARG
    assert L.svdd_x0hat(None, None, 1, 1, 0, None, None, None) == _lib.E_ARG
    assert L.svdd_tds_resample(None, None, 1.0, None, None, 1, 1, None, None, None, None) == _lib.E_ARG
    # net-side entry points added in round 3: the config-4 trunk's GEMM / window kernels, the DPS backbone's layer passes
    one = ctypes.c_void_p(64)                                              # a non-NULL pointer that is never dereferenced
    assert L.svdd_trunk_gemm(None, None, None, None, None, None, 1, 128, 32, 1, 32, 128, 0, None, 0, None, None, None, None, 0, 0, None) == _lib.E_ARG
    assert L.svdd_trunk_gemm(one, None, one, None, None, one, 1, 100, 32, 1, 32, 100, 0, None, 0, None, None, None, None, 0, 0, None) == _lib.E_ARG   # N % 128
    # strides the 16-byte row pieces cannot honour: lda % 8 (bf16 planes) / % 4 (fp32 planes), ldo % 4
    assert L.svdd_trunk_gemm(one, None, one, None, None, one, 1, 128, 32, 1, 36, 128, 0, None, 0, None, None, None, None, 0, 0, None) == _lib.E_ARG
    assert L.svdd_trunk_gemm(one, None, one, None, None, one, 1, 128, 32, 1, 32, 130, 0, None, 0, None, None, None, None, 0, 0, None) == _lib.E_ARG
    prev = _lib.set_option(_lib.OPT_TRUNK_PLANES_F32, 1)
    try:
        assert L.svdd_trunk_gemm(one, None, one, None, None, one, 1, 128, 32, 1, 34, 128, 0, None, 0, None, None, None, None, 0, 0, None) == _lib.E_ARG
        assert L.svdd_trunk_gemm(one, None, one, None, None, one, 1, 128, 32, 1, 32, 129, 0, None, 0, None, None, None, None, 0, 0, None) == _lib.E_ARG
    finally:
        _lib.set_option(_lib.OPT_TRUNK_PLANES_F32, prev)
    assert L.svdd_trunk_windows(one, one, one, 1, 4, 201, 7, 2, 4, None, one, one, one, None) == _lib.E_ARG      # an odd length below the last shared level
    assert L.svdd_trunk_windows(one, one, one, 1, 4, 200, 7, 1, 5, None, one, one, one, None) == _lib.E_ARG      # more window slots than the kernels hold
    assert L.svdd_trunk_windows(one, one, one, 1, 4, 300, 7, 1, 4, None, one, one, one, None) == _lib.E_ARG      # L > 256
    assert L.svdd_trunk_stem_unfold_win(None, 1, 200, 4, one, one, one, one, None, None) == _lib.E_ARG
    assert L.svdd_trunk_attn_pool_win(one, one, 1, 200, 768, 0, 4, one, one, one, one, 1, one, None, None, one, one, None, None, 0, None, None, None,
                                      None) == _lib.E_ARG                  # lo plane without the parent's lo plane
    # the remaining refusals of the three shared-level entries (svdd_trunk.hip): each call differs from an accepted one in one argument
    def windows(div=1, n=4, L=200, halo=7, depth=1, slots=4, ptrs=(one,) * 6):
        return L_.svdd_trunk_windows(*ptrs[:3], div, n, L, halo, depth, slots, None, *ptrs[3:], None)

    def unfold_win(n=1, L=200, slots=4, ptrs=(one,) * 5):
        return L_.svdd_trunk_stem_unfold_win(ptrs[0], n, L, slots, *ptrs[1:4], ptrs[4], None, None)

    def pool_win(n=1, L=200, C=768, in_halo=0, slots=4, div=1, parent_lo=None, out_lo=None, scale=None, shift=None, post_act=0,
                 v0=None, vlen=None, off2=None, ptrs=(one,) * 8):
        x, lg, w0, wlen, off, pidx, parent_hi, out_hi = ptrs
        return L_.svdd_trunk_attn_pool_win(x, lg, n, L, C, in_halo, slots, w0, wlen, off, pidx, div, parent_hi, parent_lo, None, out_hi, out_lo,
                                           scale, shift, post_act, v0, vlen, off2, None)
    L_ = L
    for kw in (dict(slots=0), dict(slots=-1), dict(depth=0), dict(depth=9), dict(div=0), dict(div=-2), dict(n=0), dict(L=0), dict(L=257),
               dict(halo=-1), dict(L=100, depth=4), dict(L=30, depth=3)):
        assert windows(**kw) == _lib.E_ARG, kw
    for k in range(6):
        assert windows(ptrs=tuple(None if i == k else one for i in range(6))) == _lib.E_ARG, k
    for kw in (dict(slots=0), dict(slots=5), dict(n=0), dict(L=0)):
        assert unfold_win(**kw) == _lib.E_ARG, kw
    for k in range(5):
        assert unfold_win(ptrs=tuple(None if i == k else one for i in range(5))) == _lib.E_ARG, k
    for kw in (dict(C=6), dict(C=0), dict(slots=0), dict(slots=5), dict(div=0), dict(in_halo=-1), dict(n=0), dict(L=0), dict(post_act=3),
               dict(post_act=-1), dict(scale=one), dict(shift=one), dict(v0=one), dict(v0=one, vlen=one), dict(v0=one, off2=one),
               dict(vlen=one), dict(off2=one), dict(vlen=one, off2=one), dict(out_lo=one), dict(parent_lo=one),
               dict(L=201, v0=one, vlen=one, off2=one)):
        assert pool_win(**kw) == _lib.E_ARG, kw
    for k in range(8):
        assert pool_win(ptrs=tuple(None if i == k else one for i in range(8))) == _lib.E_ARG, k
    assert L.svdd_bb_layer_fwd_f32(None, None, None, None, None, None, 1e-5, None, None, None, 1, 1, 128, None) == _lib.E_ARG
    assert L.svdd_bb_layer_fwd_f32(one, one, one, None, None, None, 1e-5, one, one, None, 1, 1, 96, None) == _lib.E_ARG    # channels not 64 / 128 / 256
    assert L.svdd_bb_layer_bwd_f32(one, one, one, one, 1e-5, one, one, one, None, 1, 1, 128, None) == _lib.E_ARG          # mask without its output
    # the one-launch backbone pair of DPS: lengths outside 104 < L <= 208, layer counts outside 1 .. 32, a dilation of 0, each NULL
    def bb_save(n=1, L=200, nl=2, dil=(1, 4), ptrs=(one,) * 9):
        d = None if dil is None else (ctypes.c_int * max(1, len(dil)))(*dil)
        return L_.svdd_backbone_cnn_save_f32(*ptrs[:6], n, L, nl, d, *ptrs[6:], None)

    def bb_grad(n=1, L=200, nl=2, dil=(1, 4), ptrs=(one,) * 9):
        d = None if dil is None else (ctypes.c_int * max(1, len(dil)))(*dil)
        return L_.svdd_backbone_cnn_grad_f32(*ptrs, n, L, nl, d, None)
    for entry in (bb_save, bb_grad):
        for kw in (dict(L=104), dict(L=209), dict(L=0), dict(nl=0, dil=()), dict(nl=33, dil=(1,) * 33), dict(dil=(1, 0)), dict(dil=(0, 1)),
                   dict(dil=(1, -4)), dict(dil=None), dict(n=0)):
            assert entry(**kw) == _lib.E_ARG, (entry.__name__, kw)
        for k in range(9):
            assert entry(ptrs=tuple(None if i == k else one for i in range(9))) == _lib.E_ARG, (entry.__name__, k)
    # svdd_conv1d_cl_f32: a tile holds 224 rows, taps are odd, four channel pairs, the fused epilogue only on the static shapes
    def conv(n=1, L=200, cin=128, cout=128, taps=9, dil=1, bias=None, f_prev=None, act=-1, tb=None, gamma=None, beta=None, hn=None, ptrs=(one,) * 3):
        return L_.svdd_conv1d_cl_f32(*ptrs, n, L, cin, cout, taps, dil, bias, f_prev, act, tb, gamma, beta, hn, None)
    for kw in (dict(L=225), dict(L=0), dict(n=0), dict(taps=8), dict(taps=0), dict(dil=0), dict(cin=32, cout=64), dict(cin=64, cout=256),
               dict(cin=96, cout=96), dict(act=3), dict(act=-2),
               dict(L=113, act=0), dict(taps=7, act=2), dict(dil=2, act=1), dict(cin=64, cout=128, taps=5, act=0),      # act >= 0 on a generic shape
               dict(act=0, hn=one), dict(act=0, hn=one, beta=one), dict(act=0, hn=one, gamma=one),                      # hn without gamma / beta
               dict(act=-1, hn=one, gamma=one, beta=one)):                                                             # hn without an epilogue
        assert conv(**kw) == _lib.E_ARG, kw
    for k in range(3):
        assert conv(ptrs=tuple(None if i == k else one for i in range(3))) == _lib.E_ARG, k
    # svdd_epilogue_ln_f32: y, f_out, hn at positions 0, 6, 7
    def epi(rows=4, C=128, act=0, y=one, gamma=one, beta=one, f_out=one, hn=one):
        return L_.svdd_epilogue_ln_f32(y, None, None, None, gamma, beta, f_out, hn, rows, C, act, None)
    for kw in (dict(C=96), dict(C=0), dict(C=512), dict(act=3), dict(act=-1), dict(f_out=None, hn=None), dict(y=None), dict(rows=0),
               dict(gamma=None), dict(beta=None)):
        assert epi(**kw) == _lib.E_ARG, kw
    # the reward net's gradient pass: the shapes its specialised kernels do not have, and NULLs
    for L_bad, taps in ((100, 5), (208, 5), (1, 5), (200, 3), (50, 9)):
        assert L.svdd_conv1d_cl_gated_f32(one, one, one, 1, L_bad, 64, 64, taps, 1, None, None, None) == _lib.E_ARG
    assert L.svdd_conv1d_cl_gated_f32(one, one, one, 1, 200, 64, 128, 5, 1, None, None, None) == _lib.E_ARG
    assert L.svdd_conv1d_cl_gated_f32(one, one, one, 1, 200, 64, 64, 5, 2, None, None, None) == _lib.E_ARG
    assert L.svdd_conv1d_cl_gated_f32(one, one, one, 0, 200, 64, 64, 5, 1, None, None, None) == _lib.E_ARG
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        assert L.svdd_conv1d_cl_gated_f32(*args, 1, 200, 64, 64, 5, 1, None, None, None) == _lib.E_ARG
    for taps in (5, 13, 17):
        assert L.svdd_reward_stem_f32(one, one, one, one, 1, 200, taps, None) == _lib.E_ARG
        assert L.svdd_reward_stem_bwd_f32(one, one, one, 1, 200, taps, None) == _lib.E_ARG
    for k in range(4):
        assert L.svdd_reward_stem_f32(*[None if i == k else one for i in range(4)], 1, 200, 15, None) == _lib.E_ARG
        assert L.svdd_sum_gate_f32(*[None if i == k else one for i in range(4)], 4, None) == _lib.E_ARG
    for k in range(3):
        assert L.svdd_reward_stem_bwd_f32(*[None if i == k else one for i in range(3)], 1, 200, 15, None) == _lib.E_ARG
    assert L.svdd_reward_stem_f32(one, one, one, one, 0, 200, 15, None) == _lib.E_ARG
    assert L.svdd_reward_stem_bwd_f32(one, one, one, 1, 0, 15, None) == _lib.E_ARG
    for count in (1, 2, 3, 5, 1030, 0, -4):
        assert L.svdd_sum_gate_f32(one, one, one, one, count, None) == _lib.E_ARG
    for k in range(9):
        ptrs = [None if i == k else one for i in range(9)]
        assert L.svdd_reward_tail_grad_f32(*ptrs[:7], 1e-5, 1, 1, *ptrs[7:], None) == _lib.E_ARG
    assert L.svdd_reward_tail_grad_f32(*[one] * 7, 1e-5, 0, 1, one, one, None) == _lib.E_ARG
    assert L.svdd_gru_bidir_train2_f32(one, one, one, None, one, one, 1, 1, None) == _lib.E_ARG                            # no gi scratch
    assert L.svdd_gru_bidir_bwd2_f32(one, one, one, one, None, None, one, 1, 1, None) == _lib.E_ARG                        # no da scratch
    assert L.svdd_gru_bidir_bwd2_f32(one, one, one, one, one, None, None, 1, 1, None) == _lib.E_ARG                        # no output


def test_incremental_backbone_entries_refuse_bad_arguments_without_gpu():
    """The refusals of svdd_backbone_incr_f32 / incr2 / incr3 / incr4, per entry: every call differs in ONE argument from a call the
    entry accepts (n = 1, L = 200, the dna config's 20 layers, lead = 8, depth 10 where there is one, items of 2 tiles, every pointer
    non-NULL) and must answer E_ARG before the profile span and before any HIP call. Only refused calls are made: an accepted one would
    go on to the device."""
    from svdd_amd import _lib
    lib = _lib.lib()
    one, two = ctypes.c_void_p(64), ctypes.c_void_p(128)                   # non-NULL pointers that are never dereferenced
    dna = (1,) * 8 + (4,) * 4 + (16,) * 4 + (64,) * 4
    pointers = ("x", "table0", "tiles", "vec", "w2", "out", "dil", "planes", "x_prev", "items")
    entries = {   # name: (has order lists, has depth, has the token pair, accepted max_item)
        "svdd_backbone_incr_f32": (False, False, False, {2, 4}),
        "svdd_backbone_incr2_f32": (True, False, False, {1, 2, 4}),
        "svdd_backbone_incr3_f32": (True, True, False, {1, 2, 4}),
        "svdd_backbone_incr4_f32": (True, True, True, {2}),
    }

    def with_dil(i, d):
        return tuple(d if k == i else v for k, v in enumerate(dna))

    for name, (ordered, deep, pair, accepted) in entries.items():
        def call(**kw):
            a = dict({p: one for p in pointers + ("stat", "order", "order_count")}, x_prev2=two, dil=dna, n=1, L=200, nlayers=20, lead=8,
                     first=0, max_item=2, depth=10, parity=0)
            assert set(kw) <= set(a), kw
            a.update(kw)
            dil = None if a["dil"] is None else (ctypes.c_int * len(a["dil"]))(*a["dil"])
            args = [a["x"], a["table0"], a["tiles"], a["vec"], a["w2"], a["out"], a["n"], a["L"], a["nlayers"], dil, a["lead"], a["planes"],
                    a["x_prev"], a["items"], a["stat"], a["first"], a["max_item"]]
            args += [a["order"], a["order_count"]] if ordered else []
            args += [a["depth"]] if deep else []
            args += [a["x_prev2"], a["parity"]] if pair else []
            return getattr(lib, name)(*args, None)

        cases = [{p: None} for p in pointers]
        cases += [dict(n=0), dict(L=104), dict(L=209), dict(nlayers=0), dict(nlayers=33), dict(lead=1), dict(lead=9)]
        cases += [dict(max_item=m) for m in (0, 1, 2, 3, 4, 8) if m not in accepted]
        cases += [dict(dil=with_dil(0, 0)), dict(dil=with_dil(19, 0)), dict(dil=with_dil(3, 2))]
        if ordered:
            cases += [dict(order=None), dict(order_count=None), dict(n=65537)]
        if deep:
            cases += [dict(depth=7), dict(depth=13), dict(depth=21), dict(dil=with_dil(8, 1)), dict(dil=with_dil(9, 1))]
        if pair:
            cases += [dict(x_prev2=None), dict(x_prev2=one), dict(parity=-1), dict(parity=2)]
        assert len(cases) == {"svdd_backbone_incr_f32": 24, "svdd_backbone_incr2_f32": 26, "svdd_backbone_incr3_f32": 31,
                              "svdd_backbone_incr4_f32": 37}[name]
        for kw in cases:
            assert call(**kw) == _lib.E_ARG, (name, kw)
        for first in (0, 1):                                               # the refusals come before the `first` branch too
            assert call(first=first, max_item=3) == _lib.E_ARG, (name, first)


def test_row_movers_refuse_what_their_copy_units_cannot_address():
    """The bounds include/svdd_hip.h states for the row gathers, refused before anything touches the device:
    svdd_advance_rows copies 4-byte units at least (rows a multiple of 4, src and dst aligned to 4); svdd_select / _compact with the row
    gather finds a unit's row with a float reciprocal that is exact below 2^22 units per wave (tests/test_sampler_contracts_cpu.py),
    the unit taken from L and the pointers; svdd_tds_resample counts a wave's units in an int."""
    from svdd_amd import _lib
    L = _lib.lib()
    al, p = ctypes.c_void_p, 1 << 20                                      # non-NULL addresses that are never dereferenced
    for src, dst in [(p + 1, p), (p + 2, p), (p, p + 1), (p, p + 2), (p + 3, p + 3)]:
        assert L.svdd_advance_rows(al(src), al(p), al(p), 1, 1, 16, al(dst), None) == _lib.E_ARG, (src, dst)
    for row_bytes in (0, 1, 2, 6, 1001):
        assert L.svdd_advance_rows(al(p), al(p), al(p), 1, 1, row_bytes, al(p), None) == _lib.E_ARG, row_bytes

    def select(B, M, Lx, cand, x_next):
        return L.svdd_select(al(p), al(cand), B, Lx, M, 0, None, al(x_next), None, None, None)

    assert select(1, 1, 1 << 19, p, p) == _lib.E_ARG                      # 64 rows per wave x (2^19 / 8) units = 2^22
    assert select(1, 1, 1 << 16, p + 1, p) == _lib.E_ARG                  # a cand view one byte off: 1-byte units, 64 x 2^16
    assert select(1, 1, 1 << 17, p, p + 2) == _lib.E_ARG                  # an x_next view two bytes off: 2-byte units
    assert select(1, 64, 1 << 22, p + 1, p) == _lib.E_ARG                 # one row per wave
    assert select(1 << 18, 10, 1 << 21, p, p) == _lib.E_ARG               # a saturated launch: 4 groups of 4 rows x 2^18 units
    assert L.svdd_select_compact(al(p), al(p), al(p), al(p), 1, 1 << 19, 1, 0, None, al(p), None, None, None, None, None) == _lib.E_ARG
    assert L.svdd_tds_resample(al(p), al(p), 1.0, al(p), al(p), 1, 1 << 25, al(p), None, al(p), None) == _lib.E_ARG


def test_schedule_table_equals_reference(golden):
    from svdd_amd.noise_schedule import LogLinearNoise, move_chance_table
    g = golden("g3_schedule.npz")
    for S in (128, 16, 8):
        tab, ts, dt = move_chance_table(LogLinearNoise(), S)
        ref = g[f"S{S}"]
        # same torch CPU ops as the reference => equal; allow 1 ulp for a different host CPU's SLEEF path
        assert np.abs(tab.numpy() - ref[:, 3:6]).max() <= 6e-8
        assert np.array_equal(ts[:S].numpy(), ref[:, 0])
        assert np.float32(ts[-1]) == g[f"S{S}_t_last"]


def test_sampler_api_surface():
    """Method names and keyword arguments of diffusion_gosai.Diffusion that decode callers use."""
    from svdd_amd.config import dna_config
    from svdd_amd.diffusion import Diffusion
    d = Diffusion(dna_config(hidden_dim=16, num_cnn_stacks=1))
    assert d.mask_index == 4 and d.vocab_size == 5 and d.sampler == "ddpm" and d.time_conditioning is False
    assert d.config.model.length == 200 and d.config.sampling.steps == 128 and d.config.sampling.noise_removal
    want = {
        "forward": ["x", "sigma"],
        "_sample": ["num_steps", "eps", "eval_sp_size", "cdq"],
        "decode_sample": ["num_steps", "eps", "eval_sp_size", "cdq"],
        "controlled_sample": ["pre_scorer_embedding", "pre_scorer_head", "num_steps", "eps", "eval_sp_size", "sample_M"],
        "controlled_sample_tweedie": ["reward_model", "num_steps", "eps", "eval_sp_size", "sample_M", "options", "task"],
        "controlled_sample_TDS": ["reward_model", "alpha", "num_steps", "eps", "eval_sp_size", "sample_M"],
        "_ddpm_update_finetune": ["x", "t", "dt"],
        "_ddpm_update_finetune_controlled": ["x", "t", "dt", "pre_scorer_embedding", "pre_scorer_head", "repeats"],
        "_ddpm_update_finetune_controlled_twedie": ["x", "t", "dt", "reward_model", "repeats", "options", "task"],
        "_ddpm_update_finetune_controlled_TDS": ["x", "t", "dt", "reward_model", "alpha"],
        "_ddpm_update_finetune_controlled_DPS": ["x", "t", "dt", "reward_model", "guidance_scale"],
        "controlled_sample_DPS": ["reward_model", "guidance_scale", "num_steps", "eps", "eval_sp_size", "sample_M"],
        "compute_gradient_DPS": ["x_onehot", "x", "reward_model", "sigma_s", "copy_flag"],
        "forward2": ["x_onehot", "x", "sigma"],
        "transform_samples": ["samples", "num_classes"],
    }
    for name, params in want.items():
        sig = inspect.signature(getattr(d, name))
        assert list(sig.parameters) == params, (name, list(sig.parameters))
    assert inspect.signature(d.controlled_sample).parameters["sample_M"].default == 10
    assert inspect.signature(d.controlled_sample).parameters["eps"].default == 1e-5
    p = d._sample_prior(3, 7)
    assert p.dtype == torch.int64 and p.shape == (3, 7) and int(p.min()) == 4
    # transform_samples on CPU tensors (host utility, same as the reference's)
    t = torch.tensor([[0, 3, 4, 1]])
    assert d.transform_samples(t).tolist() == [[[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0], [0, 1, 0, 0]]]


def test_hot_path_refuses_cpu():
    from svdd_amd import ops
    from svdd_amd.config import rna_config
    from svdd_amd.diffusion import Diffusion
    d = Diffusion(rna_config(hidden_dim=16, num_cnn_stacks=1)).eval()
    with pytest.raises(ops.SvddError):
        d.controlled_sample(lambda x: x, lambda x: x, eval_sp_size=2, sample_M=2)
    with pytest.raises(ops.SvddError):
        ops.propose(torch.zeros(1, 4, 5), torch.zeros(1, 4, dtype=torch.uint8), 0.1, 0.1, 2, ops.Rng())


def test_shard_rows():
    from svdd_amd.distributed import shard_rows
    for total, world in [(2048, 8), (10, 4), (3, 8), (256, 1)]:
        spans = [shard_rows(total, r, world) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == total
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        assert max(h - l for l, h in spans) - min(h - l for l, h in spans) <= 1


_WORKER = r"""
import os, sys, torch
sys.path.insert(0, {root!r})
import torch.distributed as dist
from svdd_amd import distributed
rank, world, local = distributed.init_from_env("gloo")
assert world == 2
total, L = {total}, 11

class Model:                       # stands in for Diffusion: rows are a pure function of the GLOBAL row index
    row_offset = 0
def sampler(eval_sp_size):
    rows = torch.arange(Model.row_offset, Model.row_offset + eval_sp_size)
    return ((rows[:, None] * 7 + torch.arange(L)[None, :]) % 4).to(torch.int64)
out = distributed.sharded_sample(Model, total, sampler)
ref = ((torch.arange(total)[:, None] * 7 + torch.arange(L)[None, :]) % 4).to(torch.int64)
assert out.dtype == torch.int64 and torch.equal(out, ref), (rank, out.shape)
assert Model.row_offset == 0
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


@pytest.mark.parametrize("total", [8, 7])
def test_sharded_decode_two_ranks_gloo(tmp_path, total):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, total=total))
    port = 29500 + os.getpid() % 2000 + total
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)]
    env = dict(os.environ, OMP_NUM_THREADS="1")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert res.stdout.count("ok") == 2


def test_dps_gradient_matches_reference(golden):
    """compute_gradient_DPS (autograd through forward2 + reward net, pure torch) against the gradients the
    reference computed in its own controlled_sample_DPS run (fixture g11), same weights, CPU fp32."""
    from svdd_amd.config import Config, ModelConfig
    from svdd_amd.diffusion import Diffusion
    from svdd_amd.value_nets import RewardModel
    from tests.test_nets_cpu import tiny_nets
    g = golden("g11_traj_dps.npz")
    bb, emb, head = tiny_nets(golden("nets_tiny.npz"))
    d = Diffusion(Config(model=ModelConfig(hidden_dim=16, num_cnn_stacks=1, length=int(g["L"]))), backbone=bb).eval()
    reward = RewardModel(emb, head).eval()
    for i in range(int(g["S"])):
        x = torch.from_numpy(g["xs"][i].astype(np.int64))
        onehot = torch.nn.functional.one_hot(x, 5).float()
        copy = (x != 4).to(x.dtype)
        grad = d.compute_gradient_DPS(onehot, x, reward, torch.zeros(x.shape[0]), copy)
        ref = torch.from_numpy(g["grad"][i])
        assert torch.allclose(grad, ref, rtol=1e-4, atol=1e-9), (i, (grad - ref).abs().max())


def test_detokenizer_roundtrip():
    """dataloader_gosai.py:13-32: ids 0..3 <-> ACGT; MASK prints as N."""
    from svdd_amd import tokens
    x = torch.tensor([[0, 1, 2, 3, 3, 0], [3, 3, 4, 0, 1, 2]])
    assert tokens.batch_dna_detokenize(x) == ["ACGTTA", "TTNACG"]
    assert tokens.batch_dna_detokenize(x.numpy().astype(np.uint8)) == ["ACGTTA", "TTNACG"]
    assert tokens.dna_detokenize(x[0]) == "ACGTTA"
    assert tokens.DNASequenceDetokenizer().detokenize(x)[1] == "TTNACG"
    assert tokens.dna_tokenize("acgtn").tolist() == [0, 1, 2, 3, 4]


def test_sharded_sample_refuses_replay_rng_across_ranks():
    """Replay mode draws from each process's own mt19937 stream: with the usual identical manual_seed every rank would decode
    the same rows. sharded_sample must refuse it for world > 1 (and accept it for a single rank)."""
    from svdd_amd import distributed

    class M:
        rng_mode, row_offset = "replay", 0
    m = M()
    with pytest.raises(ValueError, match="philox"):
        distributed.sharded_sample(m, 8, lambda **kw: None, rank=0, world=2)
    # ... unless the sampler replays the WHOLE batch's stream on every rank and reads its rows (svdd_amd.Diffusion does, round 4)
    M.replays_global_stream = True
    shards = []
    distributed.sharded_sample(m, 8, lambda eval_sp_size: shards.append(m._shard) or torch.zeros(eval_sp_size, 3, dtype=torch.uint8), rank=1, world=2)
    assert shards == [(4, 8, 8, 2)]
    del M.replays_global_stream
    out = distributed.sharded_sample(m, 8, lambda eval_sp_size: torch.zeros(eval_sp_size, 3, dtype=torch.uint8), rank=0, world=1)
    assert out.shape == (8, 3) and m.row_offset == 0
    m.rng_mode = "philox"
    seen = []
    distributed.sharded_sample(m, 10, lambda eval_sp_size: seen.append((m.row_offset, eval_sp_size)) or torch.zeros(eval_sp_size, 3, dtype=torch.uint8),
                               rank=2, world=3)
    assert seen == [(7, 3)] and m.row_offset == 0          # rows 7..9 of 10 belong to rank 2 of 3


def test_step_index_of_the_per_step_api():
    """The per-step methods receive (t, dt) like the reference's (diffusion_gosai.py:1036-1043: t_i = 1 - i dt); the step
    index derived from them keys the Philox counter, so consecutive steps never reuse a draw."""
    from svdd_amd.config import dna_config
    from svdd_amd.diffusion import Diffusion
    d = Diffusion(dna_config(hidden_dim=16, num_cnn_stacks=1))
    S, eps = 128, 1e-5
    ts = torch.linspace(1, eps, S + 1)
    dt = (1 - eps) / S
    assert [d._step_index(ts[i] * torch.ones(4, 1), dt) for i in (0, 1, 2, 63, 127)] == [0, 1, 2, 63, 127]


def test_weight_fingerprint_tracks_in_place_and_replaced_weights():
    from svdd_amd.diffusion import weight_fingerprint
    lin = torch.nn.Linear(4, 4)
    fp0 = weight_fingerprint(lin)
    assert weight_fingerprint(lin) == fp0
    with torch.no_grad():
        lin.weight.mul_(2.0)                                 # in-place update (optimizer step, load_state_dict copy_)
    fp1 = weight_fingerprint(lin)
    assert fp1 != fp0
    lin.load_state_dict({k: v.clone() for k, v in lin.state_dict().items()})
    assert weight_fingerprint(lin) != fp1
    lin.weight = torch.nn.Parameter(lin.weight.detach().clone())   # replaced tensor
    assert weight_fingerprint(lin) != fp1
    # writes through .data do not bump _version (how the reference's EMA swaps weights around sampling,
    # models/ema.py:62,87): only the content checksum sees them
    fp2, v = weight_fingerprint(lin), lin.weight._version
    saved = lin.weight.data.clone()
    lin.weight.data.copy_(saved * 0.5)
    assert lin.weight._version == v and weight_fingerprint(lin, content=False) == weight_fingerprint(lin, content=False)
    assert weight_fingerprint(lin)[0] == fp2[0] and weight_fingerprint(lin) != fp2
    lin.weight.data.copy_(saved)                                    # restore: the packed copy is valid again
    assert weight_fingerprint(lin) == fp2


_TDS_WORKER = r"""
import os, sys, numpy as np, torch
sys.path.insert(0, {root!r})
import torch.distributed as dist
from svdd_amd import distributed
rank, world, local = distributed.init_from_env("gloo")
total, L = {total}, 9
g = torch.Generator().manual_seed(5)
sample = torch.randint(0, 4, (total, L), generator=g).to(torch.uint8)
num, den = torch.randn(total, generator=g), torch.randn(total, generator=g)
u = torch.rand(total, generator=g, dtype=torch.float64)
lo, hi = distributed.shard_rows(total, rank, world)
mine = u.clone()
mine[:lo] = -1.0; mine[hi:] = -1.0                    # only this rank's slice of the uniforms may travel
extra = torch.randn(total, 5, generator=g)
out = distributed.tds_exchange((lo, hi, total, world), sample[lo:hi], num[lo:hi], den[lo:hi], mine, extra[lo:hi])
assert distributed.tds_exchange((lo, hi, total, world), sample[lo:hi], num[lo:hi], den[lo:hi], mine)[4] is None
for got, ref in zip(out, (sample, num, den, u, extra)):
    assert got.dtype == ref.dtype and torch.equal(got, ref), rank
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


@pytest.mark.parametrize("total", [8, 7])
def test_tds_exchange_two_ranks_gloo(tmp_path, total):
    """The one per-step collective of the path (SMC/TDS resample over a sharded batch): every rank ends up with the whole
    batch's proposals, rewards and uniforms, bit for bit, ragged shards included."""
    script = tmp_path / "worker.py"
    script.write_text(_TDS_WORKER.format(root=ROOT, total=total))
    port = 31500 + os.getpid() % 2000 + total
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert res.stdout.count("ok") == 2


def test_tds_exchange_needs_a_process_group():
    from svdd_amd import distributed
    with pytest.raises(RuntimeError, match="process group"):
        distributed.tds_exchange((0, 2, 4, 2), torch.zeros(2, 3, dtype=torch.uint8), torch.zeros(2), torch.zeros(2),
                                 torch.zeros(4, dtype=torch.float64))


def test_harness_batch_keys_do_not_collide_across_user_seeds():
    """Philox mode: batch k of a harness call is keyed by splitmix64(seed, k). With `seed + k` the runs at seeds 0, 1, 2, ...
    shared all but one batch each (batch k + 1 of seed s == batch k of seed s + 1)."""
    from svdd_amd.harness import batch_seed
    keys = {(s, k): batch_seed(s, k) for s in range(64) for k in range(64)}
    assert len(set(keys.values())) == len(keys)
    assert all(0 <= v < 2 ** 64 for v in keys.values())
    assert batch_seed(7, 3) == batch_seed(7, 3) and batch_seed(0, 1) != batch_seed(1, 0)


def test_bench_starts_its_own_ranks_from_a_bare_shell():
    """`python bench.py --gpus 2` with no WORLD_SIZE in the environment (how the driver invokes it): the parent spawns the
    two ranks itself (torch.distributed.run as a child, 127.0.0.1 rendezvous), relays rank 0's single JSON line and its
    exit code. --dry-run keeps the GPU out of it: launch, gloo rendezvous, barrier / max-over-ranks timing, row ownership
    and the one all-gather are the real code; the decode is a stand-in."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run", "--steps", "2",
                          "--warmup", "1", "--batch", "12"], capture_output=True, text=True, timeout=300, env=env, cwd="/tmp")
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout
    line = json.loads(lines[0])
    assert line["dry_run"] is True and line["value"] is None
    assert line["n_gpus"] == 2 and line["ranks_seen"] == 2 and line["backend"] == "gloo"
    assert line["gathered_rows_verified"] == 24 and len(line["per_rank"]["decode_ms"]) == 2
    # a failing rank must fail the whole command
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run", "--steps", "0"],
                         capture_output=True, text=True, timeout=300, env=env, cwd="/tmp")
    assert bad.returncode != 0


def _import_bench():
    import importlib
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("bench")


def test_bench_compact_line_fits_the_drivers_record():
    """Round 5's final stdout line was 24.9 KB and the driver's record (the last ~8 KB of stdout) could not be parsed. The line the
    driver reads is now bench.compact_line(full): built here from round 5's own long record (profiles/r05_bench_driver_cmd.json),
    it must be < 6144 bytes, parse, and keep every key of the bench contract with `roofline` and `cpu_baseline` intact."""
    import json
    bench = _import_bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r05_bench_driver_cmd.json")))
    s = bench.compact_line(full, "bench_full.json")
    assert "\n" not in s and len(s.encode()) < 6144, len(s)
    line = json.loads(s)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["value"] == full["value"] and line["ms_per_step"] == full["ms_per_step"] and line["config"] == full["config"]
    r, rf = line["roofline"], full["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "flops_per_launch", "avg_launch_us", "launches"):
        assert r[k] == rf[k], k
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert len(r["also"]) == len(rf["also"]) and "also_truncated" not in r
    assert all(set(e) <= {"k", "w", "frac", "issued", "us", "ms"} and len(json.dumps(e)) < 110 for e in r["also"])
    cb = line["cpu_baseline"]
    assert cb["value"] == full["cpu_baseline"]["value"] and cb["cores"] == 16 and cb["kind"] == "port" and cb["unit"] and cb["sample"]
    assert set(line["configs"]) >= {"c1_b4", "c3_pm", "c4_f32", "c4_bf16x3", "c5_tds_shard", "c5_tds_pop", "c5_dps"}
    assert line["configs"]["c3_pm"]["value"] == round(full["config3_pm"]["value"], 2)
    assert line["alt"]["f16x3"]["rows_vs_f32"] == full["alt_precision"]["f16x3"]["x0_rows_identical_vs_f32"]
    # a record that outgrows the limit sheds `also` entries / detail objects, never the contract keys
    fat = json.loads(json.dumps(full))
    fat["roofline"]["also"] = fat["roofline"]["also"] * 12
    s2 = bench.compact_line(fat, "bench_full.json")
    l2 = json.loads(s2)
    assert len(s2.encode()) <= 6144 and l2["roofline"]["also_truncated"] and l2["cpu_baseline"]["value"] == cb["value"] and l2["value"] == line["value"]
    # a leg that failed shows its error, a leg that was skipped is absent
    broken = json.loads(json.dumps(full))
    broken["config3_pm"] = {"error": "RuntimeError: boom"}
    del broken["config4_enformer"]
    l3 = json.loads(bench.compact_line(broken))
    assert "boom" in l3["configs"]["c3_pm"]["error"] and "c4_f32" not in l3["configs"] and "full_json" not in l3


def test_bench_cpu_thread_choice_is_a_rule_not_a_race():
    """cpu_baseline's thread count: fastest per-count minimum; counts within 5 % tie and ties go to the count nearest 16 (round 5's
    driver run chose 8 over 16 on 1.3459 s vs 1.3648 s, the builder's run 16: the GPU / CPU ratio moved 1.7 x between records)."""
    bench = _import_bench()
    assert bench.choose_threads({8: 1.3459, 16: 1.3648, 32: 2.7}) == 16
    assert bench.choose_threads({8: 1.5608, 16: 1.0628, 32: 2.6963}) == 16
    assert bench.choose_threads({8: 1.00, 16: 1.20, 32: 2.0}) == 8
    assert bench.choose_threads({8: 1.2, 16: 1.1, 32: 1.0}) == 32
    assert bench.choose_threads({8: 1.0, 32: 1.01}) == 8
    assert bench.choose_threads({4: 1.0}) == 4


def test_bench_emit_prints_the_compact_line_last(tmp_path, capsys):
    import json
    bench = _import_bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r05_bench_driver_cmd.json")))
    path = tmp_path / "full.json"
    bench.emit(full, str(path))
    cap = capsys.readouterr()
    out_lines = [ln for ln in cap.out.splitlines() if ln.strip()]
    assert len(out_lines) == 1 and len(out_lines[0]) < 6144 and json.loads(out_lines[0])["value"] == full["value"]
    assert cap.err.startswith("BENCH_FULL {") and json.loads(cap.err[len("BENCH_FULL "):])["roofline"] == full["roofline"]
    assert json.load(open(path))["cpu_baseline"] == full["cpu_baseline"]


def test_bench_headline_names_the_workload_it_timed():
    """bench.headline(): the keys of every line, plain or --full. value and ms_per_step come from the same wall time, and the
    workload names the value net the run used (--value-net enformer: the Enformer-shaped trunk, in both modes)."""
    import argparse
    bench = _import_bench()
    args = argparse.Namespace(batch=256, length=200, sample_M=10, diffusion_steps=128, steps=4, warmup=1, rng="philox",
                              value_net="convgru")
    out = torch.zeros(256, 200, dtype=torch.int64)
    line = bench.headline(args, 1, 2.0, out)
    assert line["value"] == 512.0 and line["ms_per_step"] == 500.0 and line["steps"] == 4 and line["dtype"] == "f32"
    assert line["x0_sha1"] == bench._digest(out) and "ConvGRU value net" in line["config"]["workload"]
    assert "Enformer" not in line["config"]["workload"]
    args.value_net = "enformer"
    assert "[value net: Enformer-shaped trunk" in bench.headline(args, 1, 2.0, out)["config"]["workload"]


def test_bench_dump_outputs_is_float32_and_bounded(tmp_path, monkeypatch):
    """--dump-outputs: the tokens as float32 x0.npy, whole when they fit; above the size limit the same seeded sample of rows on
    every call (two builds given the same arguments must stay comparable)."""
    bench = _import_bench()
    x = torch.arange(50 * 7).view(50, 7)                      # row r starts with 7 r
    bench.dump_outputs(str(tmp_path / "whole"), x)
    whole = np.load(tmp_path / "whole" / "x0.npy")
    assert whole.dtype == np.float32 and np.array_equal(whole, x.numpy().astype(np.float32))
    monkeypatch.setattr(bench, "DUMP_LIMIT", 10 * 7 * 4)
    bench.dump_outputs(str(tmp_path / "a"), x)
    bench.dump_outputs(str(tmp_path / "b"), x)
    a, b = np.load(tmp_path / "a" / "x0.npy"), np.load(tmp_path / "b" / "x0.npy")
    rows = (a[:, 0] / 7).astype(int)
    assert a.shape == (10, 7) and np.array_equal(a, b) and np.array_equal(a, whole[rows]) and np.all(np.diff(rows) > 0)


def test_dps_gradient_matches_reference_full_size(golden):
    """g20: compute_gradient_DPS of the PyTorch mirrors (CNNModel.forward2 + ConvGRU reward model, seed 44 in synthetic.build's
    order) against the gradients of the reference's own full-size controlled_sample_DPS run, on the CPU: same framework, same
    kernels — the mirrors must reproduce the reference's autograd to rounding (this is what pins forward2 at full size; the
    GPU test compares the guided q_xs)."""
    from svdd_amd import synthetic
    g = golden("g20_traj_dps_full.npz")
    torch.set_num_threads(4)
    model, _, _, reward = synthetic.build("dna", "cpu")
    for name, mod in (("backbone", model.backbone), ("reward_embedding", reward.embedding), ("reward_head", reward.head)):
        sums = np.array([float(p.double().sum()) for p in mod.state_dict().values()])
        assert np.allclose(sums, g[name + "_param_sums"], rtol=0, atol=1e-6), name
    for p in model.backbone.parameters():
        p.requires_grad_(False)
    for i in range(2):                                        # two of the four steps: a few seconds of CPU autograd
        x = torch.from_numpy(g["xs"][i].astype(np.int64))
        onehot = torch.nn.functional.one_hot(x, 5).float()
        copy = (x != 4).to(x.dtype)
        with torch.enable_grad():
            grad = model.compute_gradient_DPS(onehot, x, reward, torch.zeros(x.shape[0]), copy)
        ref = torch.from_numpy(g["grad"][i])
        assert float((grad - ref).abs().max()) <= 1e-3 * float(ref.abs().max()), (i, float((grad - ref).abs().max()), float(ref.abs().max()))


def test_torch_generator_state_conversion_for_the_device_mt19937():
    """ops.mt_state_from_torch / mt_state_to_torch (the bridge between torch's global CPU generator and the device mt19937 of
    rng_mode = "replay"): the parsed (624 words, pos) continue torch's stream when run by the oracle's mt19937, and ANY window
    of the x[n + 624] = x[n + 397] ^ tw(x[n], x[n + 1]) sequence written back as a state makes torch continue that sequence —
    the device kernel returns such a rotated window (include/svdd_hip.h, svdd_mt19937_uniform_f32)."""
    from oracle import svdd_oracle as orc
    from svdd_amd import ops
    for seed, drawn in ((0, 0), (5, 10), (44, 1010), (7, 624), (9, 623)):
        torch.manual_seed(seed)
        if drawn:
            torch.rand(drawn)
        st = torch.get_rng_state()
        wp = ops.mt_state_from_torch(st)
        assert wp[624] == (624 if drawn in (0, 624) else drawn % 624)
        m = orc.MT19937(0)
        for k in range(624):
            m.mt[k] = int(wp[k])
        m.pos = int(wp[624])
        assert np.array_equal(m.torch_rand(2000), torch.rand(2000).numpy())
    # a rotated window: x = the raw (untempered) sequence, from the oracle's successive state arrays
    torch.manual_seed(3)
    st = torch.get_rng_state()
    m = orc.MT19937(3)
    m.torch_rand(1)                                  # forces the first twist: m.mt = x[624 .. 1247] of the sequence seeded at x[0 .. 623]
    blocks = [np.array(m.mt[:], dtype=np.int64)]
    for _ in range(3):
        m.pos = 624
        m.torch_rand(1)
        blocks.append(np.array(m.mt[:], dtype=np.int64))
    x = np.concatenate(blocks)                       # x[624 ..] relative to the seed block; index 0 here = output #0
    expect = torch.rand(4 * 624).numpy()             # the outputs of exactly these words
    for E, pos in ((227, 170), (454, 624), (100, 1), (681, 333)):
        wp = np.concatenate([x[E:E + 624], [pos]])
        torch.set_rng_state(ops.mt_state_to_torch(wp, st))
        got = torch.rand(500).numpy()
        assert np.array_equal(got, expect[E + pos:E + pos + 500]), (E, pos)
    with pytest.raises(ops.SvddError):
        ops.mt_state_to_torch(np.concatenate([x[:624], [0]]), st)
    with pytest.raises(ops.SvddError):
        ops.mt_state_from_torch(torch.zeros(100, dtype=torch.uint8))


def test_generated_step_listings_are_in_sync_with_their_generator():
    """The unrolled (chunk, row tile) listings of backbone_lp_t_kernel are generated text inside svdd_lp_backbone.hip: the block
    between the markers must be exactly what tools/gen_lpt_taps.py prints (edit the generator, then --write)."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_lpt_taps", os.path.join(root, "tools", "gen_lpt_taps.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    src = open(gen.SRC).read()
    block = gen.block()
    assert block in src
    for n in (13, 7, 6, 5, 4):                       # 4 chunks x n steps, each chunk requests the next weight tile exactly once
        body = block.split(f"#define LPT_TAP{n}(S)")[1].split("#define")[0]
        assert body.count("S(") == 4 * n and body.count("LPT_WLD0(") == 4


def test_tile_plan_never_costs_more_than_one_tile_size(tmp_path):
    """csrc/svdd_spt.h (host + device code): the two-size tile plan of the fp32 backbone covers every sequence exactly once, in
    order, and under the header's own cost model never costs more than the best single tile size."""
    import subprocess
    src = tmp_path / "plan.cpp"
    src.write_text(r'''
#define __host__
#define __device__
#include <cstdio>
#include <initializer_list>
#include "svdd_spt.h"
int main() {
  long long worse = 0, cases = 0, better = 0;
  for (int L : {9, 33, 50, 100, 104}) for (int ncu : {8, 256}) for (int fixed : {9, 26}) for (int n = 1; n <= 3000; n += (n < 600 ? 1 : 7)) {
    const SvddTilePlan p = svdd_plan_tiles(n, L, ncu, fixed);
    const int tiles = svdd_plan_num_tiles(p, n);
    int next = 0;
    for (int t = 0; t < tiles; ++t) { int s0, ns; svdd_plan_tile(p, t, s0, ns); if (s0 != next || ns < 1 || ns > 208 / L) return 2; next = s0 + ns; }
    if (next < n || next - n >= (p.n1 < tiles ? p.s2 : p.s1)) return 3;
    auto cost1 = [&](int s) { long long tl = (n + s - 1) / s; return ((tl + ncu - 1) / ncu) * svdd_tile_cost((s * L + 15) / 16, fixed); };
    const long long single = cost1(svdd_choose_spt(n, L, ncu, fixed));
    const long long r = n - (long long)p.n1 * p.s1;
    long long mixed = (long long)(p.n1 / ncu) * svdd_tile_cost((p.s1 * L + 15) / 16, fixed);
    if (r > 0) { long long tl = (r + p.s2 - 1) / p.s2; mixed += ((tl + ncu - 1) / ncu) * svdd_tile_cost((p.s2 * L + 15) / 16, fixed); }
    if (p.n1 % ncu) return 4;
    worse += mixed > single; better += mixed < single; ++cases;
  }
  std::printf("%lld %lld %lld\n", cases, worse, better);
  return worse ? 1 : 0;
}''')
    exe = tmp_path / "plan"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "svdd_amd", "csrc"), "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout)
    cases, worse, better = map(int, out.stdout.split())
    assert worse == 0 and better > 0 and cases > 10000


_SAME_STATE_WORKER = r"""
import os, sys, hashlib, torch
sys.path.insert(0, {root!r})
import torch.distributed as dist
from svdd_amd import distributed
rank, world, local = distributed.init_from_env("gloo")
assert world == 2
def state_hash():
    return int.from_bytes(hashlib.sha1(torch.get_rng_state().numpy().tobytes()).digest()[:8], "little", signed=True)
torch.manual_seed(0)
distributed.assert_same_on_all_ranks(state_hash(), "generator state")          # equal seeds: passes on both ranks
torch.manual_seed(rank)                                                         # the common torchrun habit: a seed per rank
try:
    distributed.assert_same_on_all_ranks(state_hash(), "generator state")
    raised = False
except RuntimeError as e:
    raised = "differs between ranks" in str(e)
assert raised, "a per-rank seed must be refused"
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_sharded_replay_refuses_ranks_with_different_generator_states(tmp_path):
    """distributed.assert_same_on_all_ranks — the check a sharded replay decode makes at its first draw (every rank replays the WHOLE
    batch's mt19937 stream and slices its rows, which is only the reference's run if all ranks start from the same generator state):
    equal seeds pass, a seed per rank raises on every rank. Two gloo ranks on the CPU."""
    script = tmp_path / "same_state.py"
    script.write_text(_SAME_STATE_WORKER.format(root=ROOT))
    port = 31500 + os.getpid() % 2000
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert res.stdout.count("ok") == 2
