"""ctypes binding of libsvdd_hip.so (include/svdd_hip.h).

The HIP library is the product: there is NO CPU or PyTorch fallback for the hot-path
operators. Importing this module without the built library, or calling an operator
without a gfx950 device, raises.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# SVDD_HIP_LIB: load another build of the library instead (the timing-experiment scripts under tools/ build patched
# copies of the kernels in a scratch directory; the tracked sources are never edited in place)
SO_PATH = os.environ.get("SVDD_HIP_LIB") or os.path.join(CSRC, "libsvdd_hip.so")
ABI_VERSION = 17

OK, E_ARG, E_LAUNCH, E_NODEVICE = 0, -1, -2, -3
LAYOUT_BLV, LAYOUT_BVL = 0, 1
RNG_REPLAY, RNG_PHILOX = 0, 1
SELECT_ARGMAX, SELECT_MULTINOMIAL = 0, 1
TARGET_MEAN, TARGET_LOGMEANEXP = 0, 1                              # SVDD_TARGET_* of include/svdd_hip.h
EVOLVE_GLOBAL, EVOLVE_ROW = 0, 1                                   # SVDD_EVOLVE_* of include/svdd_hip.h
ATTR_GRADIENT, ATTR_TIMES_INPUT = 0, 1                             # SVDD_ATTR_* of include/svdd_hip.h
PRECISIONS = {"f32": 0, "f16x3": 1, "bf16x3": 2, "f16": 3, "bf16": 4}      # enum SVDD_PREC_* of include/svdd_hip.h
MAX_M = 1024
PATTERN_MAX_WIDTH = 32                                             # SVDD_PATTERN_MAX_WIDTH of include/svdd_hip.h (= motifs.MAX_WIDTH)

# enum SVDD_OPT_* of include/svdd_hip.h (tests/test_host_cpu.py compares names and values with the header)
OPT_FORCE_EXACT, OPT_MSPLIT, OPT_SELECT_ONE_ROW, OPT_BACKBONE_LP_VERSION, OPT_TRUNK_GEMM_VERSION = 0, 1, 2, 3, 4
OPT_CAND_ROW_STRIDE, OPT_TRUNK_PLANES_F32, OPT_BACKBONE_SPLIT, OPT_SELECT_BATCHES = 5, 6, 7, 8


class SvddRng(ctypes.Structure):
    """struct svdd_rng (include/svdd_hip.h)."""
    _fields_ = [("kind", ctypes.c_int32), ("step", ctypes.c_uint32), ("uniforms", ctypes.c_void_p),
                ("seed", ctypes.c_uint64), ("row_offset", ctypes.c_uint64),
                ("uniforms_layout", ctypes.c_int32), ("uniforms_rows", ctypes.c_int32)]


class SvddLedidiCfg(ctypes.Structure):
    """struct svdd_ledidi_cfg (include/svdd_hip.h)."""
    _fields_ = [(n, ctypes.c_float) for n in ("tau", "l", "la", "lb", "scale", "decay", "w1", "beta2", "w2", "adam_eps", "step_size",
                                              "bc2_sqrt")] + [("patience", ctypes.c_int32)]


class SvddError(RuntimeError):
    pass


vp, cstr, i32, i64, f32, f64 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double
pi32, pf64, RNG = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(SvddRng)      # host pointers
LCFG = ctypes.POINTER(SvddLedidiCfg)


class STREAM(ctypes.c_void_p):
    """The hipStream_t a launch goes to. Always the last parameter; call() fills it with torch's current stream."""


# Every exported function -> its parameter types, in the header's order (tests/test_host_cpu.py compares each entry with the
# prototype in include/svdd_hip.h). All return int (0 or a negative SVDD_E_* code).
SIGNATURES = {
    "svdd_abi_version": (),
    "svdd_device_info": (cstr, i32, pi32),
    "svdd_propose": (vp, vp, f32, f32, i32, i32, i32, i32, RNG, vp, vp, vp, STREAM),
    "svdd_sample_categorical": (vp, vp, i32, i32, i32, i32, RNG, vp, vp, STREAM),
    "svdd_select": (vp, vp, i32, i32, i32, i32, RNG, vp, vp, vp, STREAM),
    "svdd_x0hat": (vp, vp, i32, i32, i32, vp, vp, STREAM),
    "svdd_finalize": (vp, vp, i32, i32, i32, vp, vp, STREAM),
    "svdd_transform_samples": (vp, i32, i32, i32, vp, STREAM),
    "svdd_subs_logp": (vp, vp, i32, i32, i32, vp, STREAM),
    "svdd_tds_resample": (vp, vp, f64, vp, vp, i32, i32, vp, vp, vp, STREAM),
    "svdd_set_option": (i32, i32),
    "svdd_selftest_fastmath": (pf64,),
    "svdd_profile_enable": (i32,),
    "svdd_profile_collect": (i32, pf64, pi32),
    "svdd_gru_bidir_f32": (vp, vp, vp, vp, i32, i32, vp, STREAM),
    "svdd_gru_bidir_train_f32": (vp, vp, vp, vp, vp, i32, i32, STREAM),
    "svdd_gru_bidir_bwd_f32": (vp, vp, vp, vp, vp, i32, i32, STREAM),
    "svdd_epilogue_ln_f32": (vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, STREAM),
    "svdd_conv1d_cl_f32": (vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, STREAM),
    "svdd_conv1d_set_dynamic": (i32,),
    "svdd_gru_set_mode": (i32,),
    "svdd_conv_tower_f32": (vp, vp, vp, vp, i32, i32, i32, i32, vp, STREAM),
    "svdd_backbone_cnn_f32": (vp, vp, vp, vp, vp, vp, i32, i32, i32, pi32, vp, vp, i32, STREAM),
    "svdd_backbone_incr_f32": (vp, vp, vp, vp, vp, vp, i32, i32, i32, pi32, i32, vp, vp, vp, vp, i32, i32, vp),
    "svdd_backbone_incr2_f32": (vp, vp, vp, vp, vp, vp, i32, i32, i32, pi32, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp),
    "svdd_backbone_incr3_f32": (vp, vp, vp, vp, vp, vp, i32, i32, i32, pi32, i32, vp, vp, vp, vp, i32, i32, vp, vp, i32, vp),
    "svdd_backbone_incr_set_residency": (i32,),
    "svdd_value_tail_f32": (vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, STREAM),
    "svdd_candidate_windows": (vp, vp, i32, i32, i32, i32, vp, vp, STREAM),
    "svdd_conv_tower_windows_f32": (vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, STREAM),
    "svdd_k1_stats": (vp,),
    "svdd_backbone_cnn_lp": (vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, pi32, i32, vp, vp, i32, STREAM),
    "svdd_conv_tower_lp": (vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, STREAM),
    "svdd_conv_tower_windows_lp": (vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, STREAM),
    "svdd_gru_bidir_lp": (vp, vp, vp, vp, vp, vp, i32, i32, vp, i32, STREAM),
    "svdd_value_tail_lp": (vp, vp, vp, vp, vp, vp, f32, vp, i32, i32, i32, vp, i32, STREAM),
    "svdd_compact_flags": (vp, i32, vp, vp, vp, STREAM),
    "svdd_compact_by_key": (vp, i32, vp, vp, vp, i32, STREAM),
    "svdd_gather_rows": (vp, vp, vp, i32, i32, vp, STREAM),
    "svdd_advance_rows": (vp, vp, vp, i32, i32, i32, vp, STREAM),
    "svdd_select_compact": (vp, vp, vp, vp, i32, i32, i32, i32, RNG, vp, vp, vp, vp, vp, STREAM),
    "svdd_set_tower_version": (i32,),
    "svdd_set_backbone_packing": (i32,),
    "svdd_trunk_gemm": (vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, i32, vp, vp, vp, vp, i32, i32, STREAM),
    "svdd_trunk_act_split": (vp, vp, vp, i32, i64, i32, i32, i32, vp, vp, vp, STREAM),
    "svdd_trunk_layernorm_split": (vp, vp, vp, f32, i64, i32, vp, vp, vp, i32, STREAM),
    "svdd_trunk_attn_pool": (vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, STREAM),
    "svdd_trunk_stem_unfold": (vp, i32, i32, vp, vp, STREAM),
    "svdd_trunk_attn_small": (vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, STREAM),
    "svdd_trunk_windows": (vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, STREAM),
    "svdd_trunk_stem_unfold_win": (vp, i32, i32, i32, vp, vp, vp, vp, vp, STREAM),
    "svdd_trunk_attn_pool_win": (vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, STREAM),
    "svdd_bb_layer_fwd_f32": (vp, vp, vp, vp, vp, vp, f32, vp, vp, vp, i64, i32, i32, STREAM),
    "svdd_bb_layer_bwd_f32": (vp, vp, vp, vp, f32, vp, vp, vp, vp, i64, i32, i32, STREAM),
    "svdd_mt19937_uniform_f32": (vp, vp, i64, STREAM),
    "svdd_backbone_set_workspace": (vp, i64),
    "svdd_backbone_split_status": (pi32,),
    "svdd_backbone_cnn_save_f32": (vp, vp, vp, vp, vp, vp, i32, i32, i32, pi32, vp, vp, vp, STREAM),
    "svdd_backbone_cnn_grad_f32": (vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, pi32, STREAM),
    "svdd_dps_probs": (vp, vp, i32, i32, vp, STREAM),
    "svdd_dps_probs_bwd": (vp, vp, vp, i32, i32, vp, vp, STREAM),
    "svdd_dps_guided_q": (vp, vp, vp, vp, f32, f32, f32, i32, i32, vp, STREAM),
    "svdd_reward_stem_f32": (vp, vp, vp, vp, i32, i32, i32, STREAM),
    "svdd_reward_stem_bwd_f32": (vp, vp, vp, i32, i32, i32, STREAM),
    "svdd_conv1d_cl_gated_f32": (vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, STREAM),
    "svdd_reward_tail_grad_f32": (vp, vp, vp, vp, vp, vp, vp, f32, i32, i32, vp, vp, STREAM),
    "svdd_sum_gate_f32": (vp, vp, vp, vp, i64, STREAM),
    "svdd_gru_bidir_train2_f32": (vp, vp, vp, vp, vp, vp, i32, i32, STREAM),
    "svdd_gru_bidir_bwd2_f32": (vp, vp, vp, vp, vp, vp, vp, i32, i32, STREAM),
    "svdd_classifier_propose": (vp, i32, vp, vp, f32, f32, f32, i32, i32, RNG, vp, vp, vp, STREAM),
    "svdd_elbo_mask": (vp, i32, i32, i32, f64, RNG, vp, vp, vp, vp, vp, vp, STREAM),
    "svdd_elbo_nll": (vp, i32, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, STREAM),
    "svdd_refine_remask": (vp, vp, vp, vp, vp, f32, i32, i32, RNG, vp, vp, vp, vp, vp, vp, vp),
    "svdd_value_target": (vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp),
    "svdd_ism_mutants": (vp, vp, vp, i32, i32, i32, vp, vp, vp, vp),
    "svdd_ism_fold": (vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp),
    "svdd_evolve_apply": (vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp),
    "svdd_attr_path": (vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp),
    "svdd_attr_fold": (vp, f32, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp),
    "svdd_ledidi_step": (vp, vp, vp, vp, vp, LCFG, RNG, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                         vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp),
    "svdd_candidate_windows_tight": (vp, vp, i32, i32, i32, i32, vp, vp, vp),
    "svdd_kmer_counts": (vp, i32, i32, i32, vp, vp, vp),
    "svdd_pack_tokens": (vp, i32, i32, vp, vp, vp),
    "svdd_hamming_nn": (vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp),
    "svdd_edit_nn": (vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp),
    "svdd_within": (vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, i32, vp),
    "svdd_greedy_pick": (vp, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp),
    "svdd_edit_within": (vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, vp),
    "svdd_edit_pairs": (vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp),
    "svdd_motif_scan": (vp, i32, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp),
    "svdd_motif_reward": (vp, i32, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, f32, vp, vp, vp, vp),
    "svdd_candidate_parts": (vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp),
    "svdd_conv_tower_parts_f32": (vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp),
    "svdd_backbone_incr4_f32": (vp, vp, vp, vp, vp, vp, i32, i32, i32, pi32, i32, vp, vp, vp, vp, i32, i32, vp, vp, i32, vp, i32, vp),
    "svdd_pattern_mutants": (vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp),
    "svdd_pattern_fold": (vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp),
    "svdd_pattern_apply": (vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp),
    "svdd_backbone_incr_seed_f32": (vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, i32, vp),
    "svdd_value_late_step_f32": (vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp),
}
EXPORTS = tuple(SIGNATURES)


def build(force=False):
    """Compile every csrc/*.hip for gfx950 (hipcc cross-compiles without a GPU); stale = any *.hip / *.h / Makefile newer."""
    import glob
    srcs = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")) + [os.path.join(CSRC, "Makefile")])
    srcs.append(os.path.join(os.path.dirname(_HERE), "include", "svdd_hip.h"))
    if os.environ.get("SVDD_HIP_LIB"):
        return SO_PATH                                   # an explicitly chosen build is used as it is
    stale = not os.path.exists(SO_PATH) or os.path.getmtime(SO_PATH) < max(os.path.getmtime(f) for f in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC, "-B", "-j", str(min(8, os.cpu_count() or 1))])   # one job per translation unit
    return SO_PATH


_lib = None


def lib():
    """Load libsvdd_hip.so. torch is imported first so that the library binds to the HIP
    runtime already resident in the process (same libamdhip64 SONAME) instead of a second copy."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (loads torch's bundled libamdhip64.so.7 first)
    if not os.path.exists(SO_PATH):
        raise SvddError(f"{SO_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "or `make -C svdd_amd/csrc`. There is no CPU fallback for the SVDD hot path.")
    L = ctypes.CDLL(SO_PATH)
    for name in EXPORTS:
        if not hasattr(L, name):
            raise SvddError(f"libsvdd_hip.so does not export {name}")
    if L.svdd_abi_version() != ABI_VERSION:
        raise SvddError(f"libsvdd_hip.so ABI {L.svdd_abi_version()} != binding ABI {ABI_VERSION}; rebuild")
    for name, sig in SIGNATURES.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = [vp if t is STREAM else t for t in sig], ctypes.c_int
    _lib = L
    return L


_CALLS = {}            # name -> (ctypes function, parameters the caller passes, pointer positions, number positions, takes the stream)
_NUMBERS = (int, float, bool)
_Tensor = _current_stream = None


def _resolve(name):
    """The per-function facts of call(), read from SIGNATURES once per function."""
    global _Tensor, _current_stream
    if name not in SIGNATURES:
        raise SvddError(f"{name} is not a function of libsvdd_hip.so (include/svdd_hip.h)")
    import torch
    _Tensor, _current_stream = torch.Tensor, torch.cuda.current_stream
    sig = SIGNATURES[name]
    stream = bool(sig) and sig[-1] is STREAM
    sig = sig[:len(sig) - stream]
    numbers = tuple(i for i, t in enumerate(sig) if t in (i32, i64, f32, f64))
    ent = _CALLS[name] = (getattr(lib(), name), len(sig), tuple(i for i in range(len(sig)) if i not in numbers), numbers, stream)
    return ent


def call(name, *args):
    """The one door to the library: svdd_<name>(*args) on torch's current stream, return code checked under the function's own
    name. In a pointer parameter a tensor stands for its data_ptr() and None for NULL; ints and ctypes objects (byref(...), arrays)
    pass as they are. A tensor where the function takes a number raises instead of being read as an address. The stream is
    appended here for the functions whose entry in SIGNATURES ends in STREAM: callers never pass it."""
    fn, n, pointers, numbers, stream = _CALLS.get(name) or _resolve(name)
    if len(args) != n:
        raise TypeError(f"{name} takes {n} arguments{' (and the stream, which call() adds)' if stream else ''}, got {len(args)}")
    args = list(args)
    for i in pointers:
        a = args[i]
        if a is not None and isinstance(a, _Tensor):
            args[i] = a.data_ptr()
    for i in numbers:
        if args[i].__class__ not in _NUMBERS and isinstance(args[i], _Tensor):
            raise TypeError(f"{name}: argument {i} is a number, got a tensor (pass int(...) / float(...) of it)")
    if stream:
        args.append(_current_stream().cuda_stream)
    check(fn(*args), name)


def device_info():
    buf = ctypes.create_string_buffer(64)
    ncu = ctypes.c_int(0)
    rc = lib().svdd_device_info(buf, 64, ctypes.byref(ncu))
    if rc != OK:
        raise SvddError("no HIP device visible to libsvdd_hip.so")
    return buf.value.decode().split(":")[0], ncu.value


_OPTIONS = {}          # (key, sub) -> the value this process last set through set_option (absent: the library default)
_OPTION_DEFAULTS = {(OPT_TRUNK_GEMM_VERSION, "version"): 2, (OPT_TRUNK_GEMM_VERSION, "height"): 40, (OPT_TRUNK_GEMM_VERSION, "concurrency"): 51}


def _option_slot(key, value):
    """SVDD_OPT_TRUNK_GEMM_VERSION multiplexes three settings on one key (include/svdd_hip.h): kernel version, tile height (40 - 42),
    chains sharing the chip (51 - 54). Each is remembered separately."""
    if key == OPT_TRUNK_GEMM_VERSION:
        return (key, "height" if 40 <= value <= 42 else "concurrency" if 51 <= value <= 54 else "version")
    return (key, None)


def current_option(key, like=0):
    """The value last set for `key` (for OPT_TRUNK_GEMM_VERSION: for the setting `like` belongs to)."""
    slot = _option_slot(key, like)
    return _OPTIONS.get(slot, _OPTION_DEFAULTS.get(slot, 0))


def set_option(key, value):
    """svdd_set_option through one door that remembers what was set -> the PREVIOUS value of that setting, so that a scoped change
    can put back what its caller had chosen instead of a constant."""
    key, value = int(key), int(value)
    prev = current_option(key, value)
    check(lib().svdd_set_option(key, value), f"svdd_set_option({key}, {value})")
    _OPTIONS[_option_slot(key, value)] = value
    return prev


def set_force_exact(on):
    """A/B switch: K1 evaluates every draw in the exact arithmetic (same results, slower)."""
    set_option(OPT_FORCE_EXACT, int(bool(on)))


def profile_enable(on=True):
    call("svdd_profile_enable", int(bool(on)))


def profile_collect(kernel):
    """(total_ms, launches) of kernel 0 = propose / 1 = select since profiling was enabled."""
    tot, n = ctypes.c_double(0.0), ctypes.c_int(0)
    call("svdd_profile_collect", kernel, ctypes.byref(tot), ctypes.byref(n))
    return tot.value, n.value


def selftest_fastmath():
    """(max rel err of fast g over all 2^24 uniforms, of fast exp on [-80,0], of fast log on (1,4])."""
    out = (ctypes.c_double * 3)()
    call("svdd_selftest_fastmath", out)
    return tuple(out)


_ERR = {E_ARG: "invalid argument", E_LAUNCH: "kernel launch failed", E_NODEVICE: "no HIP device"}


def check(rc, what):
    if rc != OK:
        raise SvddError(f"{what}: {_ERR.get(rc, rc)}")
