"""ctypes binding of libimh_hip.so (include/imh.h).

The product path has NO CPU fallback: if the shared library is missing or fails to load,
importing any op raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"``
(hipcc --offload-arch=gfx950, in-tree).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# IMH_LIB_PATH overrides; IMH_EXPERIMENTAL=1 (the switch build.py compiles the experimental library under) selects that library by itself,
# so that the one variable builds AND loads the same file
_EXP_PATH = os.path.join(_HERE, "..", "tools", "tmp_libs", "libimh_hip_experimental.so")
LIB_PATH = os.environ.get("IMH_LIB_PATH") or (_EXP_PATH if os.environ.get("IMH_EXPERIMENTAL") == "1" else os.path.join(_HERE, "libimh_hip.so"))

ABI_VERSION = 13
IMH_DT_BF16, IMH_DT_F16 = 0, 1
GF_GEGLU, GF_ACT_GELU, GF_ACT_SILU, GF_VT_PERM, GF_OUT_F32, GF_LN_ROW, GF_LN_COL, GF_ACT_QGELU = 1, 2, 4, 8, 16, 32, 64, 128
OP_GEMM, OP_ATTN, OP_GROUPNORM, OP_LAYERNORM, OP_EW, OP_ATTN_SMALL, OP_GEMM_DUAL, OP_XATTN, OP_ATTN_ENC, OP_ATTN_ENC_CAUSAL = range(10)
OP_STEP_SEEDED, OP_RANDN_SEEDED = 10, 11      # the seeded step noise (imh.h): additive plan kinds
OP_CLIP_PREPROCESS = 13                       # imh_clip_preprocess (imh.h: kind 12 stays refused)
OP_CONTROL_ADD = 15                           # imh_control_add: the ControlNet's gated residual add (+ GroupNorm partials of the sum); 12 and 14 stay refused
OP_XATTN_REGIONS = 17                         # imh_cross_attention_regions (include/imh_regions.h): N masked image prompts; 12, 14 and 16 stay refused
# (OPS, below the argument structs, gives every kind its struct and its eager entry point)
CLIP_DT_F32 = 2                               # imh_clip_preprocess's fp32 rows (no other entry takes it)
GN_ALL, GN_STATS, GN_TABLE, GN_APPLY, GN_TABLE_APPLY = 0, 1, 2, 3, 4
(EW_TIMESTEP, EW_SILU, EW_CONCAT, EW_CONV_IN, EW_CFG_STEP, EW_CAST_F32, EW_ADD, EW_STEP_SET, EW_CFG_RESCALE, EW_SOFTMAX,
 EW_ROW_STATS, EW_STEP_ROW, EW_GATHER_ROWS, EW_CFG_MSTEP) = range(14)

# variant codes / modes that only a -DIMH_EXPERIMENTAL build compiles (csrc/imh_common.h IMH_EXP_ONLY): measured, selected by no
# tuning.json entry and no default mode.  experimental() asks the loaded library (imh_debug_set(1, 0)).
EXP_VARIANTS = {(4064, 64), (4064, 128), (4128, 64), (5256, 320), (6128, 320), (6064, 160), (7064, 160), (256, 128), (256, 256), (22128, 160),
                (3128, 128), (24128, 128), (9256, 320), (7564, 320), (7564, 160), (7328, 160), (7428, 160), (7256, 80)}


def experimental():
    return load().imh_debug_set(1, 0) == 1


def variant_built(cfg):
    """cfg = (bm, bn[, splits]): is this tile variant in the loaded library?"""
    return (int(cfg[0]), int(cfg[1])) not in EXP_VARIANTS or experimental()


_i32, _f32, _vp = C.c_int32, C.c_float, C.c_void_p


class GemmArgs(C.Structure):
    _fields_ = [("X", _vp), ("W", _vp), ("Y", _vp), ("partial", _vp), ("bias", _vp), ("rowadd", _vp),
                ("residual", _vp), ("ln_s", _vp), ("ln_c", _vp), ("ln_eps", _f32),
                ("ln_stats", _vp), ("ln_stats_out", _vp), ("ln_slots", _i32), ("ln_slots_out", _i32),
                ("gn_out", _vp), ("gn_nblk", _i32), ("gn_hw", _i32), ("gn_tab", _vp), ("gn_silu", _i32),
                ("gn_part", _vp), ("gn_part2", _vp), ("gn_gamma", _vp), ("gn_beta", _vp), ("gn_eps", _f32), ("gn_groups", _i32), ("gn_pC1", _i32),
                ("gn_pnblk", _i32), ("gn_psub", _i32), ("gn_pnpart", _i32), ("gn_pnblk2", _i32), ("gn_psub2", _i32), ("gn_pnpart2", _i32),
                ("X2", _vp), ("Cin1", _i32), ("Yt", _vp), ("yt_col0", _i32), ("ldyt", _i32),
                ("M", _i32), ("N", _i32), ("K", _i32),
                ("ldx", _i32), ("ldw", _i32), ("ldy", _i32), ("ldr", _i32), ("ldra", _i32),
                ("rows_per_batch", _i32), ("splits", _i32), ("flags", _i32),
                ("H", _i32), ("Wd", _i32), ("Cin", _i32), ("Ho", _i32), ("Wo", _i32), ("stride", _i32), ("up", _i32),
                ("dtype", _i32), ("conv", _i32), ("bm", _i32), ("bn", _i32), ("pf_ptr", _vp), ("pf_bytes", C.c_uint32), ("xcd", _i32),
                ("pad", _i32)]


class AttnArgs(C.Structure):
    _fields_ = [("Q", _vp), ("K", _vp), ("Vt", _vp), ("K2", _vp), ("Vt2", _vp), ("O", _vp),
                ("B", _i32), ("H", _i32), ("Lq", _i32), ("Lk", _i32), ("Lk_pad", _i32), ("Lk2", _i32),
                ("Lk2_pad", _i32),
                ("ldq", _i32), ("ldk", _i32), ("ldvt", _i32), ("ldk2", _i32), ("ldvt2", _i32), ("ldo", _i32),
                ("scale", _f32), ("scale2", _f32), ("scale2_tab", _vp), ("step", _vp), ("dtype", _i32),
                ("pf_ptr", _vp), ("pf_bytes", C.c_uint32)]


class XAttnArgs(C.Structure):
    _fields_ = [("X", _vp), ("Wq", _vp), ("ln_s", _vp), ("ln_c", _vp), ("ln_eps", _f32), ("ln_stats", _vp), ("ln_slots", _i32),
                ("K", _vp), ("Vt", _vp), ("K2", _vp), ("Vt2", _vp), ("O", _vp),
                ("B", _i32), ("H", _i32), ("Lq", _i32), ("C", _i32), ("Lk", _i32), ("Lk_pad", _i32), ("Lk2", _i32),
                ("Lk2_pad", _i32),
                ("ldx", _i32), ("ldw", _i32), ("ldk", _i32), ("ldvt", _i32), ("ldk2", _i32), ("ldvt2", _i32), ("ldo", _i32),
                ("scale", _f32), ("scale2", _f32), ("scale2_tab", _vp), ("step", _vp), ("dtype", _i32),
                ("pf_ptr", _vp), ("pf_bytes", C.c_uint32)]


class XAttnRegionsArgs(C.Structure):
    """imh_xattn_regions_args (include/imh_regions.h): XAttnArgs' fields, then the regions' own"""
    _fields_ = XAttnArgs._fields_ + [("n_img", _i32), ("mask", _vp), ("ldm", _i32), ("weights", _vp)]


REGIONS_MAX_IMAGES = 8


class SmallAttnArgs(C.Structure):
    _fields_ = [("Q", _vp), ("K", _vp), ("V", _vp), ("O", _vp),
                ("B", _i32), ("H", _i32), ("Lq", _i32), ("Lk", _i32), ("dq", _i32), ("dv", _i32),
                ("ldq", _i32), ("ldk", _i32), ("ldv", _i32), ("ldo", _i32), ("scale", _f32), ("dtype", _i32)]


class EncAttnArgs(C.Structure):
    _fields_ = [("Q", _vp), ("K", _vp), ("V", _vp), ("O", _vp),
                ("B", _i32), ("H", _i32), ("L", _i32), ("d", _i32),
                ("ldq", _i32), ("ldk", _i32), ("ldv", _i32), ("ldo", _i32), ("scale", _f32), ("dtype", _i32)]


class NormArgs(C.Structure):
    _fields_ = [("x", _vp), ("y", _vp), ("gamma", _vp), ("beta", _vp), ("partial", _vp),
                ("B", _i32), ("HW", _i32), ("C", _i32), ("groups", _i32), ("rows", _i32),
                ("eps", _f32), ("silu", _i32), ("dtype", _i32),
                ("mode", _i32), ("table", _vp), ("partial2", _vp), ("nblk", _i32), ("sub", _i32), ("npart", _i32), ("C1", _i32),
                ("nblk2", _i32), ("sub2", _i32), ("npart2", _i32), ("pf_ptr", _vp), ("pf_bytes", C.c_uint32)]


class EwArgs(C.Structure):
    _fields_ = [("a", _vp), ("b", _vp), ("y", _vp), ("w", _vp), ("bias", _vp), ("tab", _vp), ("step", _vp),
                ("n", C.c_int64),
                ("i0", _i32), ("i1", _i32), ("i2", _i32), ("i3", _i32), ("i4", _i32), ("i5", _i32),
                ("f0", _f32), ("f1", _f32), ("f2", _f32), ("f3", _f32), ("dtype", _i32),
                ("x2", _vp), ("noise", _vp), ("mask", _vp), ("blend_tab", _vp)]


class SeededArgs(C.Structure):
    _fields_ = [("ew", EwArgs), ("seeds", _vp), ("stream", C.c_uint32)]


class RandnArgs(C.Structure):
    _fields_ = [("y", _vp), ("seeds", _vp), ("step", _vp), ("S", _i32), ("HW", _i32), ("row", C.c_uint32), ("stream", C.c_uint32), ("raw", _i32), ("quad0", C.c_uint32)]


class ClipPreprocessArgs(C.Structure):
    _fields_ = [("x", _vp), ("y", _vp), ("S", _i32), ("H", _i32), ("W", _i32), ("nh", _i32), ("nw", _i32), ("top", _i32), ("left", _i32),
                ("size", _i32), ("patch", _i32), ("ldp", _i32), ("mean0", _f32), ("mean1", _f32), ("mean2", _f32),
                ("std0", _f32), ("std1", _f32), ("std2", _f32), ("dtype", _i32)]


class ControlAddArgs(C.Structure):
    _fields_ = [("x", _vp), ("r", _vp), ("y", _vp), ("partial", _vp), ("tab", _vp), ("step", _vp), ("scale", _f32),
                ("B", _i32), ("Br", _i32), ("HW", _i32), ("C", _i32), ("sub", _i32), ("dtype", _i32)]


class AdapterArgs(C.Structure):
    _fields_ = [("x", _vp), ("y", _vp), ("n", C.c_int64), ("mode", _i32), ("N", _i32), ("C", _i32), ("H", _i32), ("W", _i32),
                ("f", _i32), ("Cp", _i32), ("dtype", _i32)]


ADAPTER_UNSHUFFLE, ADAPTER_RELU, ADAPTER_AVGPOOL2 = range(3)      # imh_adapter_op's modes (eager only: no plan kind)


class LoraItem(C.Structure):
    """imh_lora_item (include/imh_lora.h): one adapted weight of the grouped merge; the table is an array of these, on the host and on the device"""
    _fields_ = [("base", _vp), ("dst", _vp), ("U", _vp), ("D", _vp), ("g", _vp), ("N", _i32), ("K", _i32), ("R", _i32),
                ("ld_base", _i32), ("ld_dst", _i32), ("ldu", _i32), ("ldd", _i32), ("pad", _i32)]


class LoraMergeArgs(C.Structure):
    _fields_ = [("items_host", _vp), ("items_dev", _vp), ("tile_start_dev", _vp), ("n_items", _i32), ("total_tiles", _i32), ("dtype", _i32)]


class TinyVaeArgs(C.Structure):
    """imh_tinyvae_args (include/imh_tinyvae.h): one 3 x 3 conv of the AutoencoderTiny decoder"""
    _fields_ = [("x", _vp), ("w", _vp), ("bias", _vp), ("residual", _vp), ("y", _vp), ("B", _i32), ("H", _i32), ("W", _i32),
                ("flags", _i32), ("dtype", _i32)]


TINYVAE_RELU, TINYVAE_UP2, TINYVAE_HEAD, TINYVAE_TAIL = 1, 2, 4, 8      # imh_tinyvae_conv's flags (eager only: no plan kind)


class F32Args(C.Structure):
    _fields_ = [("X", _vp), ("W", _vp), ("Y", _vp), ("bias", _vp), ("residual", _vp), ("gamma", _vp), ("beta", _vp), ("ws", _vp),
                ("M", _i32), ("N", _i32), ("K", _i32), ("ldx", _i32), ("ldw", _i32), ("ldy", _i32), ("ldr", _i32),
                ("conv", _i32), ("H", _i32), ("Wd", _i32), ("Cin", _i32), ("Ho", _i32), ("Wo", _i32), ("up", _i32),
                ("B", _i32), ("HW", _i32), ("C", _i32), ("groups", _i32), ("nblk", _i32), ("silu", _i32),
                ("eps", _f32), ("scale", _f32), ("stride", _i32), ("pad", _i32), ("add_a", _f32), ("add_b", _f32)]


F32_GEMM, F32_GN_STATS, F32_GN_TABLE, F32_GN_APPLY, F32_SOFTMAX, F32_IMG2IMG_INIT = range(6)

# every symbol include/imh.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("imh_abi_version", C.c_int, []),
    ("imh_last_error", C.c_char_p, []),
    ("imh_debug_set", C.c_int, [C.c_int, C.c_int]),
    ("imh_gemm", C.c_int, [C.POINTER(GemmArgs), _vp]),
    ("imh_gemm_dual", C.c_int, [C.POINTER(GemmArgs), C.POINTER(GemmArgs), _vp]),
    ("imh_gemm_pick_config", C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                       C.POINTER(C.c_int)]),
    ("imh_gemm_workspace_bytes", C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    ("imh_gemm_stats_slot_width", C.c_int, [C.c_int, C.c_int]),
    ("imh_gemm_gn_block_rows", C.c_int, [C.c_int, C.c_int]),
    ("imh_conv_halo_lds_bytes", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    ("imh_gemm_check", C.c_int, [C.POINTER(GemmArgs)]),
    ("imh_attention", C.c_int, [C.POINTER(AttnArgs), _vp]),
    ("imh_cross_attention", C.c_int, [C.POINTER(XAttnArgs), _vp]),
    ("imh_attention_small", C.c_int, [C.POINTER(SmallAttnArgs), _vp]),
    ("imh_attention_enc", C.c_int, [C.POINTER(EncAttnArgs), _vp]),
    ("imh_attention_enc_causal", C.c_int, [C.POINTER(EncAttnArgs), _vp]),
    ("imh_groupnorm", C.c_int, [C.POINTER(NormArgs), _vp]),
    ("imh_groupnorm_workspace_bytes", C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    ("imh_groupnorm_stats_blocks", C.c_int, [C.c_int, C.c_int]),
    ("imh_groupnorm_stats_sub", C.c_int, [C.c_int, C.c_int]),
    ("imh_layernorm", C.c_int, [C.POINTER(NormArgs), _vp]),
    ("imh_elementwise", C.c_int, [C.c_int, C.POINTER(EwArgs), _vp]),
    ("imh_step_seeded", C.c_int, [C.POINTER(SeededArgs), _vp]),
    ("imh_randn_seeded", C.c_int, [C.POINTER(RandnArgs), _vp]),
    ("imh_randn_seeded_host", C.c_int, [C.POINTER(RandnArgs)]),
    ("imh_clip_preprocess", C.c_int, [C.POINTER(ClipPreprocessArgs), _vp]),
    ("imh_control_add", C.c_int, [C.POINTER(ControlAddArgs), _vp]),
    ("imh_f32", C.c_int, [C.c_int, C.POINTER(F32Args), _vp]),
    ("imh_plan_create", _vp, []),
    ("imh_plan_destroy", None, [_vp]),
    ("imh_plan_add", C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int]),
    ("imh_plan_size", C.c_int, [_vp]),
    ("imh_plan_update", C.c_int, [_vp, C.c_int, _vp]),
    ("imh_plan_run", C.c_int, [_vp, _vp]),
    ("imh_plan_run_range", C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    ("imh_plan_capture", C.c_int, [_vp, _vp]),
    ("imh_plan_replay", C.c_int, [_vp, _vp]),
    ("imh_plan_time_ops", C.c_int, [_vp, _vp, C.POINTER(C.c_float), C.c_int]),
    ("imh_plan_get_tag", C.c_int, [_vp, C.c_int]),
    ("imh_plan_get_kind", C.c_int, [_vp, C.c_int]),
]

# the one symbol include/imh_adapter.h declares (the T2I-Adapter's per-image passes): a companion header, a companion list -- SYMBOLS is
# what include/imh.h declares, name for name
ADAPTER_SYMBOLS = [
    ("imh_adapter_op", C.c_int, [C.POINTER(AdapterArgs), _vp]),
]

# ... and the one of include/imh_regions.h (regional image prompts)
REGIONS_SYMBOLS = [
    ("imh_cross_attention_regions", C.c_int, [C.POINTER(XAttnRegionsArgs), _vp]),
]

# ... and the two of include/imh_lora.h (the grouped low-rank merge: eager only, no plan kind)
LORA_SYMBOLS = [
    ("imh_lora_merge_tiles", C.c_int, [C.c_int, C.c_int]),
    ("imh_lora_merge", C.c_int, [C.POINTER(LoraMergeArgs), _vp]),
]

# ... and the one of include/imh_tinyvae.h (the AutoencoderTiny decoder's conv: eager only, no plan kind)
TINYVAE_SYMBOLS = [
    ("imh_tinyvae_conv", C.c_int, [C.POINTER(TinyVaeArgs), _vp]),
]


# how an eager entry point takes a launch: (entry, args, element-wise op code, stream) -> status
def _launch(fn, a, op, s):
    return fn(C.byref(a), s)


def _launch_op(fn, a, op, s):                 # imh_elementwise: the op code comes first
    return fn(op, C.byref(a), s)


def _launch_pair(fn, a, op, s):               # imh_gemm_dual: a is (GemmArgs * 2), handed over as two pointers
    return fn(C.byref(a[0]), C.byref(a[1]), s)


# the op table: plan kind -> (argument struct, eager entry point, how that entry is called).  What records under a kind (imh_plan_add copies
# sizeof(struct) bytes, twice that for the pair) is what its entry launches eagerly; Ctx._emit goes through here for both
OPS = {
    OP_GEMM: (GemmArgs, "imh_gemm", _launch),
    OP_ATTN: (AttnArgs, "imh_attention", _launch),
    OP_GROUPNORM: (NormArgs, "imh_groupnorm", _launch),
    OP_LAYERNORM: (NormArgs, "imh_layernorm", _launch),
    OP_EW: (EwArgs, "imh_elementwise", _launch_op),
    OP_ATTN_SMALL: (SmallAttnArgs, "imh_attention_small", _launch),
    OP_GEMM_DUAL: (GemmArgs, "imh_gemm_dual", _launch_pair),
    OP_XATTN: (XAttnArgs, "imh_cross_attention", _launch),
    OP_ATTN_ENC: (EncAttnArgs, "imh_attention_enc", _launch),
    OP_ATTN_ENC_CAUSAL: (EncAttnArgs, "imh_attention_enc_causal", _launch),
    OP_STEP_SEEDED: (SeededArgs, "imh_step_seeded", _launch),
    OP_RANDN_SEEDED: (RandnArgs, "imh_randn_seeded", _launch),
    OP_CLIP_PREPROCESS: (ClipPreprocessArgs, "imh_clip_preprocess", _launch),
    OP_CONTROL_ADD: (ControlAddArgs, "imh_control_add", _launch),
    OP_XATTN_REGIONS: (XAttnRegionsArgs, "imh_cross_attention_regions", _launch),
}

_lib = None


class ImhError(RuntimeError):
    pass


def load():
    """Load libimh_hip.so (once).  Raises ImhError if it is not built -- there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImhError(f"{LIB_PATH} is missing: build the HIP extension first "
                       f"(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS + ADAPTER_SYMBOLS + REGIONS_SYMBOLS + LORA_SYMBOLS + TINYVAE_SYMBOLS:
        fn = getattr(lib, name)      # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    if lib.imh_abi_version() != ABI_VERSION:
        raise ImhError("libimh_hip.so ABI version mismatch")
    # measurement knob (tools/, alternating bench.py processes): IMH_DEBUG_SET="key=value,..." -> imh_debug_set at load
    for kv in filter(None, os.environ.get("IMH_DEBUG_SET", "").split(",")):
        k, v = kv.split("=")
        lib.imh_debug_set(int(k), int(v))
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().imh_last_error()
        raise ImhError(f"{what} failed (status {rc}): {msg.decode() if msg else ''}")
