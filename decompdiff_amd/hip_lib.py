"""ctypes binding of libdecompdiff_hip.so (the C ABI of include/decompdiff_hip.h).

PyTorch is used only as the owner of device memory and streams: tensors are handed to the
library as raw device pointers (``tensor.data_ptr()``) and launches go to torch's current HIP
stream.  There is NO fallback: if the shared library is missing or fails to load, every entry
point raises — the product path never computes on the CPU.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_long, c_size_t, c_uint64, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# DD_HIP_LIB selects another build of the same ABI (used by tools/ab_builds.py to compare two builds on one box)
LIB_PATH = os.environ.get("DD_HIP_LIB") or os.path.join(_HERE, "lib", "libdecompdiff_hip.so")

# the drop-in boundary: include/decompdiff_hip.h
EXPORTED_SYMBOLS = [
    "dd_status_string", "dd_abi_version", "dd_weights_form", "dd_build_flags", "dd_workspace_floats", "dd_knn", "dd_knn_masked", "dd_knn_csr", "dd_edge_weights", "dd_gemm128",
    "dd_gemm128_tn", "dd_gemm128_tn_bias", "dd_gemm128_tn_scratch_floats",
    "dd_ln_relu_scratch_floats", "dd_ln_relu_forward", "dd_ln_relu_backward",
    "dd_embed_protein", "dd_forward", "dd_sample_steps", "dd_sample_steps_graph", "dd_sample_steps_graph_multi",
    "dd_graph_create", "dd_graph_launch", "dd_graph_destroy",
    "dd_drift_armsca", "dd_drift_clash", "dd_drift_arms_repul",
    "dd_attn_aggregate_node", "dd_attn_aggregate_triplet", "dd_attn_aggregate_pos", "dd_reverse_step",
    "dd_segment_reduce", "dd_segment_softmax", "dd_sampler_reset",
    "dd_layer0_tables", "dd_layer0_prepare",
    "dd_forward_ex", "dd_sample_steps_ex", "dd_sample_steps_graph_ex", "dd_graph_create_ex", "dd_sample_steps_graph_multi_ex",
    "dd_node_out_fc",
    "dd_forward_ex2", "dd_sample_steps_ex2", "dd_sample_steps_graph_ex2", "dd_graph_create_ex2", "dd_sample_steps_graph_multi_ex2",
    "dd_attn_aggregate_node_bwd", "dd_attn_aggregate_pos_bwd",
    "dd_attn_aggregate_node_masked", "dd_attn_aggregate_pos_masked", "dd_attn_aggregate_node_bwd_masked", "dd_attn_aggregate_pos_bwd_masked",
    "dd_csr_select_scratch_bytes", "dd_csr_select_count", "dd_csr_select_fill",
    "dd_forward_opts", "dd_sample_steps_opts", "dd_sample_steps_graph_opts", "dd_graph_create_opts", "dd_sample_steps_graph_multi_opts",
    "dd_sample_steps_keyed", "dd_graph_create_keyed",
    "dd_sample_steps_fixed", "dd_graph_create_fixed", "dd_fixed_init",
    "dd_sample_steps_resample", "dd_graph_create_resample", "dd_resample_jump", "dd_sampler_reset_resample",
    "dd_chain_init",
    "dd_drift_restraint", "dd_drift_restraint2", "dd_sample_steps_guided", "dd_graph_create_guided",
]
# measurement / profiling / test access: include/decompdiff_hip_debug.h (same library, not part of the boundary)
DEBUG_SYMBOLS = [
    "dd_workspace_view", "dd_workspace_view_opts", "dd_profile_step", "dd_debug_set_clock_buffer", "dd_debug_set_fusion", "dd_debug_set_option",
    "dd_debug_node_split", "dd_debug_node_split_cache_path", "dd_debug_schedule", "dd_debug_philox", "dd_debug_options_epoch", "dd_queue_error",
    "dd_debug_gemm128_batch",
]
# exported by the measurement build only (-DDD_DEBUG_OPTIONS=1): the tile-queue schedule's sticky error word
MEASUREMENT_ONLY_SYMBOLS = ("dd_queue_error",)
BUILD_DEBUG_OPTIONS, BUILD_EXACT_MATH = 1, 2          # bits of dd_build_flags()


class DDSampler(ctypes.Structure):
    """struct dd_sampler — field order must match include/decompdiff_hip.h exactly."""
    _fields_ = [
        ("B", c_int32), ("NP", c_int32), ("NL", c_int32), ("K", c_int32), ("NF", c_int32),
        ("num_layers", c_int32), ("T", c_int32), ("t_start", c_int32),
        ("weights", c_void_p), ("slot_off", c_void_p),
        ("tab_pos", c_void_p), ("tab_v", c_void_p), ("tab_b", c_void_p), ("tab_score", c_void_p),
        ("protein_pos", c_void_p), ("protein_h", c_void_p), ("lig_aux", c_void_p), ("atom_std", c_void_p),
        ("offset", c_void_p), ("decomp_index", c_void_p), ("full_protein_pos", c_void_p),
        ("lig_pos", c_void_p), ("lig_v", c_void_p), ("lig_bond", c_void_p), ("step_counter", c_void_p),
        ("drift_armsca", c_int32), ("armsca_min_d", c_float), ("armsca_max_d", c_float), ("armsca_scale", c_int32),
        ("drift_clash", c_int32), ("clash_sigma", c_float), ("clash_gamma", c_float), ("clash_scale", c_int32),
        ("drift_norm_batch", c_int32),
        ("u_v", c_void_p), ("u_b", c_void_p), ("eps", c_void_p), ("seed", c_uint64),
        ("traj_pos", c_void_p), ("traj_v", c_void_p), ("traj_bond", c_void_p), ("traj_v0", c_void_p),
        ("traj_vt", c_void_p), ("traj_bt", c_void_p),
        ("pred_pos", c_void_p), ("pred_v", c_void_p), ("pred_bond", c_void_p),
        ("workspace", c_void_p), ("workspace_floats", c_size_t),
        ("np_real", c_void_p), ("nl_real", c_void_p), ("bl_prefix", c_void_p),
        ("l0_tables", c_void_p), ("l0_P", c_void_p), ("l0_qn", c_void_p),
        ("num_v", c_int32), ("drift_repul", c_int32), ("repul_max_d", c_float), ("repul_scale", c_int32),
    ]


BOND_HEAD_LIN, BOND_HEAD_PRE_ATT = 0, 1             # dd_bond_head.kind


class DDBondHead(ctypes.Structure):
    """struct dd_bond_head (include/decompdiff_hip.h): the bond head handed to the *_ex entry points (NULL = lin)."""
    _fields_ = [("kind", c_int32), ("num_r", c_int32), ("W_p", c_void_p), ("W_r", c_void_p), ("b1", c_void_p),
                ("offset", c_void_p), ("coeff", c_float), ("reserved", c_int32)]


class DDNodeOut(ctypes.Structure):
    """struct dd_node_out (include/decompdiff_hip.h): the node output MLPs of an x2h_out_fc model, handed to the *_ex2 entry
    points (NULL = a model without them); layer[l]: device block of packing.node_out_block."""
    _fields_ = [("num_layers", c_int32), ("reserved", c_int32), ("layer", c_void_p * 64)]


class DDModelOpts(ctypes.Structure):
    """struct dd_model_opts (include/decompdiff_hip.h): what a model is beyond its dd_sampler, handed to the *_opts entry points;
    `size` = sizeof of this struct (see `model_opts`)."""
    _fields_ = [("size", c_int32), ("bond_head", POINTER(DDBondHead)), ("node_out", POINTER(DDNodeOut)), ("num_blocks", c_int32)]


def model_opts(bond_head=None, node_out=None, num_blocks=1) -> DDModelOpts:
    """A filled dd_model_opts.  bond_head / node_out: the descriptor structs or None; the result keeps them alive."""
    o = DDModelOpts()
    o.size, o.num_blocks = ctypes.sizeof(DDModelOpts), int(num_blocks)
    if bond_head is not None:
        o.bond_head = ctypes.pointer(bond_head)
    if node_out is not None:
        o.node_out = ctypes.pointer(node_out)
    return o


FIXED_HOLD, FIXED_REPLACE = 1, 2                       # DD_FIXED_HOLD / DD_FIXED_REPLACE
FIXED_MODES = {"hold": FIXED_HOLD, "replace": FIXED_REPLACE}


class DDFixed(ctypes.Structure):
    """struct dd_fixed (include/decompdiff_hip.h): the fixed atoms of a chain, handed to the *_fixed entry points; `size` =
    sizeof of this struct, every other pointer a DEVICE pointer that the kernels read at every launch (see `fixed_struct`)."""
    _fields_ = [("size", c_int32), ("mode", c_int32), ("mask", c_void_p), ("v0", c_void_p), ("b0", c_void_p), ("x0c", c_void_p),
                ("cc", c_void_p), ("tab", c_void_p)]


def fixed_struct(mode, mask, v0, b0, x0c, cc=None, tab=None) -> DDFixed:
    """A filled dd_fixed from device tensors (the caller keeps them alive); mode: "hold" / "replace"."""
    f = DDFixed()
    f.size, f.mode = ctypes.sizeof(DDFixed), FIXED_MODES[mode]
    for name, t in (("mask", mask), ("v0", v0), ("b0", b0), ("x0c", x0c), ("cc", cc), ("tab", tab)):
        setattr(f, name, None if t is None else t.data_ptr())
    return f


class DDResample(ctypes.Structure):
    """struct dd_resample (include/decompdiff_hip.h): the resampling state of a chain with fixed atoms, handed to the *_resample
    entry points; `size` = sizeof of this struct, tab / epoch DEVICE pointers read at every launch (see `resample_struct`)."""
    _fields_ = [("size", c_int32), ("jump_length", c_int32), ("tab", c_void_p), ("epoch", c_void_p)]


def resample_struct(jump_length, tab, epoch) -> DDResample:
    """A filled dd_resample from device tensors (the caller keeps them alive): tab fp32 [6][T], epoch int32 [1]."""
    r = DDResample()
    r.size, r.jump_length = ctypes.sizeof(DDResample), int(jump_length)
    r.tab, r.epoch = tab.data_ptr(), epoch.data_ptr()
    return r


INIT_PRIOR, INIT_NOISED = 1, 2                         # DD_INIT_PRIOR / DD_INIT_NOISED
INIT_MODES = {"prior": INIT_PRIOR, "noised": INIT_NOISED}


class DDInit(ctypes.Structure):
    """struct dd_init (include/decompdiff_hip.h): what dd_chain_init draws the chain's first level from; `size` = sizeof of this
    struct, every other pointer a DEVICE pointer (see `init_struct`)."""
    _fields_ = [("size", c_int32), ("mode", c_int32), ("cc", c_void_p), ("std", c_void_p), ("atom_log_prior", c_void_p),
                ("bond_log_prior", c_void_p), ("x0c", c_void_p), ("v0", c_void_p), ("b0", c_void_p), ("tab", c_void_p)]


def init_struct(mode, cc, std, atom_log_prior=None, bond_log_prior=None, x0c=None, v0=None, b0=None, tab=None) -> DDInit:
    """A filled dd_init from device tensors (the caller keeps them alive); mode: "prior" / "noised"."""
    f = DDInit()
    f.size, f.mode = ctypes.sizeof(DDInit), INIT_MODES[mode]
    for name, t in (("cc", cc), ("std", std), ("atom_log_prior", atom_log_prior), ("bond_log_prior", bond_log_prior), ("x0c", x0c),
                    ("v0", v0), ("b0", b0), ("tab", tab)):
        setattr(f, name, None if t is None else t.data_ptr())
    return f


RESTRAINT_ANY = -3                                     # DD_RESTRAINT_ANY: every real ligand atom of the sample
RESTRAINT_NONE = -4                                    # DD_RESTRAINT_NONE: group2 of a row without a second endpoint


class DDRestraints(ctypes.Structure):
    """struct dd_restraints (include/decompdiff_hip.h): the distance restraints of a chain, sorted by sample (CSR ``ptr``); `size` =
    sizeof of this struct, every pointer a DEVICE pointer that the kernel reads at every launch (see `restraints_struct`)."""
    _fields_ = [("size", c_int32), ("R", c_int32), ("ptr", c_void_p), ("point", c_void_p), ("min_d", c_void_p), ("max_d", c_void_p),
                ("weight", c_void_p), ("atom", c_void_p), ("group", c_void_p), ("scale", c_int32), ("t_min", c_int32), ("t_max", c_int32),
                # the general form (trailing, every one NULL-able): typed atoms, pairs, the harmonic hinge, per-step rows
                ("cls", c_void_p), ("cls2", c_void_p), ("pair", c_void_p), ("atom2", c_void_p), ("group2", c_void_p), ("form", c_void_p),
                ("dist_traj", c_void_p), ("winner_traj", c_void_p), ("winner2_traj", c_void_p), ("traj_positions", c_int32)]


RESTRAINT_GENERAL_FIELDS = ("cls", "cls2", "pair", "atom2", "group2", "form", "dist_traj", "winner_traj", "winner2_traj")


def restraints_struct(R, ptr, point, min_d, max_d, weight, atom, group, scale, t_min, t_max, traj_positions=0, **general) -> DDRestraints:
    """A filled dd_restraints from device tensors (the caller keeps them alive): ptr int32 [B+1], point fp32 [R,3], min_d / max_d /
    weight fp32 [R], atom / group int32 [R] (atom: the row within the sample or -1; group: RESTRAINT_ANY, -1 scaffold, >= 0 arm).
    ``general`` -- any of RESTRAINT_GENERAL_FIELDS: cls / cls2 (class masks, int32 or uint32 [R]), pair / atom2 / group2 / form int32
    [R], dist_traj fp32 and winner_traj / winner2_traj int32 [traj_positions, R] -- sends the launches to the general kernel; left
    out (or None) they stay NULL and the struct is the one the point kernel serves."""
    if set(general) - set(RESTRAINT_GENERAL_FIELDS):
        raise TypeError(f"restraints_struct: unknown fields {sorted(set(general) - set(RESTRAINT_GENERAL_FIELDS))}")
    r = DDRestraints()
    r.size, r.R, r.scale, r.t_min, r.t_max = ctypes.sizeof(DDRestraints), int(R), int(bool(scale)), int(t_min), int(t_max)
    r.traj_positions = int(traj_positions)
    for name, t in (("ptr", ptr), ("point", point), ("min_d", min_d), ("max_d", max_d), ("weight", weight), ("atom", atom),
                    ("group", group)) + tuple(general.items()):
        setattr(r, name, None if t is None else t.data_ptr())
    return r


L0_TABLE_FLOATS = 16 * 640 + 16 * 1280 + 5 * 640 + 16 * 128 + 16 * 128 + 80 * 128      # DD_L0_TABLE_FLOATS


class DDWsView(ctypes.Structure):
    _fields_ = [("x", c_void_p), ("h", c_void_p), ("hb", c_void_p), ("ew", c_void_p), ("A", c_void_p),
                ("nbr", c_void_p), ("Anb", c_void_p), ("lin_in_node", ctypes.c_int32)]


class DDGemmJob(ctypes.Structure):
    """struct dd_gemm_job (include/decompdiff_hip_debug.h): one job of dd_debug_gemm128_batch, device pointers throughout."""
    _fields_ = [("X", c_void_p), ("x_rows_per_b", c_int), ("x_stride_b", c_long), ("ldx", c_int), ("rows", c_int),
                ("W", c_void_p), ("bias", c_void_p), ("ln", c_void_p),
                ("Y", c_void_p), ("y_rows_per_b", c_int), ("y_stride_b", c_long), ("ldy", c_int), ("ncols", c_int),
                ("accumulate", c_int), ("acc_src", c_void_p),
                ("X2", c_void_p), ("x2_N", c_int), ("x2_NP", c_int), ("x2_Eb", c_int), ("x2_NLm1", c_int), ("x2_ld", c_int)]


PROF_CATS = ["misc", "gemm", "assemble", "attn_NE", "attn_NB", "attn_BL", "attn_PE", "attn_PB", "step", "event_pair"]


ABI_VERSION = 9          # include/decompdiff_hip.h: layout of struct dd_sampler and of the tables it points to


class HipLibraryError(RuntimeError):
    pass


_lib = None


def load():
    """Load the shared library (once).  Raises HipLibraryError if it is absent — build it with
    ``python -m decompdiff_amd.build`` (or ``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(f"{LIB_PATH} not found: build it with `python -m decompdiff_amd.build`; "
                              "there is no CPU fallback for the sampling hot path")
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:                                   # e.g. libamdhip64 missing
        raise HipLibraryError(f"could not load {LIB_PATH}: {e}") from e
    lib.dd_status_string.restype = c_char_p
    lib.dd_status_string.argtypes = [c_int]
    lib.dd_abi_version.restype = c_int
    ignore_abi = os.environ.get("DD_IGNORE_ABI") == "1"                                    # (A/B timing of older builds)
    if lib.dd_abi_version() != ABI_VERSION and not ignore_abi:
        raise HipLibraryError(f"{LIB_PATH} has ABI version {lib.dd_abi_version()}, this package needs {ABI_VERSION}: rebuild it")
    S = POINTER(DDSampler)
    # name -> argtypes (restype c_int = status code unless listed in `restypes`)
    protos = {
        "dd_build_flags": [],
        "dd_weights_form": [],
        "dd_workspace_floats": [c_int, c_int, c_int, c_int],
        "dd_knn": [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p],
        "dd_knn_masked": [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
        "dd_knn_csr": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p],
        "dd_edge_weights": [c_void_p, c_void_p, c_int, c_int, c_int] + [c_void_p] * 7,
        "dd_gemm128": [c_void_p, c_int, c_long, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_long, c_int, c_int,
                       c_int, c_void_p],
        "dd_gemm128_tn_scratch_floats": [c_long, c_int],
        "dd_gemm128_tn": [c_void_p, c_int, c_int, c_void_p, c_int, c_long, c_void_p, c_void_p, c_int, c_int, c_void_p],
        "dd_gemm128_tn_bias": [c_void_p, c_int, c_int, c_void_p, c_int, c_long, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p],
        "dd_ln_relu_scratch_floats": [c_long],
        "dd_ln_relu_forward": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p],
        "dd_ln_relu_backward": [c_void_p] * 9 + [c_long, c_void_p],
        "dd_embed_protein": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
        "dd_forward": [S, c_void_p],
        "dd_sampler_reset": [S, c_void_p],
        "dd_layer0_tables": [S, c_void_p, c_void_p],
        "dd_layer0_prepare": [S, c_void_p],
        "dd_debug_options_epoch": [],
        "dd_queue_error": [S, c_void_p, POINTER(c_int)],
        "dd_sample_steps": [S, c_int, c_void_p],
        "dd_sample_steps_graph": [S, c_int, c_void_p],
        "dd_graph_create": [S, c_int, c_void_p, POINTER(c_void_p)],
        "dd_graph_launch": [c_void_p, c_int, c_void_p],
        "dd_graph_destroy": [c_void_p],
        "dd_sample_steps_graph_multi": [POINTER(S), c_int, c_int, POINTER(c_void_p)],
        "dd_forward_ex": [S, POINTER(DDBondHead), c_void_p],
        "dd_sample_steps_ex": [S, POINTER(DDBondHead), c_int, c_void_p],
        "dd_sample_steps_graph_ex": [S, POINTER(DDBondHead), c_int, c_void_p],
        "dd_graph_create_ex": [S, POINTER(DDBondHead), c_int, c_void_p, POINTER(c_void_p)],
        "dd_sample_steps_graph_multi_ex": [POINTER(S), POINTER(POINTER(DDBondHead)), c_int, c_int, POINTER(c_void_p)],
        "dd_node_out_fc": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
        "dd_forward_ex2": [S, POINTER(DDBondHead), POINTER(DDNodeOut), c_void_p],
        "dd_sample_steps_ex2": [S, POINTER(DDBondHead), POINTER(DDNodeOut), c_int, c_void_p],
        "dd_sample_steps_graph_ex2": [S, POINTER(DDBondHead), POINTER(DDNodeOut), c_int, c_void_p],
        "dd_graph_create_ex2": [S, POINTER(DDBondHead), POINTER(DDNodeOut), c_int, c_void_p, POINTER(c_void_p)],
        "dd_sample_steps_graph_multi_ex2": [POINTER(S), POINTER(POINTER(DDBondHead)), POINTER(POINTER(DDNodeOut)), c_int, c_int,
                                            POINTER(c_void_p)],
        "dd_forward_opts": [S, POINTER(DDModelOpts), c_void_p],
        "dd_sample_steps_opts": [S, POINTER(DDModelOpts), c_int, c_void_p],
        "dd_sample_steps_graph_opts": [S, POINTER(DDModelOpts), c_int, c_void_p],
        "dd_graph_create_opts": [S, POINTER(DDModelOpts), c_int, c_void_p, POINTER(c_void_p)],
        "dd_sample_steps_graph_multi_opts": [POINTER(S), POINTER(POINTER(DDModelOpts)), c_int, c_int, POINTER(c_void_p)],
        # (the _opts siblings with the device pointer sample_keys [B] uint64 after opts)
        "dd_sample_steps_keyed": [S, POINTER(DDModelOpts), c_void_p, c_int, c_void_p],
        "dd_graph_create_keyed": [S, POINTER(DDModelOpts), c_void_p, c_int, c_void_p, POINTER(c_void_p)],
        # (the _keyed siblings with the host struct dd_fixed after sample_keys; NULL: exactly the _keyed call)
        "dd_sample_steps_fixed": [S, POINTER(DDModelOpts), c_void_p, POINTER(DDFixed), c_int, c_void_p],
        "dd_graph_create_fixed": [S, POINTER(DDModelOpts), c_void_p, POINTER(DDFixed), c_int, c_void_p, POINTER(c_void_p)],
        "dd_fixed_init": [S, c_void_p, POINTER(DDFixed), c_void_p],
        # (the _fixed siblings with the host struct dd_resample after fixed; the jump; the reset that also zeroes the epoch)
        "dd_sample_steps_resample": [S, POINTER(DDModelOpts), c_void_p, POINTER(DDFixed), POINTER(DDResample), c_int, c_void_p],
        "dd_graph_create_resample": [S, POINTER(DDModelOpts), c_void_p, POINTER(DDFixed), POINTER(DDResample), c_int, c_void_p,
                                     POINTER(c_void_p)],
        "dd_resample_jump": [S, c_void_p, POINTER(DDFixed), POINTER(DDResample), c_void_p],
        "dd_sampler_reset_resample": [S, POINTER(DDResample), c_void_p],
        # (the chain's first level drawn on the device: sample_keys, the host struct dd_init)
        "dd_chain_init": [S, c_void_p, POINTER(DDInit), c_void_p],
        # (distance restraints: the op-level gradient; the last step pair -- keys, fixed, resample, restraints, each NULL-able)
        "dd_drift_restraint": [c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(DDRestraints), c_void_p, c_void_p, c_int, c_void_p,
                               c_void_p, c_void_p],
        "dd_drift_restraint2": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(DDRestraints), c_void_p, c_void_p, c_int,
                                c_void_p, c_void_p, c_void_p, c_void_p],
        "dd_sample_steps_guided": [S, POINTER(DDModelOpts), c_void_p, POINTER(DDFixed), POINTER(DDResample), POINTER(DDRestraints), c_int,
                                   c_void_p],
        "dd_graph_create_guided": [S, POINTER(DDModelOpts), c_void_p, POINTER(DDFixed), POINTER(DDResample), POINTER(DDRestraints), c_int,
                                   c_void_p, POINTER(c_void_p)],
        "dd_drift_armsca": [c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_void_p, c_int, c_void_p],
        "dd_drift_clash": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p, c_int, c_void_p],
        "dd_drift_arms_repul": [c_void_p, c_void_p, c_int, c_int, c_float, c_int, c_void_p, c_int, c_void_p],
        "dd_workspace_view": [S, POINTER(DDWsView)],
        "dd_workspace_view_opts": [S, POINTER(DDModelOpts), POINTER(DDWsView)],
        "dd_debug_set_clock_buffer": [c_void_p, c_int],
        "dd_debug_set_fusion": [c_int],
        "dd_debug_set_option": [c_int, c_int],
        "dd_debug_node_split": [c_int, c_int, c_int, c_int],
        "dd_debug_node_split_cache_path": [c_char_p, c_int],
        "dd_debug_schedule": [],
        "dd_reverse_step": [S, c_void_p, c_void_p, c_void_p, c_void_p],
        "dd_attn_aggregate_node": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p],
        "dd_attn_aggregate_triplet": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p],
        "dd_attn_aggregate_pos": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p],
        "dd_attn_aggregate_node_bwd": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int] + [c_void_p] * 7,
        "dd_attn_aggregate_pos_bwd": [c_void_p] * 6 + [c_int] + [c_void_p] * 7,
        # (the siblings' lists with member_mask after seg_ptr / n_seg)
        "dd_attn_aggregate_node_masked": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p],
        "dd_attn_aggregate_pos_masked": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p],
        "dd_attn_aggregate_node_bwd_masked": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int] + [c_void_p] * 8,
        "dd_attn_aggregate_pos_bwd_masked": [c_void_p] * 6 + [c_int] + [c_void_p] * 8,
        "dd_csr_select_scratch_bytes": [c_int64] * 4,
        "dd_csr_select_count": [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_size_t, c_void_p],
        "dd_csr_select_fill": [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int64] + [c_void_p] * 6,
        "dd_segment_reduce": [c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_void_p, c_void_p, c_void_p],
        "dd_segment_softmax": [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p],
        "dd_debug_philox": [c_uint64, c_int, c_long, c_int, c_void_p, c_void_p],
        "dd_profile_step": [S, c_int, POINTER(c_float), c_void_p],
        "dd_debug_gemm128_batch": [POINTER(DDGemmJob), c_int, c_void_p],
    }
    restypes = {"dd_workspace_floats": c_size_t, "dd_gemm128_tn_scratch_floats": c_size_t, "dd_ln_relu_scratch_floats": c_size_t,
                "dd_csr_select_scratch_bytes": c_size_t}
    for name in EXPORTED_SYMBOLS + DEBUG_SYMBOLS:
        if name in ("dd_status_string", "dd_abi_version"):
            continue
        if not hasattr(lib, name):
            # DD_IGNORE_ABI=1 with an older build (tools/ab_builds.py): entry points it lacks raise when CALLED, not at load
            if ignore_abi or name in MEASUREMENT_ONLY_SYMBOLS:
                continue
            raise HipLibraryError(f"{LIB_PATH} does not export {name}: rebuild it")
        fn = getattr(lib, name)
        if name in protos:
            fn.argtypes = protos[name]
        fn.restype = restypes.get(name, c_int)
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().dd_status_string(rc).decode()
        raise RuntimeError(f"decompdiff_hip {what} failed: {msg} (status {rc})")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_contiguous(), "decompdiff_hip needs contiguous tensors"
    return ctypes.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_gpu(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise HipLibraryError(f"{name} must live on a HIP device (got {t.device}); the sampling hot path has no "
                              "CPU implementation in this package")


def weights_form() -> int:
    """Form of the packed attention MLPs the loaded library expects (include/decompdiff_hip.h: dd_weights_form; 0 for builds
    older than ABI 9, loaded with DD_IGNORE_ABI=1 by the A/B tools)."""
    lib = load()
    return int(lib.dd_weights_form()) if hasattr(lib, "dd_weights_form") else 0


def is_measurement_build() -> bool:
    """The loaded library was compiled with -DDD_DEBUG_OPTIONS=1 (lib/libdecompdiff_hip_dbg.so: alternative launch
    schedules behind dd_debug_set_option)."""
    lib = load()
    if not hasattr(lib, "dd_build_flags"):               # (an older build loaded with DD_IGNORE_ABI=1)
        return False
    return bool(lib.dd_build_flags() & BUILD_DEBUG_OPTIONS)
