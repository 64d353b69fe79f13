"""ctypes binding of ``libfv3hip.so`` (C ABI declared in ``include/fv3hip.h``).

The library is built in-tree by ``make -C fv3net_amd/csrc`` (or ``__graft_entry__.build()``).
If it is missing, every entry point raises :class:`ExtensionMissingError` -- the product path
never falls back to a CPU implementation.
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# FV3HIP_LIBRARY points at an alternative build of the same ABI (diagnostic builds with stamps)
LIB_PATH = os.environ.get("FV3HIP_LIBRARY") or os.path.join(_HERE, "libfv3hip.so")

F32, F64, I32, I64 = 0, 1, 2, 3
OP_SUM, OP_MEAN, OP_MIN, OP_MAX, OP_MEDIAN, OP_MODE = range(6)
NAN_SKIP, NAN_PROPAGATE, NAN_OMIT = range(3)
LAYOUT_COL_LEVEL, LAYOUT_LEVEL_COL = 0, 1
TRANSFORM_NONE, TRANSFORM_LOG = 0, 1
ACT_LINEAR, ACT_RELU, ACT_TANH = 0, 1, 2
CONV_HALO_INPUT, CONV_HALO_STRIPS, CONV_HALO_CUBE = 0, 1, 2
ARITH_EXACT, ARITH_FAST = 0, 1
CYCLEGAN_CONV_REGULAR, CYCLEGAN_CONV_STRIDED, CYCLEGAN_CONV_TRANSPOSED = 0, 1, 2
CYCLEGAN_HALO_ZEROS, CYCLEGAN_HALO_CUBE = 0, 1
FMR_LOSS_MSE, FMR_LOSS_MAE = 0, 1
CODEC_DENSE, CODEC_AFFINE = 0, 1
FOREST_TRAIN_SUMS, FOREST_TRAIN_SCAN, FOREST_TRAIN_SPLIT, FOREST_TRAIN_ALL = 1, 2, 4, 7
ABI_VERSION = 3

OK, EINVAL, EUNSUPPORTED, EHIP, ENOMEM = 0, -1, -2, -3, -4


class ExtensionMissingError(ImportError):
    pass


class Fv3HipError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"libfv3hip error {code}: {message}")
        self.code = code


class DeviceInfo(ctypes.Structure):
    _fields_ = [
        ("name", ctypes.c_char * 128),
        ("arch", ctypes.c_char * 64),
        ("compute_units", c_int),
        ("wavefront_size", c_int),
        ("lds_bytes_per_cu", c_int),
        ("clock_mhz", c_int),
        ("hbm_bytes", c_size_t),
    ]


class MlpDesc(ctypes.Structure):
    _fields_ = [
        ("n_sources", c_int),
        ("n_inputs", c_int),
        ("in_source", POINTER(c_int)),
        ("in_feat_start", POINTER(c_int)),
        ("in_nfeat", POINTER(c_int)),
        ("in_transform", POINTER(c_int)),
        ("in_eps", POINTER(c_float)),
        ("in_center", POINTER(c_float)),
        ("in_scale", POINTER(c_float)),
        ("n_hidden", c_int),
        ("width", c_int),
        ("hidden_activation", c_int),
        ("hidden_kernels", POINTER(POINTER(c_float))),
        ("hidden_biases", POINTER(POINTER(c_float))),
        ("n_outputs", c_int),
        ("out_nfeat", POINTER(c_int)),
        ("out_kernel", POINTER(c_float)),
        ("out_bias", POINTER(c_float)),
        ("out_scale", POINTER(c_float)),
        ("out_center", POINTER(c_float)),
        ("out_min", POINTER(c_float)),
        ("out_max", POINTER(c_float)),
        ("out_mask", POINTER(c_float)),
        ("n_residual", c_int),
        ("res_source", POINTER(c_int)),
        ("res_output", POINTER(c_int)),
        ("hidden_output", c_int),
    ]


class ForestDesc(ctypes.Structure):
    _fields_ = [
        ("n_trees", c_int),
        ("node_offset", POINTER(c_int64)),
        ("children_left", POINTER(ctypes.c_int32)),
        ("children_right", POINTER(ctypes.c_int32)),
        ("feature", POINTER(ctypes.c_int32)),
        ("threshold", POINTER(c_float)),
        ("missing_go_to_left", POINTER(ctypes.c_uint8)),
        ("leaf_row", POINTER(ctypes.c_int32)),
        ("n_leaf_rows", c_int64),
        ("leaf_values", POINTER(c_double)),
        ("n_sources", c_int),
        ("src_feat_start", POINTER(c_int)),
        ("src_nfeat", POINTER(c_int)),
        ("n_outputs", c_int),
        ("out_nfeat", POINTER(c_int)),
        ("mean", POINTER(c_double)),
        ("std", POINTER(c_double)),
    ]


class ConvDesc(ctypes.Structure):
    _fields_ = [
        ("n_inputs", c_int),
        ("in_nfeat", POINTER(c_int)),
        ("in_center", POINTER(c_float)),
        ("in_scale", POINTER(c_float)),
        ("n_hidden", c_int),
        ("kernel_size", c_int),
        ("filters", c_int),
        ("activation", c_int),
        ("hidden_kernels", POINTER(POINTER(c_float))),
        ("hidden_biases", POINTER(POINTER(c_float))),
        ("n_outputs", c_int),
        ("out_nfeat", POINTER(c_int)),
        ("out_kernel", POINTER(c_float)),
        ("out_bias", POINTER(c_float)),
        ("out_scale", POINTER(c_float)),
        ("out_center", POINTER(c_float)),
    ]


class ReservoirTransformer(ctypes.Structure):
    _fields_ = [
        ("kind", c_int),
        ("n_variables", c_int),
        ("var_nz", POINTER(c_int)),
        ("nx", c_int),
        ("ny", c_int),
        ("center", POINTER(c_float)),
        ("scale", POINTER(c_float)),
        ("mask", POINTER(c_double)),
        ("mask_f32", c_int),
    ]


class ReservoirDesc(ctypes.Structure):
    _fields_ = [
        ("layout_x", c_int),
        ("layout_y", c_int),
        ("overlap", c_int),
        ("rank_x", c_int),
        ("rank_y", c_int),
        ("state_size", c_int),
        ("input_size", c_int),
        ("input", ReservoirTransformer),
        ("output", ReservoirTransformer),
        ("hybrid", ReservoirTransformer),
        ("w_in_indptr", POINTER(c_int64)),
        ("w_in_indices", POINTER(ctypes.c_int32)),
        ("w_in_data", POINTER(c_double)),
        ("w_in_storage", c_int),
        ("w_res_indptr", POINTER(c_int64)),
        ("w_res_indices", POINTER(ctypes.c_int32)),
        ("w_res_data", POINTER(c_double)),
        ("input_mask", POINTER(c_double)),
        ("input_mask_f32", c_int),
        ("square", c_int),
        ("n_hybrid", c_int),
        ("hybrid_mask", POINTER(c_double)),
        ("hybrid_mask_f32", c_int),
        ("coefficients", POINTER(c_double)),
        ("intercepts", POINTER(c_double)),
        ("state", POINTER(c_double)),
    ]


class CodecDesc(ctypes.Structure):
    _fields_ = [
        ("kind", c_int),
        ("n_variables", c_int),
        ("var_nz", POINTER(c_int)),
        ("n_latent", c_int),
        ("center", POINTER(c_float)),
        ("scale", POINTER(c_float)),
        ("n_enc", c_int),
        ("enc_units", POINTER(c_int)),
        ("enc_kernels", POINTER(POINTER(c_float))),
        ("enc_biases", POINTER(POINTER(c_float))),
        ("n_dec", c_int),
        ("dec_units", POINTER(c_int)),
        ("dec_kernels", POINTER(POINTER(c_float))),
        ("dec_biases", POINTER(POINTER(c_float))),
        ("head_kernels", POINTER(POINTER(c_float))),
        ("head_biases", POINTER(POINTER(c_float))),
        ("out_min", POINTER(c_float)),
        ("out_max", POINTER(c_float)),
        ("mean", POINTER(c_double)),
        ("std", POINTER(c_double)),
        ("pca_mean", POINTER(c_double)),
        ("components", POINTER(c_double)),
        ("explained_variance", POINTER(c_double)),
        ("enforce_positive", c_int),
    ]


class ForestTrain(ctypes.Structure):
    """``fv3hip_forest_train_t``: every buffer of one tree's growth (device pointers as integers)."""

    _fields_ = (
        [("n", c_int64), ("F", c_int), ("O", c_int)]
        + [(k, c_void_p) for k in ("xt", "y", "ysq", "order", "weight", "list_a", "list_b", "side", "pos_node", "seg_a", "seg_b",
                                   "node_a", "node_b", "stats", "carry", "count", "proxy", "best_proxy", "best_pos", "n_left",
                                   "dst_left", "dst_right")]
        + [("k_cap", c_int64), ("node_cap", c_int64)]
        + [(k, c_void_p) for k in ("left", "right", "feature", "threshold", "missing_left", "value", "impurity", "weighted_n",
                                   "n_samples", "level")]
    )


class EmulatorHead(ctypes.Structure):
    """``fv3hip_emulator_head_t``: one head of ``fv3hip_train_emulator_loss_grad`` (device pointers as integers)."""

    _fields_ = (
        [(k, c_int) for k in ("kind", "col0", "ncol", "single_level", "slot", "slot_after", "is_loss", "is_loss_after")]
        + [("weight", c_double), ("weight_after", c_double)]
        + [(k, c_void_p) for k in ("scale", "center", "target", "inv", "before", "target_after", "inv_after")]
        + [(k, c_int64) for k in ("ld_target", "ld_before", "ld_target_after")]
    )


EMULATOR_MAX_HEADS = 16
EMULATOR_HEAD_MSE_DENSE, EMULATOR_HEAD_MSE_LOCAL, EMULATOR_HEAD_XENT = 0, 1, 2

# name -> (restype, argtypes); every name here must be declared in include/fv3hip.h
SIGNATURES = {
    "fv3hip_last_error": (c_char_p, []),
    "fv3hip_abi_version": (c_int, []),
    "fv3hip_spin": (c_int, [c_int64, c_int, c_void_p]),
    "fv3hip_init": (c_int, [c_int]),
    "fv3hip_device_info": (c_int, [POINTER(DeviceInfo)]),
    "fv3hip_weighted_block_average": (
        c_int,
        [c_void_p, c_int, c_void_p, c_int, c_int64, c_int, c_int, c_int64, c_int, c_void_p, c_void_p],
    ),
    "fv3hip_mass_weighted_block_average": (
        c_int,
        [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_int64, c_int, c_void_p, c_void_p],
    ),
    "fv3hip_edge_weighted_block_average": (
        c_int,
        [c_void_p, c_int, c_void_p, c_int, c_int64, c_int, c_int, c_int64, c_int, c_int, c_void_p, c_void_p],
    ),
    "fv3hip_block_reduce": (
        c_int,
        [c_void_p, c_int, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    ),
    "fv3hip_block_upsample": (c_int, [c_void_p, c_int, c_int64, c_int, c_int, c_int, c_void_p, c_void_p]),
    "fv3hip_zc_squash": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int64, c_double, c_int, c_void_p, c_void_p, c_void_p]),
    "fv3hip_zc_infer_cloud": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p]),
    "fv3hip_zc_gscond_conserve": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_int,
                                          c_int, c_int, c_int64, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                          c_void_p]),
    "fv3hip_zc_precpd_conserve": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                          c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "fv3hip_zc_precip_simple": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int64, c_int64,
                                        c_int, c_void_p, c_void_p]),
    "fv3hip_zc_class_zero": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_void_p]),
    "fv3hip_non_negative_sphum": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_double, c_int, c_void_p, c_void_p,
                                          c_void_p]),
    "fv3hip_clamp": (c_int, [c_void_p, c_int, c_int64, c_double, c_double, c_int, c_int, c_void_p, c_void_p]),
    "fv3hip_level_fill": (c_int, [c_void_p, c_int, c_void_p, c_int, c_double, c_int64, c_int64, c_int64, c_int64, c_void_p,
                                  c_void_p]),
    "fv3hip_column_sum": (c_int, [c_void_p, c_int, c_int64, c_int, c_int64, c_double, c_void_p, c_void_p]),
    "fv3hip_blend_weights": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_int64, c_void_p, c_void_p]),
    "fv3hip_hydrostatic_balance": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_int64,
                                           c_double, c_void_p, c_void_p, c_void_p]),
    "fv3hip_mappm_multi": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int64, c_int64, c_int, c_int, c_int, c_int,
                                   c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "fv3hip_mappm_multi_coarse_target": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int64, c_int, c_int, c_int, c_int, c_int,
                                                 c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "fv3hip_mappm_block_mean_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "fv3hip_mappm_block_mean": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p,
                                        c_int, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "fv3hip_mask_weights_coarse": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_int64, c_int, c_int, c_int, c_int,
                                           c_int64, c_void_p, c_void_p]),
    "fv3hip_level_scale": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p]),
    "fv3hip_member_reduce": (c_int, [c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_void_p]),
    "fv3hip_tendency_to_flux": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_int64, c_int, c_int,
                                        c_void_p, c_void_p, c_void_p]),
    "fv3hip_flux_to_tendency": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_int64, c_void_p, c_void_p]),
    "fv3hip_minmax_score": (c_int, [c_void_p, c_int, c_int64, c_int64, c_int, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p,
                                    c_void_p, c_void_p, c_void_p]),
    "fv3hip_ocsvm_score": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_double, c_void_p, c_void_p]),
    "fv3hip_precip_closure": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int64, c_void_p, c_int, c_int64, c_int,
                                      c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "fv3hip_local_pack": (c_int, [c_void_p, c_int, c_int, c_int, c_double, c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p]),
    "fv3hip_local_unpack": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                    c_double, c_void_p, c_int, c_int, c_double, c_double, c_double, c_double, c_int, c_int64,
                                    c_void_p, c_void_p, c_void_p, c_void_p]),
    "fv3hip_classify_onehot": (c_int, [c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "fv3hip_interpolate_2d": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_double, c_int, c_void_p,
                                      c_void_p]),
    "fv3hip_ew": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_double, c_int, c_int64, c_int64, c_int64, c_int64, c_void_p,
                          c_void_p]),
    "fv3hip_cube_edge_rows": (c_int, [c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_void_p]),
    "fv3hip_halo_pick": (c_int, [c_void_p, c_int, c_int, c_int64, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int), c_void_p, c_void_p]),
    "fv3hip_cast": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int64, c_void_p]),
    "fv3hip_cast_many": (c_int, [c_void_p, POINTER(c_int), c_void_p, c_int, POINTER(c_int64), c_int, c_void_p]),
    "fv3hip_interp_center_to_outer": (c_int, [c_void_p, c_int, c_int64, c_int, c_int, c_int, c_void_p, c_void_p,
                                              c_void_p, c_void_p]),
    "fv3hip_interp_center_to_outer_lines": (c_int, [c_void_p, c_int, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                                    c_void_p, c_void_p]),
    "fv3hip_weighted_window_average": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int64, c_int, c_int, c_int64, c_int, c_int,
                                               c_int, c_int, c_void_p, c_void_p]),
    "fv3hip_repeat": (c_int, [c_void_p, c_int, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "fv3hip_pressure_at_interface": (
        c_int,
        [c_void_p, c_int, c_int64, c_int, c_int64, c_double, c_void_p, c_void_p],
    ),
    "fv3hip_pressure_at_midpoint_log": (
        c_int,
        [c_void_p, c_int, c_int64, c_int, c_int64, c_double, c_void_p, c_void_p],
    ),
    "fv3hip_mask_weights": (
        c_int,
        [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_int64, c_int, c_int64, c_int64, c_void_p,
         c_void_p],
    ),
    "fv3hip_mappm_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "fv3hip_mappm": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, c_int,
         c_void_p, c_size_t, c_void_p],
    ),
    "fv3hip_mlp_create": (c_int, [POINTER(MlpDesc), POINTER(c_void_p)]),
    "fv3hip_mlp_destroy": (c_int, [c_void_p]),
    "fv3hip_mlp_predict": (
        c_int,
        [c_void_p, POINTER(c_void_p), POINTER(c_int), POINTER(c_int64), POINTER(c_int64), c_int64,
         POINTER(c_void_p), c_int, POINTER(c_int64), POINTER(c_int64), c_void_p],
    ),
    "fv3hip_mlp_flops_per_sample": (c_int64, [c_void_p]),
    "fv3hip_mlp_set_small_limit": (c_int, [c_void_p, c_int64]),
    "fv3hip_mlp_last_variant": (c_char_p, [c_void_p]),
    "fv3hip_mlp3_create": (c_int, [POINTER(MlpDesc), POINTER(c_void_p)]),
    "fv3hip_mlp3_destroy": (c_int, [c_void_p]),
    "fv3hip_mlp3_flops_per_sample": (c_int64, [c_void_p]),
    "fv3hip_mlp3_predict": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_int64), c_int64, POINTER(c_void_p), POINTER(c_int64), c_void_p]),
    "fv3hip_mlp3_last_variant": (c_char_p, [c_void_p]),
    "fv3hip_forest_create": (c_int, [POINTER(ForestDesc), POINTER(c_void_p)]),
    "fv3hip_forest_destroy": (c_int, [c_void_p]),
    "fv3hip_forest_predict": (
        c_int,
        [c_void_p, POINTER(c_void_p), POINTER(c_int), POINTER(c_int64), POINTER(c_int64), c_int64,
         POINTER(c_void_p), POINTER(c_int64), POINTER(c_int64), c_void_p],
    ),
    "fv3hip_forest_apply": (
        c_int,
        [c_void_p, POINTER(c_void_p), POINTER(c_int), POINTER(c_int64), POINTER(c_int64), c_int64, c_void_p, c_void_p],
    ),
    "fv3hip_conv_create": (c_int, [POINTER(ConvDesc), POINTER(c_void_p)]),
    "fv3hip_conv_destroy": (c_int, [c_void_p]),
    "fv3hip_conv_workspace_bytes": (c_size_t, [c_void_p, c_int64, c_int, c_int, c_int]),
    "fv3hip_conv_predict": (
        c_int,
        [c_void_p, POINTER(c_void_p), POINTER(c_int), POINTER(c_int64), c_int64, c_int, c_int, c_int, c_int, c_void_p, c_int,
         POINTER(c_void_p), POINTER(c_int64), c_void_p, c_size_t, c_void_p],
    ),
    "fv3hip_reservoir_create": (c_int, [POINTER(ReservoirDesc), POINTER(c_void_p)]),
    "fv3hip_reservoir_destroy": (c_int, [c_void_p]),
    "fv3hip_reservoir_plan": (c_int, [c_void_p, POINTER(c_int64)]),
    "fv3hip_reservoir_increment": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_int), POINTER(c_int64), c_void_p]),
    "fv3hip_reservoir_predict": (
        c_int,
        [c_void_p, POINTER(c_void_p), POINTER(c_int), POINTER(c_int64), POINTER(c_void_p), POINTER(c_int64), c_void_p],
    ),
    "fv3hip_reservoir_get_state": (c_int, [c_void_p, c_void_p, c_void_p]),
    "fv3hip_reservoir_set_state": (c_int, [c_void_p, c_void_p, c_void_p]),
    "fv3hip_reservoir_reset_state": (c_int, [c_void_p, c_void_p]),
    "fv3hip_reservoir_train_series": (
        c_int,
        [c_void_p, POINTER(c_void_p), POINTER(c_int), POINTER(c_int64), c_void_p, POINTER(c_void_p), POINTER(c_int),
         POINTER(c_int64), c_int64, c_int, c_void_p, c_void_p],
    ),
    "fv3hip_reservoir_encode_targets": (
        c_int,
        [c_void_p, POINTER(c_void_p), POINTER(c_int), POINTER(c_int64), c_int64, c_void_p, c_void_p],
    ),
    "fv3hip_gram_create": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    "fv3hip_gram_destroy": (c_int, [c_void_p]),
    "fv3hip_gram_reset": (c_int, [c_void_p, c_void_p]),
    "fv3hip_gram_update": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p]),
    "fv3hip_gram_get": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "fv3hip_codec_create": (c_int, [POINTER(CodecDesc), POINTER(c_void_p)]),
    "fv3hip_codec_destroy": (c_int, [c_void_p]),
    "fv3hip_codec_encode": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_int), POINTER(c_int64), c_int, c_int, c_void_p,
                                    c_void_p]),
    "fv3hip_codec_decode": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, POINTER(c_void_p), POINTER(c_int64), c_void_p]),
    "fv3hip_group_sums_chunk": (c_int, []),
    "fv3hip_group_sums_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "fv3hip_group_sums": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int64, c_int, c_int64, c_void_p, c_int64, c_void_p,
                                  c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "fv3hip_histogram": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_int, c_void_p, c_void_p]),
    "fv3hip_histogram2d": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "fv3hip_graph_sage": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                  c_int64, c_int64, c_int, c_int, c_int, c_int, c_void_p]),
    "fv3hip_graph_pool2": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_void_p]),
    "fv3hip_graph_up2": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int, c_int,
                                 c_int, c_void_p]),
    "fv3hip_graph_pack": (c_int, [POINTER(c_void_p), POINTER(c_int), POINTER(c_int64), c_int, POINTER(c_int), c_void_p, c_void_p,
                                  c_int64, c_int, c_int, c_int, c_void_p, c_void_p]),
    "fv3hip_graph_unpack": (c_int, [c_void_p, c_int64, c_int, c_int, POINTER(c_int), c_void_p, c_void_p, POINTER(c_void_p),
                                    c_void_p]),
    "fv3hip_cyclegan_conv": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, c_int,
                                     c_void_p]),
    "fv3hip_cyclegan_conv_context": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int,
                                             c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "fv3hip_cyclegan_stats": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int, c_int, c_double,
                                      c_void_p]),
    "fv3hip_cyclegan_apply": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int64,
                                      c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_void_p]),
    "fv3hip_cyclegan_input": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                      c_int64, c_int64, c_int64, c_int, c_int, c_void_p]),
    "fv3hip_train_chunk_rows": (c_int, []),
    "fv3hip_train_backward_weight_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "fv3hip_train_loss_workspace_doubles": (c_int, []),
    "fv3hip_train_linear_forward": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                            c_int64, c_int, c_int, c_int, c_void_p]),
    "fv3hip_train_linear_backward_data": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64,
                                                  c_int64, c_int, c_int, c_void_p]),
    "fv3hip_train_linear_backward_weight": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                                    c_void_p, c_void_p, c_size_t, c_int64, c_int, c_int, c_void_p]),
    "fv3hip_train_mse_grad": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int,
                                      c_void_p]),
    "fv3hip_train_adam": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_double, c_double, c_double, c_double,
                                  c_void_p]),
    "fv3hip_train_precip_loss_grad": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                              c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                                              c_int, c_int, c_float, c_float, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "fv3hip_train_emulator_loss_workspace_doubles": (c_int, []),
    "fv3hip_train_emulator_loss_grad": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, POINTER(EmulatorHead), c_int, c_int, c_int64,
                                                c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "fv3hip_train_conv_chunk_pixels": (c_int, []),
    "fv3hip_train_conv_backward_weight_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int, c_int, c_int]),
    "fv3hip_train_conv_forward": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                          c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "fv3hip_train_conv_backward_data": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64,
                                                c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_int,
                                                c_int, c_void_p]),
    "fv3hip_train_conv_backward_weight": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int64,
                                                  c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_size_t, c_int64, c_int, c_int,
                                                  c_int, c_int, c_int, c_void_p]),
    "fv3hip_train_conv_constrain": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    "fv3hip_graph_train_chunk_cells": (c_int, []),
    "fv3hip_graph_sage_backward_weight_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int]),
    "fv3hip_graph_up2_backward_weight_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int]),
    "fv3hip_graph_sage_backward_data": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                                c_int64, c_int, c_void_p, c_int64, c_int64, c_int64, c_int, c_int64, c_int, c_int,
                                                c_int, c_void_p]),
    "fv3hip_graph_sage_backward_weight": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p,
                                                  c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_int64, c_int, c_int, c_int,
                                                  c_void_p]),
    "fv3hip_graph_up2_backward_data": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p,
                                               c_int64, c_int64, c_int64, c_int, c_int, c_int, c_void_p]),
    "fv3hip_graph_up2_backward_weight": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int,
                                                 c_void_p, c_size_t, c_int64, c_int, c_int, c_int, c_void_p]),
    "fv3hip_graph_pool2_backward": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int, c_void_p, c_int64, c_int64,
                                            c_int64, c_int, c_int, c_void_p]),
    "fv3hip_train_adamw": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_double, c_double, c_double, c_double,
                                   c_double, c_void_p]),
    "fv3hip_cyclegan_train_chunk_cells": (c_int, []),
    "fv3hip_cyclegan_train_backward_data_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int, c_int, c_int]),
    "fv3hip_cyclegan_train_backward_weight_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int, c_int, c_int]),
    "fv3hip_cyclegan_train_conv": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64,
                                           c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "fv3hip_cyclegan_train_backward_data": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64,
                                                    c_void_p, c_size_t, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "fv3hip_cyclegan_train_backward_weight": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p,
                                                      c_void_p, c_void_p, c_size_t, c_int64, c_int, c_int, c_int, c_int, c_int, c_int,
                                                      c_void_p]),
    "fv3hip_cyclegan_train_norm_backward": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p,
                                                    c_void_p, c_void_p, c_float, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64,
                                                    c_int, c_int, c_void_p]),
    "fv3hip_cyclegan_train_backward_weight_context_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int, c_int, c_int, c_int]),
    "fv3hip_cyclegan_train_backward_weight_context": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64,
                                                              c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                                              c_size_t, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "fv3hip_fmr_loss_grad_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "fv3hip_fmr_loss_grad": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int64,
                                     c_int64, c_int, c_double, c_int, c_double, c_void_p, c_void_p, c_size_t, c_void_p]),
    "fv3hip_forest_train_chunk": (c_int, []),
    "fv3hip_forest_train_begin": (c_int, [POINTER(ForestTrain), c_int64, c_void_p]),
    "fv3hip_forest_train_level": (c_int, [POINTER(ForestTrain), c_int, c_int64, c_int64, c_int64, c_int, c_int, c_int64, c_int64,
                                          c_int, c_void_p]),
    "fv3hip_timer_create": (c_int, [POINTER(c_void_p)]),
    "fv3hip_timer_start": (c_int, [c_void_p, c_void_p]),
    "fv3hip_timer_stop": (c_int, [c_void_p, c_void_p]),
    "fv3hip_timer_elapsed_ms": (c_int, [c_void_p, POINTER(c_float)]),
    "fv3hip_timer_destroy": (c_int, [c_void_p]),
}

_lib = None


def load():
    """Load libfv3hip.so (once) and attach the ABI signatures.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ExtensionMissingError(
            f"{LIB_PATH} is not built.  Run `make -C fv3net_amd/csrc` (needs hipcc) or "
            "`python -c 'import __graft_entry__ as g; g.build()'`.  There is no CPU fallback."
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError = the .so does not export a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.fv3hip_abi_version() != ABI_VERSION:
        raise ExtensionMissingError(f"{LIB_PATH} has ABI version {lib.fv3hip_abi_version()}, expected {ABI_VERSION}")
    _lib = lib
    return lib


def check(code):
    if code != OK:
        raise Fv3HipError(code, load().fv3hip_last_error().decode("utf-8", "replace"))


def call(name, *args):
    """Call an int-returning entry point and raise Fv3HipError on a non-zero status."""
    check(getattr(load(), name)(*args))


_torch = None


def call_on(where, name, *args):
    """``call`` with the HIP device of ``where`` (a torch device or tensor) current for the duration of the call, and the
    caller's device restored afterwards: the library launches on, and allocates its scratch on, the current device."""
    global _torch
    if _torch is None:
        import torch as _torch_module

        _torch = _torch_module
    dev = getattr(where, "device", where)
    idx = None if dev is None else getattr(dev, "index", None)
    lib = _lib or load()
    if idx is None or idx == _torch.cuda.current_device():
        code = getattr(lib, name)(*args)
        if code != OK:
            check(code)
        return
    with _torch.cuda.device(idx):
        check(getattr(lib, name)(*args))
