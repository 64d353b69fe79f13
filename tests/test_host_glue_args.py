"""Argument checks of the glue entry points (emulation.hip, local.hip, fit.hip, diags.hip and the column helpers of
vertical.hip): every one of them returns before the first HIP call, so they run without a GPU.

One table row per entry point: its arguments in ABI order with values that would pass every check, then what the library
returns when one of them is spoiled -- a dtype code of 7, a negative extent, a zero extent with every pointer null, one
required pointer null.  The return codes are the ones the library gave before its entry points were moved onto the shared
helpers of common.h; the odd ones are kept and marked.  No row may pass every check: that call would launch a kernel on
addresses that are no memory.
"""
import ctypes

import pytest

from fv3net_amd import _lib
from fv3net_amd._lib import EINVAL, EUNSUPPORTED, F32, F64, OK

P = ctypes.c_void_p(4096)  # a non-null address that no argument check reads
MEMBERS = (ctypes.c_void_p * 2)(4096, 4096)  # fv3hip_member_reduce walks this host array of device pointers
MEMBERS_GAP = (ctypes.c_void_p * 2)(4096, None)
NO_MASK, FORTRAN_VANISHES, CLASS_ZERO_CLOUD = 0, 1, 3


def entry(args, dtypes=(), extents=None, required=(), extra=()):
    """args: (name, good value) in ABI order; dtypes: the dtype-code arguments; extents: name -> (code for -1, code for 0
    with every pointer null); required: the pointers that must not be null at the good extents; extra: (changes, code)."""
    return dict(args=args, dtypes=dtypes, extents=extents or {}, required=required, extra=extra)


COLUMNS = {"n_batch": (EINVAL, OK), "nz": (EINVAL, OK), "n_inner": (EINVAL, OK)}
# (a column entry with levels but no columns has nothing to do; with columns but no levels it still writes per column)
COLUMNS_NEED_LEVELS = {"n_batch": (EINVAL, OK), "nz": (EINVAL, EINVAL), "n_inner": (EINVAL, OK)}
FLUX_COLUMNS = {"n_outer": (EINVAL, OK), "nz": (EINVAL, EINVAL), "n_inner": (EINVAL, OK)}  # nz >= 1 is an argument check

ENTRIES = {
    # ---- emulation.hip
    "fv3hip_zc_squash": entry(
        [("cloud", P), ("cloud_dtype", F32), ("humidity", P), ("hum_dtype", F64), ("n", 5), ("bound", 1e-3), ("out_dtype", F64),
         ("cloud_out", P), ("qv_out", P), ("stream", None)],
        dtypes=["cloud_dtype", "hum_dtype", "out_dtype"], extents={"n": (EINVAL, OK)},
        required=["cloud", "humidity", "cloud_out", "qv_out"],
        # the array dtypes are looked at after the empty return
        extra=[({"n": 0, "cloud_dtype": 7}, OK), ({"n": 0, "out_dtype": 7}, EINVAL)]),
    "fv3hip_zc_infer_cloud": entry(
        [("cloud_in", P), ("qv_in", P), ("state_dtype", F32), ("qv_emul", P), ("emul_dtype", F64), ("n", 5), ("out_dtype", F64),
         ("cloud_out", P), ("stream", None)],
        dtypes=["state_dtype", "emul_dtype", "out_dtype"], extents={"n": (EINVAL, OK)},
        required=["cloud_in", "qv_in", "qv_emul", "cloud_out"]),
    "fv3hip_zc_gscond_conserve": entry(
        [("cloud_in", P), ("qv_in", P), ("t_in", P), ("state_dtype", F64), ("cloud_emul", P), ("emul_dtype", F32),
         ("mode", FORTRAN_VANISHES), ("aux", P), ("aux_dtype", F32), ("n_class", 1), ("cls", 0), ("n0", 3), ("n1", 4),
         ("phase_dependent", 1), ("out_dtype", F64), ("cloud_out", P), ("qv_out", P), ("t_out", P), ("stream", None)],
        dtypes=["state_dtype", "emul_dtype", "aux_dtype", "out_dtype"], extents={"n0": (EINVAL, OK), "n1": (EINVAL, OK)},
        required=["cloud_in", "qv_in", "t_in", "cloud_emul", "aux", "cloud_out", "qv_out", "t_out"],
        extra=[({"mode": 5}, EINVAL), ({"mode": -1}, EINVAL), ({"mode": CLASS_ZERO_CLOUD, "cls": 1}, EINVAL),
               ({"mode": CLASS_ZERO_CLOUD, "n_class": 0}, EINVAL)]),
    "fv3hip_zc_precpd_conserve": entry(
        [("cloud_g", P), ("qv_g", P), ("t_g", P), ("delp", P), ("state_dtype", F64), ("cloud_p", P), ("qv_p", P), ("emul_dtype", F32),
         ("n0", 3), ("n1", 4), ("out_dtype", F64), ("cloud_out", P), ("qv_out", P), ("t_out", P), ("precip_out", P), ("stream", None)],
        dtypes=["state_dtype", "emul_dtype", "out_dtype"],
        # no levels: the column totals are still written, so precip_out is still needed
        extents={"n0": (EINVAL, EINVAL), "n1": (EINVAL, OK)},
        required=["cloud_g", "qv_g", "t_g", "delp", "cloud_p", "qv_p", "cloud_out", "qv_out", "t_out", "precip_out"]),
    "fv3hip_zc_precip_simple": entry(
        [("cloud_g", P), ("qv_g", P), ("delp", P), ("state_dtype", F64), ("cloud_p", P), ("qv_p", P), ("emul_dtype", F32), ("n0", 3),
         ("n1", 4), ("out_dtype", F64), ("precip_out", P), ("stream", None)],
        dtypes=["state_dtype", "emul_dtype", "out_dtype"], extents={"n0": (EINVAL, EINVAL), "n1": (EINVAL, OK)},
        required=["cloud_g", "qv_g", "delp", "cloud_p", "qv_p", "precip_out"]),
    "fv3hip_clamp": entry(
        [("x", P), ("dtype", F32), ("n", 5), ("lo", 0.0), ("hi", 1.0), ("has_lo", 1), ("has_hi", 1), ("out", P), ("stream", None)],
        dtypes=["dtype"], extents={"n": (EINVAL, OK)}, required=["x", "out"]),
    "fv3hip_level_fill": entry(
        [("emul", P), ("emul_dtype", F32), ("src", P), ("src_dtype", F64), ("fill_value", 0.0), ("n0", 3), ("n1", 4), ("start", 1),
         ("stop", 2), ("out", P), ("stream", None)],
        dtypes=["emul_dtype", "src_dtype"], extents={"n0": (EINVAL, OK), "n1": (EINVAL, OK)}, required=["emul", "out"],
        extra=[({"src": None, "src_dtype": 7, "n0": 0}, OK)]),  # without a source its dtype is not looked at
    "fv3hip_zc_class_zero": entry(
        [("x", P), ("dtype", F32), ("logits", P), ("logits_dtype", F64), ("n_class", 3), ("cls", 1), ("n", 5), ("out", P),
         ("stream", None)],
        dtypes=["dtype", "logits_dtype"], extents={"n": (EINVAL, OK)}, required=["x", "logits", "out"],
        extra=[({"cls": 3}, EINVAL), ({"cls": -1}, EINVAL), ({"n_class": 0, "cls": 0}, EINVAL), ({"n": 0, "cls": 3}, EINVAL)]),
    "fv3hip_non_negative_sphum": entry(
        [("sphum", P), ("q1", P), ("q2", P), ("dtype", F32), ("n", 5), ("dt", 900.0), ("mse_conserving", 0), ("q1_out", P),
         ("q2_out", P), ("stream", None)],
        dtypes=["dtype"], extents={"n": (EINVAL, OK)}, required=["sphum", "q2", "q1_out", "q2_out"]),
    # ---- local.hip
    "fv3hip_local_pack": entry(
        [("x", P), ("dtype", F64), ("has_levels", 1), ("transform", 1), ("eps", 1e-8), ("center", P), ("scale", P), ("nz", 3),
         ("ncol", 5), ("out", P), ("stream", None)],
        dtypes=["dtype"], extents={"nz": (EINVAL, OK), "ncol": (EINVAL, OK)}, required=["x", "center", "scale", "out"],
        extra=[({"transform": 2}, EINVAL), ({"nz": 65536}, EINVAL)]),
    "fv3hip_local_unpack": entry(
        [("yhat", P), ("yhat_level_stride", 5), ("scale", P), ("center", P), ("cond_on", P), ("cond_dtype", F64), ("edges", P),
         ("cs_scale", P), ("cs_center", P), ("n_bins", 2), ("min_scale", 0.0), ("before", P), ("before_dtype", F32), ("limit_flags", 0),
         ("value_lower", 0.0), ("value_upper", 0.0), ("after_lower", 0.0), ("after_upper", 0.0), ("nz", 3), ("ncol", 5),
         ("out_direct", P), ("out_unscaled", P), ("out_after", P), ("stream", None)],
        dtypes=["cond_dtype", "before_dtype"], extents={"nz": (EINVAL, OK), "ncol": (EINVAL, OK)},
        required=["yhat", "edges", "cs_scale", "cs_center", "out_after"],
        extra=[({"limit_flags": 16}, EINVAL), ({"yhat_level_stride": 4}, EINVAL), ({"n_bins": 0}, EINVAL), ({"nz": 65536}, EINVAL),
               ({"before": None, "out_direct": None, "out_unscaled": None, "out_after": None}, EINVAL),
               # the stride is looked at before the empty return; the optional arrays' dtypes after it
               ({"ncol": 0, "yhat_level_stride": -1}, EINVAL), ({"ncol": 0, "cond_dtype": 7}, OK)]),
    "fv3hip_classify_onehot": entry(
        [("logits", P), ("dtype", F32), ("n_class", 3), ("n", 5), ("onehot", P), ("any_of", P), ("cls_a", 0), ("cls_b", 1),
         ("stream", None)],
        dtypes=["dtype"], extents={"n_class": (EINVAL, EINVAL), "n": (EINVAL, OK)}, required=["logits", "onehot"]),
    # ---- fit.hip
    "fv3hip_level_scale": entry(
        [("x", P), ("dtype", F32), ("scale", P), ("n_outer", 2), ("nz", 3), ("n_inner", 5), ("out", P), ("stream", None)],
        dtypes=["dtype"], extents={"n_outer": (EINVAL, OK), "nz": (EINVAL, OK), "n_inner": (EINVAL, OK)},
        required=["x", "scale", "out"]),
    "fv3hip_member_reduce": entry(
        [("members", MEMBERS), ("n_members", 2), ("dtype", F32), ("op", _lib.OP_MEAN), ("n", 5), ("out", P), ("stream", None)],
        dtypes=["dtype"], extents={"n": (EINVAL, OK)}, required=["members", "out"],
        extra=[({"members": MEMBERS_GAP}, EINVAL), ({"n_members": 0}, EINVAL), ({"n_members": 33}, EINVAL),
               ({"op": _lib.OP_SUM}, EINVAL), ({"n": 0, "n_members": 0}, EINVAL)]),
    "fv3hip_tendency_to_flux": entry(
        [("tendency", P), ("delp", P), ("toa_net_flux", P), ("surface_upward_flux", P), ("dtype", F32), ("n_outer", 2), ("nz", 3),
         ("n_inner", 5), ("rectify", 1), ("closure", 0), ("net_flux", P), ("surface_downward_flux", P), ("stream", None)],
        dtypes=["dtype"], extents=FLUX_COLUMNS,
        required=["tendency", "delp", "surface_upward_flux", "net_flux", "surface_downward_flux"]),
    "fv3hip_flux_to_tendency": entry(
        [("net_flux", P), ("surface_downward_flux", P), ("surface_upward_flux", P), ("delp", P), ("dtype", F64), ("n_outer", 2),
         ("nz", 3), ("n_inner", 5), ("tendency", P), ("stream", None)],
        dtypes=["dtype"], extents=FLUX_COLUMNS,
        required=["net_flux", "surface_downward_flux", "surface_upward_flux", "delp", "tendency"]),
    "fv3hip_minmax_score": entry(
        [("x", P), ("dtype", F32), ("feat_stride", 5), ("sample_stride", 1), ("n_feat", 3), ("scale", P), ("offset", P), ("n", 5),
         ("first", 1), ("finish", 1), ("run_max", P), ("run_min", P), ("score", P), ("stream", None)],
        dtypes=["dtype"], extents={"n_feat": (EINVAL, EINVAL), "n": (EINVAL, OK)},
        required=["x", "scale", "offset", "run_max", "run_min", "score"]),
    "fv3hip_ocsvm_score": entry(
        [("x", P), ("n_feat", 3), ("n", 5), ("mean", P), ("scale", P), ("support_vectors", P), ("dual_coef", P), ("n_sv", 2),
         ("gamma", 0.5), ("score", P), ("stream", None)],
        # no support vectors is a valid model: the other arrays are still needed
        extents={"n_feat": (EINVAL, EINVAL), "n": (EINVAL, OK), "n_sv": (EINVAL, EINVAL)},
        required=["x", "mean", "scale", "support_vectors", "dual_coef", "score"],
        extra=[({"n_feat": 400}, EUNSUPPORTED)]),  # 400 * 64 float64 of LDS
    # ---- diags.hip
    "fv3hip_group_sums": entry(
        [("a", P), ("b", P), ("dtype", F32), ("weights", P), ("w_dtype", F64), ("n_batch", 1), ("nz", 2), ("n_inner", 8), ("order", P),
         ("n_order", 8), ("start", P), ("n_groups", 1), ("item_group", P), ("item_chunk", P), ("n_items", 1), ("group_item", P),
         ("sums", P), ("workspace", P), ("workspace_bytes", 160), ("stream", None)],
        dtypes=["dtype", "w_dtype"],
        # no groups or no levels: nothing to write; any other empty extent still writes (zero) sums
        extents={"n_batch": (EINVAL, EINVAL), "nz": (EINVAL, OK), "n_inner": (EINVAL, EINVAL), "n_order": (EINVAL, EINVAL),
                 "n_groups": (EINVAL, OK), "n_items": (EINVAL, EINVAL)},
        required=["a", "order", "start", "item_group", "item_chunk", "group_item", "sums", "workspace"],
        extra=[({"workspace_bytes": 159}, EINVAL), ({"nz": 65536}, EINVAL), ({"n_batch": 1 << 31}, EINVAL),
               ({"n_items": 1 << 31}, EINVAL), ({"weights": None, "w_dtype": 7, "n_groups": 0}, OK)]),
    # (these two clear `counts` before their empty return: they are covered up to the pointer check)
    "fv3hip_histogram": entry(
        [("x", P), ("dtype", F32), ("n", 5), ("edges", P), ("n_bins", 4), ("counts", P), ("stream", None)],
        dtypes=["dtype"], extents={"n": (EINVAL, EINVAL), "n_bins": (EINVAL, EINVAL)}, required=["x", "edges", "counts"],
        extra=[({"n_bins": 4097}, EINVAL)]),
    "fv3hip_histogram2d": entry(
        [("x", P), ("y", P), ("dtype", F64), ("n", 5), ("xedges", P), ("nx_bins", 4), ("yedges", P), ("ny_bins", 3), ("counts", P),
         ("stream", None)],
        dtypes=["dtype"], extents={"n": (EINVAL, EINVAL), "nx_bins": (EINVAL, EINVAL), "ny_bins": (EINVAL, EINVAL)},
        required=["x", "y", "xedges", "yedges", "counts"], extra=[({"nx_bins": 129}, EINVAL), ({"ny_bins": 129}, EINVAL)]),
    # ---- vertical.hip, outside the remap
    "fv3hip_pressure_at_interface": entry(
        [("delp", P), ("dtype", F32), ("n_batch", 2), ("nz", 3), ("n_inner", 5), ("toa_pressure", 300.0), ("out", P), ("stream", None)],
        dtypes=["dtype"], extents=COLUMNS_NEED_LEVELS, required=["delp", "out"]),
    "fv3hip_pressure_at_midpoint_log": entry(
        [("delp", P), ("dtype", F64), ("n_batch", 2), ("nz", 3), ("n_inner", 5), ("toa_pressure", 300.0), ("out", P), ("stream", None)],
        dtypes=["dtype"], extents=COLUMNS, required=["delp", "out"]),
    "fv3hip_mask_weights": entry(
        [("weights", P), ("w_dtype", F32), ("p_cmp", P), ("cmp_levels", 4), ("cmp_offset", 1), ("p_fine", P), ("p_dtype", F64),
         ("n_batch", 2), ("nz", 3), ("n_inner", 5), ("w_repeat", 1), ("out", P), ("stream", None)],
        dtypes=["w_dtype", "p_dtype"],
        # odd, kept: a negative extent is an empty product here, not an error
        extents={"n_batch": (OK, OK), "nz": (OK, OK), "n_inner": (OK, OK)}, required=["weights", "p_cmp", "p_fine", "out"],
        extra=[({"w_repeat": 0}, EINVAL), ({"w_repeat": 3}, EINVAL), ({"cmp_levels": 3}, EINVAL), ({"cmp_offset": -1}, EINVAL)]),
    "fv3hip_mask_weights_coarse": entry(
        [("weights", P), ("w_dtype", F32), ("p_cmp_coarse", P), ("cmp_levels", 4), ("cmp_offset", 1), ("p_fine", P), ("p_dtype", F64),
         ("n_batch", 2), ("nz", 3), ("ny", 4), ("nx", 4), ("factor", 2), ("w_repeat", 1), ("out", P), ("stream", None)],
        dtypes=["w_dtype", "p_dtype"],
        # odd, kept: as above for n_batch and nz; ny and nx are checked
        extents={"n_batch": (OK, OK), "nz": (OK, OK), "ny": (EINVAL, OK), "nx": (EINVAL, OK)},
        required=["weights", "p_cmp_coarse", "p_fine", "out"],
        extra=[({"factor": 0}, EINVAL), ({"factor": 3}, EINVAL), ({"w_repeat": 0}, EINVAL), ({"cmp_levels": 3}, EINVAL),
               ({"n_batch": 70000, "nz": 1, "cmp_levels": 2}, EUNSUPPORTED)]),
    "fv3hip_interpolate_2d": entry(
        [("xp", P), ("x", P), ("y", P), ("n_batch", 2), ("n_inner", 5), ("n_in", 3), ("n_out", 4), ("fill_value", 0.0),
         ("layout", _lib.LAYOUT_LEVEL_COL), ("out", P), ("stream", None)],
        extents={"n_batch": (EINVAL, OK), "n_inner": (EINVAL, OK), "n_in": (EINVAL, EINVAL), "n_out": (EINVAL, OK)},
        required=["xp", "x", "y", "out"], extra=[({"layout": 2}, EINVAL)]),
    "fv3hip_column_sum": entry(
        [("x", P), ("dtype", F32), ("n_batch", 2), ("nz", 3), ("n_inner", 5), ("addend", 1.0), ("out", P), ("stream", None)],
        dtypes=["dtype"], extents=COLUMNS_NEED_LEVELS, required=["x", "out"]),
    "fv3hip_blend_weights": entry(
        [("blending_pressure", P), ("ps_coarse", P), ("pfull_coarse", P), ("dtype", F64), ("n_batch", 2), ("nz", 3), ("n_inner", 5),
         ("out", P), ("stream", None)],
        dtypes=["dtype"], extents=COLUMNS, required=["blending_pressure", "ps_coarse", "pfull_coarse", "out"]),
    "fv3hip_hydrostatic_balance": entry(
        [("dz", P), ("phis", P), ("t", P), ("q", P), ("delp", P), ("dtype", F32), ("n_batch", 2), ("nz", 3), ("n_inner", 5),
         ("toa_pressure", 300.0), ("dz_out", P), ("phis_out", P), ("stream", None)],
        dtypes=["dtype"], extents=COLUMNS_NEED_LEVELS, required=["dz", "phis", "t", "q", "delp", "dz_out", "phis_out"]),
}


def cases(spec):
    """(label, changes to the good arguments, expected return code)"""
    is_pointer = {name: isinstance(good, (ctypes.c_void_p, ctypes.Array)) for name, good in spec["args"]}
    all_null = {name: None for name, ptr in is_pointer.items() if ptr}
    for name in spec["dtypes"]:
        yield f"{name}=7", {name: 7}, EINVAL
    for name, (negative, zero) in spec["extents"].items():
        yield f"{name}=-1", {name: -1}, negative
        yield f"{name}=0, null pointers", {**all_null, name: 0}, zero
    for name in spec["required"]:
        assert is_pointer[name], name
        yield f"{name}=null", {name: None}, EINVAL
    for changes, code in spec["extra"]:
        yield ", ".join(f"{k}={v}" for k, v in changes.items()), changes, code


def test_the_table_matches_the_signatures():
    assert set(ENTRIES) <= set(_lib.SIGNATURES)
    for name, spec in ENTRIES.items():
        assert len(spec["args"]) == len(_lib.SIGNATURES[name][1]), name
        names = [arg for arg, _ in spec["args"]]
        for arg in [*spec["dtypes"], *spec["extents"], *spec["required"], *(k for changes, _ in spec["extra"] for k in changes)]:
            assert arg in names, (name, arg)
        # every case spoils something: the good arguments themselves are never passed
        assert all(changes for _, changes, _ in cases(spec)), name


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_argument_checks(name):
    lib = _lib.load()
    fn, spec = getattr(lib, name), ENTRIES[name]
    wrong = []
    for label, changes, expected in cases(spec):
        rc = fn(*[changes.get(arg, good) for arg, good in spec["args"]])
        message = lib.fv3hip_last_error()
        if rc != expected or (rc == EINVAL and not message):
            wrong.append((label, rc, expected, message))
    assert not wrong, wrong
