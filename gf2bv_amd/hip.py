"""ctypes binding of libgf2bv_hip.so (include/gf2bv_hip.h) for packed inputs.

``LinearSystem`` reaches the solver through the CPython extension ``_internal``
(list-of-int boundary, like the reference).  Synthetic / batch workloads hand over packed
64-bit-word matrices instead -- host numpy arrays or raw device pointers (e.g.
``torch.Tensor.data_ptr()``); that path goes through this module.  No fallback: a missing
library or a missing GPU raises.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GF2BV_LIB") or os.path.join(_HERE, "libgf2bv_hip.so")   # env override: kernel experiments

MODE_SINGLE = 0
MODE_AFFINE_SPACE = 1
STATUS_SOLVED = 0
STATUS_INCONSISTENT = 1

# every symbol include/gf2bv_hip.h declares (checked by tests/test_cabi.py)
EXPORTS = [
    "gf2bv_version", "gf2bv_build_id", "gf2bv_device_count", "gf2bv_last_error",
    "gf2bv_solve_digits", "gf2bv_solve_words", "gf2bv_solve_device", "gf2bv_solve_batch_device",
    "gf2bv_solve_batch_digits", "gf2bv_solve_batch_digits_multi",
    "gf2bv_solve_rhs_digits", "gf2bv_solve_rhs_words", "gf2bv_solve_rhs_device",
    "gf2bv_factor_digits", "gf2bv_factor_words", "gf2bv_factor_device", "gf2bv_factor_solve", "gf2bv_factor_solve_device",
    "gf2bv_factor_rank", "gf2bv_factor_pivots", "gf2bv_factor_device_bytes", "gf2bv_factor_free",
    "gf2bv_factor_append_words", "gf2bv_factor_append_digits", "gf2bv_factor_append_device", "gf2bv_factor_rows",
    "gf2bv_factor_copy",
    "gf2bv_result_status", "gf2bv_result_rank", "gf2bv_result_dimension", "gf2bv_result_words",
    "gf2bv_result_origin", "gf2bv_result_basis", "gf2bv_result_pivots", "gf2bv_result_stats",
    "gf2bv_result_free", "gf2bv_space_combine", "gf2bv_space_open", "gf2bv_space_enumerate", "gf2bv_space_buffer", "gf2bv_space_close",
    "gf2bv_quad_expand_device", "gf2bv_quad_expand_words", "gf2bv_solve_quad_terms",
    "gf2bv_factor_quad_terms", "gf2bv_factor_append_quad_terms", "gf2bv_solve_rhs_quad_terms", "gf2bv_solve_batch_quad_terms",
    "gf2bv_quad_expand_batch_words",
    "gf2bv_cubic_expand_device", "gf2bv_cubic_expand_words", "gf2bv_solve_cubic_terms", "gf2bv_cubic_chunks",
    "gf2bv_quartic_expand_device", "gf2bv_quartic_expand_words", "gf2bv_solve_quartic_terms", "gf2bv_quartic_chunks",
    "gf2bv_xl3_expand_device", "gf2bv_xl3_expand_words", "gf2bv_solve_xl3_words", "gf2bv_solve_xl3_quad_terms",
    "gf2bv_quad_specialise_device", "gf2bv_quad_specialise_words", "gf2bv_xl3_expand_batch_device", "gf2bv_xl3_expand_batch_words",
    "gf2bv_solve_xl3_guess_words", "gf2bv_solve_xl3_guess_quad_terms", "gf2bv_xl3_guess_chunk", "gf2bv_xl3_guess_chunk_device",
    "gf2bv_xl4_expand_device", "gf2bv_xl4_expand_words", "gf2bv_solve_xl4_words", "gf2bv_solve_xl4_quad_terms",
    "gf2bv_xl4_expand_batch_device", "gf2bv_xl4_expand_batch_words", "gf2bv_solve_xl4_guess_words", "gf2bv_solve_xl4_guess_quad_terms",
    "gf2bv_xl4_guess_chunk", "gf2bv_xl4_guess_chunk_device", "gf2bv_xl4_quartic_root",
    "gf2bv_xl4_cubic_expand_device", "gf2bv_xl4_cubic_expand_words", "gf2bv_solve_xl4_cubic_words", "gf2bv_solve_xl4_cubic_terms",
    "gf2bv_cubic_specialise_device", "gf2bv_cubic_specialise_words", "gf2bv_xl4_cubic_expand_batch_device", "gf2bv_xl4_cubic_expand_batch_words",
    "gf2bv_solve_xl4_cubic_guess_words", "gf2bv_solve_xl4_cubic_guess_terms", "gf2bv_xl4_cubic_guess_chunk", "gf2bv_xl4_cubic_guess_chunk_device",
    "gf2bv_quad_search", "gf2bv_quad_search_alloc", "gf2bv_quad_free", "gf2bv_quad_plan", "gf2bv_quad_plan_device", "gf2bv_quad_points", "gf2bv_quad_forms_search", "gf2bv_quad_last_times",
    "gf2bv_cubic_search", "gf2bv_cubic_search_alloc", "gf2bv_cubic_plan", "gf2bv_cubic_plan_device", "gf2bv_cubic_points", "gf2bv_cubic_forms_search", "gf2bv_cubic_last_times",
    "gf2bv_quartic_search", "gf2bv_quartic_search_alloc", "gf2bv_quartic_plan", "gf2bv_quartic_plan_device", "gf2bv_quartic_points", "gf2bv_quartic_forms_search", "gf2bv_quartic_last_times",
    "gf2bv_slab_work_words", "gf2bv_slab_tiles", "gf2bv_slab_open", "gf2bv_slab_blocks", "gf2bv_slab_owner",
    "gf2bv_slab_payload_bytes", "gf2bv_slab_factor", "gf2bv_slab_apply", "gf2bv_slab_factor_on", "gf2bv_slab_apply_on",
    "gf2bv_slab_finish_local", "gf2bv_slab_solve",
    "gf2bv_slab_close",
    "gf2bv_compose_words", "gf2bv_compose_device", "gf2bv_compose_power_words", "gf2bv_compose_power_device", "gf2bv_compose_shape",
    "gf2bv_compose_last_times", "gf2bv_compose_unroll_words", "gf2bv_compose_unroll_device",
    "gf2bv_synth_device", "gf2bv_residual_device",
    "gf2bv_stream_ceiling_device", "gf2bv_lds_clock_device", "gf2bv_kernel_resources",
    "gf2bv_device_alloc", "gf2bv_device_free", "gf2bv_device_upload", "gf2bv_device_download",
    "gf2bv_pool_trim", "gf2bv_pool_idle_bytes", "gf2bv_pool_in_use", "gf2bv_host_alloc", "gf2bv_host_free", "gf2bv_host_pool_trim", "gf2bv_plan_gang",
    "gf2bv_knob_dump",
]


class Stats(ctypes.Structure):
    _fields_ = [
        ("rows", ctypes.c_int64), ("cols", ctypes.c_int64), ("stride_words", ctypes.c_int64),
        ("rank", ctypes.c_int64), ("dimension", ctypes.c_int64),
        ("status", ctypes.c_int32), ("n_panels", ctypes.c_int32), ("n_sweeps", ctypes.c_int32),
        ("panels_per_sweep", ctypes.c_int32), ("tables_per_sweep", ctypes.c_int32), ("table_bits", ctypes.c_int32),
        ("tile_words", ctypes.c_int32), ("gang_systems", ctypes.c_int32),
        ("sweep_words", ctypes.c_double), ("row_xors", ctypes.c_double),
        ("ms_pack", ctypes.c_float), ("ms_eliminate", ctypes.c_float), ("ms_sweep", ctypes.c_float),
        ("ms_backsub", ctypes.c_float), ("ms_export", ctypes.c_float), ("ms_total", ctypes.c_float),
        ("search_handovers", ctypes.c_int32), ("fast_blocks", ctypes.c_int32),
        ("hbm_words", ctypes.c_double), ("bulk_launches", ctypes.c_int32), ("outer_blocks", ctypes.c_int32),
        ("handover_retries", ctypes.c_int32), ("small_path", ctypes.c_int32),
        ("sparse_blocks", ctypes.c_int32 * 3), ("sparse_panels_first64", ctypes.c_int32), ("sparse_panels_absorb", ctypes.c_int32),
        ("sparse_panels_rounds", ctypes.c_int32), ("sparse_giveups", ctypes.c_int32), ("sparse_giveup_why", ctypes.c_int32 * 5),
        ("sparse_nz_max", ctypes.c_int32),
        ("general_unit0", ctypes.c_int32), ("general_adopted", ctypes.c_int32), ("general_merged", ctypes.c_int32),
        ("general_wide", ctypes.c_int32), ("general_two_level", ctypes.c_int32), ("general_group_adopted", ctypes.c_int32),
        ("general_group_merged", ctypes.c_int32), ("general_gj_kept", ctypes.c_int32), ("general_gj_redone", ctypes.c_int32),
        ("general_chunks", ctypes.c_int32),
        ("small_passes", ctypes.c_int32), ("small_pass_kinds", ctypes.c_int32),
    ]

    def as_dict(self) -> dict:
        """fields by name; the array fields as lists"""
        out = {}
        for name, ctype in self._fields_:
            v = getattr(self, name)
            out[name] = list(v) if issubclass(ctype, ctypes.Array) else v
        return out


class HipError(RuntimeError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = ctypes.CDLL(LIB_PATH)
        vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
        pp = ctypes.POINTER(ctypes.c_void_p)
        L.gf2bv_last_error.restype = ctypes.c_char_p
        L.gf2bv_build_id.restype = ctypes.c_char_p
        L.gf2bv_solve_digits.argtypes = [vp, vp, i32, i64, i64, i32, i32, pp]
        L.gf2bv_solve_words.argtypes = [vp, i64, i64, i64, i32, i32, pp]
        L.gf2bv_solve_device.argtypes = [vp, i64, i64, i64, i32, i32, vp, i32, pp]
        L.gf2bv_solve_batch_device.argtypes = [vp, i64, i64, i64, i64, i64, i32, i32, vp, i32, pp]
        L.gf2bv_solve_batch_digits.argtypes = [vp, vp, i32, i64, i64, i64, i32, i32, pp]
        L.gf2bv_solve_batch_digits_multi.argtypes = [vp, vp, i32, i64, i64, i64, i32, vp, i32, pp]
        L.gf2bv_solve_rhs_digits.argtypes = [vp, vp, i32, i64, i64, vp, i64, i64, i32, i32, pp]
        L.gf2bv_solve_rhs_words.argtypes = [vp, i64, i64, i64, vp, i64, i64, i32, i32, pp]
        L.gf2bv_solve_rhs_device.argtypes = [vp, i64, i64, i64, vp, i64, i64, i32, i32, vp, i32, pp]
        L.gf2bv_factor_digits.argtypes = [vp, vp, i32, i64, i64, i32, i32, pp]
        L.gf2bv_factor_words.argtypes = [vp, i64, i64, i64, i32, i32, pp]
        L.gf2bv_factor_device.argtypes = [vp, i64, i64, i64, i32, i32, vp, pp]
        L.gf2bv_factor_solve.argtypes = [vp, vp, i64, i64, pp]
        L.gf2bv_factor_solve_device.argtypes = [vp, vp, i64, i64, vp, i32, pp]
        L.gf2bv_factor_rank.argtypes = [vp]
        L.gf2bv_factor_rank.restype = i64
        L.gf2bv_factor_pivots.argtypes = [vp, vp]
        L.gf2bv_factor_device_bytes.argtypes = [vp]
        L.gf2bv_factor_device_bytes.restype = i64
        L.gf2bv_factor_free.argtypes = [vp]
        L.gf2bv_factor_free.restype = None
        L.gf2bv_factor_append_words.argtypes = [vp, vp, i64, i64]
        L.gf2bv_factor_append_digits.argtypes = [vp, vp, vp, i32, i64]
        L.gf2bv_factor_append_device.argtypes = [vp, vp, i64, i64, vp]
        L.gf2bv_factor_rows.argtypes = [vp]
        L.gf2bv_factor_rows.restype = i64
        L.gf2bv_factor_copy.argtypes = [vp, pp]
        for name, res in (("gf2bv_result_status", i32), ("gf2bv_result_rank", i64),
                          ("gf2bv_result_dimension", i64), ("gf2bv_result_words", i64)):
            getattr(L, name).restype = res
            getattr(L, name).argtypes = [vp]
        for name in ("gf2bv_result_origin", "gf2bv_result_basis", "gf2bv_result_pivots"):
            getattr(L, name).argtypes = [vp, vp]
        L.gf2bv_result_stats.argtypes = [vp, ctypes.POINTER(Stats)]
        L.gf2bv_result_free.argtypes = [vp]
        L.gf2bv_result_free.restype = None
        L.gf2bv_space_combine.argtypes = [vp, vp, i64, i64, vp, i64, vp]
        L.gf2bv_space_combine.restype = None
        L.gf2bv_space_open.argtypes = [vp, vp, i64, i64, i32, pp]
        L.gf2bv_space_enumerate.argtypes = [vp, ctypes.c_uint64, i64, i32, vp]
        L.gf2bv_space_close.argtypes = [vp]
        L.gf2bv_space_close.restype = None
        L.gf2bv_quad_search.argtypes = [vp, vp, i64, i64, i64, i32, i64, i32, vp, vp, vp]
        L.gf2bv_quad_search_alloc.argtypes = [vp, vp, i64, i64, i64, i32, i64, i32, vp, vp, pp]
        L.gf2bv_quad_free.argtypes = [vp]
        L.gf2bv_quad_free.restype = None
        L.gf2bv_quad_plan.argtypes = [vp, vp, i64, i64, i64, vp, vp, vp, vp, vp, i64]
        L.gf2bv_quad_plan_device.argtypes = [vp, vp, i64, i64, i64, i32, vp, vp, vp, vp, vp, i64]
        L.gf2bv_quad_points.argtypes = [vp, vp, i64, i64, i64, vp, i64, i64, vp]
        L.gf2bv_quad_forms_search.argtypes = [vp, i64, i64, i32, i64, vp, vp]
        L.gf2bv_quad_last_times.argtypes = [vp]
        L.gf2bv_quad_last_times.restype = None
        L.gf2bv_cubic_search.argtypes = L.gf2bv_quad_search.argtypes
        L.gf2bv_cubic_search_alloc.argtypes = L.gf2bv_quad_search_alloc.argtypes
        L.gf2bv_cubic_plan.argtypes = L.gf2bv_quad_plan.argtypes
        L.gf2bv_cubic_plan_device.argtypes = L.gf2bv_quad_plan_device.argtypes
        L.gf2bv_cubic_points.argtypes = L.gf2bv_quad_points.argtypes
        L.gf2bv_cubic_forms_search.argtypes = L.gf2bv_quad_forms_search.argtypes
        L.gf2bv_cubic_last_times.argtypes = [vp]
        L.gf2bv_cubic_last_times.restype = None
        L.gf2bv_quartic_search.argtypes = L.gf2bv_quad_search.argtypes
        L.gf2bv_quartic_search_alloc.argtypes = L.gf2bv_quad_search_alloc.argtypes
        L.gf2bv_quartic_plan.argtypes = L.gf2bv_quad_plan.argtypes
        L.gf2bv_quartic_plan_device.argtypes = L.gf2bv_quad_plan_device.argtypes
        L.gf2bv_quartic_points.argtypes = L.gf2bv_quad_points.argtypes
        L.gf2bv_quartic_forms_search.argtypes = L.gf2bv_quad_forms_search.argtypes
        L.gf2bv_quartic_last_times.argtypes = [vp]
        L.gf2bv_quartic_last_times.restype = None
        L.gf2bv_quad_expand_device.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp, i64, i32, vp]
        L.gf2bv_quad_expand_words.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp, i64, i32]
        L.gf2bv_solve_quad_terms.argtypes = [vp, vp, vp, vp, i64, i64, i64, i32, i32, pp]
        L.gf2bv_factor_quad_terms.argtypes = [vp, vp, vp, vp, i64, i64, i64, i32, i32, pp]
        L.gf2bv_factor_append_quad_terms.argtypes = [vp, vp, vp, vp, vp, i64, i64]
        L.gf2bv_solve_rhs_quad_terms.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp, i64, i64, i32, i32, pp]
        L.gf2bv_solve_batch_quad_terms.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i32, i32, pp]
        L.gf2bv_quad_expand_batch_words.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, vp, i64, i32]
        L.gf2bv_cubic_expand_device.argtypes = [vp] * 8 + [i64, i64, i64, vp, i64, i32, vp]
        L.gf2bv_cubic_expand_words.argtypes = [vp] * 8 + [i64, i64, i64, vp, i64, i32]
        L.gf2bv_solve_cubic_terms.argtypes = [vp] * 8 + [i64, i64, i64, i32, i32, pp]
        L.gf2bv_cubic_chunks.argtypes = [i64, vp, vp]
        L.gf2bv_quartic_expand_device.argtypes = [vp] * 13 + [i64, i64, i64, vp, i64, i32, vp]
        L.gf2bv_quartic_expand_words.argtypes = [vp] * 13 + [i64, i64, i64, vp, i64, i32]
        L.gf2bv_solve_quartic_terms.argtypes = [vp] * 13 + [i64, i64, i64, i32, i32, pp]
        L.gf2bv_quartic_chunks.argtypes = [i64, vp, vp, vp]
        for d in ("xl3", "xl4"):                       # the two degrees: the same signatures
            getattr(L, f"gf2bv_{d}_expand_device").argtypes = [vp, i64, i64, i64, i64, vp, i64, i32, vp]
            getattr(L, f"gf2bv_{d}_expand_words").argtypes = [vp, i64, i64, i64, i64, vp, i64, i32]
            getattr(L, f"gf2bv_solve_{d}_words").argtypes = [vp, i64, i64, i64, i32, i32, pp]
            getattr(L, f"gf2bv_solve_{d}_quad_terms").argtypes = [vp, vp, vp, vp, i64, i64, i32, i32, pp]
            getattr(L, f"gf2bv_{d}_expand_batch_device").argtypes = [vp, i64, i64, i64, i64, i64, i64, vp, i64, i64, i32, vp]
            getattr(L, f"gf2bv_{d}_expand_batch_words").argtypes = [vp, i64, i64, i64, i64, i64, i64, vp, i64, i64, i32]
            getattr(L, f"gf2bv_solve_{d}_guess_words").argtypes = [vp, i64, i64, i64, vp, i64, i64, i64, i32, i32, pp]
            getattr(L, f"gf2bv_solve_{d}_guess_quad_terms").argtypes = [vp, vp, vp, vp, i64, i64, vp, i64, i64, i64, i32, i32, pp]
            getattr(L, f"gf2bv_{d}_guess_chunk").argtypes = [i64, i64, i64, i64]
            getattr(L, f"gf2bv_{d}_guess_chunk").restype = i64
            getattr(L, f"gf2bv_{d}_guess_chunk_device").argtypes = [i64, i64, i64, i32, ctypes.POINTER(i64)]
        L.gf2bv_quad_specialise_device.argtypes = [vp, i64, i64, i64, vp, i64, i64, i64, vp, i64, i64, i32, vp]
        L.gf2bv_quad_specialise_words.argtypes = [vp, i64, i64, i64, vp, i64, i64, i64, vp, i64, i32]
        L.gf2bv_xl4_quartic_root.argtypes = [i64]
        L.gf2bv_xl4_quartic_root.restype = i64
        L.gf2bv_xl4_cubic_expand_device.argtypes = [vp, i64, i64, i64, i64, vp, i64, i32, vp]
        L.gf2bv_xl4_cubic_expand_words.argtypes = [vp, i64, i64, i64, i64, vp, i64, i32]
        L.gf2bv_solve_xl4_cubic_words.argtypes = [vp, i64, i64, i64, i32, i32, pp]
        L.gf2bv_solve_xl4_cubic_terms.argtypes = [vp] * 8 + [i64, i64, i32, i32, pp]
        L.gf2bv_cubic_specialise_device.argtypes = L.gf2bv_quad_specialise_device.argtypes
        L.gf2bv_cubic_specialise_words.argtypes = L.gf2bv_quad_specialise_words.argtypes
        L.gf2bv_xl4_cubic_expand_batch_device.argtypes = L.gf2bv_xl4_expand_batch_device.argtypes
        L.gf2bv_xl4_cubic_expand_batch_words.argtypes = L.gf2bv_xl4_expand_batch_words.argtypes
        L.gf2bv_solve_xl4_cubic_guess_words.argtypes = L.gf2bv_solve_xl4_guess_words.argtypes
        L.gf2bv_solve_xl4_cubic_guess_terms.argtypes = [vp] * 8 + [i64, i64, vp, i64, i64, i64, i32, i32, pp]
        L.gf2bv_xl4_cubic_guess_chunk.argtypes = [i64, i64, i64, i64]
        L.gf2bv_xl4_cubic_guess_chunk.restype = i64
        L.gf2bv_xl4_cubic_guess_chunk_device.argtypes = [i64, i64, i64, i32, ctypes.POINTER(i64)]
        L.gf2bv_slab_work_words.argtypes = [i64, i64]
        L.gf2bv_slab_work_words.restype = i64
        L.gf2bv_slab_tiles.argtypes = [i64]
        L.gf2bv_slab_tiles.restype = i64
        L.gf2bv_slab_open.argtypes = [vp, i64, i64, i64, vp, i64, i32, i32, i32, pp]
        L.gf2bv_slab_blocks.argtypes = [vp]
        L.gf2bv_slab_blocks.restype = i64
        L.gf2bv_slab_owner.argtypes = [vp, i32]
        L.gf2bv_slab_payload_bytes.argtypes = [vp]
        L.gf2bv_slab_payload_bytes.restype = i64
        L.gf2bv_slab_factor.argtypes = [vp, i32, vp]
        L.gf2bv_slab_apply.argtypes = [vp, i32, vp]
        L.gf2bv_slab_factor_on.argtypes = [vp, i32, vp, vp]
        L.gf2bv_slab_apply_on.argtypes = [vp, i32, vp, vp]
        L.gf2bv_slab_finish_local.argtypes = [vp]
        L.gf2bv_slab_solve.argtypes = [vp, pp]
        L.gf2bv_slab_close.argtypes = [vp]
        L.gf2bv_slab_close.restype = None
        L.gf2bv_compose_words.argtypes = [vp, i64, i64, i64, vp, i64, i64, vp, i64, i32]
        L.gf2bv_compose_device.argtypes = [vp, i64, i64, i64, vp, i64, i64, vp, i64, i32, vp]
        L.gf2bv_compose_power_words.argtypes = [vp, i64, i64, vp, i64, vp, i64, i32]
        L.gf2bv_compose_power_device.argtypes = [vp, i64, i64, vp, i64, vp, i64, i32, vp]
        L.gf2bv_compose_unroll_words.argtypes = [vp, i64, i64, i64, vp, i64, vp, i64, vp, i64, i64, vp, i64, i32]
        L.gf2bv_compose_unroll_device.argtypes = [vp, i64, i64, i64, vp, i64, vp, i64, vp, i64, i64, vp, i64, i32, vp]
        L.gf2bv_compose_shape.argtypes = [vp]
        L.gf2bv_compose_last_times.argtypes = [vp]
        L.gf2bv_compose_last_times.restype = None
        L.gf2bv_synth_device.argtypes = [vp, i64, i64, i64, ctypes.c_uint64, i32, vp]
        L.gf2bv_residual_device.argtypes = [vp, i64, i64, i64, vp, i32, vp, ctypes.POINTER(i64)]
        L.gf2bv_stream_ceiling_device.argtypes = [i32, i64, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
        L.gf2bv_lds_clock_device.argtypes = [i32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
        L.gf2bv_kernel_resources.argtypes = [i32, ctypes.POINTER(ctypes.c_int32), i32]
        L.gf2bv_device_alloc.argtypes = [i32, i64, pp]
        L.gf2bv_device_free.argtypes = [i32, vp]
        L.gf2bv_device_upload.argtypes = [i32, vp, vp, i64]
        L.gf2bv_device_download.argtypes = [i32, vp, vp, i64]
        L.gf2bv_host_alloc.argtypes = [i64, pp]
        L.gf2bv_host_free.argtypes = [vp]
        L.gf2bv_host_free.restype = None
        L.gf2bv_host_pool_trim.argtypes = []
        L.gf2bv_host_pool_trim.restype = i64
        L.gf2bv_plan_gang.argtypes = [i64, i64, i64, i64]
        L.gf2bv_plan_gang.restype = i64
        L.gf2bv_knob_dump.argtypes = [ctypes.c_char_p, i64]
        L.gf2bv_pool_trim.argtypes = [i32]
        L.gf2bv_pool_trim.restype = i64
        L.gf2bv_pool_idle_bytes.argtypes = [i32]
        L.gf2bv_pool_idle_bytes.restype = i64
        L.gf2bv_pool_in_use.argtypes = [i32, ctypes.POINTER(i64)]
        _lib = L
    return _lib


def _check(rc: int):
    if rc != 0:
        msg = lib().gf2bv_last_error().decode(errors="replace")
        if rc == 1:
            raise ValueError(msg)
        raise HipError(f"gf2bv_hip error {rc}: {msg}")


def build_id() -> str:
    """Content hash of the sources the loaded libgf2bv_hip.so was compiled from (gf2bv_amd/build.py)."""
    return lib().gf2bv_build_id().decode()


def device_count() -> int:
    return int(lib().gf2bv_device_count())


@dataclass
class Solution:
    """What one solve returns (the packed-words twin of m4ri_solve's result)."""
    status: int
    rank: int
    dimension: int
    origin: np.ndarray                         # ceil(cols/64) uint64 words, bit j = variable j
    basis: np.ndarray                          # dimension x words (mode 1), else 0 x words
    pivots: np.ndarray                         # column rank profile
    stats: dict = field(default_factory=dict)

    @property
    def solved(self) -> bool:
        return self.status == STATUS_SOLVED

    def origin_int(self) -> int:
        return int.from_bytes(self.origin.tobytes(), "little")

    def basis_ints(self) -> tuple:
        return tuple(int.from_bytes(b.tobytes(), "little") for b in self.basis)


def _take(handle, mode: int) -> Solution:
    L = lib()
    try:
        words = int(L.gf2bv_result_words(handle))
        rank = int(L.gf2bv_result_rank(handle))
        dim = int(L.gf2bv_result_dimension(handle))
        status = int(L.gf2bv_result_status(handle))
        origin = np.zeros(max(words, 1), dtype=np.uint64)
        _check(L.gf2bv_result_origin(handle, origin.ctypes.data))
        nb = dim if (mode == MODE_AFFINE_SPACE and status == STATUS_SOLVED) else 0
        basis = np.zeros((nb, words), dtype=np.uint64)
        if nb:
            _check(L.gf2bv_result_basis(handle, basis.ctypes.data))
        piv = np.zeros(max(rank, 1), dtype=np.int32)
        _check(L.gf2bv_result_pivots(handle, piv.ctypes.data))
        st = Stats()
        _check(L.gf2bv_result_stats(handle, ctypes.byref(st)))
        return Solution(status, rank, dim, origin[:words], basis, piv[:rank].copy(), st.as_dict())
    finally:
        L.gf2bv_result_free(handle)


def solve_words(aug: np.ndarray, rows: int, cols: int, mode: int = MODE_SINGLE, device: int = 0) -> Solution:
    """Solve a packed augmented system held in host memory (rows x stride uint64)."""
    aug = np.ascontiguousarray(aug, dtype=np.uint64)
    stride = aug.shape[1] if aug.ndim == 2 else (cols + 1 + 63) // 64
    h = ctypes.c_void_p()
    _check(lib().gf2bv_solve_words(aug.ctypes.data, rows, cols, stride, mode, device, ctypes.byref(h)))
    return _take(h, mode)


def solve_digits(digits: np.ndarray, offsets: np.ndarray, bits_per_digit: int, rows: int, cols: int,
                 mode: int = MODE_SINGLE, device: int = 0) -> Solution:
    digits = np.ascontiguousarray(digits, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    h = ctypes.c_void_p()
    _check(lib().gf2bv_solve_digits(digits.ctypes.data, offsets.ctypes.data, bits_per_digit, rows, cols, mode,
                                    device, ctypes.byref(h)))
    return _take(h, mode)


def solve_device(d_ptr: int, rows: int, cols: int, stride: int, mode: int = MODE_SINGLE, device: int = 0,
                 stream: int = 0, time_kernels: bool = False) -> Solution:
    """Solve a row-major augmented matrix resident in device memory (the matrix is left untouched)."""
    h = ctypes.c_void_p()
    _check(lib().gf2bv_solve_device(d_ptr, rows, cols, stride, mode, device, stream or None,
                                    1 if time_kernels else 0, ctypes.byref(h)))
    return _take(h, mode)


def solve_batch_device(d_ptr: int, nsys: int, sys_stride: int, rows: int, cols: int, stride: int,
                       mode: int = MODE_SINGLE, device: int = 0, stream: int = 0, time_kernels: bool = False) -> list:
    """nsys equal-shape systems resident in device memory, solved as lock-step gangs.  `stream` = the stream that
    produced the matrices (0 = the null stream): the gangs are ordered after it."""
    hs = _handles(nsys)
    rc = lib().gf2bv_solve_batch_device(d_ptr, nsys, sys_stride, rows, cols, stride, mode, device, stream or None,
                                        1 if time_kernels else 0, hs)
    return _take_all(hs, nsys, rc, mode)


def _handles(n: int):
    """the out[] of an entry that makes n results (never of length 0)"""
    return (ctypes.c_void_p * max(n, 1))()


def _take_all(hs, nsys: int, rc: int, mode: int) -> list:
    if rc != 0:
        for h in hs:
            if h:
                lib().gf2bv_result_free(h)
        _check(rc)
    return [_take(ctypes.c_void_p(hs[i]), mode) for i in range(nsys)]


def solve_batch_digits(digits: np.ndarray, offsets: np.ndarray, bits_per_digit: int, nsys: int, rows: int,
                       cols: int, mode: int = MODE_SINGLE, device: int = 0, devices=None) -> list:
    """nsys equal-shape systems as digit arrays; offsets has nsys*rows + 1 entries (system-major).
    `devices` (a sequence of device indices, repeats allowed) shards the systems in contiguous blocks over them, one
    host thread per entry (gf2bv_solve_batch_digits_multi); default: everything on `device`."""
    digits = np.ascontiguousarray(digits, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    hs = _handles(nsys)
    if devices is None:
        rc = lib().gf2bv_solve_batch_digits(digits.ctypes.data, offsets.ctypes.data, bits_per_digit, nsys, rows, cols,
                                            mode, device, hs)
    else:
        devs = np.ascontiguousarray(list(devices), dtype=np.int32)
        rc = lib().gf2bv_solve_batch_digits_multi(digits.ctypes.data, offsets.ctypes.data, bits_per_digit, nsys, rows,
                                                  cols, mode, devs.ctypes.data, len(devs), hs)
    return _take_all(hs, nsys, rc, mode)


def solve_batch_words(augs, rows: int, cols: int, mode: int = MODE_SINGLE, device: int = 0) -> list:
    """nsys equal-shape packed systems in host memory ([nsys, rows, stride] uint64): one upload, gang solve."""
    augs = np.ascontiguousarray(augs, dtype=np.uint64)
    nsys, stride = augs.shape[0], augs.shape[2]
    pad = (-stride) % 2                                   # the device entry wants an even stride
    if pad:
        augs = np.concatenate([augs, np.zeros((nsys, rows, pad), dtype=np.uint64)], axis=2)
        stride += pad
    buf = DeviceBuffer(max(augs.nbytes, 16), device)
    try:
        buf.upload(augs)
        return solve_batch_device(buf.ptr, nsys, rows * stride, rows, cols, stride, mode, device)
    finally:
        buf.free()


def _rhs_array(rhs: np.ndarray) -> np.ndarray:
    rhs = np.ascontiguousarray(rhs, dtype=np.uint64)
    if rhs.ndim == 1:
        rhs = rhs.reshape(1, -1)
    return rhs


def solve_rhs_words(aug: np.ndarray, rows: int, cols: int, rhs: np.ndarray, mode: int = MODE_SINGLE, device: int = 0) -> list:
    """Many right-hand sides of one matrix, one elimination (gf2bv_solve_rhs_words).  aug: the augmented matrix as for
    solve_words (its column `cols` is ignored); rhs: [nrhs, >= ceil(rows / 64)] uint64, bit r of row j = affine term of
    equation r in system j.  Element j is what solve_words returns for the matrix with right-hand side j."""
    aug = np.ascontiguousarray(aug, dtype=np.uint64)
    stride = aug.shape[1] if aug.ndim == 2 else (cols + 1 + 63) // 64
    rhs = _rhs_array(rhs)
    nrhs = rhs.shape[0]
    hs = _handles(nrhs)
    rc = lib().gf2bv_solve_rhs_words(aug.ctypes.data, rows, cols, stride, rhs.ctypes.data, nrhs, rhs.shape[1], mode, device, hs)
    return _take_all(hs, nrhs, rc, mode)


def solve_rhs_digits(digits: np.ndarray, offsets: np.ndarray, bits_per_digit: int, rows: int, cols: int, rhs: np.ndarray,
                     mode: int = MODE_SINGLE, device: int = 0) -> list:
    """solve_rhs_words with the matrix given as digit arrays (see solve_digits; bit 0 of every equation is ignored)."""
    digits = np.ascontiguousarray(digits, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    rhs = _rhs_array(rhs)
    nrhs = rhs.shape[0]
    hs = _handles(nrhs)
    rc = lib().gf2bv_solve_rhs_digits(digits.ctypes.data, offsets.ctypes.data, bits_per_digit, rows, cols, rhs.ctypes.data, nrhs,
                                      rhs.shape[1], mode, device, hs)
    return _take_all(hs, nrhs, rc, mode)


def solve_rhs_device(d_ptr: int, rows: int, cols: int, stride: int, d_rhs: int, nrhs: int, rhs_words: int,
                     mode: int = MODE_SINGLE, device: int = 0, stream: int = 0, time_kernels: bool = False) -> list:
    """solve_rhs_words with matrix and right-hand sides resident in device memory (both left untouched)."""
    hs = _handles(nrhs)
    rc = lib().gf2bv_solve_rhs_device(d_ptr, rows, cols, stride, d_rhs, nrhs, rhs_words, mode, device, stream or None,
                                      1 if time_kernels else 0, hs)
    return _take_all(hs, max(nrhs, 0), rc, mode)


class Factor:
    """A kept factorization of one matrix (gf2bv_factor_*): solve(rhs) equals solve_rhs_words on the same matrix and right-hand
    sides, result for result, for every call in any order.  The handle holds its device memory until close()."""

    def __init__(self, handle: ctypes.c_void_p, rows: int, cols: int, mode: int):
        self._h = handle
        self._rows, self.cols, self.mode = rows, cols, mode

    def _handle(self):
        if not self._h:
            raise ValueError("the factorization is closed")
        return self._h

    @property
    def rows(self) -> int:
        """the stacked row count: the factored rows plus every appended one"""
        if self._h:
            self._rows = int(lib().gf2bv_factor_rows(self._h))
        return self._rows

    def append_words(self, aug: np.ndarray, rows: int | None = None) -> None:
        """Append equations in factor_words' layout ([rows, >= ceil((cols + 1) / 64)] uint64, column `cols` ignored): the handle
        then behaves as a factorization of the stacked matrix"""
        aug = np.ascontiguousarray(aug, dtype=np.uint64)
        if aug.ndim != 2:
            raise ValueError("aug must be a [rows, words] array")
        rows = aug.shape[0] if rows is None else rows
        _check(lib().gf2bv_factor_append_words(self._handle(), aug.ctypes.data, rows, aug.shape[1]))

    def append_digits(self, digits: np.ndarray, offsets: np.ndarray, bits_per_digit: int, rows: int) -> None:
        """append_words with the equations given as digit arrays (see factor_digits)"""
        digits = np.ascontiguousarray(digits, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        _check(lib().gf2bv_factor_append_digits(self._handle(), digits.ctypes.data, offsets.ctypes.data, bits_per_digit,
                                                rows))

    def append_device(self, d_ptr: int, rows: int, stride: int, stream: int = 0) -> None:
        """append_words with the equations resident in device memory (16-byte aligned, even stride; left untouched)"""
        _check(lib().gf2bv_factor_append_device(self._handle(), d_ptr, rows, stride, stream or None))

    def append_quad_terms(self, lin, term_off, ta, tb, n_lin: int) -> None:
        """Append factored quadratic equations (the arrays of quad_expand_words, every row live): expanded on the device and
        appended there (gf2bv_factor_append_quad_terms); n_lin must be the one the factorization was made with"""
        lin, term_off, ta, tb = _terms(n_lin, lin, term_off, ta, tb)
        _check(lib().gf2bv_factor_append_quad_terms(self._handle(), *_ptrs(lin, term_off, ta, tb),
                                                    len(lin), n_lin))

    def copy(self) -> "Factor":
        """An independent handle with the same state (a device-to-device copy, no factorization)"""
        h = ctypes.c_void_p()
        _check(lib().gf2bv_factor_copy(self._handle(), ctypes.byref(h)))
        return Factor(h, self.rows, self.cols, self.mode)

    @property
    def rank(self) -> int:
        return int(lib().gf2bv_factor_rank(self._handle()))

    @property
    def pivots(self) -> np.ndarray:
        """the pivot columns of one state of the handle: ONE locked call into a buffer of cols entries pre-filled with -1 (an
        append on another thread may raise the rank between two calls, so the count comes from what was written)"""
        piv = np.full(max(self.cols, 1), -1, dtype=np.int32)
        _check(lib().gf2bv_factor_pivots(self._handle(), piv.ctypes.data))
        return piv[:int(np.count_nonzero(piv >= 0))].copy()

    @property
    def device_bytes(self) -> int:
        return int(lib().gf2bv_factor_device_bytes(self._handle()))

    def solve(self, rhs: np.ndarray) -> list:
        """rhs: [nrhs, >= ceil(rows / 64)] uint64 (see solve_rhs_words); one Solution per right-hand side"""
        rhs = _rhs_array(rhs)
        nrhs = rhs.shape[0]
        hs = _handles(nrhs)
        rc = lib().gf2bv_factor_solve(self._handle(), rhs.ctypes.data, nrhs, rhs.shape[1], hs)
        return _take_all(hs, nrhs, rc, self.mode)

    def solve_device(self, d_rhs: int, nrhs: int, rhs_words: int, stream: int = 0) -> list:
        """solve() with the right-hand sides resident in device memory"""
        hs = _handles(nrhs)
        rc = lib().gf2bv_factor_solve_device(self._handle(), d_rhs, nrhs, rhs_words, stream or None, 0, hs)
        return _take_all(hs, max(nrhs, 0), rc, self.mode)

    def close(self) -> None:
        if self._h:
            lib().gf2bv_factor_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _factor(rc: int, h: ctypes.c_void_p, rows: int, cols: int, mode: int) -> Factor:
    if rc != 0:
        _check(rc)
    return Factor(h, rows, cols, mode)


def factor_words(aug: np.ndarray, rows: int, cols: int, mode: int = MODE_SINGLE, device: int = 0) -> Factor:
    """Factor the matrix of solve_words' augmented input (its column `cols` is ignored) once; Factor.solve then takes
    right-hand sides as solve_rhs_words does."""
    aug = np.ascontiguousarray(aug, dtype=np.uint64)
    stride = aug.shape[1] if aug.ndim == 2 else (cols + 1 + 63) // 64
    h = ctypes.c_void_p()
    rc = lib().gf2bv_factor_words(aug.ctypes.data, rows, cols, stride, mode, device, ctypes.byref(h))
    return _factor(rc, h, rows, cols, mode)


def factor_digits(digits: np.ndarray, offsets: np.ndarray, bits_per_digit: int, rows: int, cols: int,
                  mode: int = MODE_SINGLE, device: int = 0) -> Factor:
    """factor_words with the matrix given as digit arrays (see solve_digits; bit 0 of every equation is ignored)."""
    digits = np.ascontiguousarray(digits, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    h = ctypes.c_void_p()
    rc = lib().gf2bv_factor_digits(digits.ctypes.data, offsets.ctypes.data, bits_per_digit, rows, cols, mode, device,
                                   ctypes.byref(h))
    return _factor(rc, h, rows, cols, mode)


def factor_device(d_ptr: int, rows: int, cols: int, stride: int, mode: int = MODE_SINGLE, device: int = 0,
                  stream: int = 0) -> Factor:
    """factor_words with the matrix resident in device memory (left untouched)."""
    h = ctypes.c_void_p()
    rc = lib().gf2bv_factor_device(d_ptr, rows, cols, stride, mode, device, stream or None, ctypes.byref(h))
    return _factor(rc, h, rows, cols, mode)


def space_enumerate(origin: np.ndarray, basis: np.ndarray, first: int, count: int, gray: bool = True,
                    device: int = 0) -> np.ndarray:
    """Elements first .. first+count-1 of the affine space origin + span(basis), materialised on the device
    ([count, words] uint64): Gray order (AffineSpaceIterator) or binary order (AffineSpaceIteratorSlow / get)."""
    origin = np.ascontiguousarray(origin, dtype=np.uint64)
    basis = np.ascontiguousarray(basis, dtype=np.uint64).reshape(-1, len(origin))
    h = ctypes.c_void_p()
    _check(lib().gf2bv_space_open(origin.ctypes.data, basis.ctypes.data, basis.shape[0], len(origin), device, ctypes.byref(h)))
    try:
        out = np.zeros((count, len(origin)), dtype=np.uint64)
        _check(lib().gf2bv_space_enumerate(h, first, count, 1 if gray else 0, out.ctypes.data))
        return out
    finally:
        lib().gf2bv_space_close(h)


def _ints_to_words(vals, words: int) -> np.ndarray:
    out = np.zeros((max(len(vals), 1), words), dtype=np.uint64)
    for k, v in enumerate(vals):
        out[k] = np.frombuffer(int(v).to_bytes(words * 8, "little"), dtype=np.uint64)
    return out


def _words_to_ints(arr: np.ndarray, n: int) -> list:
    return [int.from_bytes(arr[k].tobytes(), "little") for k in range(n)]


def quad_words(n_lin: int) -> int:
    """words of a QuadraticSystem point with n_lin linear unknowns (n_lin + n_lin(n_lin-1)/2 columns)"""
    return (n_lin + n_lin * (n_lin - 1) // 2 + 63) // 64


def cubic_cols(n_lin: int) -> int:
    return n_lin + n_lin * (n_lin - 1) // 2 + n_lin * (n_lin - 1) * (n_lin - 2) // 6


def quartic_cols(n_lin: int) -> int:
    return cubic_cols(n_lin) + n_lin * (n_lin - 1) * (n_lin - 2) * (n_lin - 3) // 24


# The quad_*, cubic_* and quartic_* search functions below are one body each, taking the kind: "quad" (gf2bv_quad_*, points over the
# n_lin + n_lin(n_lin-1)/2 columns of a QuadraticSystem), "cubic" (gf2bv_cubic_*, over cubic_cols(n_lin) columns, cubic forms) or
# "quartic" (gf2bv_quartic_*, over quartic_cols(n_lin) columns, quartic forms)
def _space_words(kind: str, n_lin: int) -> int:
    return quad_words(n_lin) if kind == "quad" else ((cubic_cols if kind == "cubic" else quartic_cols)(n_lin) + 63) // 64


def _search_plan(kind: str, origin: int, basis, n_lin: int, device: int | None) -> dict:
    words = _space_words(kind, n_lin)
    o, b = _ints_to_words([origin], words), _ints_to_words(list(basis), words)
    r, re, m, fw = (ctypes.c_int64() for _ in range(4))
    host, on_device = getattr(lib(), f"gf2bv_{kind}_plan"), getattr(lib(), f"gf2bv_{kind}_plan_device")

    def plan(forms, cap):
        head = (o.ctypes.data, b.ctypes.data, len(basis), words, n_lin)
        tail = (ctypes.byref(r), ctypes.byref(re), ctypes.byref(m), ctypes.byref(fw), forms, cap)
        _check(host(*head, *tail) if device is None else on_device(*head, device, *tail))

    plan(None, 0)
    forms = np.zeros((max(m.value, 1), max(fw.value, 1)), dtype=np.uint64)
    plan(forms.ctypes.data, m.value)
    return {"r": r.value, "r_eff": re.value, "forms": _words_to_ints(forms, m.value)}


def _search_points(kind: str, origin: int, basis, n_lin: int, ys, yw: int) -> list:
    words = _space_words(kind, n_lin)
    o, b = _ints_to_words([origin], words), _ints_to_words(list(basis), words)
    y = _ints_to_words(list(ys), yw)
    out = np.zeros((max(len(ys), 1), words), dtype=np.uint64)
    _check(getattr(lib(), f"gf2bv_{kind}_points")(o.ctypes.data, b.ctypes.data, len(basis), words, n_lin, y.ctypes.data, len(ys), yw,
                                                  out.ctypes.data))
    return _words_to_ints(out, len(ys))


def _forms_search(kind: str, forms, fw: int, r_eff: int, device: int, max_out: int) -> tuple:
    f = _ints_to_words(list(forms), fw)
    cnt = ctypes.c_int64()
    out = np.zeros(max(max_out, 1), dtype=np.uint64)
    _check(getattr(lib(), f"gf2bv_{kind}_forms_search")(f.ctypes.data, len(forms), r_eff, device, max_out, ctypes.byref(cnt), out.ctypes.data))
    return cnt.value, [int(v) for v in out[:min(cnt.value, max_out)]]


def _last_times(kind: str) -> dict:
    v = (ctypes.c_double * 8)()
    getattr(lib(), f"gf2bv_{kind}_last_times")(v)
    keys = ("ms_reduce", "ms_forms", "ms_affine", "ms_search", "ms_relin", "ms_total", "levels", "candidates")
    return dict(zip(keys, list(v)))


def quad_plan(origin: int, basis, n_lin: int, device: int | None = None) -> dict:
    """gf2bv_quad_plan (host only): r, r_eff (-1: not reduced), and the forms as equation ints over r_eff unknowns.  With a
    device: gf2bv_quad_plan_device, the same plan with the forms built by k_quad_forms on that device."""
    return _search_plan("quad", origin, basis, n_lin, device)


def quad_points(origin: int, basis, n_lin: int, ys) -> list:
    """gf2bv_quad_points (host only): the points of the space that common zeros `ys` of quad_plan's forms stand for."""
    return _search_points("quad", origin, basis, n_lin, ys, max(1, max((int(y).bit_length() for y in ys), default=0) // 64 + 1))


def quad_forms_search(forms, r_eff: int, device: int = 0, max_out: int = 1 << 22) -> tuple:
    """gf2bv_quad_forms_search: (count, ascending common zeros) of forms given as equation ints over r_eff unknowns."""
    return _forms_search("quad", forms, (r_eff + r_eff * (r_eff - 1) // 2 + 64) // 64, r_eff, device, max_out)


def quad_last_times() -> dict:
    """this thread's last gf2bv_quad_search: phase times in ms, levels, first-pass candidates"""
    return _last_times("quad")


def cubic_plan(origin: int, basis, n_lin: int, device: int | None = None) -> dict:
    """gf2bv_cubic_plan (host only): r, r_eff (-1: r above 64, not reduced), and the forms as equation ints of a PackedCubicSystem of
    r_eff unknowns.  With a device: gf2bv_cubic_plan_device, the forms built by k_forms_products<3> / k_forms_sum on that device."""
    return _search_plan("cubic", origin, basis, n_lin, device)


def cubic_points(origin: int, basis, n_lin: int, ys) -> list:
    """gf2bv_cubic_points (host only): the points of the space that common zeros `ys` (ints below 2^64) of cubic_plan's forms stand for."""
    return _search_points("cubic", origin, basis, n_lin, ys, 1)


def cubic_forms_search(forms, r_eff: int, device: int = 0, max_out: int = 1 << 22) -> tuple:
    """gf2bv_cubic_forms_search: (count, ascending common zeros) of cubic forms given as equation ints over r_eff unknowns."""
    return _forms_search("cubic", forms, (cubic_cols(r_eff) + 64) // 64, r_eff, device, max_out)


def cubic_last_times() -> dict:
    """this thread's last gf2bv_cubic_search: phase times in ms, rounds of the affine elimination, first-pass candidates"""
    return _last_times("cubic")


def quartic_plan(origin: int, basis, n_lin: int, device: int | None = None) -> dict:
    """gf2bv_quartic_plan (host only): r, r_eff (-1: r above 64, not reduced), and the forms as equation ints of a PackedQuarticSystem
    of r_eff unknowns.  With a device: gf2bv_quartic_plan_device, the forms built by k_forms_products<4> / k_forms_sum on that device."""
    return _search_plan("quartic", origin, basis, n_lin, device)


def quartic_points(origin: int, basis, n_lin: int, ys) -> list:
    """gf2bv_quartic_points (host only): the points of the space that common zeros `ys` (ints below 2^64) of quartic_plan's forms stand for."""
    return _search_points("quartic", origin, basis, n_lin, ys, 1)


def quartic_forms_search(forms, r_eff: int, device: int = 0, max_out: int = 1 << 22) -> tuple:
    """gf2bv_quartic_forms_search: (count, ascending common zeros) of quartic forms given as equation ints over r_eff unknowns."""
    return _forms_search("quartic", forms, (quartic_cols(r_eff) + 64) // 64, r_eff, device, max_out)


def quartic_last_times() -> dict:
    """this thread's last gf2bv_quartic_search: phase times in ms, rounds of the affine elimination, first-pass candidates"""
    return _last_times("quartic")


def quad_cols(n_lin: int) -> int:
    """columns of a linearised quadratic system in n_lin unknowns: the unknowns and their n_lin(n_lin-1)/2 products"""
    return n_lin + n_lin * (n_lin - 1) // 2


def xl3_cols(n_lin: int) -> int:
    """columns of the degree-3 XL system in n_lin unknowns: the unknowns, their pairs and their triples"""
    return quad_cols(n_lin) + n_lin * (n_lin - 1) * (n_lin - 2) // 6


def xl4_cols(n_lin: int) -> int:
    """columns of the degree-4 XL system in n_lin unknowns: degree 3's and the quadruples"""
    return xl3_cols(n_lin) + n_lin * (n_lin - 1) * (n_lin - 2) * (n_lin - 3) // 24


# how the messages name a group's offsets and its operands
_GROUP_NAMES = (("term_off", "ta and tb"), ("off3", "ua, ub and uc"), ("off4", "va, vb, vc and vd"))


def _terms(n_lin: int, lin, *groups) -> tuple:
    """the factored form of gf2bv_*_expand_* -- lin, then per group of products (of 2, 3, 4 forms) its offsets and its operand arrays,
    flat -- as contiguous arrays, shapes checked against each other"""
    wl = (n_lin + 1 + 63) // 64
    out, at = [np.ascontiguousarray(lin, dtype=np.uint64).reshape(-1, wl)], 0
    for arity, (off_name, op_names) in zip((2, 3, 4), _GROUP_NAMES):
        if at == len(groups):
            break
        off = np.ascontiguousarray(groups[at], dtype=np.int64).reshape(-1)
        ops = [np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, wl) for x in groups[at + 1:at + 1 + arity]]
        if len(off) != len(out[0]) + 1 or len({len(x) for x in ops}) != 1 or (len(off) and off[-1] != len(ops[0])):
            raise ValueError(f"{off_name} needs one entry per row of lin and one more, ending at the number of operands in {op_names}")
        out += [off] + ops
        at += 1 + arity
    return tuple(out)


def _ptrs(*arrays):
    return [a.ctypes.data for a in arrays]


# The quad_*, cubic_* and quartic_* functions below are one body each, taking the degree (2, 3, 4: one, two, three groups of products)
_DEGREE = {2: ("quad", quad_cols), 3: ("cubic", xl3_cols), 4: ("quartic", xl4_cols)}


def _expand_words(degree: int, terms, n_lin: int, rows: int | None, stride_words: int | None, device: int) -> np.ndarray:
    name, cols = _DEGREE[degree]
    terms = _terms(n_lin, *terms)
    rows = len(terms[0]) if rows is None else rows
    stride = (cols(n_lin) + 1 + 63) // 64 if stride_words is None else stride_words
    out = np.empty((max(rows, 0), max(stride, 0)), dtype=np.uint64)
    _check(getattr(lib(), f"gf2bv_{name}_expand_words")(*_ptrs(*terms), len(terms[0]), rows, n_lin, out.ctypes.data, stride, device))
    return out


def _expand_device(degree: int, d_terms, rows_live: int, rows: int, n_lin: int, d_aug: int, stride: int, device: int, stream: int) -> None:
    _check(getattr(lib(), f"gf2bv_{_DEGREE[degree][0]}_expand_device")(*d_terms, rows_live, rows, n_lin, d_aug, stride, device, stream or None))


def _solve_terms(degree: int, terms, n_lin: int, rows: int | None, mode: int, device: int) -> Solution:
    name, cols = _DEGREE[degree]
    terms = _terms(n_lin, *terms)
    rows = max(len(terms[0]), cols(n_lin)) if rows is None else rows
    h = ctypes.c_void_p()
    _check(getattr(lib(), f"gf2bv_solve_{name}_terms")(*_ptrs(*terms), len(terms[0]), rows, n_lin, mode, device, ctypes.byref(h)))
    return _take(h, mode)


def quad_expand_words(lin, term_off, ta, tb, n_lin: int, rows: int | None = None, stride_words: int | None = None,
                      device: int = 0) -> np.ndarray:
    """Factored quadratic equations (lin[r] ^ XOR of the products ta[t] * tb[t], t in term_off[r] .. term_off[r + 1]; linear forms of
    ceil((n_lin + 1) / 64) words, bit 0 constant, bit 1 + g unknown g) expanded on the device into the linearised rows of the
    augmented-words layout: [rows, stride_words] uint64, rows beyond len(lin) zero (gf2bv_quad_expand_words)."""
    return _expand_words(2, (lin, term_off, ta, tb), n_lin, rows, stride_words, device)


def quad_expand_device(d_lin: int, d_term_off: int, d_ta: int, d_tb: int, rows_live: int, rows: int, n_lin: int, d_aug: int,
                       stride: int, device: int = 0, stream: int = 0) -> None:
    """quad_expand_words with everything resident in device memory: the kernel is enqueued on `stream` and the call returns; a
    solve_device / factor_device on the same stream reads the finished rows."""
    _expand_device(2, (d_lin, d_term_off, d_ta, d_tb), rows_live, rows, n_lin, d_aug, stride, device, stream)


def solve_quad_terms(lin, term_off, ta, tb, n_lin: int, rows: int | None = None, mode: int = MODE_SINGLE, device: int = 0) -> Solution:
    """The factored system uploaded, expanded on the device and solved there (gf2bv_solve_quad_terms): what solve_words returns for
    quad_expand_words of the same arrays.  rows (default: max(len(lin), columns)) >= the columns."""
    return _solve_terms(2, (lin, term_off, ta, tb), n_lin, rows, mode, device)


def factor_quad_terms(lin, term_off, ta, tb, n_lin: int, rows: int | None = None, mode: int = MODE_SINGLE, device: int = 0) -> Factor:
    """The factored system uploaded, expanded on the device and factored there (gf2bv_factor_quad_terms): what factor_words returns
    for quad_expand_words of the same arrays.  rows (default: max(len(lin), columns)) >= the columns."""
    lin, term_off, ta, tb = _terms(n_lin, lin, term_off, ta, tb)
    rows = max(len(lin), quad_cols(n_lin)) if rows is None else rows
    h = ctypes.c_void_p()
    rc = lib().gf2bv_factor_quad_terms(*_ptrs(lin, term_off, ta, tb), len(lin), rows, n_lin,
                                       mode, device, ctypes.byref(h))
    return _factor(rc, h, rows, quad_cols(n_lin), mode)


def solve_rhs_quad_terms(lin, term_off, ta, tb, n_lin: int, rhs: np.ndarray, rows: int | None = None, mode: int = MODE_SINGLE,
                         device: int = 0) -> list:
    """Many right-hand sides of one factored system, one elimination (gf2bv_solve_rhs_quad_terms): what solve_rhs_words returns for
    quad_expand_words of the same arrays (the constants of the factored rows are ignored: rhs holds them)."""
    lin, term_off, ta, tb = _terms(n_lin, lin, term_off, ta, tb)
    rows = max(len(lin), quad_cols(n_lin)) if rows is None else rows
    rhs = _rhs_array(rhs)
    nrhs = rhs.shape[0]
    hs = _handles(nrhs)
    rc = lib().gf2bv_solve_rhs_quad_terms(*_ptrs(lin, term_off, ta, tb), len(lin), rows, n_lin,
                                          rhs.ctypes.data, nrhs, rhs.shape[1], mode, device, hs)
    return _take_all(hs, nrhs, rc, mode)


# ---- composition: affine maps substituted into affine forms, powers of a self-map (gf2bv_compose_*) --------------------------------
def form_words(unknowns: int) -> int:
    """64-bit words of an affine form over `unknowns` unknowns: the constant and one bit each"""
    return (unknowns + 1 + 63) // 64


def exponent_words(k: int) -> np.ndarray:
    """a non-negative int as little-endian uint64 words, at least one (the exponent of gf2bv_compose_power_*)"""
    k = int(k)
    if k < 0:
        raise ValueError("the exponent must not be negative")
    nw = max(1, (k.bit_length() + 63) // 64)
    return np.frombuffer(k.to_bytes(8 * nw, "little"), dtype=np.uint64).copy()


def compose_shape() -> dict:
    """gf2bv_compose_shape (no device): k_compose's bits of `a` per table slice, rows per workgroup, words per column tile, LDS bytes"""
    v = (ctypes.c_int32 * 4)()
    _check(lib().gf2bv_compose_shape(v))
    return dict(zip(("slice_bits", "rows_per_workgroup", "tile_words", "lds_bytes"), (int(x) for x in v)))


def compose_last_times() -> dict:
    """this thread's last composition entry: upload, kernels, download in ms, and the number of products"""
    v = (ctypes.c_double * 4)()
    lib().gf2bv_compose_last_times(v)
    return {"ms_upload": v[0], "ms_kernels": v[1], "ms_download": v[2], "products": int(v[3])}


def _forms(x, unknowns: int, what: str) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.uint64)
    if x.ndim != 2 or x.shape[1] < form_words(unknowns):
        raise ValueError(f"{what} must be a 2-D uint64 array of at least {form_words(unknowns)} words a row")
    return x


def compose_words(a, n: int, b, nb: int, stride_words: int | None = None, device: int = 0) -> np.ndarray:
    """The forms a ([ra, >= ceil((n + 1) / 64)] uint64, bit 0 the constant, bit 1 + g unknown g) with the images b ([n, >= ceil((nb + 1) / 64)],
    row g replaces unknown g) substituted on the device: [ra, stride_words] uint64 over nb unknowns (gf2bv_compose_words)."""
    a, b = _forms(a, n, "a"), _forms(b, nb, "b")
    if len(b) != n:
        raise ValueError("b needs one image row per unknown of a")
    stride = form_words(nb) if stride_words is None else stride_words
    out = np.empty((len(a), max(stride, 0)), dtype=np.uint64)
    _check(lib().gf2bv_compose_words(a.ctypes.data if len(a) else out.ctypes.data, len(a), a.shape[1], n, b.ctypes.data, b.shape[1], nb,
                                     out.ctypes.data, stride, device))
    return out


def compose_device(d_a: int, ra: int, a_stride: int, n: int, d_b: int, b_stride: int, nb: int, d_out: int, out_stride: int,
                   device: int = 0, stream: int = 0) -> None:
    """compose_words with everything resident in device memory: the kernel is enqueued on `stream` and the call returns."""
    _check(lib().gf2bv_compose_device(d_a, ra, a_stride, n, d_b, b_stride, nb, d_out, out_stride, device, stream or None))


def compose_power_words(b, n: int, k: int, stride_words: int | None = None, device: int = 0) -> np.ndarray:
    """The self-map b ([n, >= ceil((n + 1) / 64)] uint64) substituted into itself k times by square-and-multiply on the device:
    [n, stride_words] uint64; k = 0 the identity (gf2bv_compose_power_words)."""
    b, kw = _forms(b, n, "b"), exponent_words(k)
    if len(b) != n:
        raise ValueError("b needs one image row per unknown")
    stride = form_words(n) if stride_words is None else stride_words
    out = np.empty((n, max(stride, 0)), dtype=np.uint64)
    _check(lib().gf2bv_compose_power_words(b.ctypes.data, b.shape[1], n, kw.ctypes.data, len(kw), out.ctypes.data, stride, device))
    return out


def compose_power_device(d_b: int, b_stride: int, n: int, k: int, d_out: int, out_stride: int, device: int = 0, stream: int = 0) -> None:
    """compose_power_words on device memory: works on `stream` behind what is queued there and waits for it (its buffers go back to
    the pool); d_out may be d_b."""
    kw = exponent_words(k)
    _check(lib().gf2bv_compose_power_device(d_b, b_stride, n, kw.ctypes.data, len(kw), d_out, out_stride, device, stream or None))


def compose_unroll_words(a, n: int, b, count: int, start: int = 0, step: int = 1, stride_words: int | None = None,
                         device: int = 0) -> np.ndarray:
    """The forms a ([ra, >= ceil((n + 1) / 64)] uint64) watched while the self-map b ([n, >= ceil((n + 1) / 64)]) steps on the device:
    [count * ra, stride_words] uint64, time-major -- row i * ra + r is a[r] with b substituted start + i * step times
    (gf2bv_compose_unroll_words)."""
    a, b = _forms(a, n, "a"), _forms(b, n, "b")
    if len(b) != n:
        raise ValueError("b needs one image row per unknown")
    sw, pw = exponent_words(start), exponent_words(step)
    stride = form_words(n) if stride_words is None else stride_words
    out = np.empty((max(count, 0) * len(a), max(stride, 0)), dtype=np.uint64)
    # (no rows: the library still wants pointers)
    _check(lib().gf2bv_compose_unroll_words(a.ctypes.data if len(a) else b.ctypes.data, len(a), a.shape[1], n, b.ctypes.data, b.shape[1],
                                            sw.ctypes.data, len(sw), pw.ctypes.data, len(pw), count,
                                            out.ctypes.data if out.size else b.ctypes.data, stride, device))
    return out


def compose_unroll_device(d_a: int, ra: int, a_stride: int, n: int, d_b: int, b_stride: int, count: int, d_out: int, out_stride: int,
                          start: int = 0, step: int = 1, device: int = 0, stream: int = 0) -> None:
    """compose_unroll_words on device memory: count * ra rows at d_out, out_stride words apart.  Works on `stream` behind what is queued
    there and waits for it (its buffers go back to the pool); d_out must not overlap d_a or d_b."""
    sw, pw = exponent_words(start), exponent_words(step)
    _check(lib().gf2bv_compose_unroll_device(d_a, ra, a_stride, n, d_b, b_stride, sw.ctypes.data, len(sw), pw.ctypes.data, len(pw), count,
                                             d_out, out_stride, device, stream or None))


def _sys_row_off(sys_row_off, nrows: int) -> np.ndarray:
    sys_row_off = np.ascontiguousarray(sys_row_off, dtype=np.int64).reshape(-1)
    if len(sys_row_off) < 1 or sys_row_off[-1] != nrows:
        raise ValueError("sys_row_off needs one entry per system and one more, ending at the rows of lin")
    return sys_row_off


def solve_batch_quad_terms(lin, term_off, ta, tb, sys_row_off, n_lin: int, rows: int | None = None, mode: int = MODE_SINGLE,
                           device: int = 0) -> list:
    """Independent factored systems over the same n_lin as one concatenated term set (system s: rows sys_row_off[s] ..
    sys_row_off[s + 1]), expanded by one launch -- each padded to `rows` rows on the device -- and solved as lock-step gangs
    (gf2bv_solve_batch_quad_terms).  Element s is what solve_quad_terms returns for system s with the same `rows`."""
    lin, term_off, ta, tb = _terms(n_lin, lin, term_off, ta, tb)
    sys_row_off = _sys_row_off(sys_row_off, len(lin))
    nsys = len(sys_row_off) - 1
    rows = max(int(np.diff(sys_row_off).max(initial=0)), quad_cols(n_lin)) if rows is None else rows
    hs = _handles(nsys)
    rc = lib().gf2bv_solve_batch_quad_terms(*_ptrs(lin, term_off, ta, tb), sys_row_off.ctypes.data,
                                            nsys, rows, n_lin, mode, device, hs)
    return _take_all(hs, nsys, rc, mode)


def quad_expand_batch_words(lin, term_off, ta, tb, sys_row_off, n_lin: int, rows: int, stride_words: int | None = None,
                            device: int = 0) -> np.ndarray:
    """The batched expansion alone (gf2bv_quad_expand_batch_words): [nsys, rows, stride_words] uint64, system s the rows
    sys_row_off[s] .. sys_row_off[s + 1] of the term set expanded and the rows behind them zero."""
    lin, term_off, ta, tb = _terms(n_lin, lin, term_off, ta, tb)
    sys_row_off = _sys_row_off(sys_row_off, len(lin))
    nsys = len(sys_row_off) - 1
    stride = (quad_cols(n_lin) + 1 + 63) // 64 if stride_words is None else stride_words
    out = np.empty((nsys, max(rows, 0), max(stride, 0)), dtype=np.uint64)
    _check(lib().gf2bv_quad_expand_batch_words(*_ptrs(lin, term_off, ta, tb),
                                               sys_row_off.ctypes.data, nsys, rows, n_lin, out.ctypes.data, stride, device))
    return out


def cubic_chunks(n_lin: int) -> tuple:
    """(quadratic, cubic) terms of a row that one pass of the cubic expansion kernel holds in LDS (gf2bv_cubic_chunks, host only)"""
    q, c = ctypes.c_int32(), ctypes.c_int32()
    _check(lib().gf2bv_cubic_chunks(n_lin, ctypes.byref(q), ctypes.byref(c)))
    return q.value, c.value


def cubic_expand_words(lin, off2, ta, tb, off3, ua, ub, uc, n_lin: int, rows: int | None = None, stride_words: int | None = None,
                       device: int = 0) -> np.ndarray:
    """Factored cubic equations (lin[r] ^ XOR of ta[t] * tb[t], t in off2[r] .. off2[r + 1] ^ XOR of ua[u] * ub[u] * uc[u], u in
    off3[r] .. off3[r + 1]; affine forms of ceil((n_lin + 1) / 64) words, bit 0 constant, bit 1 + g unknown g; the products exact in
    GF(2)[x] / (x_i^2 + x_i)) expanded on the device into rows over the xl3_cols(n_lin) columns of the augmented-words layout:
    [rows, stride_words] uint64, rows beyond len(lin) zero (gf2bv_cubic_expand_words)."""
    return _expand_words(3, (lin, off2, ta, tb, off3, ua, ub, uc), n_lin, rows, stride_words, device)


def cubic_expand_device(d_lin: int, d_off2: int, d_ta: int, d_tb: int, d_off3: int, d_ua: int, d_ub: int, d_uc: int, rows_live: int,
                        rows: int, n_lin: int, d_aug: int, stride: int, device: int = 0, stream: int = 0) -> None:
    """cubic_expand_words with everything resident in device memory: the kernel is enqueued on `stream` and the call returns; a
    solve_device on the same stream reads the finished rows."""
    _expand_device(3, (d_lin, d_off2, d_ta, d_tb, d_off3, d_ua, d_ub, d_uc), rows_live, rows, n_lin, d_aug, stride, device, stream)


def solve_cubic_terms(lin, off2, ta, tb, off3, ua, ub, uc, n_lin: int, rows: int | None = None, mode: int = MODE_SINGLE,
                      device: int = 0) -> Solution:
    """The factored cubic system uploaded, expanded on the device and solved there (gf2bv_solve_cubic_terms): what solve_words
    returns for cubic_expand_words of the same arrays.  rows (default: max(len(lin), columns)) >= the columns."""
    return _solve_terms(3, (lin, off2, ta, tb, off3, ua, ub, uc), n_lin, rows, mode, device)


# -- quartic systems kept factored: the cubic functions above one arity up (gf2bv_hip.h, "quartic expansion") ------------------------------
def quartic_chunks(n_lin: int) -> tuple:
    """(quadratic, cubic, quartic) terms of a row that one pass of the quartic expansion kernel holds in LDS (gf2bv_quartic_chunks,
    host only); ValueError for an n_lin whose staged cubic rows do not fit the LDS"""
    q, c, v = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    _check(lib().gf2bv_quartic_chunks(n_lin, ctypes.byref(q), ctypes.byref(c), ctypes.byref(v)))
    return q.value, c.value, v.value


def quartic_expand_words(lin, off2, ta, tb, off3, ua, ub, uc, off4, va, vb, vc, vd, n_lin: int, rows: int | None = None,
                         stride_words: int | None = None, device: int = 0) -> np.ndarray:
    """Factored quartic equations (cubic_expand_words' rows ^ XOR of va[v] * vb[v] * vc[v] * vd[v], v in off4[r] .. off4[r + 1]; the
    products exact in GF(2)[x] / (x_i^2 + x_i)) expanded on the device into rows over the xl4_cols(n_lin) columns of the
    augmented-words layout: [rows, stride_words] uint64, rows beyond len(lin) zero (gf2bv_quartic_expand_words)."""
    return _expand_words(4, (lin, off2, ta, tb, off3, ua, ub, uc, off4, va, vb, vc, vd), n_lin, rows, stride_words, device)


def quartic_expand_device(d_lin: int, d_off2: int, d_ta: int, d_tb: int, d_off3: int, d_ua: int, d_ub: int, d_uc: int, d_off4: int, d_va: int,
                          d_vb: int, d_vc: int, d_vd: int, rows_live: int, rows: int, n_lin: int, d_aug: int, stride: int, device: int = 0,
                          stream: int = 0) -> None:
    """quartic_expand_words with everything resident in device memory: the kernel is enqueued on `stream` and the call returns; a
    solve_device on the same stream reads the finished rows."""
    _expand_device(4, (d_lin, d_off2, d_ta, d_tb, d_off3, d_ua, d_ub, d_uc, d_off4, d_va, d_vb, d_vc, d_vd), rows_live, rows, n_lin, d_aug,
                   stride, device, stream)


def solve_quartic_terms(lin, off2, ta, tb, off3, ua, ub, uc, off4, va, vb, vc, vd, n_lin: int, rows: int | None = None,
                        mode: int = MODE_SINGLE, device: int = 0) -> Solution:
    """The factored quartic system uploaded, expanded on the device and solved there (gf2bv_solve_quartic_terms): what solve_words
    returns for quartic_expand_words of the same arrays.  rows (default: max(len(lin), columns)) >= the columns."""
    return _solve_terms(4, (lin, off2, ta, tb, off3, ua, ub, uc, off4, va, vb, vc, vd), n_lin, rows, mode, device)


# The xl3_* and xl4_* functions below are one body each, taking the degree (3: multipliers 1 and x_k, n + 1 rows an equation; 4: also
# x_a x_b, 1 + n + C(n,2) rows an equation -- gf2bv_hip.h, "degree-4 XL")
def _xl_cols(degree: int, n_lin: int) -> int:
    return xl4_cols(n_lin) if degree == 4 else xl3_cols(n_lin)


def _xl_rows_per_eq(degree: int, n_lin: int) -> int:
    return 1 + quad_cols(n_lin) if degree == 4 else n_lin + 1


def _xl_fn(degree: int, name: str):
    return getattr(lib(), name.format(degree))


def _quad_rows(quad) -> np.ndarray:
    """quadratic rows of the augmented-words layout (what quad_expand_words returns) as a contiguous [m, stride] array"""
    quad = np.ascontiguousarray(quad, dtype=np.uint64)
    if quad.ndim != 2:
        raise ValueError("the quadratic rows must be a 2-D uint64 array, one row per equation")
    return quad


def _xl_expand_words(degree: int, quad, n_lin: int, rows: int | None = None, stride_words: int | None = None, device: int = 0) -> np.ndarray:
    """XL on the device (gf2bv_xl3_expand_words / gf2bv_xl4_expand_words): `quad` holds m quadratic rows as quad_expand_words returns
    them; the result is [rows, stride_words] uint64 over xl3_cols(n_lin) / xl4_cols(n_lin) columns.  Degree 3: rows e(n+1) .. e(n+1) + n
    equation e and its product with every unknown; degree 4: the 1 + n + C(n,2) rows from e(1 + n + C(n,2)), the products with every
    pair of unknowns behind those.  Rows beyond the live ones zero."""
    quad = _quad_rows(quad)
    m = len(quad)
    rows = m * _xl_rows_per_eq(degree, n_lin) if rows is None else rows
    stride = (_xl_cols(degree, n_lin) + 1 + 63) // 64 if stride_words is None else stride_words
    out = np.empty((max(rows, 0), max(stride, 0)), dtype=np.uint64)
    _check(_xl_fn(degree, "gf2bv_xl{}_expand_words")(quad.ctypes.data, m, quad.shape[1], n_lin, rows, out.ctypes.data, stride, device))
    return out


def _xl_expand_device(degree: int, d_quad: int, m: int, quad_stride: int, n_lin: int, rows: int, d_aug: int, stride: int, device: int = 0,
                      stream: int = 0) -> None:
    """xl3_expand_words with everything resident in device memory: the kernel is enqueued on `stream` and the call returns; a
    solve_device / factor_device on the same stream reads the finished rows."""
    _check(_xl_fn(degree, "gf2bv_xl{}_expand_device")(d_quad, m, quad_stride, n_lin, rows, d_aug, stride, device, stream or None))


def _solve_xl_words(degree: int, quad, n_lin: int, mode: int = MODE_SINGLE, device: int = 0) -> Solution:
    """Quadratic rows uploaded, multiplied on the device and solved there (gf2bv_solve_xl3_words / gf2bv_solve_xl4_words): what
    solve_words returns for the expansion of the same rows padded with zero rows up to the columns of that degree."""
    quad = _quad_rows(quad)
    h = ctypes.c_void_p()
    _check(_xl_fn(degree, "gf2bv_solve_xl{}_words")(quad.ctypes.data, len(quad), quad.shape[1], n_lin, mode, device, ctypes.byref(h)))
    return _take(h, mode)


def _solve_xl_quad_terms(degree: int, lin, term_off, ta, tb, n_lin: int, mode: int = MODE_SINGLE, device: int = 0) -> Solution:
    """The factored system uploaded, expanded, multiplied and solved on the device (gf2bv_solve_xl3_quad_terms / _xl4_): what
    solve_xl3_words / solve_xl4_words returns for quad_expand_words of the same arrays."""
    lin, term_off, ta, tb = _terms(n_lin, lin, term_off, ta, tb)
    h = ctypes.c_void_p()
    _check(_xl_fn(degree, "gf2bv_solve_xl{}_quad_terms")(*_ptrs(lin, term_off, ta, tb), len(lin), n_lin, mode, device, ctypes.byref(h)))
    return _take(h, mode)


# -- hybrid XL: guessed unknowns, every assignment's system in one batch (gf2bv_hip.h, "hybrid XL") ---------------------------------------
def _guess(guess) -> np.ndarray:
    return np.ascontiguousarray(guess, dtype=np.int32).reshape(-1)


def _assignments(guess: np.ndarray, a0: int, na: int | None) -> int:
    return max((1 << len(guess)) - a0, 0) if na is None else na


def quad_specialise_words(quad, n_lin: int, guess, a0: int = 0, na: int | None = None, stride_words: int | None = None,
                          device: int = 0) -> np.ndarray:
    """The guessed unknowns substituted into m quadratic rows on the device (gf2bv_quad_specialise_words): [na, m, stride_words]
    uint64, element s the rows of assignment a0 + s (bit t of it is the value of unknown guess[t]) over the n_lin - len(guess)
    remaining unknowns.  na defaults to every assignment from a0 on."""
    quad, guess = _quad_rows(quad), _guess(guess)
    na = _assignments(guess, a0, na)
    stride = (quad_cols(n_lin - len(guess)) + 1 + 63) // 64 if stride_words is None else stride_words
    out = np.empty((max(na, 0), len(quad), max(stride, 0)), dtype=np.uint64)
    _check(lib().gf2bv_quad_specialise_words(quad.ctypes.data, len(quad), quad.shape[1], n_lin, guess.ctypes.data, len(guess), a0, na,
                                             out.ctypes.data, stride, device))
    return out


def quad_specialise_device(d_quad: int, m: int, quad_stride: int, n_lin: int, guess, a0: int, na: int, d_out: int, out_stride: int,
                           sys_stride: int, device: int = 0, stream: int = 0) -> None:
    """quad_specialise_words with the rows resident in device memory (the guess stays a host array): system s at
    d_out + s * sys_stride words; the kernel is enqueued on `stream` and the call returns."""
    guess = _guess(guess)
    _check(lib().gf2bv_quad_specialise_device(d_quad, m, quad_stride, n_lin, guess.ctypes.data, len(guess), a0, na, d_out, out_stride,
                                              sys_stride, device, stream or None))


def _xl_expand_batch_words(degree: int, quads, n_lin: int, rows: int | None = None, stride_words: int | None = None, sys_stride_words: int | None = None,
                           device: int = 0) -> np.ndarray:
    """The degree-3 XL expansion of nsys systems in one launch (gf2bv_xl3_expand_batch_words): `quads` is [nsys, m, quad_stride]
    uint64; the result is [nsys, sys_stride_words] uint64, system s its `rows` rows stride_words apart from word 0 of element s
    (what xl3_expand_words gives for quads[s]) and the words behind them as numpy left them."""
    quads = np.ascontiguousarray(quads, dtype=np.uint64)
    if quads.ndim != 3:
        raise ValueError("the systems must be a 3-D uint64 array: system, equation, word")
    nsys, m, qs = quads.shape
    rows = m * _xl_rows_per_eq(degree, n_lin) if rows is None else rows
    stride = (_xl_cols(degree, n_lin) + 1 + 63) // 64 if stride_words is None else stride_words
    sys_stride = rows * stride if sys_stride_words is None else sys_stride_words
    out = np.zeros((nsys, max(sys_stride, 0)), dtype=np.uint64)
    _check(_xl_fn(degree, "gf2bv_xl{}_expand_batch_words")(quads.ctypes.data, nsys, m * qs, m, qs, n_lin, rows, out.ctypes.data, stride, sys_stride,
                                              device))
    return out


def _xl_expand_batch_device(degree: int, d_quad: int, nsys: int, quad_sys_stride: int, m: int, quad_stride: int, n_lin: int, rows: int, d_aug: int,
                            stride: int, sys_stride: int, device: int = 0, stream: int = 0) -> None:
    """xl3_expand_batch_words with everything resident in device memory: enqueued on `stream`, the call returns; a
    solve_batch_device with the same stream reads the finished systems."""
    _check(_xl_fn(degree, "gf2bv_xl{}_expand_batch_device")(d_quad, nsys, quad_sys_stride, m, quad_stride, n_lin, rows, d_aug, stride, sys_stride,
                                               device, stream or None))


def _solve_xl_guess_words(degree: int, quad, n_lin: int, guess, a0: int = 0, na: int | None = None, mode: int = MODE_SINGLE, device: int = 0) -> list:
    """Hybrid XL (gf2bv_solve_xl3_guess_words): the quadratic rows uploaded, specialised for the assignments a0 .. a0 + na - 1 of the
    guessed unknowns, every assignment's rows multiplied and all systems solved as lock-step gangs.  Element s is what
    solve_xl3_words returns for quad_specialise_words(...)[s] over n_lin - len(guess) unknowns."""
    quad, guess = _quad_rows(quad), _guess(guess)
    na = _assignments(guess, a0, na)
    hs = _handles(na)
    rc = _xl_fn(degree, "gf2bv_solve_xl{}_guess_words")(quad.ctypes.data, len(quad), quad.shape[1], n_lin, guess.ctypes.data, len(guess), a0, na,
                                           mode, device, hs)
    return _take_all(hs, max(na, 0), rc, mode)


def _solve_xl_guess_quad_terms(degree: int, lin, term_off, ta, tb, n_lin: int, guess, a0: int = 0, na: int | None = None, mode: int = MODE_SINGLE,
                               device: int = 0) -> list:
    """solve_xl3_guess_words on a factored system: expanded on the device first (gf2bv_solve_xl3_guess_quad_terms)."""
    lin, term_off, ta, tb = _terms(n_lin, lin, term_off, ta, tb)
    guess = _guess(guess)
    na = _assignments(guess, a0, na)
    hs = _handles(na)
    rc = _xl_fn(degree, "gf2bv_solve_xl{}_guess_quad_terms")(*_ptrs(lin, term_off, ta, tb), len(lin), n_lin, guess.ctypes.data, len(guess), a0, na,
                                                mode, device, hs)
    return _take_all(hs, max(na, 0), rc, mode)


def _xl_guess_chunk(degree: int, m: int, n_lin: int, nguess: int, free_bytes: int | None = None, device: int = 0) -> int:
    """How many assignments one solve_xl3_guess_* call should take: the largest count (at most 2^nguess) whose specialised rows and
    expansions fit a quarter of free_bytes; 0 when one system does not fit.  free_bytes None: the free memory of `device`
    (gf2bv_xl3_guess_chunk_device); given: a pure function, no device is touched (gf2bv_xl3_guess_chunk)."""
    if free_bytes is None:
        chunk = ctypes.c_int64()
        _check(_xl_fn(degree, "gf2bv_xl{}_guess_chunk_device")(m, n_lin, nguess, device, ctypes.byref(chunk)))
        return int(chunk.value)
    chunk = int(_xl_fn(degree, "gf2bv_xl{}_guess_chunk")(m, n_lin, nguess, free_bytes))
    if chunk < 0:
        raise ValueError("m, n_lin, nguess or free_bytes out of range")
    return chunk


# -- the public names: each body above for degree 3 and for degree 4 ---------------------------------------------------------------------
def xl3_expand_words(quad, n_lin: int, rows: int | None = None, stride_words: int | None = None, device: int = 0) -> np.ndarray:
    """_xl_expand_words for degree 3"""
    return _xl_expand_words(3, quad, n_lin, rows, stride_words, device)


def xl4_expand_words(quad, n_lin: int, rows: int | None = None, stride_words: int | None = None, device: int = 0) -> np.ndarray:
    """_xl_expand_words for degree 4"""
    return _xl_expand_words(4, quad, n_lin, rows, stride_words, device)


def xl3_expand_device(d_quad: int, m: int, quad_stride: int, n_lin: int, rows: int, d_aug: int, stride: int, device: int = 0, stream: int = 0) -> None:
    """_xl_expand_device for degree 3"""
    return _xl_expand_device(3, d_quad, m, quad_stride, n_lin, rows, d_aug, stride, device, stream)


def xl4_expand_device(d_quad: int, m: int, quad_stride: int, n_lin: int, rows: int, d_aug: int, stride: int, device: int = 0, stream: int = 0) -> None:
    """_xl_expand_device for degree 4"""
    return _xl_expand_device(4, d_quad, m, quad_stride, n_lin, rows, d_aug, stride, device, stream)


def solve_xl3_words(quad, n_lin: int, mode: int = MODE_SINGLE, device: int = 0) -> Solution:
    """_solve_xl_words for degree 3"""
    return _solve_xl_words(3, quad, n_lin, mode, device)


def solve_xl4_words(quad, n_lin: int, mode: int = MODE_SINGLE, device: int = 0) -> Solution:
    """_solve_xl_words for degree 4"""
    return _solve_xl_words(4, quad, n_lin, mode, device)


def solve_xl3_quad_terms(lin, term_off, ta, tb, n_lin: int, mode: int = MODE_SINGLE, device: int = 0) -> Solution:
    """_solve_xl_quad_terms for degree 3"""
    return _solve_xl_quad_terms(3, lin, term_off, ta, tb, n_lin, mode, device)


def solve_xl4_quad_terms(lin, term_off, ta, tb, n_lin: int, mode: int = MODE_SINGLE, device: int = 0) -> Solution:
    """_solve_xl_quad_terms for degree 4"""
    return _solve_xl_quad_terms(4, lin, term_off, ta, tb, n_lin, mode, device)


def xl3_expand_batch_words(quads, n_lin: int, rows: int | None = None, stride_words: int | None = None, sys_stride_words: int | None = None, device: int = 0) -> np.ndarray:
    """_xl_expand_batch_words for degree 3"""
    return _xl_expand_batch_words(3, quads, n_lin, rows, stride_words, sys_stride_words, device)


def xl4_expand_batch_words(quads, n_lin: int, rows: int | None = None, stride_words: int | None = None, sys_stride_words: int | None = None, device: int = 0) -> np.ndarray:
    """_xl_expand_batch_words for degree 4"""
    return _xl_expand_batch_words(4, quads, n_lin, rows, stride_words, sys_stride_words, device)


def xl3_expand_batch_device(d_quad: int, nsys: int, quad_sys_stride: int, m: int, quad_stride: int, n_lin: int, rows: int, d_aug: int, stride: int, sys_stride: int, device: int = 0, stream: int = 0) -> None:
    """_xl_expand_batch_device for degree 3"""
    return _xl_expand_batch_device(3, d_quad, nsys, quad_sys_stride, m, quad_stride, n_lin, rows, d_aug, stride, sys_stride, device, stream)


def xl4_expand_batch_device(d_quad: int, nsys: int, quad_sys_stride: int, m: int, quad_stride: int, n_lin: int, rows: int, d_aug: int, stride: int, sys_stride: int, device: int = 0, stream: int = 0) -> None:
    """_xl_expand_batch_device for degree 4"""
    return _xl_expand_batch_device(4, d_quad, nsys, quad_sys_stride, m, quad_stride, n_lin, rows, d_aug, stride, sys_stride, device, stream)


def solve_xl3_guess_words(quad, n_lin: int, guess, a0: int = 0, na: int | None = None, mode: int = MODE_SINGLE, device: int = 0) -> list:
    """_solve_xl_guess_words for degree 3"""
    return _solve_xl_guess_words(3, quad, n_lin, guess, a0, na, mode, device)


def solve_xl4_guess_words(quad, n_lin: int, guess, a0: int = 0, na: int | None = None, mode: int = MODE_SINGLE, device: int = 0) -> list:
    """_solve_xl_guess_words for degree 4"""
    return _solve_xl_guess_words(4, quad, n_lin, guess, a0, na, mode, device)


def solve_xl3_guess_quad_terms(lin, term_off, ta, tb, n_lin: int, guess, a0: int = 0, na: int | None = None, mode: int = MODE_SINGLE, device: int = 0) -> list:
    """_solve_xl_guess_quad_terms for degree 3"""
    return _solve_xl_guess_quad_terms(3, lin, term_off, ta, tb, n_lin, guess, a0, na, mode, device)


def solve_xl4_guess_quad_terms(lin, term_off, ta, tb, n_lin: int, guess, a0: int = 0, na: int | None = None, mode: int = MODE_SINGLE, device: int = 0) -> list:
    """_solve_xl_guess_quad_terms for degree 4"""
    return _solve_xl_guess_quad_terms(4, lin, term_off, ta, tb, n_lin, guess, a0, na, mode, device)


def xl3_guess_chunk(m: int, n_lin: int, nguess: int, free_bytes: int | None = None, device: int = 0) -> int:
    """_xl_guess_chunk for degree 3"""
    return _xl_guess_chunk(3, m, n_lin, nguess, free_bytes, device)


def xl4_guess_chunk(m: int, n_lin: int, nguess: int, free_bytes: int | None = None, device: int = 0) -> int:
    """_xl_guess_chunk for degree 4"""
    return _xl_guess_chunk(4, m, n_lin, nguess, free_bytes, device)


# -- degree-4 XL on cubic rows: multipliers 1 and x_k, n + 1 rows an equation (gf2bv_hip.h, "degree-4 XL on cubic equations") ------------
def _cubic_rows(cubic) -> np.ndarray:
    """cubic rows of the augmented-words layout (what cubic_expand_words returns) as a contiguous [m, stride] array"""
    cubic = np.ascontiguousarray(cubic, dtype=np.uint64)
    if cubic.ndim != 2:
        raise ValueError("the cubic rows must be a 2-D uint64 array, one row per equation")
    return cubic


def xl4_cubic_expand_words(cubic, n_lin: int, rows: int | None = None, stride_words: int | None = None, device: int = 0) -> np.ndarray:
    """Degree-4 XL of cubic rows on the device (gf2bv_xl4_cubic_expand_words): `cubic` holds m rows as cubic_expand_words returns
    them; the result is [rows, stride_words] uint64 over xl4_cols(n_lin) columns, rows e(n+1) .. e(n+1) + n equation e and its product
    with every unknown, rows beyond m(n+1) zero."""
    cubic = _cubic_rows(cubic)
    m = len(cubic)
    rows = m * (n_lin + 1) if rows is None else rows
    stride = (xl4_cols(n_lin) + 1 + 63) // 64 if stride_words is None else stride_words
    out = np.empty((max(rows, 0), max(stride, 0)), dtype=np.uint64)
    _check(lib().gf2bv_xl4_cubic_expand_words(cubic.ctypes.data, m, cubic.shape[1], n_lin, rows, out.ctypes.data, stride, device))
    return out


def xl4_cubic_expand_device(d_cubic: int, m: int, cubic_stride: int, n_lin: int, rows: int, d_aug: int, stride: int, device: int = 0,
                            stream: int = 0) -> None:
    """xl4_cubic_expand_words with everything resident in device memory: the kernel is enqueued on `stream` and the call returns; a
    solve_device on the same stream reads the finished rows."""
    _check(lib().gf2bv_xl4_cubic_expand_device(d_cubic, m, cubic_stride, n_lin, rows, d_aug, stride, device, stream or None))


def solve_xl4_cubic_words(cubic, n_lin: int, mode: int = MODE_SINGLE, device: int = 0) -> Solution:
    """Cubic rows uploaded, multiplied on the device and solved there (gf2bv_solve_xl4_cubic_words): what solve_words returns for
    xl4_cubic_expand_words of the same rows padded with zero rows up to xl4_cols(n_lin)."""
    cubic = _cubic_rows(cubic)
    h = ctypes.c_void_p()
    _check(lib().gf2bv_solve_xl4_cubic_words(cubic.ctypes.data, len(cubic), cubic.shape[1], n_lin, mode, device, ctypes.byref(h)))
    return _take(h, mode)


def solve_xl4_cubic_terms(lin, off2, ta, tb, off3, ua, ub, uc, n_lin: int, mode: int = MODE_SINGLE, device: int = 0) -> Solution:
    """The factored cubic system uploaded, expanded, multiplied and solved on the device (gf2bv_solve_xl4_cubic_terms): what
    solve_xl4_cubic_words returns for cubic_expand_words of the same arrays."""
    terms = _terms(n_lin, lin, off2, ta, tb, off3, ua, ub, uc)
    h = ctypes.c_void_p()
    _check(lib().gf2bv_solve_xl4_cubic_terms(*_ptrs(*terms), len(terms[0]), n_lin, mode, device, ctypes.byref(h)))
    return _take(h, mode)


# -- hybrid degree-4 XL on cubic rows: the hybrid functions above one degree up (gf2bv_hip.h, "hybrid degree-4 XL on cubic equations") ----
def cubic_specialise_words(cubic, n_lin: int, guess, a0: int = 0, na: int | None = None, stride_words: int | None = None,
                           device: int = 0) -> np.ndarray:
    """The guessed unknowns substituted into m cubic rows on the device (gf2bv_cubic_specialise_words): [na, m, stride_words] uint64,
    element s the rows of assignment a0 + s (bit t of it is the value of unknown guess[t]) over the xl3_cols of the
    n_lin - len(guess) remaining unknowns.  na defaults to every assignment from a0 on."""
    cubic, guess = _cubic_rows(cubic), _guess(guess)
    na = _assignments(guess, a0, na)
    stride = (xl3_cols(n_lin - len(guess)) + 1 + 63) // 64 if stride_words is None else stride_words
    out = np.empty((max(na, 0), len(cubic), max(stride, 0)), dtype=np.uint64)
    _check(lib().gf2bv_cubic_specialise_words(cubic.ctypes.data, len(cubic), cubic.shape[1], n_lin, guess.ctypes.data, len(guess), a0, na,
                                              out.ctypes.data, stride, device))
    return out


def cubic_specialise_device(d_cubic: int, m: int, cubic_stride: int, n_lin: int, guess, a0: int, na: int, d_out: int, out_stride: int,
                            sys_stride: int, device: int = 0, stream: int = 0) -> None:
    """cubic_specialise_words with the rows resident in device memory (the guess stays a host array): system s at
    d_out + s * sys_stride words; the kernel is enqueued on `stream` and the call returns."""
    guess = _guess(guess)
    _check(lib().gf2bv_cubic_specialise_device(d_cubic, m, cubic_stride, n_lin, guess.ctypes.data, len(guess), a0, na, d_out, out_stride,
                                               sys_stride, device, stream or None))


def xl4_cubic_expand_batch_words(cubics, n_lin: int, rows: int | None = None, stride_words: int | None = None,
                                 sys_stride_words: int | None = None, device: int = 0) -> np.ndarray:
    """xl4_cubic_expand_words of nsys systems in one launch (gf2bv_xl4_cubic_expand_batch_words): `cubics` is [nsys, m, cubic_stride]
    uint64; the result is [nsys, sys_stride_words] uint64, system s its `rows` rows stride_words apart from word 0 of element s and
    the words behind them as numpy left them."""
    cubics = np.ascontiguousarray(cubics, dtype=np.uint64)
    if cubics.ndim != 3:
        raise ValueError("the systems must be a 3-D uint64 array: system, equation, word")
    nsys, m, cs = cubics.shape
    rows = m * (n_lin + 1) if rows is None else rows
    stride = (xl4_cols(n_lin) + 1 + 63) // 64 if stride_words is None else stride_words
    sys_stride = rows * stride if sys_stride_words is None else sys_stride_words
    out = np.zeros((nsys, max(sys_stride, 0)), dtype=np.uint64)
    _check(lib().gf2bv_xl4_cubic_expand_batch_words(cubics.ctypes.data, nsys, m * cs, m, cs, n_lin, rows, out.ctypes.data, stride, sys_stride,
                                                    device))
    return out


def xl4_cubic_expand_batch_device(d_cubic: int, nsys: int, cubic_sys_stride: int, m: int, cubic_stride: int, n_lin: int, rows: int, d_aug: int,
                                  stride: int, sys_stride: int, device: int = 0, stream: int = 0) -> None:
    """xl4_cubic_expand_batch_words with everything resident in device memory: enqueued on `stream`, the call returns; a
    solve_batch_device with the same stream reads the finished systems."""
    _check(lib().gf2bv_xl4_cubic_expand_batch_device(d_cubic, nsys, cubic_sys_stride, m, cubic_stride, n_lin, rows, d_aug, stride, sys_stride,
                                                     device, stream or None))


def solve_xl4_cubic_guess_words(cubic, n_lin: int, guess, a0: int = 0, na: int | None = None, mode: int = MODE_SINGLE, device: int = 0) -> list:
    """Hybrid degree-4 XL on cubic rows (gf2bv_solve_xl4_cubic_guess_words): the rows uploaded, specialised for the assignments
    a0 .. a0 + na - 1 of the guessed unknowns, every assignment's rows multiplied and all systems solved as lock-step gangs.  Element s
    is what solve_xl4_cubic_words returns for cubic_specialise_words(...)[s] over n_lin - len(guess) unknowns."""
    cubic, guess = _cubic_rows(cubic), _guess(guess)
    na = _assignments(guess, a0, na)
    hs = _handles(na)
    rc = lib().gf2bv_solve_xl4_cubic_guess_words(cubic.ctypes.data, len(cubic), cubic.shape[1], n_lin, guess.ctypes.data, len(guess), a0, na,
                                                 mode, device, hs)
    return _take_all(hs, max(na, 0), rc, mode)


def solve_xl4_cubic_guess_terms(lin, off2, ta, tb, off3, ua, ub, uc, n_lin: int, guess, a0: int = 0, na: int | None = None,
                                mode: int = MODE_SINGLE, device: int = 0) -> list:
    """solve_xl4_cubic_guess_words on a factored cubic system: expanded on the device first (gf2bv_solve_xl4_cubic_guess_terms)."""
    terms = _terms(n_lin, lin, off2, ta, tb, off3, ua, ub, uc)
    guess = _guess(guess)
    na = _assignments(guess, a0, na)
    hs = _handles(na)
    rc = lib().gf2bv_solve_xl4_cubic_guess_terms(*_ptrs(*terms), len(terms[0]), n_lin, guess.ctypes.data, len(guess), a0, na, mode, device, hs)
    return _take_all(hs, max(na, 0), rc, mode)


def xl4_cubic_guess_chunk(m: int, n_lin: int, nguess: int, free_bytes: int | None = None, device: int = 0) -> int:
    """xl4_guess_chunk for the systems of solve_xl4_cubic_guess_* (gf2bv_xl4_cubic_guess_chunk / _chunk_device)"""
    if free_bytes is None:
        chunk = ctypes.c_int64()
        _check(lib().gf2bv_xl4_cubic_guess_chunk_device(m, n_lin, nguess, device, ctypes.byref(chunk)))
        return int(chunk.value)
    chunk = int(lib().gf2bv_xl4_cubic_guess_chunk(m, n_lin, nguess, free_bytes))
    if chunk < 0:
        raise ValueError("m, n_lin, nguess or free_bytes out of range")
    return chunk


def synth_device(d_ptr: int, rows: int, cols: int, stride: int, seed: int, device: int = 0, stream: int = 0):
    _check(lib().gf2bv_synth_device(d_ptr, rows, cols, stride, seed, device, stream or None))


def _mix64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def planted_solution(cols: int, seed: int) -> np.ndarray:
    """The solution the synthetic generator plants (gf2bv_synth_device / k_synth: pseudo-row 0xFFFFF of the same counter-based
    generator, RHS = <row, planted>): ceil(cols / 64) words.  A full-rank system has no other solution -- what the bench's
    parity gate and the large-size tests compare solve_one with."""
    cw = (cols + 63) // 64
    s = _mix64(np.array([seed], dtype=np.uint64))[0]
    x = _mix64(s ^ (np.uint64(0xFFFFF << 20) | np.arange(cw, dtype=np.uint64)))
    if cols & 63:
        x[-1] &= np.uint64((1 << (cols & 63)) - 1)
    return x


def residual_device(d_ptr: int, rows: int, cols: int, stride: int, x: np.ndarray, device: int = 0,
                    stream: int = 0) -> int:
    x = np.ascontiguousarray(x, dtype=np.uint64)
    bad = ctypes.c_int64(-1)
    _check(lib().gf2bv_residual_device(d_ptr, rows, cols, stride, x.ctypes.data, device, stream or None,
                                       ctypes.byref(bad)))
    return int(bad.value)


def stream_ceiling(nbytes: int = 2 << 30, device: int = 0) -> dict:
    """Measured streaming rates of this GPU (GB/s): in-place read-XOR-write and read-only."""
    rmw, rd = ctypes.c_double(0), ctypes.c_double(0)
    _check(lib().gf2bv_stream_ceiling_device(device, nbytes, ctypes.byref(rmw), ctypes.byref(rd)))
    return {"rmw_gbs": rmw.value, "read_gbs": rd.value}


def lds_clock(device: int = 0) -> dict:
    """Shader clock (MHz) under an LDS-bound load and the LDS bytes per clock and CU that load reached."""
    mhz, bpc = ctypes.c_double(0), ctypes.c_double(0)
    _check(lib().gf2bv_lds_clock_device(device, ctypes.byref(mhz), ctypes.byref(bpc)))
    return {"shader_mhz": mhz.value, "lds_bytes_per_clk_cu": bpc.value}


def kernel_resources(device: int = 0) -> dict:
    """VGPRs per lane and static LDS bytes of the bulk-update kernel and of the panel kernels that run beside it."""
    out = (ctypes.c_int32 * 20)()
    _check(lib().gf2bv_kernel_resources(device, out, 20))
    names = ("update", "block_fast", "narrow_all", "prio_window", "panel_step")
    res = {nm: {"vgprs": int(out[2 * k]), "lds": int(out[2 * k + 1])} for k, nm in enumerate(names)}
    res["update_outer"] = {"vgprs": int(out[10]), "lds": int(out[11]), "scratch": int(out[12])}      # k_update16k (two-level)
    res["block_fast_narrow"] = {"vgprs": int(out[13]), "lds": int(out[14])}                          # search + narrow step in one launch
    res["block_sparse"] = {"vgprs": int(out[15]), "lds": int(out[16])}                               # k_block_sparse<256, 4> (round 5)
    return res


def pool_trim(device: int = 0) -> int:
    """Return every idle buffer of the library's pool on `device` to the device; bytes freed (gf2bv_pool_trim)."""
    return int(lib().gf2bv_pool_trim(device))


def knobs() -> dict:
    """The GF2BV_* environment switches as the library parses them now (gf2bv_knob_dump; DESIGN.md, "Environment switches"):
    name -> value as text, after defaults and clamps; "unset" where an unset variable leaves the choice to the solve.  No GPU needed."""
    buf = ctypes.create_string_buffer(4096)
    _check(lib().gf2bv_knob_dump(buf, len(buf)))
    return dict(line.split("=", 1) for line in buf.value.decode().splitlines())


def host_pool_trim() -> int:
    """Free the idle page-locked staging buffers (gf2bv_host_pool_trim); bytes released."""
    return int(lib().gf2bv_host_pool_trim())


def pool_idle_bytes(device: int = 0) -> int:
    """Bytes of idle buffers the pool keeps on `device` right now."""
    return int(lib().gf2bv_pool_idle_bytes(device))


def pool_in_use(device: int = 0) -> dict:
    """What the pool has handed out on `device` and not yet got back (gf2bv_pool_in_use): {"buffers", "streams", "events"}.
    Between calls these count only what kept handles own.  No GPU needed."""
    out = (ctypes.c_int64 * 3)()
    if lib().gf2bv_pool_in_use(device, out) != 0:
        raise ValueError("device must not be negative")
    return {"buffers": int(out[0]), "streams": int(out[1]), "events": int(out[2])}


class DeviceBuffer:
    """hipMalloc'd scratch for callers that do not bring torch (tests, plain ctypes users)."""

    def __init__(self, nbytes: int, device: int = 0):
        self.device, self.nbytes = device, nbytes
        p = ctypes.c_void_p()
        _check(lib().gf2bv_device_alloc(device, nbytes, ctypes.byref(p)))
        self.ptr = p.value

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        _check(lib().gf2bv_device_upload(self.device, self.ptr, arr.ctypes.data, arr.nbytes))

    def download(self, dtype=np.uint64) -> np.ndarray:
        out = np.zeros(self.nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        _check(lib().gf2bv_device_download(self.device, out.ctypes.data, self.ptr, self.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().gf2bv_device_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def padded_stride(cols: int, multiple: int = 32) -> int:
    """Row stride (in 64-bit words) for a device-resident system: cols+1 bits, 256-byte rows."""
    wt = (cols + 1 + 63) // 64
    return (wt + multiple - 1) // multiple * multiple
