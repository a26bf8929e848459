"""ctypes loader for the in-tree HIP engine (gffx_amd/lib/libgffx_hip.so, C-ABI include/gffx_hip.h).

The library is the product's only compute path: loading fails loudly when it has not been
built, and every compute call fails (GFFX_E_NO_DEVICE) when no MI355X is visible.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgffx_hip.so")

u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
vp = C.c_void_p

# every symbol include/gffx_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "gffx_hip_abi_version": (C.c_int, []),
    "gffx_hip_device_count": (C.c_int, []),
    "gffx_hip_warmup": (C.c_int, [C.c_int]),
    "gffx_hip_last_error": (C.c_char_p, []),
    "gffx_hip_index_create": (C.c_int, [C.c_uint32, u32p, u32p, u32p, u32p, C.c_int, C.POINTER(vp)]),
    "gffx_hip_index_destroy": (None, [vp]),
    "gffx_hip_index_n_chr": (C.c_uint32, [vp]),
    "gffx_hip_index_n_roots": (C.c_uint64, [vp]),
    "gffx_hip_index_device": (C.c_int, [vp]),
    "gffx_hip_index_sorted_fids": (u32p, [vp]),
    "gffx_hip_index_clone": (C.c_int, [vp, C.c_int, C.POINTER(vp)]),
    "gffx_hip_regions_create": (C.c_int, [C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(vp)]),
    "gffx_hip_regions_destroy": (None, [vp]),
    "gffx_hip_regions_staging": (vp, [vp, C.c_int]),
    "gffx_hip_regions_wait_staging": (C.c_int, [vp, C.c_int]),
    "gffx_hip_regions_append": (C.c_int, [vp, C.c_int, C.c_uint64]),
    "gffx_hip_regions_append_parts": (C.c_int, [vp, C.c_int, C.c_uint32, u64p, u64p]),
    "gffx_hip_regions_rows": (C.c_uint64, [vp]),
    "gffx_hip_batch_set_regions_store": (C.c_int, [vp, vp, C.c_int, C.c_uint64, C.c_uint64]),
    "gffx_hip_allgather_counts": (C.c_int, [C.c_int, C.POINTER(C.c_int), u64p, u64p]),
    "gffx_hip_lines_test_store": (C.c_int, [vp, vp, C.c_uint32, C.c_int, u8p]),
    "gffx_hip_batch_create": (C.c_int, [vp, C.c_uint64, C.POINTER(vp)]),
    "gffx_hip_batch_destroy": (None, [vp]),
    "gffx_hip_batch_set_regions_host": (C.c_int, [vp, u32p, C.c_uint64]),
    "gffx_hip_batch_set_regions_soa_host": (C.c_int, [vp, u32p, u32p, u32p, C.c_uint64]),
    "gffx_hip_batch_set_regions_device": (C.c_int, [vp, vp, vp, vp, C.c_uint64]),
    "gffx_hip_batch_run": (C.c_int, [vp, C.c_int, C.c_int, C.c_uint32, C.c_int]),
    "gffx_hip_batch_wait": (C.c_int, [vp]),
    "gffx_hip_batch_sync": (C.c_int, [vp]),
    "gffx_hip_batch_n_queries": (C.c_uint64, [vp]),
    "gffx_hip_batch_total_hits": (C.c_uint64, [vp]),
    "gffx_hip_batch_copy_counts": (C.c_int, [vp, u32p]),
    "gffx_hip_batch_copy_offsets": (C.c_int, [vp, u64p]),
    "gffx_hip_batch_copy_offsets32": (C.c_int, [vp, u32p]),
    "gffx_hip_batch_copy_segbase": (C.c_int, [vp, u64p]),
    "gffx_hip_batch_copy_query_records": (C.c_int, [vp, u32p, u32p, u64p]),
    "gffx_hip_batch_copy_fids": (C.c_int, [vp, u32p]),
    "gffx_hip_batch_copy_triples": (C.c_int, [vp, u32p]),
    "gffx_hip_batch_copy_root_bitmap": (C.c_int, [vp, u64p, C.c_uint64]),
    "gffx_hip_batch_device_counts": (vp, [vp]),
    "gffx_hip_batch_device_fids": (vp, [vp]),
    "gffx_hip_batch_device_triples": (vp, [vp]),
    "gffx_hip_batch_device_regions": (vp, [vp]),
    "gffx_hip_batch_device_offsets": (vp, [vp]),
    "gffx_hip_batch_device_offsets32": (vp, [vp]),
    "gffx_hip_batch_device_segbase": (vp, [vp]),
    "gffx_hip_batch_reserve_hits": (C.c_int, [vp, C.c_uint64]),
    "gffx_hip_batch_kept_pairs_accumulated": (C.c_int, [vp, u64p]),
    "gffx_hip_batch_set_option": (C.c_int, [vp, C.c_char_p, C.c_long]),
    "gffx_hip_batch_options": (C.c_int, [vp, C.c_char_p, C.c_size_t]),
    "gffx_hip_index_options": (C.c_int, [vp, C.c_char_p, C.c_size_t]),
    "gffx_hip_batch_set_profiling": (C.c_int, [vp, C.c_int]),
    "gffx_hip_batch_kernel_ms": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double), u64p]),
    "gffx_hip_batch_reset_profile": (C.c_int, [vp]),
    "gffx_hip_batch_block_threads": (C.c_uint32, [vp]),
    "gffx_hip_batch_block_count": (C.c_uint32, [vp]),
    "gffx_hip_batch_block_share": (C.c_uint32, [vp]),
    "gffx_hip_group_descriptors_fit": (C.c_int, [C.c_uint64, C.c_uint64, C.c_int]),
    "gffx_hip_batch_filter_level": (C.c_uint32, [vp]),
    "gffx_hip_batch_wide_form": (C.c_int, [vp]),
    "gffx_hip_batches_run_n": (C.c_int, [C.POINTER(vp), C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_uint64]),
    "gffx_hip_batches_plan": (C.c_int, [C.POINTER(vp), C.c_uint32, u32p, u32p, u32p]),
    "gffx_hip_batches_timed_runs": (C.c_int, [C.POINTER(vp), C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_uint32,
                                    C.POINTER(C.c_double), u32p]),
    "gffx_hip_batch_timed_runs": (C.c_int, [vp, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(C.c_double)]),
    "gffx_hip_query_features": (C.c_int, [vp, u32p, C.c_uint64, C.c_int, C.c_int, C.POINTER(u32p), u64p]),
    "gffx_hip_free_host": (None, [vp]),
    "gffx_hip_lines_create": (C.c_int, [C.c_int, C.c_uint64, u32p, u32p, u32p, C.POINTER(vp)]),
    "gffx_hip_lines_destroy": (None, [vp]),
    "gffx_hip_lines_test": (C.c_int, [vp, u32p, C.c_uint64, C.c_uint32, C.c_int, u8p]),
    "gffx_hip_lines_test_device": (C.c_int, [vp, vp, C.c_uint64, C.c_uint32, C.c_int, u8p]),
    "gffx_hip_lines_last_kernel_ms": (C.c_double, [vp]),
    "gffx_hip_lines_last_prep_ms": (C.c_double, [vp]),
    "gffx_hip_lines_last_sort_passes": (C.c_int, [vp]),
    "gffx_hip_lines_copy_tables": (C.c_int, [vp, u64p, u32p, u32p, u32p, u32p]),
    "gffx_hip_lines_copy_dirs": (C.c_int, [vp, u64p, u32p, u32p]),
    "gffx_hip_lines_copy_degenerate": (C.c_int, [vp, u64p, u64p, u32p]),
    "gffx_hip_segments_covered": (C.c_int, [C.c_int, C.c_uint64, u32p, u32p, u32p, u32p, C.c_uint64, C.c_uint32, u32p]),
    "gffx_hip_union_create": (C.c_int, [C.c_int, C.c_uint32, C.POINTER(vp)]),
    "gffx_hip_union_add_host": (C.c_int, [vp, u32p, C.c_uint64]),
    "gffx_hip_union_add_store": (C.c_int, [vp, vp, C.c_int, C.c_uint64, C.c_uint64]),
    "gffx_hip_union_add_spans": (C.c_int, [vp, u64p, u32p, u32p]),
    "gffx_hip_union_finish": (C.c_int, [vp]),
    "gffx_hip_union_n_spans": (C.c_uint64, [vp]),
    "gffx_hip_union_copy_spans": (C.c_int, [vp, u64p, u32p, u32p, u64p]),
    "gffx_hip_union_segments_covered": (C.c_int, [vp, C.c_uint64, u32p, u32p, u32p, u32p]),
    "gffx_hip_union_stats": (C.c_int, [vp, C.POINTER(C.c_double), u64p, u64p]),
    "gffx_hip_union_destroy": (None, [vp]),
    "gffx_hip_pileup_create": (C.c_int, [C.c_int, C.c_uint32, C.c_uint64, u32p, u32p, u32p, C.POINTER(vp)]),
    "gffx_hip_pileup_add_host": (C.c_int, [vp, u32p, C.c_uint64]),
    "gffx_hip_pileup_add_store": (C.c_int, [vp, vp, C.c_int, C.c_uint64, C.c_uint64]),
    "gffx_hip_pileup_copy": (C.c_int, [vp, u64p]),
    "gffx_hip_pileup_reset": (C.c_int, [vp]),
    "gffx_hip_pileup_stats": (C.c_int, [vp, C.POINTER(C.c_double), u64p, u64p]),
    "gffx_hip_pileup_stage_ms": (C.c_int, [vp] + [C.POINTER(C.c_double)] * 4),
    "gffx_hip_pileup_fold_rows": (C.c_uint64, []),
    "gffx_hip_pileup_scan_tile": (C.c_uint32, []),
    "gffx_hip_pileup_destroy": (None, [vp]),
    "gffx_hip_pileup_meta_set": (C.c_int, [vp, C.c_uint64, u32p, u32p, u32p, u8p, u32p, vp, C.c_int]),
    "gffx_hip_pileup_meta_copy": (C.c_int, [vp, u64p, u64p, u64p, u64p]),
    "gffx_hip_pileup_meta_ms": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "gffx_hip_pileup_meta_columns": (C.c_uint64, [vp]),
    "gffx_hip_pileup_meta_max_columns": (C.c_uint32, []),
    "gffx_hip_pileup_meta_tile": (C.c_uint32, []),
    "gffx_hip_closest_create": (C.c_int, [vp, C.c_uint64, C.POINTER(vp)]),
    "gffx_hip_closest_run_host": (C.c_int, [vp, u32p, C.c_uint64, C.c_uint32]),
    "gffx_hip_closest_run_store": (C.c_int, [vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32]),
    "gffx_hip_closest_wait": (C.c_int, [vp]),
    "gffx_hip_closest_total_pairs": (C.c_int, [vp, u64p]),
    "gffx_hip_closest_copy_counts": (C.c_int, [vp, u32p]),
    "gffx_hip_closest_copy_offsets": (C.c_int, [vp, u64p]),
    "gffx_hip_closest_copy_triples": (C.c_int, [vp, u32p]),
    "gffx_hip_closest_copy_gaps": (C.c_int, [vp, u32p]),
    "gffx_hip_closest_copy_end_table": (C.c_int, [vp, u32p, u32p]),
    "gffx_hip_closest_last_kernel_ms": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "gffx_hip_closest_last_grid": (C.c_int, [vp, u32p, u64p]),
    "gffx_hip_closest_stats": (C.c_int, [vp, C.POINTER(C.c_double), u64p]),
    "gffx_hip_closest_destroy": (None, [vp]),
    "gffx_hip_classmap_create": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(vp)]),
    "gffx_hip_classmap_add_rows_host": (C.c_int, [vp, u32p, C.c_uint64]),
    "gffx_hip_classmap_finish": (C.c_int, [vp]),
    "gffx_hip_classmap_n_points": (C.c_uint64, [vp]),
    "gffx_hip_classmap_copy_points": (C.c_int, [vp, u64p, u32p, C.POINTER(C.c_uint8)]),
    "gffx_hip_classmap_copy_bases": (C.c_int, [vp, u64p]),
    "gffx_hip_classmap_run_host": (C.c_int, [vp, u32p, C.c_uint64]),
    "gffx_hip_classmap_run_store": (C.c_int, [vp, vp, C.c_int, C.c_uint64, C.c_uint64]),
    "gffx_hip_classmap_wait": (C.c_int, [vp]),
    "gffx_hip_classmap_copy_counts": (C.c_int, [vp, u32p]),
    "gffx_hip_classmap_copy_class": (C.c_int, [vp, C.POINTER(C.c_uint8)]),
    "gffx_hip_classmap_last_kernel_ms": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "gffx_hip_classmap_stage_ms": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "gffx_hip_classmap_scan_tile": (C.c_uint32, []),
    "gffx_hip_classmap_carry_tiles": (C.c_uint32, []),
    "gffx_hip_classmap_block_size": (C.c_uint32, []),
    "gffx_hip_classmap_destroy": (None, [vp]),
    "gffx_hip_classmap_perm_begin": (C.c_int, [vp, u32p, C.c_uint32, C.c_uint64]),
    "gffx_hip_classmap_perm_run_host": (C.c_int, [vp, u32p, C.c_uint64, C.c_uint64]),
    "gffx_hip_classmap_perm_run_store": (C.c_int, [vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64]),
    "gffx_hip_classmap_perm_wait": (C.c_int, [vp]),
    "gffx_hip_classmap_perm_copy_totals": (C.c_int, [vp, u64p, u64p, u64p]),
    "gffx_hip_classmap_perm_last_kernel_ms": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "gffx_hip_classmap_perm_group": (C.c_uint32, []),
    "gffx_hip_profile_create": (C.c_int, [C.c_int, C.c_uint32, C.POINTER(vp)]),
    "gffx_hip_profile_add_host": (C.c_int, [vp, u32p, C.c_uint64]),
    "gffx_hip_profile_add_store": (C.c_int, [vp, vp, C.c_int, C.c_uint64, C.c_uint64]),
    "gffx_hip_profile_add_points": (C.c_int, [vp, u64p, u32p, u32p]),
    "gffx_hip_profile_finish": (C.c_int, [vp]),
    "gffx_hip_profile_n_points": (C.c_uint64, [vp]),
    "gffx_hip_profile_copy_points": (C.c_int, [vp, u64p, u32p, u32p]),
    "gffx_hip_profile_union_at_least": (C.c_int, [vp, C.c_uint32, C.POINTER(vp)]),
    "gffx_hip_profile_reset": (C.c_int, [vp]),
    "gffx_hip_profile_stats": (C.c_int, [vp, C.POINTER(C.c_double), u64p, u64p]),
    "gffx_hip_profile_stage_ms": (C.c_int, [vp] + [C.POINTER(C.c_double)] * 4),
    "gffx_hip_profile_fold_rows": (C.c_uint64, []),
    "gffx_hip_profile_scan_tile": (C.c_uint32, []),
    "gffx_hip_profile_destroy": (None, [vp]),
    "gffx_hip_depth_create": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, u64p, u32p, u32p, u32p, C.c_uint32, u32p,
                                        C.POINTER(vp)]),
    "gffx_hip_depth_destroy": (None, [vp]),
    "gffx_hip_depth_accumulate": (C.c_int, [vp, vp]),
    "gffx_hip_depth_reset": (C.c_int, [vp]),
    "gffx_hip_depth_copy": (C.c_int, [vp, u64p, u32p, u32p]),
    "gffx_hip_bgzf_inflate": (C.c_int, [C.c_int, u8p, C.c_uint64, u8p, C.c_uint64, u64p]),
    "gffx_hip_bam_create": (C.c_int, [C.c_int, C.c_uint32, u32p, C.c_uint64, C.c_uint64, C.POINTER(vp)]),
    "gffx_hip_bam_feed": (C.c_int, [vp, u8p, C.c_uint64]),
    "gffx_hip_bam_finish": (C.c_int, [vp]),
    "gffx_hip_bam_rows": (C.c_uint64, [vp]),
    "gffx_hip_bam_counts": (C.c_int, [vp, u64p, u64p, u64p, u64p]),
    "gffx_hip_bam_stage_ms": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "gffx_hip_bam_copy_rows": (C.c_int, [vp, u32p]),
    "gffx_hip_bam_destroy": (None, [vp]),
    "gffx_hip_sam_create": (C.c_int, [C.c_int, C.c_uint32, C.c_char_p, u64p, u32p, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(vp)]),
    "gffx_hip_sam_feed": (C.c_int, [vp, u8p, C.c_uint64]),
    "gffx_hip_sam_finish": (C.c_int, [vp]),
    "gffx_hip_sam_rows": (C.c_uint64, [vp]),
    "gffx_hip_sam_counts": (C.c_int, [vp, u64p, u64p, u64p, u64p]),
    "gffx_hip_sam_stage_ms": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "gffx_hip_sam_copy_rows": (C.c_int, [vp, u32p]),
    "gffx_hip_sam_destroy": (None, [vp]),
    "gffx_hip_bed_create": (C.c_int, [C.c_int, C.c_uint32, C.c_char_p, u64p, C.c_int, C.c_uint64, C.c_int, C.POINTER(vp)]),
    "gffx_hip_bed_feed": (C.c_int, [vp, u8p, C.c_uint64]),
    "gffx_hip_bed_finish": (C.c_int, [vp]),
    "gffx_hip_bed_rows": (C.c_uint64, [vp]),
    "gffx_hip_bed_counts": (C.c_int, [vp, u64p, u64p, u64p, u64p]),
    "gffx_hip_bed_stage_ms": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "gffx_hip_bed_copy_rows": (C.c_int, [vp, u32p]),
    "gffx_hip_bed_destroy": (None, [vp]),
    "gffx_hip_ids_create": (C.c_int, [C.c_int, C.c_uint64, u8p, u64p, C.c_uint64, u32p, C.c_int, C.POINTER(vp)]),
    "gffx_hip_ids_destroy": (None, [vp]),
    "gffx_hip_ids_n": (C.c_uint64, [vp]),
    "gffx_hip_ids_options": (C.c_int, [vp, C.c_char_p, C.c_size_t]),
    "gffx_hip_ids_resolve": (C.c_int, [vp, C.c_uint64, u8p, u64p, u32p, u32p]),
    "gffx_hip_ids_reset": (C.c_int, [vp]),
    "gffx_hip_ids_copy_root_bitmap": (C.c_int, [vp, u64p, C.c_uint64]),
    "gffx_hip_ids_copy_requested_bitmap": (C.c_int, [vp, u64p, C.c_uint64]),
    "gffx_hip_ids_filter_lines": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint64, u64p, u32p, C.c_int, C.c_uint32, u8p, u32p, u8p]),
    "gffx_hip_ids_stage_ms": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "gffx_hip_attrs_create": (C.c_int, [C.c_int, C.c_uint64, u8p, u64p, C.c_uint64, u32p, C.c_uint64, u32p, u8p, C.c_uint32, C.c_int, C.c_int,
                                        C.POINTER(vp)]),
    "gffx_hip_attrs_destroy": (None, [vp]),
    "gffx_hip_attrs_n": (C.c_uint64, [vp]),
    "gffx_hip_attrs_options": (C.c_int, [vp, C.c_char_p, C.c_size_t]),
    "gffx_hip_attrs_match_exact": (C.c_int, [vp, C.c_uint64, u8p, u64p]),
    "gffx_hip_attrs_match_dfa": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, u8p, C.POINTER(C.c_uint16)]),
    "gffx_hip_attrs_dfa_kernel": (C.c_char_p, [vp]),
    "gffx_hip_attrs_reset": (C.c_int, [vp]),
    "gffx_hip_attrs_resolve": (C.c_int, [vp]),
    "gffx_hip_attrs_copy_matched_bitmap": (C.c_int, [vp, u64p, C.c_uint64]),
    "gffx_hip_attrs_copy_fid_bitmap": (C.c_int, [vp, u64p, C.c_uint64]),
    "gffx_hip_attrs_copy_root_bitmap": (C.c_int, [vp, u64p, C.c_uint64]),
    "gffx_hip_attrs_copy_invalid_bitmap": (C.c_int, [vp, u64p, C.c_uint64]),
    "gffx_hip_attrs_filter_lines": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint64, u64p, u32p, C.c_int, C.c_uint32, u8p, u32p, u8p]),
    "gffx_hip_attrs_stage_ms": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "gffx_hip_gff_create": (C.c_int, [C.c_int, C.c_char_p, C.c_uint32, C.c_char_p, u32p, C.c_uint64, C.c_int, C.POINTER(vp)]),
    "gffx_hip_gff_feed": (C.c_int, [vp, u8p, C.c_uint64]),
    "gffx_hip_gff_finish": (C.c_int, [vp]),
    "gffx_hip_gff_error": (C.c_int, [vp, u64p, C.POINTER(C.c_int)]),
    "gffx_hip_gff_counts": (C.c_int, [vp] + [u64p] * 8),
    "gffx_hip_gff_stage_ms": (C.c_int, [vp] + [C.POINTER(C.c_double)] * 5),
    "gffx_hip_gff_n_rows": (C.c_uint64, [vp]),
    "gffx_hip_gff_n_roots": (C.c_uint64, [vp]),
    "gffx_hip_gff_fts_bytes": (C.c_uint64, [vp]),
    "gffx_hip_gff_atn_bytes": (C.c_uint64, [vp]),
    "gffx_hip_gff_seqids_bytes": (C.c_uint64, [vp]),
    "gffx_hip_gff_n_skipped_lines": (C.c_uint64, [vp]),
    "gffx_hip_gff_n_warn_rows": (C.c_uint64, [vp]),
    "gffx_hip_gff_copy_fts": (C.c_int, [vp, u8p]),
    "gffx_hip_gff_copy_fid": (C.c_int, [vp, u32p]),
    "gffx_hip_gff_copy_prt": (C.c_int, [vp, u32p]),
    "gffx_hip_gff_copy_a2f": (C.c_int, [vp, u32p]),
    "gffx_hip_gff_copy_atn": (C.c_int, [vp, u8p]),
    "gffx_hip_gff_copy_seqids": (C.c_int, [vp, u8p]),
    "gffx_hip_gff_copy_gof": (C.c_int, [vp, u8p]),
    "gffx_hip_gff_copy_roots": (C.c_int, [vp, u32p]),
    "gffx_hip_gff_copy_skipped_lines": (C.c_int, [vp, u64p]),
    "gffx_hip_gff_copy_warn_rows": (C.c_int, [vp, u32p]),
    "gffx_hip_gff_destroy": (None, [vp]),
    "gffx_hip_genome_create": (C.c_int, [C.c_int, C.c_uint64, C.POINTER(vp)]),
    "gffx_hip_genome_reserve": (C.c_int, [vp, C.c_uint64]),
    "gffx_hip_genome_feed": (C.c_int, [vp, u8p, C.c_uint64]),
    "gffx_hip_genome_finish": (C.c_int, [vp]),
    "gffx_hip_genome_device": (C.c_int, [vp]),
    "gffx_hip_genome_n_seq": (C.c_uint32, [vp]),
    "gffx_hip_genome_n_bases": (C.c_uint64, [vp]),
    "gffx_hip_genome_name_bytes": (C.c_uint64, [vp]),
    "gffx_hip_genome_copy_names": (C.c_int, [vp, u8p, u64p]),
    "gffx_hip_genome_copy_seqs": (C.c_int, [vp, u64p, u32p]),
    "gffx_hip_genome_copy_bases": (C.c_int, [vp, C.c_uint64, C.c_uint64, u8p]),
    "gffx_hip_genome_stage_ms": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "gffx_hip_genome_destroy": (None, [vp]),
    "gffx_hip_scan64_tile": (C.c_uint32, []),
    "gffx_hip_scan64_carry_tiles": (C.c_uint32, []),
    "gffx_hip_seq_tile": (C.c_uint32, []),
    "gffx_hip_seq_create": (C.c_int, [vp, C.c_uint64, u32p, C.c_uint64, u8p, C.c_int, C.c_uint32, C.POINTER(vp)]),
    "gffx_hip_seq_body_bytes": (C.c_uint64, [vp]),
    "gffx_hip_seq_copy_offsets": (C.c_int, [vp, u64p, u8p]),
    "gffx_hip_seq_emit_start": (C.c_int, [vp, C.c_int, C.c_uint64, C.c_uint64]),
    "gffx_hip_seq_emit_wait": (C.c_int, [vp, C.c_int, C.POINTER(u8p)]),
    "gffx_hip_seq_stage_ms": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "gffx_hip_seq_destroy": (None, [vp]),
    "gffx_hip_effect_record_bytes": (C.c_uint32, []),
    "gffx_hip_effect_create": (C.c_int, [vp, C.c_uint64, u32p, C.c_uint64, u8p, C.c_uint64, C.POINTER(vp)]),
    "gffx_hip_effect_copy_transcripts": (C.c_int, [vp, u8p, u32p]),
    "gffx_hip_effect_run_start": (C.c_int, [vp, C.c_int, u32p, C.c_uint64]),
    "gffx_hip_effect_run_any_start": (C.c_int, [vp, C.c_int, u32p, C.c_uint64, u8p, C.c_uint64]),
    "gffx_hip_effect_run_wait": (C.c_int, [vp, C.c_int, C.POINTER(u64p), C.POINTER(u8p), C.POINTER(u8p), u64p]),
    "gffx_hip_effect_stage_ms": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "gffx_hip_effect_stats": (C.c_int, [vp, u64p, u64p]),
    "gffx_hip_effect_arena_grows": (C.c_int, [vp, u64p]),
    "gffx_hip_effect_destroy": (None, [vp]),
}

# the regex compiler of `gffx search -r` in libgffx_host.so (include/gffx_host.h "gffx_host_regex_*"): name -> (restype, argtypes)
HOST_LIB_PATH = os.path.join(_HERE, "lib", "libgffx_host.so")
HOST_SIGNATURES = {
    "gffx_host_regex_compile": (C.c_int, [C.c_uint64, u8p, u64p, C.c_uint32, C.POINTER(vp), C.c_char_p, C.c_size_t]),
    "gffx_host_regex_groups": (C.c_uint32, [vp]),
    "gffx_host_regex_group_info": (C.c_int, [vp, C.c_uint32, u32p, u32p, u32p, u32p, u32p]),
    "gffx_host_regex_group_tables": (C.c_int, [vp, C.c_uint32, u8p, C.POINTER(C.c_uint16)]),
    "gffx_host_regex_match": (C.c_int, [vp, C.c_uint64, u8p, u64p, u8p]),
    "gffx_host_regex_destroy": (None, [vp]),
}

_lib = None
_host = None


class GffxHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("gffx_hip error %d: %s" % (code, msg))
        self.code = code


def lib():
    """Load libgffx_hip.so (no fallback: raises if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s not found: build the HIP engine first (python -c 'import __graft_entry__ as g; g.build()' "
                "or make -C gffx_amd/csrc). There is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)  # AttributeError == missing export
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise GffxHipError(rc, lib().gffx_hip_last_error().decode(errors="replace"))


def host_lib():
    """Load libgffx_host.so for the entry points of HOST_SIGNATURES (they need no device)."""
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise ImportError("%s not found: build the host side first (make -C gffx_amd/csrc)" % HOST_LIB_PATH)
        L = C.CDLL(HOST_LIB_PATH)
        for name, (res, args) in HOST_SIGNATURES.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _host = L
    return _host
