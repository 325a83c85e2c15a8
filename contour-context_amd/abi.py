"""The ctypes signature of every function include/cont2_amd.h declares, in one table, and bind() to apply it to a loaded
library (the product's, the CPU harness's, another build).  tests/test_abi_layout.py holds the table against the header.
The extension headers beside it have tables of their own, which bind() applies as well: EXTENSIONS (include/cont2_amd_images.h) and
the open-ended ADDONS (include/cont2_amd_filter.h, include/cont2_amd_coords.h, include/cont2_amd_paths.h, include/cont2_amd_cands.h and whatever follows).

One line per prototype, in the header's order: return code, name, one code per parameter.
  parameters   P any pointer or array   I int / int32_t   Q int64_t   Z size_t   D double   F float   (- : none)
  return       I int   V void   S const char *   P any other pointer"""
import ctypes as C

_SPEC = """
V cc_default_manager_cfg P
V cc_default_db_cfg P
V cc_default_thresholds PP
S cc_last_error -
I cc_version -
I cc_runtime_init II
I cc_create IPIP
I cc_destroy P
I cc_profile_enable PI
I cc_profile_read PPP
I cc_ingest_batch PPPIPPP
I cc_ingest_host PPPIP
I cc_ingest_host_bev PPPIPP
I cc_ingest_points PPPPIPPPP
I cc_ingest_points_host PPPPIPPP
I cc_ingest_segments PPPIPPP
I cc_ingest_segments_host PPPIPP
I cc_ingest_points_motion PPPPPIPPPPP
I cc_ingest_points_motion_host PPPPPIPPPP
V cc_motion_knots PPDIP
I cc_range_sensor_create PPP
I cc_range_sensor_destroy P
I cc_ingest_ranges PPPIPPPP
I cc_ingest_ranges_host PPPIPPP
P cc_stage_points PQ
P cc_stage_points_slot PQI
I cc_stage_points_cancel PP
I cc_scan_ingest PPQIP
I cc_scan_ingest_batch PPPIP
I cc_scan_ingest_points PPPQPIP
I cc_scan_ingest_points_batch PPPPIPP
I cc_scan_ingest_segments PPIIP
I cc_scan_ingest_points_motion PPPPQPPIP
I cc_scan_ingest_ranges PPPPIP
I cc_scan_ready P
I cc_scan_desc PP
I cc_scan_bev PP
I cc_scan_offload P
I cc_scan_on_device P
I cc_scan_release P
I cc_db_create PPIP
I cc_db_destroy P
I cc_db_size P
I cc_db_knn_stride P
I cc_db_add_scans PPIPPP
I cc_db_add_scans_prepare PPIP
I cc_db_query_batch PPIPPPPPPP
I cc_db_query_submit PPIPPPPPPP
I cc_db_query_wait P
I cc_db_add_scan_host PPDI
I cc_db_query_host PPPPP
I cc_db_query_scan PPPPP
I cc_db_add_scan PPDI
I cc_db_query_scan_submit PPIPPP
I cc_db_query_collect PPI
I cc_db_add_scan_prepare PP
I cc_db_add_scan_batch PPIPP
I cc_db_query_scan_batch_submit PPIPPPP
I cc_db_add_scans_host PPIPP
I cc_db_query_batch_host PPIPPPP
I cc_db_check_hints PPPIPPIPPP
I cc_db_check_hints_host PPPIPPIPP
I cc_db_verify_submit PPIPPIPPPPPPP
I cc_db_verify_batch PPIPPIPPPPPPP
I cc_db_verify_batch_host PPIPPIPPPP
I cc_db_query_submit_ranked PPIPPPPPPPP
I cc_db_query_batch_host_ranked PPIPPPPP
I cc_db_query_scan_batch_submit_ranked PPIPPPPP
I cc_db_verify_submit_ranked PPIPPIPPPPPPPP
I cc_db_check_hints_ranked PPPIPPIPPPP
I cc_db_verify_batch_host_ranked PPIPPIPPPPP
I cc_db_check_hints_host_ranked PPPIPPIPPP
I cc_db_query_submit_ranked_detail PPIPPPPPPPPP
I cc_db_query_batch_host_ranked_detail PPIPPPPPP
I cc_db_query_scan_batch_submit_ranked_detail PPIPPPPPP
I cc_db_verify_submit_ranked_detail PPIPPIPPPPPPPPP
I cc_db_verify_batch_host_ranked_detail PPIPPIPPPPPP
I cc_db_check_hints_ranked_detail PPPIPPIPPPPP
I cc_db_check_hints_host_ranked_detail PPPIPPIPPPP
I cc_db_pose_submit PPIPIPPPPPP
I cc_db_pose_batch PPIPIPPPPPP
I cc_db_pose_batch_host PPIPIPPPPP
I cc_db_query_submit_packed PPPIPPPPPPPPP
I cc_db_verify_submit_packed PPPPIPPPPPPPPP
I cc_db_pose_submit_packed PPPIPPPPPP
I cc_db_query_submit_masked PPPPIPPPPPPPPPP
I cc_db_query_batch_host_masked PPIPPPPPPP
I cc_mask_gates PPIPIPIP
I cc_db_debug_knn_chunks PP
I cc_db_debug_passes PPIP
V cc_packed_sizes PP
I cc_pack_scans PPIPPP
I cc_db_add_packed PPPIPPP
P cc_db_hot_ptr P
P cc_db_feat_ptr P
I cc_db_profile_enable PI
I cc_db_profile_read PPP
I cc_db_set_lanes PI
I cc_db_set_dynamic_thres PI
I cc_db_bucket_state PPP
I cc_comm_unique_id P
I cc_comm_create IIIPP
I cc_comm_create_from_env PPP
I cc_comm_rank P
I cc_comm_world P
I cc_comm_allgather_packed PPPZP
I cc_comm_destroy P
V cc_est_sens_tf PIIP
V cc_est_sens_info PPIIP
"""

_ARG = {"P": C.c_void_p, "I": C.c_int, "Q": C.c_int64, "Z": C.c_size_t, "D": C.c_double, "F": C.c_float}
_RET = {"I": C.c_int, "V": None, "S": C.c_char_p, "P": C.c_void_p}


def _table(spec):
    return {name: (_RET[ret], [_ARG[a] for a in args.strip("-")]) for ret, name, args in (ln.split() for ln in spec.split("\n") if ln)}


# symbol -> (restype, argtypes)
SIGNATURES = _table(_SPEC)

# The extension headers beside include/cont2_amd.h, each with a table of its own in the same codes: header -> {symbol: (restype, argtypes)}.
# tests/test_abi_images.py holds them against their headers.
_EXT_SPEC = {
    "cont2_amd_images.h": """
I cc_ingest_images PPPIPPPP
I cc_ingest_images_host PPPIPPP
I cc_scan_ingest_image PPPPIP
""",
}
EXTENSIONS = {hdr: _table(spec) for hdr, spec in _EXT_SPEC.items()}

# The add-on headers: every later header of include/ joins HERE, one entry each, and nothing else has to know how many there are.
# (EXTENSIONS stays the one header it was made for: its test holds the dictionary itself to that header.)  Each add-on's own test
# holds its entry against its header, as tests/test_abi_filter.py does.
_ADDON_SPEC = {
    "cont2_amd_filter.h": """
I cc_ingest_points_filtered PPPPPIPPPP
I cc_ingest_points_filtered_host PPPPPIPPP
I cc_scan_ingest_points_filtered PPPPQPIP
""",
    "cont2_amd_coords.h": """
I cc_ingest_coords PPPIPPPPP
I cc_ingest_coords_host PPPIPPPP
I cc_scan_ingest_coords PPQPPIP
""",
    "cont2_amd_paths.h": """
I cc_ingest_path_counts PP
""",
    "cont2_amd_cands.h": """
I cc_db_debug_cands PPIP
""",
    "cont2_amd_rig.h": """
I cc_ingest_rig PPPIPIPPPP
I cc_ingest_rig_host PPPIPIPPP
I cc_scan_ingest_rig PPIPIPIP
""",
    "cont2_amd_matches.h": """
I cc_match_pairs PPI
I cc_db_query_submit_matched PPPPIPPPPPPPPPPP
I cc_db_verify_submit_matched PPIPPPIPPPPPPPPPP
I cc_db_check_hints_matched PPPIPPIPPPPPP
I cc_db_query_scan_batch_submit_matched PPIPPPPPPP
I cc_db_query_batch_host_matched PPIPPPPPPPP
I cc_db_verify_batch_host_matched PPIPPIPPPPPPP
I cc_db_check_hints_host_matched PPPIPPIPPPPP
""",
    "cont2_amd_lists.h": """
I cc_db_query_submit_listed PPPPIPPPPPPPPPPP
I cc_db_query_batch_host_listed PPIPPPPPPPP
I cc_db_debug_knn_chunks_listed PP
""",
    "cont2_amd_keyview.h": """
I cc_db_debug_key_view PIIPPPP
""",
}
ADDONS = {hdr: _table(spec) for hdr, spec in _ADDON_SPEC.items()}


def bind(cdll):
    """Give every function of the tables its restype and argtypes on `cdll` (a library that lacks one is an AttributeError)."""
    for table in [SIGNATURES] + list(EXTENSIONS.values()) + list(ADDONS.values()):
        for name, (restype, argtypes) in table.items():
            fn = getattr(cdll, name)
            fn.restype, fn.argtypes = restype, argtypes
    return cdll
