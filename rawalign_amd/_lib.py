"""ctypes binding to librawdtw.so (the C ABI declared in include/rawdtw.h)."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class LibraryMissing(RuntimeError):
    pass


class RawDTWError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"rawdtw status {status}: {msg}")
        self.status = status


def library_path() -> str:
    return os.environ.get("RAWDTW_LIBRARY", os.path.join(HERE, "librawdtw.so"))


class AlignOpt(C.Structure):
    _fields_ = [
        ("border_constraint", C.c_int),
        ("fill_method", C.c_int),
        ("band_radius_frac", C.c_float),
        ("match_bonus", C.c_float),
        ("min_score", C.c_float),
        ("fused_score", C.c_int),
    ]


class ChainRec(C.Structure):
    """rawdtw_chain_t"""
    _fields_ = [
        ("chaining_score", C.c_float),
        ("alignment_score", C.c_float),
        ("reference_sequence_index", C.c_uint32),
        ("start_position", C.c_uint32),
        ("end_position", C.c_uint32),
        ("n_anchors", C.c_uint32),
        ("strand", C.c_int32),
        ("mapq", C.c_uint32),
        ("tag", C.c_uint32),
    ]


class SelectOpt(C.Structure):
    """rawdtw_select_opt_t"""
    _fields_ = [
        ("evaluate_chains", C.c_int),
        ("min_bestmap_ratio", C.c_float),
        ("min_meanmap_ratio", C.c_float),
        ("min_chain_anchor", C.c_uint32),
    ]


class ChainOpt(C.Structure):
    """rawdtw_chain_opt_t, defaults of src/roptions.c:13-19"""
    _fields_ = [
        ("max_gap_length", C.c_int),
        ("max_target_gap_length", C.c_int),
        ("chaining_band_length", C.c_int),
        ("max_num_skips", C.c_int),
        ("min_num_anchors", C.c_int),
        ("num_best_chains", C.c_int),
        ("min_chaining_score", C.c_float),
        ("e", C.c_int),
        ("disable_score_filtering", C.c_int),
    ]


class ChainOut(C.Structure):
    _fields_ = [("chaining_score", C.c_float), ("start_position", C.c_uint32), ("end_position", C.c_uint32),
                ("n_anchors", C.c_uint32)]


class MapperOpt(C.Structure):
    """rawdtw_mapper_opt_t"""
    _fields_ = [
        ("flag", C.c_int), ("align", AlignOpt), ("chain", ChainOpt),
        ("min_bestmap_ratio", C.c_float), ("min_meanmap_ratio", C.c_float), ("min_chain_anchor", C.c_uint32),
        ("bp_per_sec", C.c_uint32), ("sample_rate", C.c_uint32), ("chunk_size", C.c_uint32), ("max_num_chunk", C.c_uint32),
        ("slot_events", C.c_uint32), ("max_reads", C.c_uint32), ("carry", C.c_int), ("min_events", C.c_uint32),
        ("threads", C.c_int), ("groups", C.c_int), ("device_chain", C.c_int),
    ]


class SuOpt(C.Structure):
    """rawdtw_su_opt_t, defaults of src/roptions.c:43-46"""
    _fields_ = [("t_threshold", C.c_float), ("tn_samples", C.c_uint32), ("ttest_freq", C.c_uint32), ("tmin_reads", C.c_uint32),
                ("contracted", C.c_int)]


class EventOpt(C.Structure):
    """rawdtw_event_opt_t, defaults of src/roptions.c:37-41"""
    _fields_ = [("window_length1", C.c_uint32), ("window_length2", C.c_uint32), ("threshold1", C.c_float), ("threshold2", C.c_float),
                ("peak_height", C.c_float), ("contracted", C.c_int)]


class Channel(C.Structure):
    """rawdtw_channel_t: ri_sig_t's dig, ran, offset (src/rsig.h:16)"""
    _fields_ = [("digitisation", C.c_float), ("range", C.c_float), ("offset", C.c_float)]


class RoundOut(C.Structure):
    """rawdtw_round_out_t"""
    _fields_ = [("n_primary", C.c_uint32), ("mapq", C.c_uint32), ("flags", C.c_uint32)]


RAWDTW_SU_NO_STOP = 0xFFFFFFFF  # rawdtw_mapper_su_apply: no stop


class SeedHit(C.Structure):
    """rawdtw_seed_hit_t"""
    _fields_ = [("ref_seq", C.c_uint32), ("strand", C.c_int32), ("target_position", C.c_uint32), ("query_position", C.c_uint32)]


class SeedPars(C.Structure):
    """rawdtw_seed_pars_t: ri_idx_t's w, e, n, q, lq, k (defaults of ri_idxopt_init, src/rawindex.cpp:465-472)"""
    _fields_ = [("w", C.c_uint32), ("e", C.c_uint32), ("n", C.c_uint32), ("q", C.c_uint32), ("lq", C.c_uint32), ("k", C.c_uint32)]


class SeedResidentStats(C.Structure):
    """rawdtw_seed_resident_stats_t (rawdtw_seed_index_build_resident_stats)"""
    _fields_ = [("tile", C.c_uint32), ("log2_slots", C.c_uint32), ("tiles", C.c_uint64), ("kept", C.c_uint64), ("entries", C.c_uint64),
                ("keys", C.c_uint64), ("displaced", C.c_uint64), ("next_ms", C.c_float), ("chain_ms", C.c_float), ("mark_ms", C.c_float),
                ("emit_ms", C.c_float), ("sort_ms", C.c_float), ("table_ms", C.c_float)]


# rawdtw_scorer_fn (rawdtw_mapper_set_scorer)
SCORER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                        C.c_void_p, C.c_void_p)


class PlanInfo(C.Structure):
    _fields_ = [
        ("n_jobs", C.c_uint64),
        ("cells", C.c_uint64),
        ("algorithmic_bytes", C.c_uint64),
        ("n_lane_jobs", C.c_uint64),
        ("n_wave_band_jobs", C.c_uint64),
        ("n_full_jobs", C.c_uint64),
        ("workspace_bytes", C.c_uint64),
        ("n_launches", C.c_uint32),
    ]


# every symbol include/rawdtw.h declares: name -> (restype, argtypes)
VP, U64, U32, I32, F32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_float
SYMBOLS = {
    "rawdtw_abi_version": (I32, []),
    "rawdtw_device_count": (I32, [C.POINTER(I32)]),
    "rawdtw_create": (I32, [I32, C.POINTER(VP)]),
    "rawdtw_destroy": (I32, [VP]),
    "rawdtw_last_error": (C.c_char_p, [VP]),
    "rawdtw_status_string": (C.c_char_p, [I32]),
    "rawdtw_sync": (I32, [VP]),
    "rawdtw_set_option": (I32, [VP, C.c_char_p, C.c_int64]),
    "rawdtw_stream": (I32, [VP, C.POINTER(VP)]),
    "rawdtw_upload_reference": (I32, [VP, U32, VP, VP, VP]),
    "rawdtw_reference_offset": (I32, [VP, U32, I32, C.POINTER(U64)]),
    "rawdtw_set_reference_device": (I32, [VP, VP, U64]),
    "rawdtw_share_reference": (I32, [VP, VP]),
    "rawdtw_index_open": (I32, [C.c_char_p, C.POINTER(VP)]),
    "rawdtw_index_info": (I32, [VP, C.POINTER(U32), VP]),
    "rawdtw_index_seq": (I32, [VP, U32, C.POINTER(C.c_char_p), C.POINTER(U32)]),
    "rawdtw_index_upload": (I32, [VP, VP]),
    "rawdtw_index_read_signal": (I32, [VP, U32, I32, VP]),
    "rawdtw_index_close": (I32, [VP]),
    "rawdtw_upload_events": (I32, [VP, VP, U64]),
    "rawdtw_set_events_device": (I32, [VP, VP, U64]),
    "rawdtw_events_reserve": (I32, [VP, U64]),
    "rawdtw_events_append": (I32, [VP, VP, U64, U32, VP, VP]),
    "rawdtw_events_fetch": (I32, [VP, U32, VP, VP, VP, VP, U64]),
    "rawdtw_host_alloc": (I32, [U64, C.POINTER(VP)]),
    "rawdtw_host_free": (I32, [VP]),
    "rawdtw_host_is_page_locked": (I32, [VP]),
    "rawdtw_score_batch": (I32, [VP, VP, U64, VP, U64, VP]),
    "rawdtw_plan_create": (I32, [VP, VP, U64, C.POINTER(VP)]),
    "rawdtw_plan_info": (I32, [VP, C.POINTER(PlanInfo)]),
    "rawdtw_plan_dry_run": (I32, [U64, U64, VP, U64, C.c_int, VP, VP, U32, C.POINTER(PlanInfo), C.POINTER(U64), VP, U32]),
    "rawdtw_plan_run": (I32, [VP, VP]),
    "rawdtw_plan_fetch": (I32, [VP, VP, VP]),
    "rawdtw_plan_device_costs": (I32, [VP, C.POINTER(VP), C.POINTER(VP)]),
    "rawdtw_plan_run_timed": (I32, [VP, VP, VP, VP, U32]),
    "rawdtw_plan_destroy": (I32, [VP]),
    "rawdtw_traceback_batch": (I32, [VP, VP, U64, VP, U64, VP, VP, VP, VP, VP, VP]),
    "rawdtw_traceback_batch_steps": (I32, [VP, VP, U64, VP, U64, VP, VP, VP, VP, VP]),
    "rawdtw_traceback_arena_steps": (I32, [VP, VP, U64, VP, VP, VP, VP, VP]),
    "rawdtw_dtw_global": (I32, [VP, VP, U32, VP, U32, I32, C.POINTER(F32)]),
    "rawdtw_dtw_global_slantedbanded_antidiagonalwise": (I32, [VP, VP, U32, VP, U32, I32, I32, C.POINTER(F32)]),
    "rawdtw_dtw_global_tb": (I32, [VP, VP, U32, VP, U32, I32, C.POINTER(F32), C.POINTER(U32), VP, VP, VP]),
    "rawdtw_semiglobal_batch": (I32, [VP, VP, U64, VP, U64, VP, VP]),
    "rawdtw_semiglobal_traceback_steps": (I32, [VP, VP, U64, VP, U64, VP, VP, VP, VP, VP, VP]),
    "rawdtw_semiglobal_timing": (I32, [VP, C.POINTER(F32), C.POINTER(F32), C.POINTER(U64), C.POINTER(U64)]),
    "rawdtw_dtw_semiglobal": (I32, [VP, VP, U32, VP, U32, I32, C.POINTER(F32)]),
    "rawdtw_dtw_semiglobal_tb": (I32, [VP, VP, U32, VP, U32, I32, C.POINTER(F32), C.POINTER(U32), VP, VP, VP]),
    "rawdtw_semiglobal_host": (I32, [VP, U32, VP, U32, I32, C.POINTER(F32), C.POINTER(U32)]),
    "rawdtw_semiglobal_tb_host": (I32, [VP, U32, VP, U32, I32, C.POINTER(F32), C.POINTER(U32), C.POINTER(U32), VP, VP, VP]),
    "rawdtw_semiglobal_span_batch": (I32, [VP, VP, U64, VP, U64, VP, VP, VP]),
    "rawdtw_dtw_semiglobal_span": (I32, [VP, VP, U32, VP, U32, I32, C.POINTER(F32), C.POINTER(U32), C.POINTER(U32)]),
    "rawdtw_semiglobal_span_host": (I32, [VP, U32, VP, U32, I32, C.POINTER(F32), C.POINTER(U32), C.POINTER(U32)]),
    "rawdtw_set_semiglobal_window": (I32, [VP, U32]),
    "rawdtw_get_semiglobal_window": (I32, [VP, C.POINTER(U32)]),
    "rawdtw_semiglobal_window_stats": (I32, [VP, C.POINTER(U64), C.POINTER(U64), C.POINTER(U64), C.POINTER(U64)]),
    "rawdtw_semiglobal_tb_window_host": (I32, [VP, U32, VP, U32, I32, U32, C.POINTER(F32), C.POINTER(U32), C.POINTER(U32), VP, VP, VP,
                                              C.POINTER(U32)]),
    "rawdtw_banded_traceback_steps": (I32, [VP, VP, U64, VP, U64, VP, VP, VP, VP, VP]),
    "rawdtw_banded_traceback_timing": (I32, [VP, C.POINTER(F32), C.POINTER(F32), C.POINTER(U64), C.POINTER(U64)]),
    "rawdtw_dtw_global_banded_tb": (I32, [VP, VP, U32, VP, U32, I32, I32, C.POINTER(F32), C.POINTER(U32), VP, VP, VP]),
    "rawdtw_banded_tb_host": (I32, [VP, U32, VP, U32, I32, I32, C.POINTER(F32), C.POINTER(U32), VP, VP, VP]),
    "rawdtw_mapper_set_banded_cigar": (I32, [VP, I32]),
    "rawdtw_mapper_set_device_text": (I32, [VP, I32]),
    "rawdtw_aln_text_host": (I32, [VP, VP, VP, VP, VP, U64, I32, VP, VP, U64, C.POINTER(U64)]),
    "rawdtw_aln_text_bound": (U64, [VP, VP, U64]),
    "rawdtw_aln_text_steps": (I32, [VP, VP, VP, VP, VP, VP, U64, VP, VP, U64, C.POINTER(U64)]),
    "rawdtw_traceback_batch_text": (I32, [VP, VP, U64, VP, U64, VP, VP, VP, VP, VP, U64, C.POINTER(U64)]),
    "rawdtw_traceback_arena_text": (I32, [VP, VP, U64, VP, VP, VP, VP, VP, U64, C.POINTER(U64)]),
    "rawdtw_aln_text_timing": (I32, [VP, C.POINTER(F32), C.POINTER(F32), C.POINTER(U64)]),
    "rawdtw_set_border_local": (I32, [VP, I32]),
    "rawdtw_get_border_local": (I32, [VP, VP]),
    "rawdtw_batch_hand_over_stats": (I32, [VP, VP, VP, VP]),
    "rawdtw_chain_job_count": (U32, [C.POINTER(AlignOpt), U32]),
    "rawdtw_chain_build_jobs": (I32, [C.POINTER(AlignOpt), VP, U32, U64, U32, I32, VP]),
    "rawdtw_chain_replay": (F32, [C.POINTER(AlignOpt), VP, U32, VP, F32]),
    "rawdtw_read_replay": (U32, [C.POINTER(AlignOpt), U32, VP, VP, VP, VP, VP, VP]),
    "rawdtw_gen_primary_chains": (U32, [VP, U32, C.POINTER(SelectOpt), VP]),
    "rawdtw_is_mapped_with_high_confidence": (I32, [VP, U32, C.POINTER(SelectOpt)]),
    "rawdtw_find_outlier": (F32, [VP, U32, U32]),
    "rawdtw_find_outlier_contracted": (F32, [VP, U32, U32]),
    "rawdtw_su_create": (I32, [U32, VP, C.POINTER(VP)]),
    "rawdtw_su_feed": (I32, [VP, U32, VP, VP, VP, C.POINTER(U32)]),
    "rawdtw_su_state": (I32, [VP, VP, VP, VP, VP]),
    "rawdtw_su_destroy": (I32, [VP]),
    "rawdtw_chain_anchors": (I32, [C.POINTER(ChainOpt), VP, U32, C.POINTER(F32), VP, VP, VP, U32, U64]),
    "rawdtw_sort_by_chaining_score": (I32, [VP, U32, VP]),
    "rawdtw_batch_build_jobs": (I32, [C.POINTER(AlignOpt), U64, VP, VP, VP, VP, VP, VP, U64, C.POINTER(U64)]),
    "rawdtw_batch_create": (I32, [VP, C.POINTER(AlignOpt), U64, VP, VP, VP, VP, VP, C.POINTER(VP)]),
    "rawdtw_batch_verify_plan": (I32, [VP, VP, VP, U64, C.POINTER(C.c_int), VP, U32]),
    "rawdtw_batch_info": (I32, [VP, C.POINTER(PlanInfo), C.POINTER(U64)]),
    "rawdtw_batch_run": (I32, [VP, VP]),
    "rawdtw_batch_run_timed": (I32, [VP, VP, VP, VP, U32, C.POINTER(U32)]),
    "rawdtw_batch_run_reps": (I32, [VP, VP, U32, VP, VP, U32, C.POINTER(U32)]),
    "rawdtw_batch_enqueue": (I32, [VP, VP, I32]),
    "rawdtw_batch_collect": (I32, [VP, VP, VP, VP, U32, C.POINTER(U32), C.POINTER(U32)]),
    "rawdtw_batch_launch_stats": (I32, [VP, U32, C.POINTER(U32), C.POINTER(I32), C.POINTER(U64), C.POINTER(U64), C.POINTER(U64)]),
    "rawdtw_batch_fetch": (I32, [VP, VP, VP, VP, VP]),
    "rawdtw_batch_plan_ms": (I32, [VP, VP, C.POINTER(F32)]),
    "rawdtw_batch_wide_ms": (I32, [VP, VP, C.POINTER(F32)]),
    "rawdtw_batch_stream_counters": (I32, [VP, VP, VP, U32, VP]),
    "rawdtw_batch_chunk_profile": (I32, [VP, VP, C.c_int, VP, U32, VP]),
    "rawdtw_batch_destroy": (I32, [VP]),
    "rawdtw_batch_submit": (I32, [VP, VP, U64, VP, VP, VP, VP, VP, VP]),
    "rawdtw_batch_submit_device": (I32, [VP, VP, U64, VP, VP, VP, VP, VP, VP]),
    "rawdtw_chain_round": (I32, [VP, C.POINTER(ChainOpt), U64, VP, VP, VP, U32, VP, VP, VP, VP, U64, VP, VP, VP, VP]),
    "rawdtw_chain_round_begin": (I32, [VP, C.POINTER(ChainOpt), U64, VP, VP, VP, U32, VP, VP, VP, VP, U64, VP]),
    "rawdtw_chain_round_end": (I32, [VP, VP, VP, VP]),
    "rawdtw_batch_fetch_destroy": (I32, [VP, VP, VP, VP]),
    "rawdtw_batch_submit_carry": (I32, [VP, VP, U64, VP, VP, VP, VP, VP, VP, VP, VP, VP, VP]),
    "rawdtw_batch_can_carry": (I32, [VP, VP, VP]),
    "rawdtw_batch_round_stats": (I32, [VP, VP, VP, VP]),
    "rawdtw_round_match_chains": (I32, [U64, VP, VP, VP, VP, VP, VP, VP, VP, VP, VP, VP, VP, VP, VP]),
    "rawdtw_batch_stream_counter_index": (I32, [C.c_char_p]),
    "rawdtw_mapper_create": (I32, [VP, VP, U32, VP, VP, VP]),
    "rawdtw_mapper_add_read": (I32, [VP, C.c_char_p, U32, U32, VP]),
    "rawdtw_mapper_round": (I32, [VP, U32, VP, VP, VP, VP, VP]),
    "rawdtw_mapper_read_state": (I32, [VP, U32, VP, VP]),
    "rawdtw_mapper_finish": (I32, [VP]),
    "rawdtw_mapper_paf": (I32, [VP, U32, VP, U32, VP]),
    "rawdtw_mapper_log": (I32, [VP, VP]),
    "rawdtw_mapper_stats": (I32, [VP, VP, VP, VP]),
    "rawdtw_mapper_last_error": (C.c_char_p, [VP]),
    "rawdtw_mapper_destroy": (I32, [VP]),
    "rawdtw_mapper_release_read": (I32, [VP, U32]),
    "rawdtw_mapper_timing": (I32, [VP, VP]),
    "rawdtw_mapper_set_scorer": (I32, [VP, VP, VP]),
    "rawdtw_mapper_set_sequence_until": (I32, [VP, VP]),
    "rawdtw_mapper_su_batch": (I32, [VP, U32, VP, C.POINTER(U32)]),
    "rawdtw_mapper_batch_records": (I32, [VP, U32, VP, VP, VP, VP]),
    "rawdtw_mapper_su_apply": (I32, [VP, U32, VP, U32]),
    "rawdtw_mapper_su_state": (I32, [VP, C.POINTER(I32), C.POINTER(U32)]),
    "rawdtw_context_device": (I32, [VP, C.POINTER(I32)]),
    "rawdtw_anchors_pack": (I32, [U64, VP, VP, VP, VP, VP, VP, U64, VP]),
    "rawdtw_anchors_unpack": (I32, [U64, VP, VP, VP, VP, VP, U64, VP]),
    "rawdtw_batch_submit_compact": (I32, [VP, VP, U64, VP, VP, VP, VP, VP, VP, U64, VP, VP, VP]),
    "rawdtw_traceback_timing": (I32, [VP, VP, VP, VP, VP]),
    "rawdtw_batch_replay": (I32, [C.POINTER(AlignOpt), U64, VP, VP, VP, VP, VP, VP, VP]),
    "rawdtw_detect_events": (I32, [C.POINTER(EventOpt), U32, VP, VP, C.POINTER(U32)]),
    "rawdtw_detect_events_host": (I32, [C.POINTER(EventOpt), U32, VP, VP, VP, VP, U64, I32]),
    "rawdtw_detect_begin": (I32, [VP, C.POINTER(EventOpt), U32, VP, VP, VP, VP, U64]),
    "rawdtw_detect_end": (I32, [VP, C.POINTER(F32)]),
    "rawdtw_signal_to_pa": (I32, [VP, U64, VP, VP, C.POINTER(U64)]),
    "rawdtw_signal_chunk_table": (I32, [VP, U64, VP, U32, U32, C.POINTER(U64), C.POINTER(U32), VP]),
    "rawdtw_detect_raw_host": (I32, [C.POINTER(EventOpt), U32, VP, VP, VP, VP, VP, VP, U64, I32]),
    "rawdtw_detect_raw_begin": (I32, [VP, C.POINTER(EventOpt), U32, VP, VP, VP, VP, VP, VP, U64]),
    "rawdtw_seed_index_build": (I32, [U32, VP, VP, VP, C.POINTER(SeedPars), I32, C.POINTER(VP)]),
    "rawdtw_seed_index_load": (I32, [VP, C.POINTER(VP)]),
    "rawdtw_seed_index_get": (I32, [VP, U64, C.POINTER(VP), C.POINTER(U32)]),
    "rawdtw_seed_index_info": (I32, [VP, C.POINTER(U32), C.POINTER(U64), C.POINTER(U64), C.POINTER(U64), C.POINTER(SeedPars)]),
    "rawdtw_seed_index_keys": (I32, [VP, VP]),
    "rawdtw_seed_index_destroy": (I32, [VP]),
    "rawdtw_seed_sketch": (I32, [C.POINTER(SeedPars), VP, U32, VP, VP, C.POINTER(U32)]),
    "rawdtw_seed_hits_host": (I32, [VP, U32, VP, VP, VP, VP, U64, I32]),
    "rawdtw_seed_index_upload": (I32, [VP, VP]),
    "rawdtw_seed_begin": (I32, [VP, U32, VP, VP, VP, VP, U64]),
    "rawdtw_seed_end": (I32, [VP, C.POINTER(F32)]),
    "rawdtw_mapper_round_seeded": (I32, [VP, VP, U32, VP, VP, VP]),
    "rawdtw_seed_resident_begin": (I32, [VP, U32, VP, VP, VP]),
    "rawdtw_seed_resident_end": (I32, [VP, C.POINTER(F32)]),
    "rawdtw_seed_resident_fetch": (I32, [VP, VP, U64]),
    "rawdtw_chain_round_begin_resident": (I32, [VP, C.POINTER(ChainOpt), U64, VP, VP, VP, VP, VP, VP, U32, VP, VP, VP, VP, U64, VP]),
    "rawdtw_mapper_round_seeded_resident": (I32, [VP, VP, U32, VP, VP, VP]),
    "rawdtw_mapper_resident_stats": (I32, [VP, VP, VP, VP, VP]),
    "rawdtw_chain_round_stats": (I32, [VP, VP, VP, VP, VP]),
    "rawdtw_chain_order_stats": (I32, [VP, VP, VP, VP]),
    "rawdtw_sort_by_chaining_score_restated": (I32, [VP, U32, VP, VP]),
    "rawdtw_get_option": (I32, [VP, C.c_char_p, C.POINTER(C.c_int64)]),
    "rawdtw_detect_resident_begin": (I32, [VP, C.POINTER(EventOpt), U32, VP, VP, VP, VP, U64]),
    "rawdtw_detect_raw_resident_begin": (I32, [VP, C.POINTER(EventOpt), U32, VP, VP, VP, VP, VP, U64]),
    "rawdtw_detect_resident_end": (I32, [VP, VP, VP, C.POINTER(U64), C.POINTER(F32)]),
    "rawdtw_seed_detected_begin": (I32, [VP, VP]),
    "rawdtw_mapper_round_signal_resident": (I32, [VP, VP, C.POINTER(EventOpt), U32, VP, VP, VP]),
    "rawdtw_mapper_round_raw_resident": (I32, [VP, VP, C.POINTER(EventOpt), U32, VP, VP, VP, VP]),
    "rawdtw_mapper_signal_stats": (I32, [VP, VP, VP, VP, VP]),
    "rawdtw_mapper_read_events": (I32, [VP, U32, VP, U32, VP]),
    "rawdtw_round_end_host": (I32, [C.POINTER(SelectOpt), U64, VP, VP, VP, VP, VP, VP]),
    "rawdtw_round_end": (I32, [VP, C.POINTER(SelectOpt), U64, VP, VP, VP, VP, VP, VP]),
    "rawdtw_batch_round_end_begin": (I32, [VP, VP, C.POINTER(SelectOpt), VP, I32]),
    "rawdtw_batch_round_end_fetch": (I32, [VP, VP, VP, VP]),
    "rawdtw_chain_round_recs": (I32, [VP, C.POINTER(VP)]),
    "rawdtw_mapper_round_end_stats": (I32, [VP, VP, VP, VP]),
    "rawdtw_chain_keep_reserve": (I32, [VP, U64, U64]),
    "rawdtw_round_keep_host": (I32, [U64, VP, VP, VP, VP, VP, VP, U32, VP, VP, VP]),
    "rawdtw_round_keep": (I32, [VP, U64, VP, VP, VP, VP, VP, VP, VP, VP]),
    "rawdtw_batch_round_end_keep": (I32, [VP, VP, VP]),
    "rawdtw_batch_round_keep_fetch": (I32, [VP, VP, VP]),
    "rawdtw_chain_kept_fetch": (I32, [VP, U32, VP, U32, VP]),
    "rawdtw_chain_round_begin_resident_kept": (I32, [VP, VP, U64, VP, VP, VP, VP, VP, VP, VP, U32, VP, VP, VP, VP, U64, VP]),
    "rawdtw_mapper_kept_stats": (I32, [VP, VP, VP, VP, VP, VP]),
    "rawdtw_mapper_decline_stats": (I32, [VP, VP, VP, VP, VP, VP]),
    "rawdtw_chain_round_declined": (I32, [VP, C.POINTER(U64), C.POINTER(VP), C.POINTER(VP)]),
    "rawdtw_chain_round_declined_seeds": (I32, [VP, VP, VP, U64]),
    "rawdtw_chain_round_append": (I32, [VP, U64, VP, VP, VP, VP, VP, VP, C.POINTER(VP), C.POINTER(VP), C.POINTER(VP)]),
    "rawdtw_chain_decline_host": (I32, [C.POINTER(ChainOpt), U64, VP, VP, U32, U32, U32, VP, VP]),
    "rawdtw_pore_model_load": (I32, [C.c_char_p, C.POINTER(U32), VP, U64]),
    "rawdtw_seq_to_sig_host": (I32, [VP, U32, VP, U32, I32, I32, VP, C.POINTER(U32)]),
    "rawdtw_seq_sums_restated": (I32, [VP, U64, C.POINTER(C.c_double), C.POINTER(C.c_double), VP, VP]),
    "rawdtw_reference_from_bases": (I32, [VP, U32, VP, VP, VP, U32, I32]),
    "rawdtw_reference_fetch": (I32, [VP, U32, I32, VP, U64]),
    "rawdtw_reference_build_stats": (I32, [VP, VP, VP, VP]),
    "rawdtw_seed_index_build_device": (I32, [VP, C.POINTER(SeedPars), C.POINTER(VP)]),
    "rawdtw_seed_index_build_stats": (I32, [VP, VP]),
    "rawdtw_seed_index_build_device_min": (I32, [VP, C.POINTER(SeedPars), C.POINTER(VP)]),
    "rawdtw_seed_sketch_windowed": (I32, [C.POINTER(SeedPars), VP, U32, VP, VP, U32, C.POINTER(U32)]),
    "rawdtw_seed_index_build_min_stats": (I32, [VP, C.POINTER(U64), C.POINTER(U64), VP]),
    "rawdtw_seed_index_build_resident": (I32, [VP, C.POINTER(SeedPars), C.POINTER(VP)]),
    "rawdtw_seed_index_is_resident": (I32, [VP]),
    "rawdtw_seed_index_fetch": (I32, [VP, VP]),
    "rawdtw_seed_index_from_entries": (I32, [C.POINTER(SeedPars), U32, U64, VP, VP, C.POINTER(VP)]),
    "rawdtw_seed_table_from_entries": (I32, [VP, C.POINTER(SeedPars), U32, U64, VP, VP, C.POINTER(VP)]),
    "rawdtw_seed_index_build_resident_stats": (I32, [VP, C.POINTER(SeedResidentStats)]),
}


def load_library():
    """Load librawdtw.so; raises LibraryMissing (never falls back to anything else)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise LibraryMissing(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C rawalign_amd/csrc` (hipcc, --offload-arch=gfx950)"
        )
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the ABI lost a symbol
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib
