"""ctypes binding of include/enspara_hip.h (libenspara_hip.so, in-tree).

There is no CPU fallback: if the library is missing, or no HIP device is
visible when a device call is made, this raises.  torch is imported first so
that the library binds to the HIP runtime torch already loaded (both carry
the soname libamdhip64.so.7); torch itself is only plumbing here
(torch.distributed for the multi-GPU exchange).
"""
import collections
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ENSPARA_HIP_LIB",
                          os.path.join(HERE, "libenspara_hip.so"))

EK_TILE = 256
EK_OK, EK_EARG, EK_EHIP, EK_ESTATE, EK_ENOMEM = 0, -1, -2, -3, -4

# every symbol include/enspara_hip.h declares (tests check the export table)
SYMBOLS = [
    "ek_abi_version", "ek_last_error", "ek_device_count",
    "ek_ctx_create", "ek_ctx_destroy", "ek_ctx_sync", "ek_ctx_stream",
    "ek_load_frames", "ek_rmsd_to_center",
    "ek_state_reset", "ek_state_download", "ek_state_upload",
    "ek_record_bytes", "ek_local_candidate", "ek_own_record",
    "ek_kcenters_step", "ek_kcenters_run",
    "ek_history_download", "ek_history_reset",
    "ek_spec_candidates", "ek_round_candidates", "ek_quad_copy_ready",
    "ek_spec_begin", "ek_spec_round", "ek_spec_localmax",
    "ek_spec_apply", "ek_spec_round_end", "ek_spec_progress", "ek_spec_rounds",
    "ek_spec_chain_bytes", "ek_spec_chain_rows", "ek_spec_chain_max",
    "ek_spec_chain_apply", "ek_run_stats", "ek_ti_stats", "ek_view_stats",
    "ek_last_run_form",
    "ek_view_layout_check",
    "ek_ms_setup", "ek_ms_mailbox", "ek_ms_connect", "ek_ms_begin", "ek_ms_local",
    "ek_ms_global", "ek_ms_end", "ek_ms_run", "ek_ms_state", "ek_ms_diag",
    "ek_assign_nearest",
    "ek_pam_begin", "ek_pam_count_members", "ek_pam_select_member",
    "ek_pam_propose", "ek_pam_propose_member", "ek_pam_commit",
    "ek_pam_count_members_batch", "ek_pam_select_members_batch",
    "ek_pam_prefetch", "ek_pam_propose_ex", "ek_pam_prefetch_stats",
    "ek_pam_prefetch_window", "ek_pam_prefetch_passes", "ek_pam_sparse_stats", "ek_pam_ahead_stats", "ek_pam_window_run", "ek_pam_sweep", "ek_np_choice_draws",
    "ek_pam_window_max",
    "ek_pam_prefetch_centers_window",
    "ek_centered_frames", "ek_pam_begin_table", "ek_pam_prefetch_centers",
    "ek_pam_propose_center",
    "ek_msm_counts", "ek_msm_counts_ctx", "ek_msm_row_normalize",
    "ek_msm_mle_prinz", "ek_msm_bace_prune", "ek_msm_bace_run",
    "ek_msm_boot_open", "ek_msm_boot_fetch", "ek_msm_boot_build", "ek_msm_boot_last_timing",
    "ek_msm_boot_close",
    "ek_lu_solve", "ek_lu_set_timing", "ek_lu_last_timing",
    "ek_tpt_committors", "ek_tpt_mfpts_sinks", "ek_tpt_mfpts_all", "ek_tpt_fluxes",
    "ek_tpt_paths_open", "ek_tpt_paths_next", "ek_tpt_paths_stats", "ek_tpt_paths_close",
    "ek_mi_open", "ek_mi_add", "ek_mi_load_counts", "ek_mi_counts", "ek_mi_information",
    "ek_mi_last_timing", "ek_mi_close",
    "ek_cards_open", "ek_cards_add", "ek_cards_stats", "ek_cards_disorder",
    "ek_cards_disorder_codes", "ek_cards_matrices", "ek_cards_counts",
    "ek_cards_last_timing", "ek_cards_close", "ek_cards_scan_chunk",
    "ek_sasa_open", "ek_sasa_run", "ek_sasa_last_timing", "ek_sasa_close",
    "ek_rmsf_open", "ek_rmsf_run", "ek_rmsf_fetch", "ek_rmsf_last_timing", "ek_rmsf_close",
    "ek_wmi_run", "ek_wmi_last_timing",
    "ek_ent_kl_rows", "ek_ent_js_rows", "ek_ent_shannon_rows", "ek_ent_kl_counts",
    "ek_ent_last_timing", "ek_ent_state_counts_open", "ek_ent_state_counts_add",
    "ek_ent_state_counts_read", "ek_ent_state_counts_last_timing",
    "ek_ent_state_counts_close",
    "ek_kmc_create", "ek_kmc_destroy", "ek_kmc_next", "ek_kmc_trajectories",
    "ek_kmc_ensemble", "ek_kmc_fret_probs", "ek_kmc_fret_bursts", "ek_kmc_last_timing",
    "ek_dye_pair_create", "ek_dye_pair_destroy", "ek_dye_pair_table", "ek_dye_pair_resolve",
    "ek_dye_pair_static", "ek_dye_pair_last_timing",
    "ek_dye_bursts_lifetimes", "ek_dye_bursts_k2", "ek_dye_photons_lifetimes",
    "ek_dye_photons_k2", "ek_dye_pick_events", "ek_dye_bursts_last_timing",
    "ek_pockets_open", "ek_pockets_run", "ek_pockets_counts", "ek_pockets_fetch",
    "ek_pockets_last_timing", "ek_pockets_close", "ek_pockets_touches", "ek_pockets_ranks",
    "ek_pockets_labels",
    "ek_dyes_open", "ek_dyes_run", "ek_dyes_counts", "ek_dyes_fetch", "ek_dyes_last_timing",
    "ek_dyes_close", "ek_dyes_touches", "ek_dyes_pair_hist",
    "ek_dye_map_open", "ek_dye_map_max_centres", "ek_dye_map_run", "ek_dye_map_fetch",
    "ek_dye_map_stats", "ek_dye_map_last_timing", "ek_dye_map_close",
    "ek_rotamer_states", "ek_dihedral_angles", "ek_dihedral_rotamers",
    "ek_krylov_create", "ek_krylov_destroy", "ek_krylov_set_vector",
    "ek_krylov_get_vector", "ek_krylov_step", "ek_krylov_rotate",
    "ek_krylov_combine", "ek_krylov_expand", "ek_krylov_set_filter",
    "ek_feat_create", "ek_feat_destroy", "ek_feat_load", "ek_feat_distance",
    "ek_feat_kcenters", "ek_feat_pam_sweep", "ek_feat_pam_release",
    "ek_feat_record_bytes", "ek_feat_create_sharded", "ek_feat_state_reset",
    "ek_feat_state_upload", "ek_feat_state_download", "ek_feat_local_candidate",
    "ek_feat_kcenters_step", "ek_feat_history_download", "ek_feat_history_reset",
    "ek_feat_pam_count_batch", "ek_feat_pam_select_batch", "ek_feat_pam_gather_rows",
    "ek_feat_pam_begin", "ek_feat_pam_propose", "ek_feat_pam_commit",
    "ek_feat_assign_nearest",
    "ek_set_frames_per_lane", "ek_set_option", "ek_get_option", "ek_last_run_timing",
    "ek_reserve_centers",
    "ek_debug_guards",
    "ek_timing_begin", "ek_timing_end", "ek_timing_form", "ek_hbm_copy_rate",
    "ek_qcp_probe", "ek_pam_pairs_probe",
    "ek_live_resources", "ek_fail_alloc_at",
]


# enum ek_option of include/enspara_hip.h (tests/test_abi.py holds the two equal)
EK_OPT_NONTEMPORAL = 1
EK_OPT_ASSIGN_KERNEL = 2
EK_OPT_CANDIDATES = 4
EK_OPT_CHAINED = 5
EK_OPT_PAM_PRUNE = 6
EK_OPT_STATE_EXACT = 7
EK_OPT_ADAPTIVE = 8
EK_OPT_PASS_FORM = 9
EK_OPT_FUSED_ROUNDS = 10
EK_OPT_TRIANGLE = 11
EK_OPT_PAM_ONE_WORKGROUP = 12
EK_OPT_PAM_MAX_PAIRS = 13
EK_OPT_PAM_BOTH_SUMS = 14
EK_OPT_FINE_PICK = 15
EK_OPT_PAM_BOUNDS = 16
EK_OPT_PICK_CAP = 17
EK_OPT_SMALL_SHARDS = 18
EK_OPT_PAM_AHEAD = 19
EK_OPT_PAM_ZERO_COPY = 20
EK_OPT_PAM_PAIRS_MFMA = 21
EK_OPT_PASS_SWEEP = 22
EK_OPT_MS_TWO_PHASE = 23
EK_OPT_ACTIVE_VIEW = 24
EK_OPT_VIEW_RHO = 25
EK_OPT_VIEW_RATIO = 26
OPTIONS = {k[7:].lower(): v for k, v in list(globals().items())
           if k.startswith("EK_OPT_")}


class HipLibraryMissing(RuntimeError):
    pass


class HipError(RuntimeError):
    pass


_lib = None


def load():
    """Load libenspara_hip.so (once).  Raises HipLibraryMissing if it has not
    been built (python -m enspara_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryMissing(
            "%s not found: the HIP extension is not built "
            "(run `python -m enspara_amd.build`); there is no CPU fallback."
            % LIB_PATH)
    if os.environ.get("ENSPARA_NO_TORCH") != "1":   # (measurement switch: the system's
        try:                                        # HIP runtime instead of torch's copy)
            import torch  # noqa: F401  (loads libamdhip64.so.7 first)
        except Exception:  # pragma: no cover - torch is plumbing, not required
            pass
    try:
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:
        raise HipLibraryMissing("cannot load %s: %s" % (LIB_PATH, e))
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    f32p, i32p, i64p = (C.POINTER(C.c_float), C.POINTER(C.c_int32),
                        C.POINTER(C.c_int64))
    L.ek_abi_version.restype = C.c_int
    L.ek_last_error.restype = C.c_char_p
    L.ek_device_count.restype = C.c_int
    L.ek_ctx_create.argtypes = [C.c_int, i64, i32, i64, vp, C.POINTER(vp)]
    L.ek_ctx_destroy.argtypes = [vp]
    L.ek_ctx_sync.argtypes = [vp]
    L.ek_ctx_stream.restype = vp
    L.ek_ctx_stream.argtypes = [vp]
    L.ek_load_frames.argtypes = [vp, vp, i64, i64, C.c_int]
    L.ek_rmsd_to_center.argtypes = [vp, i64, f32p, f32p]
    L.ek_state_reset.argtypes = [vp]
    L.ek_state_download.argtypes = [vp, f32p, i32p]
    L.ek_state_upload.argtypes = [vp, f32p, i32p]
    L.ek_record_bytes.restype = C.c_size_t
    L.ek_record_bytes.argtypes = [i32]
    L.ek_local_candidate.argtypes = [vp, vp]
    L.ek_own_record.restype = vp
    L.ek_own_record.argtypes = [vp]
    L.ek_kcenters_step.argtypes = [vp, vp, i32, i32, C.c_double, vp]
    L.ek_kcenters_run.argtypes = [vp, i32, i32, C.c_double, i32p, i64p, f32p, f32p]
    L.ek_history_download.argtypes = [vp, i32, i32, i64p, f32p, i32p]
    L.ek_history_reset.argtypes = [vp]
    L.ek_spec_candidates.argtypes = [vp]
    L.ek_round_candidates.argtypes = [vp]
    L.ek_quad_copy_ready.argtypes = [vp]
    L.ek_spec_begin.argtypes = [vp, i32, i32, vp]
    L.ek_spec_round.argtypes = [vp, vp, i32, C.c_double]
    L.ek_spec_localmax.argtypes = [vp, vp]
    L.ek_spec_apply.argtypes = [vp, vp, i32, C.c_double]
    L.ek_spec_chain_bytes.argtypes = [i32p, i32p]
    L.ek_spec_chain_rows.argtypes = [vp, vp]
    L.ek_spec_chain_max.argtypes = [vp, vp, i32, vp]
    L.ek_spec_chain_apply.argtypes = [vp, vp, i32, C.c_double]
    L.ek_spec_round_end.argtypes = [vp, vp]
    L.ek_spec_progress.argtypes = [vp, i32p, i32p]
    L.ek_spec_rounds.argtypes = [vp, i32p]
    L.ek_run_stats.argtypes = [vp, i64p, i64p]
    L.ek_ms_setup.argtypes = [vp, i32, i32, C.POINTER(C.c_size_t)]
    L.ek_ms_mailbox.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), vp, vp]
    L.ek_ms_connect.argtypes = [vp, i32, vp, vp, vp, vp]
    L.ek_ms_begin.argtypes = [vp, i32, i32]
    L.ek_ms_local.argtypes = [vp, C.c_double, vp]
    L.ek_ms_global.argtypes = [vp, C.c_double, vp]
    L.ek_ms_end.argtypes = [vp]
    L.ek_ms_state.argtypes = [vp, i32p, i32p, i32p]
    L.ek_ms_run.argtypes = [vp, i32, i32, C.c_double, i32p, i64p, f32p, f32p]
    L.ek_ti_stats.argtypes = [vp, i64p, i64p]
    L.ek_view_stats.argtypes = [vp, i64p]
    L.ek_last_run_form.argtypes = [vp, i64p]
    L.ek_view_layout_check.argtypes = [vp, f32, i64p]
    L.ek_assign_nearest.argtypes = [vp, f32p, i32]
    f64p = C.POINTER(C.c_double)
    L.ek_ms_diag.argtypes = [vp, i64p, f64p]
    L.ek_pam_begin.argtypes = [vp, i64p, i32]
    L.ek_pam_count_members.argtypes = [vp, i32, i64p]
    L.ek_pam_select_member.argtypes = [vp, i32, i64, i64p]
    L.ek_pam_propose.argtypes = [vp, i32, i64, f64p, f64p, i64p]
    L.ek_pam_propose_member.argtypes = [vp, i32, i64, i64p, f64p, f64p, i64p]
    L.ek_pam_commit.argtypes = [vp, C.c_int]
    L.ek_pam_count_members_batch.argtypes = [vp, i32, i32, i64p]
    L.ek_pam_select_members_batch.argtypes = [vp, i32, i32, i64p, i64p]
    L.ek_pam_prefetch.argtypes = [vp, i64p, i32]
    L.ek_pam_propose_ex.argtypes = [vp, i32, i64, i64, i32, i32, f64p, f64p,
                                    i64p, C.POINTER(C.c_uint32)]
    L.ek_pam_prefetch_stats.argtypes = [vp, i64p, i64p]
    L.ek_pam_window_run.argtypes = [vp, i32, i32, i64p, i64p, i32, i32, i32p, i32p,
                                    f64p, f64p, i64p]
    L.ek_pam_window_max.argtypes = []
    L.ek_pam_window_max.restype = i32
    L.ek_pam_prefetch_window.argtypes = [vp, i64p, i32, i32, i32]
    L.ek_pam_prefetch_passes.argtypes = [vp, i64p, i64p]
    L.ek_pam_sparse_stats.argtypes = [vp, i64p, i64p]
    L.ek_pam_ahead_stats.argtypes = [vp, i64p]
    L.ek_np_choice_draws.argtypes = [C.POINTER(C.c_uint32), i64, i64p, i64p, i64, i64p]
    L.ek_np_choice_draws.restype = i64
    L.ek_pam_sweep.argtypes = [vp, i32, i32, C.POINTER(C.c_uint32), i64, i64p, i64p, i32p, i64p,
                               i32p, f64p, f64p, i64p, i32p]
    L.ek_pam_prefetch_centers_window.argtypes = [vp, vp, vp, i32, i32, i32]
    L.ek_centered_frames.argtypes = [vp, i64p, i32p, i32, vp, vp]
    L.ek_pam_begin_table.argtypes = [vp, vp, vp, i32]
    L.ek_pam_prefetch_centers.argtypes = [vp, vp, vp, i32]
    L.ek_pam_propose_center.argtypes = [vp, i32, i32, vp, vp, i64, i32, i32, vp]
    L.ek_msm_counts.argtypes = [C.c_int, i32p, i64p, i64, i32, i32, i32, i64,
                                i32p, i32p, i64p, i64p]
    L.ek_msm_counts_ctx.argtypes = [vp, i64p, i64, i32, i32, i32, i64, i32p, i32p,
                                    i64p, i64p]
    L.ek_msm_row_normalize.argtypes = [C.c_int, i64p, f64p, i64, f64p, f64p]
    L.ek_msm_mle_prinz.argtypes = [C.c_int, i32, i64, i32, i64p, i32p, i32p, f64p,
                                   f64p, f64p, f64p, f64p, f64p, f64p, C.c_double,
                                   i64, i64p, f64p]
    L.ek_msm_bace_prune.argtypes = [C.c_int, i32, f64p, f64p, f32p]
    L.ek_msm_bace_run.argtypes = [C.c_int, i32, f64p, f64p, i32p, i32, i32, i32, vp,
                                  i32, f32p]
    L.ek_msm_boot_open.argtypes = [C.c_int, i32p, i64p, i64, i32, i32, i32, i64, i64p, i32p,
                                   i32, i32p, i32, C.POINTER(vp)]
    L.ek_msm_boot_fetch.argtypes = [vp, i32, i32, i64p]
    L.ek_msm_boot_build.argtypes = [vp, i64, i64p, i64p, i64p, f64p, f64p]
    L.ek_msm_boot_last_timing.argtypes = [vp, f64p]
    L.ek_msm_boot_close.argtypes = [vp]
    L.ek_lu_solve.argtypes = [C.c_int, i32, f64p, i32, f64p, f64p, i32p, i32p]
    L.ek_lu_set_timing.argtypes = [C.c_int]
    L.ek_lu_last_timing.argtypes = [f64p, f64p]
    L.ek_tpt_committors.argtypes = [C.c_int, i32, f64p, i32p, i32, i32p, i32, f64p, i32p]
    L.ek_tpt_mfpts_sinks.argtypes = [C.c_int, i32, f64p, i32p, i32, C.c_double, f64p, i32p]
    L.ek_tpt_mfpts_all.argtypes = [C.c_int, i32, f64p, f64p, C.c_double, f64p, i32p]
    L.ek_tpt_fluxes.argtypes = [C.c_int, i32, f64p, i32p, i32, i32p, i32, f64p, i32, f64p,
                                f64p, i32p]
    L.ek_tpt_paths_open.argtypes = [C.c_int, i32, f64p, i64p, i32p, f64p, i32p, i32, i32p, i32,
                                    i32, i64, C.c_double, C.c_double, i32, i32, i32p,
                                    C.POINTER(vp)]
    L.ek_tpt_paths_next.argtypes = [vp, i32p, i32p, f64p, i32p, i32p, i32p]
    L.ek_tpt_paths_stats.argtypes = [vp, i64p, f64p]
    L.ek_tpt_paths_close.argtypes = [vp]
    u8p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    L.ek_mi_open.argtypes = [C.c_int, i32, i32, i32, i32, C.POINTER(vp)]
    L.ek_mi_add.argtypes = [vp, u8p, u8p, i64]
    L.ek_mi_load_counts.argtypes = [vp, u32p, C.c_uint64]
    L.ek_mi_counts.argtypes = [vp, u32p]
    L.ek_mi_information.argtypes = [vp, f64p]
    L.ek_mi_last_timing.argtypes = [vp, f64p]
    L.ek_mi_close.argtypes = [vp]
    L.ek_cards_open.argtypes = [C.c_int, i32, i32, C.POINTER(vp)]
    L.ek_cards_add.argtypes = [vp, u8p, i64]
    L.ek_cards_stats.argtypes = [vp, i64p]
    L.ek_cards_disorder.argtypes = [vp, i64p, i64p]
    L.ek_cards_disorder_codes.argtypes = [vp, i32, u8p]
    L.ek_cards_matrices.argtypes = [vp, f64p]
    L.ek_cards_counts.argtypes = [vp, i32, u32p]
    L.ek_cards_last_timing.argtypes = [vp, f64p]
    L.ek_cards_close.argtypes = [vp]
    L.ek_cards_scan_chunk.argtypes = []
    L.ek_cards_scan_chunk.restype = C.c_int
    L.ek_sasa_open.argtypes = [C.c_int, i32, f32p, i32, f32p, i32, i32p, i32p, C.POINTER(vp)]
    L.ek_sasa_run.argtypes = [vp, f32p, i64, i64, i32p, f32p, f32p]
    L.ek_sasa_last_timing.argtypes = [vp, f64p]
    L.ek_sasa_close.argtypes = [vp]
    L.ek_rmsf_open.argtypes = [C.c_int, i32, i32, i32p, f32p, i32, i32p, i32p, C.POINTER(vp)]
    L.ek_rmsf_run.argtypes = [vp, f32p, i64, f64p, i64, i64, f32p, f64p, f32p,
                              C.POINTER(C.c_uint32)]
    L.ek_rmsf_fetch.argtypes = [vp, f64p, f64p]
    L.ek_rmsf_last_timing.argtypes = [vp, f64p]
    L.ek_rmsf_close.argtypes = [vp]
    L.ek_wmi_run.argtypes = [C.c_int, u8p, f64p, i64, i32, i32, f64p, f64p]
    L.ek_wmi_last_timing.argtypes = [f64p]
    L.ek_ent_kl_rows.argtypes = [C.c_int, i64, i64, f64p, f64p, f64p, u32p]
    L.ek_ent_js_rows.argtypes = [C.c_int, i64, i64, f64p, f64p, f64p, f64p, u32p]
    L.ek_ent_shannon_rows.argtypes = [C.c_int, i64, i64, f64p, i32, f64p]
    L.ek_ent_kl_counts.argtypes = [C.c_int, i32, f64p, i64, i32p, i32p, i64p, C.c_double,
                                   f64p, u32p]
    L.ek_ent_last_timing.argtypes = [f64p]
    L.ek_ent_state_counts_open.argtypes = [C.c_int, i32, i32, C.POINTER(vp)]
    L.ek_ent_state_counts_add.argtypes = [vp, u8p, i64]
    L.ek_ent_state_counts_read.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.ek_ent_state_counts_last_timing.argtypes = [vp, f64p]
    L.ek_ent_state_counts_close.argtypes = [vp]
    u64 = C.c_uint64
    L.ek_kmc_create.argtypes = [C.c_int, i32, i64p, i32p, f64p, C.POINTER(vp)]
    L.ek_kmc_destroy.argtypes = [vp]
    L.ek_kmc_next.argtypes = [vp, i64, i32p, f64p, i32p, i64p]
    L.ek_kmc_trajectories.argtypes = [vp, u64, i64, i64, i32p, i64, i32, i64, i32p, i64p]
    L.ek_kmc_ensemble.argtypes = [C.c_int, i32, f64p, i64p, i32p, f64p, f64p, i64, f64p,
                                  f64p, f64p]
    L.ek_kmc_fret_probs.argtypes = [C.c_int, u64, i64, i64, i32p, i32, i64p, f64p, f64p,
                                    C.c_double, C.c_double, f64p]
    L.ek_kmc_fret_bursts.argtypes = [vp, u64, i64, i64, i64p, i64p, f64p, i64p, f64p, f64p,
                                     C.c_double, C.c_double, i64, u8p, i32p, i64p]
    L.ek_kmc_last_timing.argtypes = [f64p]
    i8p = C.POINTER(C.c_int8)
    L.ek_dye_pair_create.argtypes = [C.c_int, i32, i64p, i64p, i32p, f64p, f64p, f64p, i64p,
                                     i64p, i32p, f64p, f64p, f64p, f64p, C.POINTER(vp)]
    L.ek_dye_pair_destroy.argtypes = [vp]
    L.ek_dye_pair_table.argtypes = [vp, i32, f64p, f64p, f64p, f64p]
    L.ek_dye_pair_resolve.argtypes = [vp, u64, i64, i64, i64, i64, i32p, i8p, i32p, i32p, i64,
                                      i64p, i64p]
    L.ek_dye_pair_static.argtypes = [vp, u64, i64, i64, f64p, i8p, i32p, i32p]
    L.ek_dye_pair_last_timing.argtypes = [f64p]
    L.ek_dye_bursts_lifetimes.argtypes = [vp, u64, i64, i64, i64p, i64p, f64p, i64p, f64p, u8p,
                                          i64, u8p, f64p, i32p, i32p, i64p, i64p]
    L.ek_dye_bursts_k2.argtypes = [vp, u64, i64, i64, i64p, i64p, f64p, i64p, f64p, i64p, f64p,
                                   C.c_double, i64, u8p, f64p, f64p, i32p, i32p, i32p, i32p,
                                   i64p, i64p]
    L.ek_dye_photons_lifetimes.argtypes = [C.c_int, u64, i64, i64, i32p, i32, i64p, f64p, u8p,
                                           u8p, f64p, i64p]
    L.ek_dye_photons_k2.argtypes = [C.c_int, u64, i64, i64, i32p, i32, i64p, f64p, i64p, f64p,
                                    C.c_double, u8p, f64p, f64p, i32p, i32p, i64p]
    L.ek_dye_pick_events.argtypes = [C.c_int, i64, i32p, f64p, i32, i64p, i64p, i64p]
    L.ek_dye_bursts_last_timing.argtypes = [f64p]
    L.ek_pockets_open.argtypes = [C.c_int, i32, f64p, C.c_double, i32, C.POINTER(vp)]
    L.ek_pockets_run.argtypes = [vp, f32p, i64, f32p, i32p, i64]
    L.ek_pockets_counts.argtypes = [vp, i64, i64p]
    L.ek_pockets_fetch.argtypes = [vp, i32p, i32p]
    L.ek_pockets_last_timing.argtypes = [vp, f64p]
    L.ek_pockets_close.argtypes = [vp]
    L.ek_pockets_touches.argtypes = [C.c_int, f32p, i32, f64p, C.c_double, f32p, i32p, u8p]
    L.ek_pockets_ranks.argtypes = [C.c_int, u8p, i32p, u8p]
    L.ek_pockets_labels.argtypes = [C.c_int, u8p, i32p, i32p]
    L.ek_dyes_open.argtypes = [C.c_int, i32, f64p, i32, f32p, i32, f32p, C.c_double,
                               C.POINTER(vp)]
    L.ek_dyes_run.argtypes = [vp, f32p, i64, f32p, i64]
    L.ek_dyes_counts.argtypes = [vp, i64, i32p, i32p]
    L.ek_dyes_fetch.argtypes = [vp, i64p]
    L.ek_dyes_last_timing.argtypes = [vp, f64p]
    L.ek_dyes_close.argtypes = [vp]
    L.ek_dyes_touches.argtypes = [C.c_int, f32p, i32, f64p, f32p, i32, u8p]
    L.ek_dyes_pair_hist.argtypes = [C.c_int, f32p, i32, f32p, i32, C.c_double, i32p, i64p]
    L.ek_dye_map_open.argtypes = [C.c_int, i32, f64p, i32, i32p, i32, i32, f32p, i32, i32p, i32p,
                                  i32, i32, i32, C.POINTER(vp)]
    L.ek_dye_map_max_centres.argtypes = [vp, i32, C.POINTER(i64)]
    L.ek_dye_map_run.argtypes = [vp, f32p, i64, i32]
    L.ek_dye_map_fetch.argtypes = [vp, i64, i32p, f64p, u8p, f32p]
    L.ek_dye_map_stats.argtypes = [vp, i64, i32p, f64p]
    L.ek_dye_map_last_timing.argtypes = [vp, f64p]
    L.ek_dye_map_close.argtypes = [vp]
    L.ek_rotamer_states.argtypes = [C.c_int, f32p, i64, i32, u8p, i32, i32p, f64p, f32p,
                                    C.c_double, u8p, f64p]
    L.ek_dihedral_angles.argtypes = [C.c_int, f32p, i64, i32, i32p, i32, f32p, f64p]
    L.ek_dihedral_rotamers.argtypes = [C.c_int, f32p, i64, i32, i32p, i32, u8p, i32, i32p,
                                       f64p, f32p, C.c_double, u8p, f32p, f64p]
    L.ek_krylov_create.argtypes = [C.c_int, i64, i64p, i32p, f64p, i32,
                                   C.POINTER(vp)]
    L.ek_krylov_destroy.argtypes = [vp]
    L.ek_krylov_set_vector.argtypes = [vp, i32, f64p]
    L.ek_krylov_get_vector.argtypes = [vp, i32, f64p]
    L.ek_krylov_step.argtypes = [vp, i32, i32, f64p]
    L.ek_krylov_set_filter.argtypes = [vp, i32, C.c_double, C.c_double]
    L.ek_krylov_rotate.argtypes = [vp, i32, i32, f64p, i32]
    L.ek_krylov_combine.argtypes = [vp, i32, i32, f64p, f64p]
    L.ek_krylov_expand.argtypes = [vp, i32, i32, f64p, i32]
    L.ek_feat_create.argtypes = [C.c_int, i64, i32, i32, C.POINTER(vp)]
    L.ek_feat_destroy.argtypes = [vp]
    L.ek_feat_load.argtypes = [vp, vp, i64, i64]
    L.ek_feat_distance.argtypes = [vp, i32, vp, f64p]
    L.ek_feat_pam_sweep.argtypes = [vp, i32, i32, i64p, i64p, C.POINTER(C.c_uint32), i64,
                                    i64p, f64p, i32p, i32p, i32p, i32p]
    L.ek_feat_pam_release.argtypes = [vp]
    L.ek_feat_pam_release.restype = None
    L.ek_feat_kcenters.argtypes = [vp, i32, i32, i32, C.c_double, f64p, i32p, i64p,
                                   i32p, f64p]
    L.ek_feat_record_bytes.restype = C.c_size_t
    L.ek_feat_record_bytes.argtypes = [i32, i32]
    L.ek_feat_create_sharded.argtypes = [C.c_int, i64, i32, i32, i64, vp,
                                         C.POINTER(vp)]
    L.ek_feat_state_reset.argtypes = [vp]
    L.ek_feat_state_upload.argtypes = [vp, f64p, i32p]
    L.ek_feat_state_download.argtypes = [vp, f64p, i32p]
    L.ek_feat_local_candidate.argtypes = [vp, vp]
    L.ek_feat_kcenters_step.argtypes = [vp, i32, vp, i32, i32, C.c_double, vp]
    L.ek_feat_history_download.argtypes = [vp, i32, i32, i64p, f64p, i32p]
    L.ek_feat_history_reset.argtypes = [vp]
    L.ek_feat_pam_count_batch.argtypes = [vp, i32, i32, i64p]
    L.ek_feat_pam_select_batch.argtypes = [vp, i32, i32, i64p, i64p]
    L.ek_feat_pam_gather_rows.argtypes = [vp, i32, i64p, i64p, vp]
    L.ek_feat_pam_begin.argtypes = [vp, i32, vp, i32]
    L.ek_feat_pam_propose.argtypes = [vp, i32, vp, i32, i32, vp]
    L.ek_feat_pam_commit.argtypes = [vp, i32]
    L.ek_feat_assign_nearest.argtypes = [vp, i32, vp, i32]
    L.ek_set_frames_per_lane.argtypes = [vp, C.c_int]
    L.ek_set_option.argtypes = [vp, i32, i32]
    L.ek_get_option.argtypes = [vp, i32, i32p]
    L.ek_reserve_centers.argtypes = [vp, i32]
    if os.environ.get("ENSPARA_HIP_LIB") is None or hasattr(L, "ek_debug_guards"):
        L.ek_debug_guards.argtypes = [vp]     # (a variant library from before it: tools/)
    L.ek_last_run_timing.argtypes = [vp, f32p, i32p]
    L.ek_timing_begin.argtypes = [vp, i32, i32]
    L.ek_timing_end.argtypes = [vp, f32p, i32p]
    L.ek_timing_form.argtypes = [vp, i32p]
    L.ek_hbm_copy_rate.argtypes = [C.c_int, C.c_size_t, f64p]
    L.ek_qcp_probe.argtypes = [C.c_int, vp, vp, vp, i32, vp, C.c_int64, vp, vp, vp]
    L.ek_pam_pairs_probe.argtypes = [C.c_int, i32, i32, vp, vp, i64, vp, vp, i32, i32, i32,
                                     i32, i32, vp, vp, vp, vp, vp, i64, i64, vp]
    L.ek_live_resources.argtypes = [i64p]
    L.ek_fail_alloc_at.argtypes = [i64]
    L.ek_fail_alloc_at.restype = i64
    for name in SYMBOLS:
        if name == "ek_debug_guards" and os.environ.get("ENSPARA_HIP_LIB"):
            continue        # (a variant library from before it: tools/)
        getattr(L, name)
    _lib = L
    return L


def check(rc):
    if rc != 0:
        msg = load().ek_last_error().decode("utf-8", "replace")
        raise HipError("enspara_hip error %d: %s" % (rc, msg))


LiveResources = collections.namedtuple(
    "LiveResources", ["dev_allocs", "dev_bytes", "pinned_allocs", "pinned_bytes",
                      "streams", "events", "dev_allocs_total"])


def live_resources():
    """What the library holds right now, counted inside it (ek_live_resources):
    live device / pinned allocations and their bytes, live streams and events,
    and the monotonic count of device allocations since it was loaded."""
    out = (C.c_int64 * 7)()
    check(load().ek_live_resources(out))
    return LiveResources(*[int(v) for v in out])


def fail_alloc_at(k):
    """Test aid (ek_fail_alloc_at): the k-th device allocation from now fails
    once, without touching the device; k < 0 disarms.  Returns the arm that was
    pending (-1: none)."""
    return int(load().ek_fail_alloc_at(int(k)))


def f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def f64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def i64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def u8p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def i8p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int8))


def u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))
