"""ctypes binding of libnlam_hip.so (the C-ABI declared in include/nlam_hip.h).

The shared library is built in-tree by ``__graft_entry__.build()`` /
``python -m neural_lam_amd.build``.  There is no CPU fallback: if the library is
missing, or a tensor is not on a HIP device, the product path raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

HERE = Path(__file__).resolve().parent
# NLAM_LIB lets the profiling tools load an instrumented build (tools/phase_timing.py); the product default is the in-tree library
LIB_PATH = Path(os.environ["NLAM_LIB"]) if os.environ.get("NLAM_LIB") else HERE / "libnlam_hip.so"

NLAM_MAX_SRC = 3
NLAM_MAX_CAT = 6
NLAM_MAX_REDUCE_JOBS = 40
NLAM_MAX_GROUP = 8
F_ADD_SRC0, F_ADD_SRC1, F_MEAN, F_SILU_B, F_PRE_ADD, F_LEAF_WGRAD, F_WPACK_READY, F_NO_ACT = 1, 2, 4, 8, 16, 32, 64, 128
F_STORE_BF16, F_A_BF16, F_S_BF16 = 1 << 10, 1 << 10, 1 << 11
F_ACC_DSRC0 = 1 << 12
F_WGRAD_SOLO = 1 << 13
TUNE_WBF_MIN_SUPERTILES = 1   # nlam_set_tuning keys (include/nlam_hip.h)
TUNE_WGRAD_CHUNKS = 2
TUNE_LIN_WGS = 3
TUNE_WGRAD_MIN_PARTS = 4
TUNE_WGRAD_BIG_MIN_ROWS = 5
TUNE_WBF_HALF = 6
TUNE_LIN_GEMM = 7
TUNE_WBF_V4 = 8
TUNE_WGRAD_LDMA = 9
TUNE_WGRAD_LDMA_VAR = 10
TUNE_WBF_EDGE = 11
TUNE_WGRAD_MAX_WGS = 12
TUNE_CHAIN_CUS = 13
TUNE_WGRAD_DMA_R = 14
# nlam_wgrad_plan codes (include/nlam_hip.h): the kernel family nlam_wgrad launches
WGP_SMALLN, WGP_DMA, WGP_NARROW, WGP_WIDE, WGP_WBF, WGP_WBF_BIG, WGP_WBF_B, WGP_WBF_B_BIG, WGP_LDMA_B, WGP_LDMA_1, WGP_LDMA_3 = range(1, 12)
# nlam_mlp_fwd_plan / nlam_mlp_bwd_plan codes (include/nlam_hip.h, NLAM_MLPP_*): the instantiation a narrow launch runs
MLPP_NOT_NARROW = 0
MLPP_FWD_GENERIC, MLPP_FWD_FAST, MLPP_FWD_BF = 1, 2, 3
MLPP_BWD_GENERIC, MLPP_BWD_FAST = 1, 2
MLPP_RAG, MLPP_RES, MLPP_PRE, MLPP_CAT, MLPP_EMPTY = 1 << 8, 1 << 9, 1 << 10, 1 << 11, 1 << 12


def mlpp_code(kernel, hb, ob, ns, bits=0):
    """NLAM_MLPP_CODE: kernel | HB | OB | executed term count, plus NLAM_MLPP_RAG / RES / PRE / CAT bits."""
    return kernel | (hb << 2) | (ob << 4) | (ns << 6) | bits


def mlpp_fields(code):
    """(kernel, HB, OB, NS, bits) of a plan code."""
    return code & 3, (code >> 2) & 3, (code >> 4) & 3, (code >> 6) & 3, code & ~0xFF


# nlam_mlp_fwd_wide_plan / nlam_mlp_bwd_wide_plan codes (include/nlam_hip.h, NLAM_MLPW_*): the instantiation a wide launch runs
MLPW_NOT_WIDE = 0
MLPW_WIDE, MLPW_WBF, MLPW_EDGE = 1, 2, 3
MLPW_V4, MLPW_SBF, MLPW_EMPTY = 1 << 13, 1 << 14, 1 << 15


def mlpw_code(kernel, ns=0, plan=0, nwv=0, fb=0, bits=0):
    """NLAM_MLPW_CODE: kernel | executed term count | plan | <NWV, FB>, plus the NLAM_MLPW_V4 / NLAM_MLPW_SBF bits."""
    return kernel | (ns << 2) | (plan << 4) | (nwv << 7) | (fb << 11) | bits


def mlpw_fields(code):
    """(kernel, NS, plan, NWV, FB, bits) of a wide plan code."""
    return code & 3, (code >> 2) & 3, (code >> 4) & 7, (code >> 7) & 15, (code >> 11) & 3, code & (MLPW_V4 | MLPW_SBF | MLPW_EMPTY)


# nlam_linear_plan codes (include/nlam_hip.h, NLAM_LINP_*): the instantiation an nlam_linear launch runs
LINP_BF, LINP_BFW, LINP_GEMM = 1, 2, 3
LINP_RESIDENT, LINP_TA, LINP_DUAL, LINP_EMPTY = 1 << 8, 1 << 14, 1 << 15, 1 << 16


def linp_bf(ns, kb, mb):
    """linear_bf_kernel<KB, MB, NS>"""
    return LINP_BF | (ns << 2) | (kb << 4) | (mb << 6)


def linp_bfw(ns, resident, dual=False):
    """linear_bfw_kernel<NS>, resident or streamed weight strip"""
    return LINP_BFW | (ns << 2) | (LINP_RESIDENT if resident else 0) | (LINP_DUAL if dual else 0)


def linp_gemm(ns, wn, sk, ta=False, dual=False):
    """linear_gemm_kernel<NS, WN, TA, SK>"""
    return LINP_GEMM | (ns << 2) | (wn << 9) | (sk << 11) | (LINP_TA if ta else 0) | (LINP_DUAL if dual else 0)


TILE_SPLIT = 1 << 30
# training-loss kinds (NLAM_LOSS_*), keyed by the reference's metric names (metrics.DEFINED_METRICS)
LOSS_KINDS = {"mse": 1, "mae": 2, "wmse": 3, "wmae": 4, "nll": 5, "crps_gauss": 6}
LOSS_MSE, LOSS_MAE, LOSS_WMSE, LOSS_WMAE, LOSS_NLL, LOSS_CRPS_GAUSS = 1, 2, 3, 4, 5, 6
LOSS_MAX_VARS = 4096
# NLAM_CLAMP_*: the output clamp of one state variable (nlam_step_tail_t.clamp_mode_host)
CLAMP_NONE, CLAMP_BOTH, CLAMP_LOWER, CLAMP_UPPER = 0, 1, 2, 3
EVAL_MAX_MAPS = 32    # NLAM_EVAL_MAX_MAPS: lead times of one nlam_eval_metrics call's loss maps
EVAL_MAX_VARS = 256   # NLAM_EVAL_MAX_VARS
ENS_MAX_MEMBERS = 64  # NLAM_ENS_MAX_MEMBERS: members of one nlam_ens_scores call
ENS_MAX_EVENTS = 32   # NLAM_ENS_MAX_EVENTS: threshold events of one nlam_ens_products call
ENS_MAX_QUANTILES = 16   # NLAM_ENS_MAX_QUANTILES: quantile levels of one nlam_ens_products call
NBR_MAX_SCALES = 8    # NLAM_NBR_MAX_SCALES: window radii of one nlam_ens_neighbourhood call
SPEC_MAX_SOURCES = 3  # NLAM_SPEC_MAX_SOURCES: sources of one nlam_dct_spectra call
MOMENTS_MAX_VARS = 256   # NLAM_MOMENTS_MAX_VARS: features of one nlam_window_moments call
# learning-rate schedules of nlam_adamw_step_controlled (NLAM_SCHED_*) and the words of its control block
SCHED_KINDS = {"constant": 1, "warmup_cosine": 2, "warmup_linear": 3}
SCHED_NONE = 0
OPTCTL_WORDS = 8
OPTCTL_LR, OPTCTL_COEF, OPTCTL_NORM, OPTCTL_SKIP, OPTCTL_SKIPPED = range(5)
# the words of nlam_accum_t.accum (gradient accumulation: nlam_accum_begin, nlam_adamw_step_accum)
ACCUM_WORDS = 4
ACCUM_INDEX, ACCUM_HOLD, ACCUM_LOSS_SUM, ACCUM_WINDOW_LOSS = range(4)

EXPORTS = [
    "nlam_abi_version",
    "nlam_grid_waves",
    "nlam_num_blocks",
    "nlam_max_width",
    "nlam_set_tuning",
    "nlam_affine_mix",
    "nlam_mlp_fwd_wpack_floats",
    "nlam_mlp_bwd_wpack_floats",
    "nlam_mlp_bwd_blocks",
    "nlam_mlp_bwd_dz2_ld",
    "nlam_wgrad_nparts",
    "nlam_wgrad_plan",
    "nlam_mlp_fwd_plan",
    "nlam_mlp_bwd_plan",
    "nlam_mlp_fwd_wide_plan",
    "nlam_mlp_bwd_wide_plan",
    "nlam_mlp_fwd",
    "nlam_mlp_bwd",
    "nlam_mlp_fwd_gemm_workspace_floats",
    "nlam_mlp_bwd_gemm_workspace_floats",
    "nlam_mlp_bwd_gemm_blocks",
    "nlam_mlp_fwd_gemm",
    "nlam_mlp_bwd_gemm",
    "nlam_mlp_pack_floats",
    "nlam_mlp_pack",
    "nlam_mlp_fwd_pack_records",
    "nlam_mlp_bwd_pack_records",
    "nlam_pack_records",
    "nlam_wgrad",
    "nlam_segment_sum",
    "nlam_segment_sum_acc",
    "nlam_segment_sum_add",
    "nlam_split_combine",
    "nlam_segment_sum_bf16",
    "nlam_store_bf16_supported",
    "nlam_reduce_partials",
    "nlam_reduce_jobs",
    "nlam_reduce_jobs_waves",
    "nlam_wmse_fwd",
    "nlam_wmse_bwd",
    "nlam_adamw_step",
    "nlam_adamw_step_resident",
    "nlam_standardize",
    "nlam_mlp_group_blocks",
    "nlam_mlp_fwd_group",
    "nlam_mlp_bwd_group",
    "nlam_mlp_fwd_family",
    "nlam_mlp_bwd_family",
    "nlam_mlp_bwd_group_blocks",
    "nlam_wgrad_group",
    "nlam_wgrad_dma_group",
    "nlam_wgrad_dma_group_supported",
    "nlam_linear",
    "nlam_linear_plan",
    "nlam_segment_sum_groups",
    "nlam_pre_add_supported",
    "nlam_step_tail_fwd",
    "nlam_step_tail_bwd",
    "nlam_loss_fwd",
    "nlam_loss_bwd",
    "nlam_step_tail_loss_fwd",
    "nlam_step_tail_loss_bwd",
    "nlam_step_tail_ext_fwd",
    "nlam_step_tail_ext_bwd",
    "nlam_eval_metrics",
    "nlam_eval_workspace_floats",
    "nlam_concat",
    "nlam_window_len",
    "nlam_window_batch",
    "nlam_window_batch_ens",
    "nlam_window_moments",
    "nlam_moments_workspace_doubles",
    "nlam_grad_sumsq_workspace_doubles",
    "nlam_grad_sumsq",
    "nlam_adamw_step_controlled",
    "nlam_accum_begin",
    "nlam_adamw_step_accum",
    "nlam_adamw_step_resident_ema",
    "nlam_adamw_step_controlled_ema",
    "nlam_flat_swap",
    "nlam_forecast_init",
    "nlam_forecast_head",
    "nlam_forecast_tail",
    "nlam_forecast_finish",
    "nlam_forecast_workspace_floats",
    "nlam_forecast_init_strided",
    "nlam_forecast_head_strided",
    "nlam_philox_normal_fill",
    "nlam_latent_sample",
    "nlam_ens_scores",
    "nlam_ens_scores_workspace_floats",
    "nlam_ens_products",
    "nlam_ens_products_workspace_floats",
    "nlam_ens_neighbourhood",
    "nlam_ens_neighbourhood_workspace_floats",
    "nlam_dct_spectra",
    "nlam_dct_spectra_workspace_floats",
    "nlam_latent_kl_fwd",
    "nlam_latent_kl_bwd",
    "nlam_latent_kl_workspace_floats",
    "nlam_latent_draw_fwd",
    "nlam_latent_draw_bwd",
    "nlam_crps_ens_fwd",
    "nlam_crps_ens_bwd",
    "nlam_crps_ens_workspace_floats",
    "nlam_series_range_workspace_words",
    "nlam_series_range",
    "nlam_series_pack_q16",
    "nlam_window_batch_q16",
    "nlam_window_moments_q16",
    "nlam_forecast_init_q16",
    "nlam_forecast_head_q16",
]


class Src(C.Structure):
    _fields_ = [
        ("ptr", C.c_void_p),
        ("idx", C.c_void_p),
        ("bstride", C.c_int64),
        ("width", C.c_int32),
        ("_pad", C.c_int32),
    ]


class MlpFwd(C.Structure):
    _fields_ = [
        ("src", Src * NLAM_MAX_SRC),
        ("nsrc", C.c_int32),
        ("batch", C.c_int32),
        ("rows", C.c_int32),
        ("ntiles", C.c_int32),
        ("tiles", C.c_void_p),
        ("W1", C.c_void_p),
        ("b1", C.c_void_p),
        ("W2", C.c_void_p),
        ("b2", C.c_void_p),
        ("ln_w", C.c_void_p),
        ("ln_b", C.c_void_p),
        ("eps", C.c_float),
        ("hid", C.c_int32),
        ("dout", C.c_int32),
        ("flags", C.c_uint32),
        ("out", C.c_void_p),
        ("out_idx", C.c_void_p),
        ("out_bstride", C.c_int64),
        ("aggr", C.c_void_p),
        ("rowptr", C.c_void_p),
        ("inv_deg", C.c_void_p),
        ("nseg_total", C.c_int32),
        ("ldw1", C.c_int32),
        ("z1", C.c_void_p),
        ("xhat", C.c_void_p),
        ("rstd", C.c_void_p),
        ("wpack", C.c_void_p),
        ("wpack_floats", C.c_int64),
        ("ncat", C.c_int32),
        ("_pad3", C.c_int32),
        ("cat_ptr", C.c_void_p * NLAM_MAX_CAT),
        ("cat_bstride", C.c_int64 * NLAM_MAX_CAT),
        ("cat_width", C.c_int32 * NLAM_MAX_CAT),
        ("cat_out", C.c_void_p),
    ]


class MlpBwd(C.Structure):
    _fields_ = [
        ("src", Src * NLAM_MAX_SRC),
        ("nsrc", C.c_int32),
        ("batch", C.c_int32),
        ("rows", C.c_int32),
        ("ntiles", C.c_int32),
        ("tiles", C.c_void_p),
        ("W1", C.c_void_p),
        ("W2", C.c_void_p),
        ("ln_w", C.c_void_p),
        ("hid", C.c_int32),
        ("dout", C.c_int32),
        ("flags", C.c_uint32),
        ("nseg_total", C.c_int32),
        ("g_out", C.c_void_p),
        ("out_idx", C.c_void_p),
        ("out_bstride", C.c_int64),
        ("g_aggr", C.c_void_p),
        ("seg_of_row", C.c_void_p),
        ("rowptr", C.c_void_p),
        ("inv_deg", C.c_void_p),
        ("z1", C.c_void_p),
        ("xhat", C.c_void_p),
        ("rstd", C.c_void_p),
        ("dz1", C.c_void_p),
        ("dz2", C.c_void_p),
        ("dsrc", C.c_void_p * NLAM_MAX_SRC),
        ("dsrc_bstride", C.c_int64 * NLAM_MAX_SRC),
        ("dmode", C.c_int32 * NLAM_MAX_SRC),
        ("ldw1", C.c_int32),
        ("vec_partials", C.c_void_p),
        ("vec_partials_rows", C.c_int32),
        ("vec_stride", C.c_int32),
        ("wpack", C.c_void_p),
        ("wpack_floats", C.c_int64),
        ("b1", C.c_void_p),
        ("dz2_ld", C.c_int32),
        ("_pad2", C.c_int32),
    ]


class Wgrad(C.Structure):
    _fields_ = [
        ("A", C.c_void_p),
        ("m", C.c_int32),
        ("batch", C.c_int32),
        ("rows", C.c_int32),
        ("nsrc", C.c_int32),
        ("src", Src * NLAM_MAX_SRC),
        ("flags", C.c_uint32),
        ("n", C.c_int32),
        ("partials", C.c_void_p),
        ("nparts", C.c_int32),
        ("_pad", C.c_int32),
    ]


class ReduceJob(C.Structure):
    _fields_ = [
        ("partials", C.c_void_p),
        ("out", C.c_void_p),
        ("stride", C.c_int64),
        ("nparts", C.c_int32),
        ("n", C.c_int32),
        ("accumulate", C.c_int32),
        ("ncols", C.c_int32),
        ("ld", C.c_int32),
        ("_pad", C.c_int32),
    ]


class ReduceJobs(C.Structure):
    _fields_ = [("job", ReduceJob * NLAM_MAX_REDUCE_JOBS), ("njobs", C.c_int32), ("_pad", C.c_int32)]


class Linear(C.Structure):
    _fields_ = [
        ("x", C.c_void_p),
        ("W", C.c_void_p),
        ("out", C.c_void_p),
        ("rows", C.c_int64),
        ("ldn", C.c_int64),
        ("ldk", C.c_int64),
        ("k", C.c_int32),
        ("n", C.c_int32),
        ("accumulate", C.c_int32),
        ("flags", C.c_uint32),
        ("W2", C.c_void_p),
        ("out2", C.c_void_p),
    ]


class Cat(C.Structure):
    _fields_ = [
        ("ptr", C.c_void_p * 6),
        ("bstride", C.c_int64 * 6),
        ("width", C.c_int32 * 6),
        ("nsrc", C.c_int32),
        ("batch", C.c_int32),
        ("nodes", C.c_int32),
        ("_pad", C.c_int32),
        ("out", C.c_void_p),
    ]


class Window(C.Structure):
    _fields_ = [
        ("state", C.c_void_p),
        ("forcing", C.c_void_p),
        ("times", C.c_void_p),
        ("sample_idx", C.c_void_p),
        ("init_states", C.c_void_p),
        ("target_states", C.c_void_p),
        ("forcing_windowed", C.c_void_p),
        ("target_times", C.c_void_p),
        ("state_mean", C.c_void_p),
        ("state_std", C.c_void_p),
        ("forcing_mean", C.c_void_p),
        ("forcing_std", C.c_void_p),
        ("n_times", C.c_int64),
        ("nodes", C.c_int32),
        ("d_state", C.c_int32),
        ("d_forcing", C.c_int32),
        ("batch", C.c_int32),
        ("ar_steps", C.c_int32),
        ("num_past_forcing_steps", C.c_int32),
        ("num_future_forcing_steps", C.c_int32),
        ("_pad", C.c_int32),
    ]


class Forecast(C.Structure):
    """nlam_forecast_t: one recorded AR step replayed per lead time; ``clamp_mode_host`` points at HOST memory."""
    _fields_ = [
        ("state", C.c_void_p),
        ("forcing", C.c_void_p),
        ("times", C.c_void_p),
        ("start", C.c_void_p),
        ("lead", C.c_void_p),
        ("state_mean", C.c_void_p),
        ("state_std", C.c_void_p),
        ("forcing_mean", C.c_void_p),
        ("forcing_std", C.c_void_p),
        ("prev", C.c_void_p),
        ("prev_prev", C.c_void_p),
        ("forcing_windowed", C.c_void_p),
        ("truth", C.c_void_p),
        ("delta", C.c_void_p),
        ("dstd", C.c_void_p),
        ("dmean", C.c_void_p),
        ("bmask", C.c_void_p),
        ("row_weight", C.c_void_p),
        ("clamp_mode_host", C.c_void_p),
        ("clamp_lo", C.c_void_p),
        ("clamp_hi", C.c_void_p),
        ("out_state", C.c_void_p),
        ("out_std", C.c_void_p),
        ("valid_times", C.c_void_p),
        ("sq", C.c_void_p),
        ("ab", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_floats", C.c_int64),
        ("n_times", C.c_int64),
        ("nodes", C.c_int32),
        ("d_state", C.c_int32),
        ("d_forcing", C.c_int32),
        ("batch", C.c_int32),
        ("max_lead", C.c_int32),
        ("num_past_forcing_steps", C.c_int32),
        ("num_future_forcing_steps", C.c_int32),
        ("delta_ld", C.c_int32),
    ]


class ForecastSrc(C.Structure):
    """nlam_forecast_src_t: the strided (forecast / ensemble) series nlam_forecast_init_strided / _head_strided read."""
    _fields_ = [
        ("state", C.c_void_p),
        ("forcing", C.c_void_p),
        ("sample_idx", C.c_void_p),
        ("state_stride_sample", C.c_int64),
        ("state_stride_step", C.c_int64),
        ("state_stride_member", C.c_int64),
        ("forcing_stride_sample", C.c_int64),
        ("forcing_stride_step", C.c_int64),
        ("forcing_stride_member", C.c_int64),
        ("n_times", C.c_int64),
        ("state_steps", C.c_int32),
        ("forcing_steps", C.c_int32),
        ("is_forecast", C.c_int32),
        ("members", C.c_int32),
    ]


class LatentSample(C.Structure):
    """nlam_latent_sample_t: the reparameterised draw of one lead for every batch item of an ensemble forecast."""

    _fields_ = [
        ("params", C.c_void_p),
        ("noise_in", C.c_void_p),
        ("noise_out", C.c_void_p),
        ("latent", C.c_void_p),
        ("start", C.c_void_p),
        ("lead", C.c_void_p),
        ("seed", C.c_void_p),
        ("batch", C.c_int32),
        ("members", C.c_int32),
        ("rows", C.c_int32),
        ("latent_dim", C.c_int32),
        ("diagonal", C.c_int32),
        ("max_lead", C.c_int32),
    ]


class EnsScores(C.Structure):
    """nlam_ens_scores_t: the ensemble verification of one lead."""

    _fields_ = [
        ("prev", C.c_void_p),
        ("truth", C.c_void_p),
        ("row_weight", C.c_void_p),
        ("state_mean", C.c_void_p),
        ("state_std", C.c_void_p),
        ("lead", C.c_void_p),
        ("ens_sq", C.c_void_p),
        ("ens_var", C.c_void_p),
        ("ens_abs", C.c_void_p),
        ("ens_pair", C.c_void_p),
        ("rank_hist", C.c_void_p),
        ("out_mean", C.c_void_p),
        ("out_spread", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_floats", C.c_int64),
        ("starts", C.c_int32),
        ("members", C.c_int32),
        ("nodes", C.c_int32),
        ("d_state", C.c_int32),
        ("max_lead", C.c_int32),
        ("_pad", C.c_int32),
    ]


class EnsProducts(C.Structure):
    """nlam_ens_products_t: exceedance probabilities, quantile fields and their scores of one lead."""

    _fields_ = [
        ("prev", C.c_void_p),
        ("truth", C.c_void_p),
        ("row_weight", C.c_void_p),
        ("state_mean", C.c_void_p),
        ("state_std", C.c_void_p),
        ("lead", C.c_void_p),
        ("event_var", C.c_void_p),
        ("event_sense", C.c_void_p),
        ("event_thr", C.c_void_p),
        ("q_index", C.c_void_p),
        ("q_frac", C.c_void_p),
        ("q_level", C.c_void_p),
        ("prob", C.c_void_p),
        ("quant", C.c_void_p),
        ("brier", C.c_void_p),
        ("rel_count", C.c_void_p),
        ("rel_obs", C.c_void_p),
        ("pinball", C.c_void_p),
        ("below", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_floats", C.c_int64),
        ("starts", C.c_int32),
        ("members", C.c_int32),
        ("nodes", C.c_int32),
        ("d_state", C.c_int32),
        ("max_lead", C.c_int32),
        ("events", C.c_int32),
        ("quantiles", C.c_int32),
        ("_pad", C.c_int32),
    ]


class EnsNeighbourhood(C.Structure):
    """nlam_ens_neighbourhood_t: neighbourhood probabilities and the sums of the fractions skill score of one lead."""

    _fields_ = [
        ("prev", C.c_void_p),
        ("truth", C.c_void_p),
        ("row_weight", C.c_void_p),
        ("lead", C.c_void_p),
        ("event_var", C.c_void_p),
        ("event_sense", C.c_void_p),
        ("event_thr", C.c_void_p),
        ("radius", C.c_void_p),
        ("nprob", C.c_void_p),
        ("fbs", C.c_void_p),
        ("fbs_ref", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_floats", C.c_int64),
        ("starts", C.c_int32),
        ("members", C.c_int32),
        ("nx", C.c_int32),
        ("ny", C.c_int32),
        ("d_state", C.c_int32),
        ("max_lead", C.c_int32),
        ("events", C.c_int32),
        ("scales", C.c_int32),
    ]


class DctSpectraSrc(C.Structure):
    """nlam_dct_spectra_src_t: one source of nlam_dct_spectra."""

    _fields_ = [
        ("x", C.c_void_p),
        ("spec", C.c_void_p),
        ("batch_stride", C.c_int64),
        ("lead_stride", C.c_int64),
        ("batch", C.c_int32),
        ("physical", C.c_int32),
    ]


class DctSpectra(C.Structure):
    """nlam_dct_spectra_t: binned DCT variance spectra of up to SPEC_MAX_SOURCES sources of one lead."""

    _fields_ = [
        ("src", DctSpectraSrc * SPEC_MAX_SOURCES),
        ("origin", C.c_void_p),
        ("basis_x", C.c_void_p),
        ("basis_y", C.c_void_p),
        ("var", C.c_void_p),
        ("bin_ptr", C.c_void_p),
        ("bin_idx", C.c_void_p),
        ("state_std", C.c_void_p),
        ("lead", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_floats", C.c_int64),
        ("sources", C.c_int32),
        ("nx", C.c_int32),
        ("ny", C.c_int32),
        ("d_state", C.c_int32),
        ("vars", C.c_int32),
        ("bins", C.c_int32),
        ("bin_entries", C.c_int32),
        ("max_lead", C.c_int32),
        ("cx", C.c_int32),
        ("cy", C.c_int32),
    ]


class LatentKl(C.Structure):
    """nlam_latent_kl_t: the posterior draw and the KL term of one AR step of the Graph-EFM training objective."""

    _fields_ = [
        ("pq", C.c_void_p),
        ("pp", C.c_void_p),
        ("noise_in", C.c_void_p),
        ("kl_weight", C.c_void_p),
        ("seed", C.c_void_p),
        ("draw", C.c_void_p),
        ("eps", C.c_void_p),
        ("latent", C.c_void_p),
        ("kl", C.c_void_p),
        ("kl_term", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_floats", C.c_int64),
        ("g_latent", C.c_void_p),
        ("g_kl_term", C.c_void_p),
        ("g_pq", C.c_void_p),
        ("g_pp", C.c_void_p),
        ("batch", C.c_int32),
        ("rows", C.c_int32),
        ("latent_dim", C.c_int32),
        ("diagonal", C.c_int32),
        ("t", C.c_int32),
        ("_pad", C.c_int32),
    ]


class LatentDraw(C.Structure):
    """nlam_latent_draw_t: the prior draw of one AR step of the member rollout, with its gradient."""

    _fields_ = [
        ("params", C.c_void_p),
        ("noise_in", C.c_void_p),
        ("seed", C.c_void_p),
        ("draw", C.c_void_p),
        ("eps", C.c_void_p),
        ("latent", C.c_void_p),
        ("g_latent", C.c_void_p),
        ("g_params", C.c_void_p),
        ("batch", C.c_int32),
        ("rows", C.c_int32),
        ("latent_dim", C.c_int32),
        ("diagonal", C.c_int32),
        ("t", C.c_int32),
        ("_pad", C.c_int32),
    ]


class CrpsEns(C.Structure):
    """nlam_crps_ens_t: the unbiased ensemble CRPS of one AR step of the member rollout."""

    _fields_ = [
        ("pred", C.c_void_p),
        ("target", C.c_void_p),
        ("row_weight", C.c_void_p),
        ("var_weight", C.c_void_p),
        ("weight", C.c_void_p),
        ("crps", C.c_void_p),
        ("term", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_floats", C.c_int64),
        ("g_term", C.c_void_p),
        ("g_pred", C.c_void_p),
        ("batch", C.c_int32),
        ("members", C.c_int32),
        ("nodes", C.c_int32),
        ("nvars", C.c_int32),
    ]


CRPS_MAX_MEMBERS = 16   # NLAM_CRPS_MAX_MEMBERS


class WindowEns(C.Structure):
    """nlam_window_ens_t: the window batch over strided (forecast / ensemble) series."""
    _fields_ = [
        ("state", C.c_void_p),
        ("forcing", C.c_void_p),
        ("times", C.c_void_p),
        ("elapsed", C.c_void_p),
        ("sample_idx", C.c_void_p),
        ("init_states", C.c_void_p),
        ("target_states", C.c_void_p),
        ("forcing_windowed", C.c_void_p),
        ("target_times", C.c_void_p),
        ("state_mean", C.c_void_p),
        ("state_std", C.c_void_p),
        ("forcing_mean", C.c_void_p),
        ("forcing_std", C.c_void_p),
        ("state_stride_sample", C.c_int64),
        ("state_stride_step", C.c_int64),
        ("state_stride_member", C.c_int64),
        ("forcing_stride_sample", C.c_int64),
        ("forcing_stride_step", C.c_int64),
        ("forcing_stride_member", C.c_int64),
        ("n_times", C.c_int64),
        ("state_steps", C.c_int32),
        ("forcing_steps", C.c_int32),
        ("is_forecast", C.c_int32),
        ("members", C.c_int32),
        ("nodes", C.c_int32),
        ("d_state", C.c_int32),
        ("d_forcing", C.c_int32),
        ("batch", C.c_int32),
        ("ar_steps", C.c_int32),
        ("num_past_forcing_steps", C.c_int32),
        ("num_future_forcing_steps", C.c_int32),
        ("_pad", C.c_int32),
    ]


class Moments(C.Structure):
    """nlam_moments_t: per-sample means and second moments of a strided resident series."""
    _fields_ = [
        ("series", C.c_void_p),
        ("mean", C.c_void_p),
        ("std", C.c_void_p),
        ("workspace", C.c_void_p),
        ("out_mean", C.c_void_p),
        ("out_sq", C.c_void_p),
        ("workspace_doubles", C.c_int64),
        ("stride_sample", C.c_int64),
        ("stride_step", C.c_int64),
        ("stride_member", C.c_int64),
        ("n_times", C.c_int64),
        ("first", C.c_int64),
        ("count", C.c_int64),
        ("is_forecast", C.c_int32),
        ("members", C.c_int32),
        ("steps", C.c_int32),
        ("nodes", C.c_int32),
        ("nvars", C.c_int32),
        ("row_begin", C.c_int32),
        ("nrows", C.c_int32),
        ("step", C.c_int32),
    ]


class Q16Src(C.Structure):
    """nlam_q16_src_t: the packed int16 series of a _q16 entry and their decode tables (a NULL series is read as fp32)."""
    _fields_ = [
        ("state", C.c_void_p),
        ("forcing", C.c_void_p),
        ("state_scale", C.c_void_p),
        ("state_offset", C.c_void_p),
        ("forcing_scale", C.c_void_p),
        ("forcing_offset", C.c_void_p),
    ]


class Loss(C.Structure):
    _fields_ = [
        ("pred", C.c_void_p),
        ("target", C.c_void_p),
        ("std", C.c_void_p),
        ("var_std", C.c_void_p),
        ("row_weight", C.c_void_p),
        ("gscalar", C.c_void_p),
        ("partials", C.c_void_p),
        ("dpred", C.c_void_p),
        ("dstd", C.c_void_p),
        ("rows", C.c_int64),
        ("nodes", C.c_int32),
        ("nvars", C.c_int32),
        ("kind", C.c_int32),
        ("nparts", C.c_int32),
        ("scale", C.c_float),
        ("_pad", C.c_int32),
    ]


class StepTail(C.Structure):
    """nlam_step_tail_t; ``clamp_mode_host`` points at HOST memory (an ``(C.c_int32 * nvars)`` array the caller keeps alive)."""

    _fields_ = [
        ("delta", C.c_void_p),
        ("prev", C.c_void_p),
        ("truth", C.c_void_p),
        ("target", C.c_void_p),
        ("dstd", C.c_void_p),
        ("dmean", C.c_void_p),
        ("bmask", C.c_void_p),
        ("row_weight", C.c_void_p),
        ("consts", C.c_void_p),
        ("clamp_mode_host", C.c_void_p),
        ("clamp_lo", C.c_void_p),
        ("clamp_hi", C.c_void_p),
        ("pred", C.c_void_p),
        ("pred_std", C.c_void_p),
        ("partials", C.c_void_p),
        ("g_pred", C.c_void_p),
        ("g_std", C.c_void_p),
        ("gloss", C.c_void_p),
        ("d_delta", C.c_void_p),
        ("d_prev", C.c_void_p),
        ("rows", C.c_int64),
        ("nodes", C.c_int32),
        ("nvars", C.c_int32),
        ("delta_ld", C.c_int32),
        ("kind", C.c_int32),
        ("nparts", C.c_int32),
        ("scale", C.c_float),
    ]


class Eval(C.Structure):
    _fields_ = [
        ("pred", C.c_void_p),
        ("target", C.c_void_p),
        ("std", C.c_void_p),
        ("var_std", C.c_void_p),
        ("row_weight", C.c_void_p),
        ("workspace", C.c_void_p),
        ("step_loss", C.c_void_p),
        ("sq", C.c_void_p),
        ("ab", C.c_void_p),
        ("std_mean", C.c_void_p),
        ("maps", C.c_void_p),
        ("workspace_floats", C.c_int64),
        ("batch", C.c_int32),
        ("steps", C.c_int32),
        ("nodes", C.c_int32),
        ("nvars", C.c_int32),
        ("kind", C.c_int32),
        ("nmaps", C.c_int32),
        ("map_steps", C.c_int32 * EVAL_MAX_MAPS),
    ]


class StdJob(C.Structure):
    _fields_ = [
        ("x", C.c_void_p),
        ("out", C.c_void_p),
        ("mean", C.c_void_p),
        ("std", C.c_void_p),
        ("rows", C.c_int64),
        ("width", C.c_int32),
        ("rep", C.c_int32),
    ]


class StdJobs(C.Structure):
    _fields_ = [("job", StdJob * 4), ("njobs", C.c_int32), ("_pad", C.c_int32)]


class PackJob(C.Structure):
    _fields_ = [
        ("W1", C.c_void_p),
        ("W2", C.c_void_p),
        ("fwd_image", C.c_void_p),
        ("bwd_image", C.c_void_p),
        ("hid", C.c_int32),
        ("dout", C.c_int32),
        ("nsrc", C.c_int32),
        ("ldw1", C.c_int32),
        ("width", C.c_int32 * NLAM_MAX_SRC),
        ("flags", C.c_uint32),
    ]


class OptCtl(C.Structure):
    """nlam_optctl_t: the AdamW update with norm, clipping, schedule and skip decided on the device."""
    _fields_ = [
        ("param", C.c_void_p),
        ("grad", C.c_void_p),
        ("exp_avg", C.c_void_p),
        ("exp_avg_sq", C.c_void_p),
        ("step_count_dev", C.c_void_p),
        ("bias_corr_dev", C.c_void_p),
        ("partials", C.c_void_p),
        ("control", C.c_void_p),
        ("n", C.c_int64),
        ("partials_doubles", C.c_int64),
        ("lr", C.c_float),
        ("beta1", C.c_float),
        ("beta2", C.c_float),
        ("eps", C.c_float),
        ("weight_decay", C.c_float),
        ("grad_scale", C.c_float),
        ("max_grad_norm", C.c_float),
        ("min_ratio", C.c_float),
        ("schedule", C.c_int32),
        ("warmup_steps", C.c_int32),
        ("total_steps", C.c_int32),
        ("skip_nonfinite", C.c_int32),
    ]


class Accum(C.Structure):
    """nlam_accum_t: the device block that gates the step's head and tail, this micro-batch's loss, the window length K."""
    _fields_ = [("accum", C.c_void_p), ("loss", C.c_void_p), ("steps", C.c_int32)]


class Ema(C.Structure):
    """nlam_ema_t: the moving average of the weights kept by the AdamW update launch (buffer, decay, first averaged update)."""
    _fields_ = [("ema", C.c_void_p), ("decay", C.c_float), ("start_step", C.c_int32)]


class PackRec(C.Structure):
    _fields_ = [("bytes", C.c_ubyte * 64)]


ABI_VERSION = 8
_lib = None


def lib_path() -> Path:
    return LIB_PATH


def load():
    """dlopen the in-tree library once; fail loudly if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()').  "
            "neural_lam_amd has no CPU / eager fallback."
        )
    import torch  # noqa: F401  (loads torch's libamdhip64.so.7 first so both share one HIP runtime)

    lib = C.CDLL(str(LIB_PATH))
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise RuntimeError(f"{LIB_PATH} does not export {name}")
    i32, i64, vp, f32 = C.c_int32, C.c_int64, C.c_void_p, C.c_float
    lib.nlam_abi_version.restype = i32
    lib.nlam_grid_waves.restype = i32
    lib.nlam_max_width.restype = i32
    lib.nlam_affine_mix.restype = i32
    lib.nlam_affine_mix.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, vp]
    lib.nlam_set_tuning.restype = i32
    lib.nlam_set_tuning.argtypes = [i32, i32]
    lib.nlam_num_blocks.argtypes = [i64]
    lib.nlam_num_blocks.restype = i32
    lib.nlam_mlp_fwd_wpack_floats.argtypes = [C.POINTER(MlpFwd)]
    lib.nlam_mlp_fwd_wpack_floats.restype = i64
    lib.nlam_mlp_bwd_wpack_floats.argtypes = [C.POINTER(MlpBwd)]
    lib.nlam_mlp_bwd_wpack_floats.restype = i64
    lib.nlam_mlp_bwd_dz2_ld.argtypes = [C.POINTER(MlpBwd)]
    lib.nlam_mlp_bwd_dz2_ld.restype = i32
    lib.nlam_mlp_bwd_blocks.argtypes = [C.POINTER(MlpBwd)]
    lib.nlam_mlp_bwd_blocks.restype = i32
    lib.nlam_wgrad_nparts.argtypes = [C.POINTER(Wgrad)]
    lib.nlam_wgrad_nparts.restype = i32
    lib.nlam_wgrad_plan.argtypes = [C.POINTER(Wgrad)]
    lib.nlam_wgrad_plan.restype = i32
    lib.nlam_mlp_fwd_plan.argtypes = [C.POINTER(MlpFwd)]
    lib.nlam_mlp_fwd_plan.restype = i32
    lib.nlam_mlp_bwd_plan.argtypes = [C.POINTER(MlpBwd)]
    lib.nlam_mlp_bwd_plan.restype = i32
    lib.nlam_mlp_fwd_wide_plan.argtypes = [C.POINTER(MlpFwd)]
    lib.nlam_mlp_fwd_wide_plan.restype = i32
    lib.nlam_mlp_bwd_wide_plan.argtypes = [C.POINTER(MlpBwd)]
    lib.nlam_mlp_bwd_wide_plan.restype = i32
    lib.nlam_mlp_pack_floats.argtypes = [C.POINTER(PackJob), i32]
    lib.nlam_mlp_pack_floats.restype = i64
    lib.nlam_mlp_pack.argtypes = [vp, i32, vp]
    lib.nlam_mlp_pack.restype = i32
    lib.nlam_mlp_fwd_pack_records.argtypes = [C.POINTER(MlpFwd), C.POINTER(PackRec), i32, C.POINTER(C.c_int32)]
    lib.nlam_mlp_fwd_pack_records.restype = i32
    lib.nlam_mlp_bwd_pack_records.argtypes = [C.POINTER(MlpBwd), C.POINTER(PackRec), i32, C.POINTER(C.c_int32)]
    lib.nlam_mlp_bwd_pack_records.restype = i32
    lib.nlam_pack_records.argtypes = [vp, i32, i32, vp]
    lib.nlam_pack_records.restype = i32
    lib.nlam_mlp_fwd.argtypes = [C.POINTER(MlpFwd), vp]
    lib.nlam_mlp_fwd.restype = i32
    lib.nlam_mlp_bwd.argtypes = [C.POINTER(MlpBwd), vp]
    lib.nlam_mlp_bwd.restype = i32
    lib.nlam_mlp_fwd_gemm_workspace_floats.argtypes = [C.POINTER(MlpFwd)]
    lib.nlam_mlp_fwd_gemm_workspace_floats.restype = i64
    lib.nlam_mlp_bwd_gemm_workspace_floats.argtypes = [C.POINTER(MlpBwd)]
    lib.nlam_mlp_bwd_gemm_workspace_floats.restype = i64
    lib.nlam_mlp_bwd_gemm_blocks.argtypes = [C.POINTER(MlpBwd)]
    lib.nlam_mlp_bwd_gemm_blocks.restype = i32
    lib.nlam_mlp_fwd_gemm.argtypes = [C.POINTER(MlpFwd), vp]
    lib.nlam_mlp_fwd_gemm.restype = i32
    lib.nlam_mlp_bwd_gemm.argtypes = [C.POINTER(MlpBwd), vp]
    lib.nlam_mlp_bwd_gemm.restype = i32
    lib.nlam_wgrad.argtypes = [C.POINTER(Wgrad), vp]
    lib.nlam_wgrad.restype = i32
    lib.nlam_segment_sum.argtypes = [vp, i64, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.nlam_segment_sum.restype = i32
    lib.nlam_segment_sum_acc.argtypes = [vp, i64, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.nlam_segment_sum_acc.restype = i32
    lib.nlam_segment_sum_add.argtypes = [vp, i64, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.nlam_segment_sum_add.restype = i32
    lib.nlam_segment_sum_bf16.argtypes = [vp, i64, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.nlam_segment_sum_bf16.restype = i32
    lib.nlam_store_bf16_supported.argtypes = [C.POINTER(MlpFwd)]
    lib.nlam_store_bf16_supported.restype = i32
    lib.nlam_split_combine.argtypes = [vp, i64, vp, vp, vp, i32, i32, i32, vp]
    lib.nlam_split_combine.restype = i32
    lib.nlam_reduce_partials.argtypes = [vp, i32, i64, i32, vp, i32, vp]
    lib.nlam_reduce_partials.restype = i32
    lib.nlam_reduce_jobs.argtypes = [C.POINTER(ReduceJobs), vp]
    lib.nlam_reduce_jobs.restype = i32
    lib.nlam_reduce_jobs_waves.restype = i32
    lib.nlam_wmse_fwd.argtypes = [vp, vp, vp, vp, i64, i32, i32, f32, vp, i32, vp]
    lib.nlam_wmse_fwd.restype = i32
    lib.nlam_wmse_bwd.argtypes = [vp, vp, vp, vp, vp, i64, i32, i32, f32, vp, vp]
    lib.nlam_wmse_bwd.restype = i32
    lib.nlam_adamw_step.argtypes = [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, i32, f32, vp]
    lib.nlam_adamw_step.restype = i32
    lib.nlam_adamw_step_resident.argtypes = [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, vp, vp, f32, vp]
    lib.nlam_adamw_step_resident.restype = i32
    lib.nlam_step_tail_fwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, f32, vp, vp, i32, i64, i32, i32, vp]
    lib.nlam_step_tail_fwd.restype = i32
    lib.nlam_step_tail_bwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, f32, vp, vp, i64, i32, i32, vp]
    lib.nlam_step_tail_bwd.restype = i32
    lib.nlam_loss_fwd.argtypes = [C.POINTER(Loss), vp]
    lib.nlam_loss_fwd.restype = i32
    lib.nlam_loss_bwd.argtypes = [C.POINTER(Loss), vp]
    lib.nlam_loss_bwd.restype = i32
    lib.nlam_step_tail_ext_fwd.argtypes = [C.POINTER(StepTail), vp]
    lib.nlam_step_tail_ext_fwd.restype = i32
    lib.nlam_step_tail_ext_bwd.argtypes = [C.POINTER(StepTail), vp]
    lib.nlam_step_tail_ext_bwd.restype = i32
    lib.nlam_step_tail_loss_fwd.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, f32, vp, vp, i32, i64, i32, i32, vp]
    lib.nlam_step_tail_loss_fwd.restype = i32
    lib.nlam_step_tail_loss_bwd.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, vp, f32, vp, vp, i64, i32, i32, vp]
    lib.nlam_step_tail_loss_bwd.restype = i32
    lib.nlam_eval_metrics.argtypes = [C.POINTER(Eval), vp]
    lib.nlam_eval_metrics.restype = i32
    lib.nlam_eval_workspace_floats.argtypes = [i32, i32, i32, i32]
    lib.nlam_eval_workspace_floats.restype = i64
    lib.nlam_concat.argtypes = [C.POINTER(Cat), vp]
    lib.nlam_concat.restype = i32
    lib.nlam_window_len.argtypes = [i64, i64, i32, i32, i32]
    lib.nlam_window_len.restype = i64
    lib.nlam_window_batch.argtypes = [C.POINTER(Window), vp]
    lib.nlam_window_batch.restype = i32
    lib.nlam_window_batch_ens.argtypes = [C.POINTER(WindowEns), vp]
    lib.nlam_window_batch_ens.restype = i32
    for entry in (lib.nlam_forecast_init, lib.nlam_forecast_head, lib.nlam_forecast_tail, lib.nlam_forecast_finish):
        entry.argtypes = [C.POINTER(Forecast), vp]
        entry.restype = i32
    for entry in (lib.nlam_forecast_init_strided, lib.nlam_forecast_head_strided):
        entry.argtypes = [C.POINTER(Forecast), C.POINTER(ForecastSrc), vp]
        entry.restype = i32
    lib.nlam_forecast_workspace_floats.argtypes = [i32, i32, i32]
    lib.nlam_forecast_workspace_floats.restype = i64
    lib.nlam_philox_normal_fill.argtypes = [vp, i64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp]
    lib.nlam_philox_normal_fill.restype = i32
    lib.nlam_latent_sample.argtypes = [C.POINTER(LatentSample), vp]
    lib.nlam_latent_sample.restype = i32
    lib.nlam_ens_scores.argtypes = [C.POINTER(EnsScores), vp]
    lib.nlam_ens_scores.restype = i32
    lib.nlam_ens_scores_workspace_floats.argtypes = [i32, i32, i32, i32]
    lib.nlam_ens_scores_workspace_floats.restype = i64
    lib.nlam_ens_products.argtypes = [C.POINTER(EnsProducts), vp]
    lib.nlam_ens_products.restype = i32
    lib.nlam_ens_products_workspace_floats.argtypes = [i32, i32, i32, i32, i32, i32]
    lib.nlam_ens_products_workspace_floats.restype = i64
    lib.nlam_ens_neighbourhood.argtypes = [C.POINTER(EnsNeighbourhood), vp]
    lib.nlam_ens_neighbourhood.restype = i32
    lib.nlam_ens_neighbourhood_workspace_floats.argtypes = [i32, i32, i32, i32, i32, i32, i32]
    lib.nlam_ens_neighbourhood_workspace_floats.restype = i64
    lib.nlam_dct_spectra.argtypes = [C.POINTER(DctSpectra), vp]
    lib.nlam_dct_spectra.restype = i32
    lib.nlam_dct_spectra_workspace_floats.argtypes = [i32, i32, i32, i32]
    lib.nlam_dct_spectra_workspace_floats.restype = i64
    lib.nlam_latent_kl_fwd.argtypes = [C.POINTER(LatentKl), vp]
    lib.nlam_latent_kl_fwd.restype = i32
    lib.nlam_latent_kl_bwd.argtypes = [C.POINTER(LatentKl), vp]
    lib.nlam_latent_kl_bwd.restype = i32
    lib.nlam_latent_kl_workspace_floats.argtypes = [i32, i32, i32]
    lib.nlam_latent_kl_workspace_floats.restype = i64
    for name, struct in (("nlam_latent_draw_fwd", LatentDraw), ("nlam_latent_draw_bwd", LatentDraw), ("nlam_crps_ens_fwd", CrpsEns),
                         ("nlam_crps_ens_bwd", CrpsEns)):
        getattr(lib, name).argtypes = [C.POINTER(struct), vp]
        getattr(lib, name).restype = i32
    lib.nlam_crps_ens_workspace_floats.argtypes = [i32, i32, i32, i32]
    lib.nlam_crps_ens_workspace_floats.restype = i64
    lib.nlam_window_moments.argtypes = [C.POINTER(Moments), vp]
    lib.nlam_window_moments.restype = i32
    lib.nlam_moments_workspace_doubles.argtypes = [i32, i32, i64, i32]
    lib.nlam_moments_workspace_doubles.restype = i64
    lib.nlam_series_range_workspace_words.argtypes = [i64, i32]
    lib.nlam_series_range_workspace_words.restype = i64
    lib.nlam_series_range.argtypes = [vp, i64, i32, vp, vp, vp, vp, i64, vp]
    lib.nlam_series_range.restype = i32
    lib.nlam_series_pack_q16.argtypes = [vp, i64, i32, vp, vp, vp, i64, vp]
    lib.nlam_series_pack_q16.restype = i32
    lib.nlam_window_batch_q16.argtypes = [C.POINTER(WindowEns), C.POINTER(Q16Src), vp]
    lib.nlam_window_batch_q16.restype = i32
    lib.nlam_window_moments_q16.argtypes = [C.POINTER(Moments), vp, vp, vp, vp]
    lib.nlam_window_moments_q16.restype = i32
    for entry in (lib.nlam_forecast_init_q16, lib.nlam_forecast_head_q16):
        entry.argtypes = [C.POINTER(Forecast), C.POINTER(ForecastSrc), C.POINTER(Q16Src), vp]
        entry.restype = i32
    lib.nlam_grad_sumsq_workspace_doubles.argtypes = [i64]
    lib.nlam_grad_sumsq_workspace_doubles.restype = i64
    lib.nlam_grad_sumsq.argtypes = [vp, i64, vp, i64, f32, vp, vp]
    lib.nlam_grad_sumsq.restype = i32
    lib.nlam_adamw_step_controlled.argtypes = [C.POINTER(OptCtl), vp]
    lib.nlam_adamw_step_controlled.restype = i32
    lib.nlam_accum_begin.argtypes = [vp, i64, vp, vp]
    lib.nlam_accum_begin.restype = i32
    lib.nlam_adamw_step_accum.argtypes = [C.POINTER(OptCtl), C.POINTER(Accum), vp]
    lib.nlam_adamw_step_accum.restype = i32
    lib.nlam_adamw_step_resident_ema.argtypes = [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, vp, vp, f32, vp, C.POINTER(Ema)]
    lib.nlam_adamw_step_resident_ema.restype = i32
    lib.nlam_adamw_step_controlled_ema.argtypes = [C.POINTER(OptCtl), C.POINTER(Accum), C.POINTER(Ema), vp]
    lib.nlam_adamw_step_controlled_ema.restype = i32
    lib.nlam_flat_swap.argtypes = [vp, vp, i64, vp]
    lib.nlam_flat_swap.restype = i32
    lib.nlam_mlp_group_blocks.argtypes = [C.POINTER(C.c_int64), i32, C.POINTER(C.c_int32)]
    lib.nlam_mlp_group_blocks.restype = i32
    lib.nlam_mlp_fwd_group.argtypes = [C.POINTER(MlpFwd), i32, vp]
    lib.nlam_mlp_fwd_group.restype = i32
    lib.nlam_mlp_bwd_group.argtypes = [C.POINTER(MlpBwd), i32, vp]
    lib.nlam_mlp_bwd_group.restype = i32
    lib.nlam_mlp_fwd_family.argtypes = [C.POINTER(MlpFwd)]
    lib.nlam_mlp_fwd_family.restype = i32
    lib.nlam_mlp_bwd_family.argtypes = [C.POINTER(MlpBwd)]
    lib.nlam_mlp_bwd_family.restype = i32
    lib.nlam_mlp_bwd_group_blocks.argtypes = [C.POINTER(MlpBwd), i32, C.POINTER(i32)]
    lib.nlam_mlp_bwd_group_blocks.restype = i32
    lib.nlam_wgrad_group.argtypes = [C.POINTER(Wgrad), i32, vp]
    lib.nlam_wgrad_group.restype = i32
    lib.nlam_wgrad_dma_group.argtypes = [C.POINTER(Wgrad), i32, vp]
    lib.nlam_wgrad_dma_group.restype = i32
    lib.nlam_wgrad_dma_group_supported.argtypes = [C.POINTER(Wgrad)]
    lib.nlam_wgrad_dma_group_supported.restype = i32
    lib.nlam_pre_add_supported.argtypes = [C.POINTER(MlpFwd)]
    lib.nlam_pre_add_supported.restype = i32
    lib.nlam_linear.argtypes = [C.POINTER(Linear), vp]
    lib.nlam_linear.restype = i32
    lib.nlam_linear_plan.argtypes = [C.POINTER(Linear)]
    lib.nlam_linear_plan.restype = i32
    lib.nlam_segment_sum_groups.argtypes = [i64, i32, i32]
    lib.nlam_segment_sum_groups.restype = i32
    lib.nlam_standardize.argtypes = [C.POINTER(StdJobs), vp]
    lib.nlam_standardize.restype = i32
    if lib.nlam_abi_version() != ABI_VERSION:
        raise RuntimeError("libnlam_hip.so ABI version mismatch")
    if os.environ.get("NLAM_LIN_WGS"):
        lib.nlam_set_tuning(TUNE_LIN_WGS, int(os.environ["NLAM_LIN_WGS"]))
    if os.environ.get("NLAM_WGRAD_BIG_MIN_ROWS"):
        lib.nlam_set_tuning(TUNE_WGRAD_BIG_MIN_ROWS, int(os.environ["NLAM_WGRAD_BIG_MIN_ROWS"]))
    if os.environ.get("NLAM_WGRAD_MIN_PARTS"):
        lib.nlam_set_tuning(TUNE_WGRAD_MIN_PARTS, int(os.environ["NLAM_WGRAD_MIN_PARTS"]))
    if os.environ.get("NLAM_WBF_HALF"):
        check(lib.nlam_set_tuning(TUNE_WBF_HALF, int(os.environ["NLAM_WBF_HALF"])), "nlam_set_tuning(NLAM_WBF_HALF)")
    if os.environ.get("NLAM_WBF_V4"):
        lib.nlam_set_tuning(TUNE_WBF_V4, int(os.environ["NLAM_WBF_V4"]))
    if os.environ.get("NLAM_LIN_GEMM"):
        lib.nlam_set_tuning(TUNE_LIN_GEMM, int(os.environ["NLAM_LIN_GEMM"]))
    if os.environ.get("NLAM_WGRAD_LDMA"):
        check(lib.nlam_set_tuning(TUNE_WGRAD_LDMA, int(os.environ["NLAM_WGRAD_LDMA"])), "nlam_set_tuning(NLAM_WGRAD_LDMA)")
    if os.environ.get("NLAM_WBF_EDGE"):
        check(lib.nlam_set_tuning(TUNE_WBF_EDGE, int(os.environ["NLAM_WBF_EDGE"])), "nlam_set_tuning(NLAM_WBF_EDGE)")
    if os.environ.get("NLAM_WGRAD_LDMA_VAR"):
        check(lib.nlam_set_tuning(TUNE_WGRAD_LDMA_VAR, int(os.environ["NLAM_WGRAD_LDMA_VAR"])), "nlam_set_tuning(NLAM_WGRAD_LDMA_VAR)")
    if os.environ.get("NLAM_WGRAD_DMA_R"):
        check(lib.nlam_set_tuning(TUNE_WGRAD_DMA_R, int(os.environ["NLAM_WGRAD_DMA_R"])), "nlam_set_tuning(NLAM_WGRAD_DMA_R)")
    if os.environ.get("NLAM_CHAIN_CUS"):
        check(lib.nlam_set_tuning(TUNE_CHAIN_CUS, int(os.environ["NLAM_CHAIN_CUS"])), "nlam_set_tuning(NLAM_CHAIN_CUS)")
    if os.environ.get("NLAM_WGRAD_MAX_WGS"):
        check(lib.nlam_set_tuning(TUNE_WGRAD_MAX_WGS, int(os.environ["NLAM_WGRAD_MAX_WGS"])), "nlam_set_tuning(NLAM_WGRAD_MAX_WGS)")
    if os.environ.get("NLAM_WGRAD_CHUNKS"):
        lib.nlam_set_tuning(TUNE_WGRAD_CHUNKS, int(os.environ["NLAM_WGRAD_CHUNKS"]))
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        kind = {-1: "NLAM_EINVAL (bad arguments)", -2: "NLAM_EUNSUP (width not instantiated in this build)"}.get(
            rc, f"hipError_t {rc}"
        )
        raise RuntimeError(f"{what} failed: {kind}")


SLICES = (1, 2, 3, 4, 5, 6)   # -DNLAM_TU=k translation-unit slices of csrc/nlam_hip.hip (see the comment at its top)


def source_stamp() -> str:
    """Hash of the library's sources (csrc/*.hip, csrc/*.inc, include/nlam_hip.h): measurements that belong to one build
    of the kernels (profiles/roundN/pmc_traffic.json) carry it, and bench.py refuses them when it no longer matches."""
    import hashlib

    h = hashlib.sha256()
    csrc = HERE / "csrc"
    for f in sorted([*csrc.glob("*.hip"), *csrc.glob("*.inc"), HERE.parent / "include" / "nlam_hip.h"]):
        h.update(f.read_bytes())
    return h.hexdigest()[:16]


def build(verbose: bool = False, out: Path | None = None, defines=(), single_tu: bool | None = None) -> Path:
    """Compile csrc/nlam_hip.hip for gfx950 into the in-tree shared library.

    Default: the six -DNLAM_TU=k slices are compiled in parallel (objects under csrc/_obj/, re-used when neither the
    sources nor the flags changed) and linked.  ``single_tu=True`` (and any build with extra ``defines``, e.g. the
    NLAM_TIMING instrumentation) is the one-command build: one hipcc invocation, everything in one translation unit."""
    import hashlib
    import subprocess
    from concurrent.futures import ThreadPoolExecutor

    csrc = HERE / "csrc"
    src = csrc / "nlam_hip.hip"
    out = Path(out) if out is not None else HERE / "libnlam_hip.so"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    base = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *[f"-D{d}" for d in defines]]
    if single_tu is None:
        single_tu = bool(defines) or os.environ.get("NLAM_SINGLE_TU") == "1"
    if single_tu:
        cmd = [*base, "-shared", str(src), "-o", str(out)]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
        return out

    objdir = csrc / "_obj"
    objdir.mkdir(exist_ok=True)
    h = hashlib.sha256(" ".join(base).encode())
    for f in sorted([*csrc.glob("*.hip"), *csrc.glob("*.inc"), HERE.parent / "include" / "nlam_hip.h"]):
        h.update(f.read_bytes())
    stamp = h.hexdigest()[:16]

    def compile_slice(k):
        obj = objdir / f"nlam_tu{k}_{stamp}.o"
        if not obj.exists():
            for old in objdir.glob(f"nlam_tu{k}_*.o"):
                old.unlink()
            cmd = [*base, f"-DNLAM_TU={k}", "-c", str(src), "-o", str(obj)]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
        return obj

    with ThreadPoolExecutor(len(SLICES)) as ex:
        objs = list(ex.map(compile_slice, SLICES))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *map(str, objs), "-o", str(out)]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return out
