/* nlam_hip.h -- C-ABI of the MI355X (gfx950) GNN message-passing hot path.
 *
 * The reference (mllam/neural-lam) has no FFI seam for this path: its "operator
 * interface" is the Python class API of neural_lam/gnn_layers.py and
 * neural_lam/utils/networks.py executed through ATen/PyG ops (SURVEY.md §2.4,
 * §8b).  This header is the seam a maintainer binds instead (ctypes stub in
 * INTEGRATION.md).  Every entry point takes plain device pointers + sizes and a
 * HIP stream; nothing allocates, nothing synchronises, no torch types.
 *
 * All float tensors are fp32, row-major, innermost dimension contiguous.
 * All index tensors are int32 on the device.  Return value: 0 on success,
 * a negative NLAM_E* code on bad arguments, a positive hipError_t on launch
 * failure.
 *
 * Replaces, per entry point:
 *   nlam_mlp_fwd / nlam_mlp_bwd
 *       utils.make_mlp blocks  Linear -> SiLU -> Linear [-> LayerNorm]
 *       (neural_lam/utils/networks.py:8-40) together with the torch.cat of their
 *       inputs and the residual add around them:
 *         aggr_mlp(cat(rec_rep, aggr)) + residual   gnn_layers.py:148-151
 *         grid_emb + encoding_grid_mlp(grid_emb)    models/step_predictors/graph/base.py:308
 *         grid_embedder / *_embedder / output_map    graph/base.py:286-295, 322
 *   nlam_mlp_fwd / nlam_mlp_bwd with three gathered sources, a tile schedule and `aggr` set
 *       InteractionNet / PropagationNet message + aggregate (+ edge update):
 *         PyG propagate: x_j/x_i index_select, message() = edge_mlp(cat(edge, x_j, x_i))
 *         [+ x_j], aggregate() = scatter sum/mean onto num_rec receivers,
 *         edge_rep + edge_diff                       gnn_layers.py:144-155, 168-189, 241-249
 *   nlam_wgrad
 *       autograd's weight gradients of the nn.Linear layers inside those MLPs.
 *   nlam_segment_sum, nlam_segment_sum_acc
 *       autograd of index_select (= index_add by sender), as a CSC segment sum; _acc adds onto
 *       an existing gradient buffer (what autograd's accumulation would do with one more launch).
 *   nlam_split_combine
 *       the deterministic form of PyG's scatter for receivers that exceed one tile
 *       (gnn_layers.py:175-189 under Trainer(deterministic=True), train_model.py:566).
 *   nlam_affine_mix
 *       the elementwise tail of an AR step: prev_state + delta * diff_std + diff_mean
 *       (step_predictors/graph/base.py:331-343) and the boundary overwrite
 *       (forecasters/autoregressive.py:128-131), forward and backward.
 *   nlam_wmse_fwd / nlam_wmse_bwd
 *       metrics.wmse + mask_and_reduce_metric (metrics.py:37-137) with the batch / step means of
 *       models/module.py:463-510.
 *   nlam_loss_fwd / nlam_loss_bwd, nlam_step_tail_loss_fwd / nlam_step_tail_loss_bwd
 *       the other losses of --loss (train_model.py:271-276): metrics.mse / mae / wmae / nll / crps_gauss
 *       (and wmse), per-variable or per-entry (predicted) std, the same reduction; the step-tail pair fuses
 *       them into the AR step's state update: the kernels of nlam_step_tail_fwd / _bwd, instantiated on the kind's
 *       loss term and its std where those two take inv_var = 1 / std^2.
 *   nlam_step_tail_ext_fwd, nlam_step_tail_ext_bwd
 *       that step tail with the output clamps of get_clamped_new_state (step_predictors/base.py) and / or the softplus
 *       of a predicted std (output_std) inside the pass; the loss term takes the predicted std per entry.
 *   nlam_eval_metrics, nlam_eval_workspace_floats
 *       the evaluation tensors of validation_step / test_step (models/module.py:546-576, :607-681): per-step loss,
 *       per-variable masked MSE / MAE / mean std, per-node loss maps; one pass over the rollout + a fixed-order reduction.
 *   nlam_forecast_init, nlam_forecast_head, nlam_forecast_tail, nlam_forecast_finish, nlam_forecast_workspace_floats
 *       a forecast of any length as replays of ONE recorded AR step: a lead counter in device memory ties the data path
 *       (this lead's forcing window and boundary truth, cut from the resident series) to the inference step tail, which
 *       rotates the state in place and writes this lead's physical fields, valid time and verification sums.
 *   nlam_forecast_init_strided, nlam_forecast_head_strided
 *       that data path over forecast-type and ensemble series: nlam_window_batch_ens's (sample, member, lead-time row) addressing
 *       from a flat sample index read on the device.
 *   nlam_philox_normal_fill, nlam_latent_sample, nlam_ens_scores, nlam_ens_scores_workspace_floats
 *       sampled ensembles inside that recorded step (Graph-EFM): the reparameterised draw of the latent variable from a
 *       counter-based generator keyed by the lead counter, and the ensemble verification of every lead (ensemble-mean error,
 *       spread, the two terms of fair CRPS, rank histogram, mean and spread fields) as one reduction over the member axis.
 *   nlam_ens_products, nlam_ens_products_workspace_floats
 *       what the ensemble is made for, per lead of that step: exceedance probabilities of threshold events and quantile fields
 *       from the sorted members, with Brier score, reliability table, pinball loss and coverage counts.
 *   nlam_ens_neighbourhood, nlam_ens_neighbourhood_workspace_floats
 *       the same events on the grid as a lattice: the fraction of (member, cell) pairs in the event inside square windows of a
 *       ladder of radii, and the two sums of the fractions skill score, from integer summed-area tables.
 *   nlam_dct_spectra, nlam_dct_spectra_workspace_floats
 *       at which scales a forecast holds variance, per lead of that step: binned variance spectra of lattice fields from a 2-D
 *       orthonormal DCT, as two fp32 matrix products on the matrix cores and a fixed-order sum per bin.
 *   nlam_latent_kl_fwd, nlam_latent_kl_bwd, nlam_latent_kl_workspace_floats
 *       the variational training objective of Graph-EFM: the reparameterised posterior draw from that generator and the KL
 *       divergence from the prior as one pass with a fixed-order reduction, and its elementwise backward.
 *   nlam_latent_draw_fwd, nlam_latent_draw_bwd, nlam_crps_ens_fwd, nlam_crps_ens_bwd, nlam_crps_ens_workspace_floats
 *       the ensemble CRPS fine-tuning term of Graph-EFM: the reparameterised draw from the prior with its gradient, and the
 *       unbiased ensemble CRPS of the members rolled out from it as one pass with a fixed-order reduction; both backwards
 *       elementwise.
 *   nlam_window_moments, nlam_moments_workspace_doubles
 *       the per-sample means and second moments of npyfilesmeps/compute_standardization_stats.py (values and
 *       standardized one-step differences), read in place from the resident series of the data path.
 *   nlam_series_range, nlam_series_range_workspace_words, nlam_series_pack_q16, nlam_window_batch_q16,
 *   nlam_window_moments_q16, nlam_forecast_init_q16, nlam_forecast_head_q16
 *       the resident series kept as packed int16 (per-feature scale and offset, as GRIB and packed netCDF ship them): the
 *       exact range and the encoding of an fp32 chunk on upload, and the batch, moments and forecast data kernels with the
 *       decode in flight; a packed series gives the bits of an fp32 series that holds its decoded values.
 *   nlam_reduce_partials
 *       deterministic second stage of the per-workgroup partial sums.
 *   nlam_adamw_step
 *       torch.optim.AdamW(lr, betas=(0.9, 0.95)) of models/module.py:293-304 on
 *       one flat fp32 parameter buffer.
 *   nlam_grad_sumsq, nlam_grad_sumsq_workspace_doubles, nlam_adamw_step_controlled
 *       the global gradient norm, and the AdamW update with clipping by that norm, a closed-form learning-rate schedule
 *       and the skip of a non-finite step decided on the device (what Lightning's gradient_clip_val and LR scheduler
 *       give the reference's loop), in launches whose arguments do not depend on the step.
 *   nlam_accum_begin, nlam_adamw_step_accum
 *       Lightning's accumulate_grad_batches: the zero of the gradient and the controlled update gated on the device by the
 *       index of the micro-batch, so that one recorded step serves every micro-step of a window.
 *   nlam_adamw_step_resident_ema, nlam_adamw_step_controlled_ema, nlam_flat_swap
 *       Lightning's EMAWeightAveraging (torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn): the moving average
 *       of the weights, kept by the AdamW update launch itself, and the in-place exchange of weights and average.
 */
#ifndef NLAM_HIP_H
#define NLAM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NLAM_ABI_VERSION 8
#define NLAM_MAX_SRC 3
#define NLAM_MAX_CAT 6

#define NLAM_EINVAL (-1)   /* inconsistent sizes / null pointers        */
#define NLAM_EUNSUP (-2)   /* width outside what this build instantiates */

/* flags */
#define NLAM_F_ADD_SRC0   1u   /* out  = msg + src[0]   (edge update / node residual)          */
#define NLAM_F_ADD_SRC1   2u   /* msg  = mlp + src[1]   (PropagationNet sender / aggr residual) */
#define NLAM_F_MEAN       4u   /* aggregate = mean over in-edges (sum otherwise)               */
#define NLAM_F_SILU_B     8u   /* wgrad: apply SiLU to the B operand while loading             */
/* Factorised first Linear of an edge MLP (gnn_layers.py:168-172, edge_mlp(cat(edge_attr, x_j, x_i))):
 *   W1 [e | x_j | x_i] = W1_e e + (W1_j x)[sender] + (W1_i x)[receiver],
 * the two node-level products being computed once per NODE (nlam_linear) instead of once per EDGE.  With this flag
 * only src[0] goes through the first GEMM (columns 0 .. src[0].width of W1, whose rows are `ldw1` floats apart);
 * src[1..] are gathered pre-activation ADDENDS of width hid:  z1 = W1_e src0 + b1 + sum_k src[k][idx_k].
 * Backward: dmode[0] as usual; dmode[k >= 1] = 3 segment-sums dz1 over the tile's receivers into dsrc[k]
 * ((nseg_total, hid): the gradient of a receiver-gathered addend), 0 / 2 leave it to the caller (a CSC
 * nlam_segment_sum over the dz1 rows gives the gradient of a sender-gathered addend).  Split-bf16 matrix modes,
 * widths that are multiples of 32 and <= 64 (NLAM_EUNSUP otherwise); not combined with NLAM_F_ADD_SRC1. */
#define NLAM_F_PRE_ADD   16u
/* nlam_mlp_bwd_group only: a leaf MLP (no data gradients) of <= 4 input columns accumulates its weight gradients in the
 * backward kernel itself -- dz1 / dz2 are never written: `dz2` receives the (workgroups, dout, hid) partial sums of dW2,
 * `dz1` is unused, `vec_partials` has SEVEN rows per workgroup: db1, db2, dgamma, dbeta, dW1[:, 0], dW1[:, 1], dW1[:, 2].
 * z1 may be NULL (then `b1` is required): the forward of such an MLP need not save its pre-activation. */
#define NLAM_F_LEAF_WGRAD 32u
/* wide launches (a width above 64) of nlam_mlp_fwd / nlam_mlp_bwd: `wpack` already holds the packed weights of exactly this
 * launch -- written by nlam_pack_records from the records nlam_mlp_*_pack_records gave for it, since the weights last
 * changed -- so the pack launch in front of the kernel is skipped. */
#define NLAM_F_WPACK_READY 64u
/* NLAM_F_NO_ACT: no activation between the two Linears (z1 goes into the second GEMM as it is, silu' = 1 in backward).  With
 * W2 = identity, b2 = 0 the launch is `Linear [-> LayerNorm]` with the full gather / concat / residual / aggregation geometry:
 * how utils.make_mlp's hidden_layers = 0 case (utils/networks.py:8-40: blueprint [in, out]) runs on the fused kernels.  fp32
 * matrix path only (NLAM_F_MM_* bits must be 0: NLAM_EUNSUP otherwise); not for grouped / factorised / concatenated launches. */
#define NLAM_F_NO_ACT 128u
/* NLAM_F_STORE_BF16 (nlam_mlp_fwd / nlam_mlp_bwd): z1, xhat (forward: written, backward: read) and dz1, dz2 (backward: written)
 * are rows of bfloat16 instead of float -- the pointers of the structs are then reinterpreted, (batch, rows, width) contiguous.
 * What Lightning's --precision bf16-mixed (train_model.py:163-168) makes of the reference's nn.Linear outputs and their
 * gradients; halves the bytes a layer saves for and hands to its own backward.  Only where nlam_store_bf16_supported() says so
 * (one-term split-bf16 wide kernels, hid and dout whole 32-column blocks); NLAM_EUNSUP otherwise.
 * nlam_wgrad: NLAM_F_A_BF16 = `A` (dz1 / dz2) is bf16, NLAM_F_S_BF16 = src[0] (z1; nsrc must be 1, no gather index) is bf16. */
#define NLAM_F_STORE_BF16 (1u << 10)
#define NLAM_F_A_BF16     (1u << 10)
/* NLAM_F_ACC_DSRC0 (nlam_mlp_bwd, round 6): the data gradient of source 0 (dmode 1: rows scattered through the unique gather
 * index) is ADDED to what dsrc[0] holds instead of overwriting it -- a tensor every autoregressive step of a rollout consumes (the
 * static edge embeddings, models/forecasters/autoregressive.py:63-149) then collects its gradient in ONE buffer, in the order the
 * steps are back-propagated, instead of T buffers and T - 1 add launches over 0.1-0.5 GB each.  Split-bf16 super-tile family
 * only (nlam_mlp_bwd_family == 2): NLAM_EUNSUP elsewhere. */
#define NLAM_F_ACC_DSRC0  (1u << 12)
#define NLAM_F_S_BF16     (1u << 11)
/* NLAM_F_WGRAD_SOLO (nlam_wgrad / nlam_wgrad_nparts, round 6): the launch has the chip to itself -- every launch of the step on one
 * stream, the reference's drop-in path launched from Python -- so its row slices are chosen for ISOLATED speed: up to one
 * workgroup per CU and at least 64 slices (the rounds 2-5 shape).  Without it a big split-bf16 gradient takes at most
 * NLAM_TUNE_WGRAD_MAX_WGS workgroups: it is sized to run beside the data-gradient chain (DESIGN.md finding 53). */
#define NLAM_F_WGRAD_SOLO (1u << 13)
/* matrix path of the GEMMs (bits 8-9): 0 = v_mfma_f32_32x32x2_f32 (exact fp32 fmaf chains);
 * n = 1..3: operands split into n bf16 terms on the bf16 matrix cores, fp32 accumulate
 * (1 = plain bf16 operands, 2 = ~2^-16 product error, 3 = fp32-class ~2^-24).  Shapes the
 * split kernels do not cover (widths not multiples of 32) run the fp32 path.  Wide launches (a width above 64): hid and the
 * source widths must be multiples of 4 and the launch at or above the super-tile threshold; a forward that aggregates
 * (aggr != NULL) with a dout that is no multiple of 4 runs the fp32 path too -- the super-tile aggregation writes whole float4s
 * of a receiver's row -- and is NLAM_EUNSUP together with NLAM_F_PRE_ADD.  nlam_mlp_*_wide_plan says what a launch runs. */
#define NLAM_F_MM_SHIFT   8
#define NLAM_F_MM_MASK    (3u << NLAM_F_MM_SHIFT)
#define NLAM_F_MM_BF16X1  (1u << NLAM_F_MM_SHIFT)
#define NLAM_F_MM_BF16X2  (2u << NLAM_F_MM_SHIFT)
#define NLAM_F_MM_BF16X3  (3u << NLAM_F_MM_SHIFT)

typedef struct {
    const float* ptr;     /* (batch|1, n_rows_of_source, width) */
    const int32_t* idx;   /* per tile-row gather index into the source rows, or NULL = row id */
    int64_t bstride;      /* elements between batches; 0 = shared by all batches */
    int32_t width;        /* columns taken from this source */
    int32_t _pad;
} nlam_src_t;

/* One wave-tile of <= 32 consecutive rows (CSR positions) made of whole receivers. */
typedef struct {
    int32_t row0;    /* first row (CSR position)                   */
    int32_t nrows;   /* rows in tile, 0..32                        */
    int32_t seg0;    /* first receiver covered                     */
    int32_t nseg;    /* receivers covered (bit 30 set: partial sum of a split receiver -> atomic add) */
} nlam_tile_t;
#define NLAM_TILE_SPLIT (1 << 30)

typedef struct {
    /* ---- inputs: concatenated (and gathered) sources ---- */
    nlam_src_t src[NLAM_MAX_SRC];
    int32_t nsrc;
    int32_t batch;
    int32_t rows;          /* rows per batch (edges or nodes) */
    int32_t ntiles;        /* tiles per batch; tiles==NULL -> ceil(rows/32) dense tiles */
    const nlam_tile_t* tiles;
    /* ---- MLP parameters (torch.nn.Linear layout: weight (out, in)) ---- */
    const float* W1; const float* b1;   /* (hid, kin), (hid) ; kin = sum of src widths */
    const float* W2; const float* b2;   /* (dout, hid), (dout) */
    const float* ln_w; const float* ln_b; /* (dout) or NULL = no LayerNorm */
    float eps;
    int32_t hid;
    int32_t dout;
    uint32_t flags;
    /* ---- outputs ---- */
    float* out;            /* (batch, out_rows, dout) row output or NULL */
    const int32_t* out_idx;/* per tile-row scatter index (unique) or NULL = row id */
    int64_t out_bstride;
    float* aggr;           /* (batch, nseg_total, dout) segment-reduced msg or NULL */
    const int32_t* rowptr; /* (nseg_total + 1) CSR row pointers (needed with aggr)  */
    const float* inv_deg;  /* (nseg_total) 1/max(deg,1) (needed with NLAM_F_MEAN)   */
    int32_t nseg_total;
    int32_t ldw1;          /* NLAM_F_PRE_ADD: floats between rows of W1 (0 = sum of the source widths) */
    /* ---- saved for backward (all nullable; tile-row order) ---- */
    float* z1;             /* (batch, rows, hid)  pre-activation  */
    float* xhat;           /* (batch, rows, dout) normalised, pre-affine (LN only) */
    float* rstd;           /* (batch, rows) */
    /* ---- scratch for the wide kernels (hid or dout or a source wider than 64) ---- */
    float* wpack;          /* >= nlam_mlp_fwd_wpack_floats(p) floats, or NULL when that is 0 */
    int64_t wpack_floats;  /* capacity of wpack */
    /* ---- optional: src[0] as a row-wise CONCATENATION of ncat pieces ----
     * The torch.cat of the grid input features in front of grid_embedder (step_predictors/graph/base.py:275-286:
     * prev_state | prev_prev_state | forcing | static features) folded into the MLP's first load instead of a launch of its
     * own that materialises (batch, rows, 56).  With ncat > 0: nsrc == 1, src[0].ptr is ignored, src[0].idx must be NULL,
     * src[0].width = sum of cat_width (<= 64); piece k holds rows of cat_width[k] floats, cat_bstride[k] floats apart between
     * batch items (0 = shared: expand_to_batch).  cat_out (optional, (batch, rows, src[0].width)): the kernel also writes the
     * concatenated rows -- what the weight gradient and the backward pass read as the MLP's input.  Served by the
     * split-bf16 narrow kernels (NLAM_EUNSUP otherwise: concatenate with nlam_concat and launch without pieces). */
    int32_t ncat;
    int32_t _pad3;
    const float* cat_ptr[NLAM_MAX_CAT];
    int64_t cat_bstride[NLAM_MAX_CAT];
    int32_t cat_width[NLAM_MAX_CAT];
    float* cat_out;
} nlam_mlp_fwd_t;

typedef struct {
    /* forward geometry, exactly as in the forward call */
    nlam_src_t src[NLAM_MAX_SRC];
    int32_t nsrc;
    int32_t batch;
    int32_t rows;
    int32_t ntiles;
    const nlam_tile_t* tiles;
    const float* W1; const float* W2;
    const float* ln_w;     /* NULL = no LayerNorm */
    int32_t hid;
    int32_t dout;
    uint32_t flags;
    int32_t nseg_total;
    /* upstream gradients */
    const float* g_out;    /* grad of `out` (batch, out_rows, dout) or NULL */
    const int32_t* out_idx;
    int64_t out_bstride;
    const float* g_aggr;   /* grad of `aggr` (batch, nseg_total, dout) or NULL */
    const int32_t* seg_of_row; /* (rows) receiver of each tile-row (needed with g_aggr) */
    const int32_t* rowptr;     /* (nseg_total + 1) CSR row pointers (needed with dmode 3) */
    const float* inv_deg;
    /* saved */
    const float* z1; const float* xhat; const float* rstd;
    /* outputs */
    float* dz1;            /* (batch, rows, hid)   for nlam_wgrad */
    float* dz2;            /* (batch, rows, dout)  for nlam_wgrad */
    float* dsrc[NLAM_MAX_SRC];     /* gradient wrt each source, see dmode */
    int64_t dsrc_bstride[NLAM_MAX_SRC];
    int32_t dmode[NLAM_MAX_SRC];   /* 0 none | 1 rows scattered through src[k].idx (unique)
                                      | 2 tile-row order (rows, width) for a later segment sum
                                      | 3 segment-summed over the tile's receivers -> (nseg_total, width) */
    int32_t ldw1;          /* NLAM_F_PRE_ADD: floats between rows of W1 (0 = sum of the source widths) */
    float* vec_partials;   /* (nblocks, 4, vec_stride): per-workgroup db1, db2, dgamma, dbeta partial sums */
    int32_t vec_partials_rows; /* capacity in rows; must be >= nlam_mlp_bwd_blocks(p) */
    int32_t vec_stride;    /* row stride of vec_partials: multiple of 64, >= max(hid, dout) */
    float* wpack;          /* >= nlam_mlp_bwd_wpack_floats(p) floats, or NULL when that is 0 */
    int64_t wpack_floats;
    const float* b1;       /* NLAM_F_LEAF_WGRAD only (required there): first-layer bias; that kernel recomputes the pre-activation
                              z1 = W1 x + b1 from the (<= 4-column) input row and never reads `z1` (which may be NULL) */
    int32_t dz2_ld;        /* floats between rows of dz2: MUST equal nlam_mlp_bwd_dz2_ld(p) -- 0 = dout, except for an output width
                              that is not a multiple of 32 on the split-bf16 kernel (output_map, dout = 17): then 32-padded, and
                              nlam_wgrad takes dz2 with m = that stride.  The narrow kernel writes the columns past dout as zeros;
                              the wide kernels (a width above 64, dout no multiple of 4) write the dout real columns only and
                              leave the padding as it is: the caller zero-fills it once (it must read as zeros in nlam_wgrad) */
    int32_t _pad2;
} nlam_mlp_bwd_t;

typedef struct {
    const float* A;        /* (batch*rows, m) contiguous: dz1 or dz2 */
    int32_t m;
    int32_t batch;
    int32_t rows;
    int32_t nsrc;
    nlam_src_t src[NLAM_MAX_SRC]; /* B operand = concat of gathered sources (tile-row order idx) */
    uint32_t flags;        /* NLAM_F_SILU_B */
    int32_t n;             /* sum of widths */
    float* partials;       /* (nparts, m, n) */
    int32_t nparts;        /* number of row-slices = workgroups launched */
    int32_t _pad;
} nlam_wgrad_t;

/* number of persistent waves the fwd/bwd kernels launch (for sizing vec_partials) */
int32_t nlam_grid_waves(void);
int32_t nlam_abi_version(void);
/* workgroups nlam_mlp_fwd / nlam_mlp_bwd launch for `total_tiles` = ntiles * batch */
int32_t nlam_num_blocks(int64_t total_tiles);
/* widest hidden/output width the fused kernels of this build instantiate */
int32_t nlam_max_width(void);

/* Launch-shape tuning (process-wide; tests use it to force a kernel family at small sizes).
 *   NLAM_TUNE_WBF_MIN_SUPERTILES: wide (> 64) fused-MLP launches with fewer super tiles than `value`
 *   run on the fp32 MFMA kernels even when a split-bf16 matrix mode is requested (default 192:
 *   a 128-row super tile per workgroup needs that many to occupy 256 CUs).
 * Returns 0, or NLAM_EINVAL for an unknown key / negative value. */
#define NLAM_TUNE_WBF_MIN_SUPERTILES 1
/*   NLAM_TUNE_WGRAD_CHUNKS: 32-row chunks a weight-gradient workgroup streams through before it writes its (m x n)
 *   partial, for problems of more than 128 chunks (default 8; 1 = one partial per chunk up to the cap of 512 workgroups;
 *   larger values trade launch width for less partial-sum traffic). */
#define NLAM_TUNE_WGRAD_CHUNKS 2
/*   NLAM_TUNE_LIN_WGS: workgroups of an nlam_linear launch with k <= 256 on the wide kernel, whose weight strip stays in
 *   LDS for the whole launch (default 256 = one per CU; 0 = stream the strip through two LDS buffers as for k > 256). */
#define NLAM_TUNE_LIN_WGS 3
/*   NLAM_TUNE_WGRAD_MIN_PARTS: least number of row slices (= partial sums per element) a weight gradient over more than that
 *   many 32-row chunks is cut into (default 128; for weight matrices of more than 128 rows as many as give 64 workgroups:
 *   64 / number of 256 x 256 windows -- launch width for the mid-size problems; smaller = less partial-sum traffic; setting it
 *   sets both to the given slice count). */
#define NLAM_TUNE_WGRAD_MIN_PARTS 4
/*   NLAM_TUNE_WGRAD_BIG_MIN_ROWS: rows (x batch) from which a split-bf16 weight gradient with more than 128 output rows uses
 *   256 x 256 windows; below it 128 x 128 windows (same launch width, a quarter of the row slices and partial sums). */
#define NLAM_TUNE_WGRAD_BIG_MIN_ROWS 5
/*   NLAM_TUNE_WBF_HALF: split-bf16 wide kernels on 4-wave workgroups of half the rows, TWO co-resident per CU, so that one
 *   workgroup's load / store phases overlap the other's matrix phases (bit 0: forward, bit 1: backward; shapes without a
 *   half-size instantiation keep the 8-wave kernels).  Bit 2 (round 6): the one-term forward above d = 256 on 4-wave workgroups
 *   of 64 rows (two MFMAs per weight fragment fetched from L2 instead of one). */
#define NLAM_TUNE_WBF_HALF 6
/*   NLAM_TUNE_LIN_GEMM: nlam_linear with n % 128 == 0 on the LDS-tiled GEMM: 1 (default) = where it beats the strip kernel of
 *   rounds 2-4 (one term: everywhere; two / three terms: 6 561-row class up to K = 256, 63 784-row class from K = 512), 0 = never,
 *   2 = wherever it applies (tests); a value above 2 sets the row count from which its tiles are 128 rows high (default 32 768). */
#define NLAM_TUNE_LIN_GEMM 7
/*   NLAM_TUNE_WBF_V4: the split-bf16 wide kernels' instantiations with branch-free 16-byte chunk accesses for launches whose
 *   widths are all multiples of 4 (default 1; 0 = the generic lane-predicated accessors everywhere, for A/B runs). */
#define NLAM_TUNE_WBF_V4 8
/*   NLAM_TUNE_WGRAD_LDMA (round 6): one-term weight gradients with 256 x 256 windows on wgrad_ldma_kernel (both operands streamed
 *   by LDS-DMA into a 3-stage ring, bf16 operands read with the LDS transpose read): bit 0 = launches with bf16 operands
 *   (NLAM_F_A_BF16), bit 1 = fp32-operand one-term launches, bit 2 = fp32-class (three-term) launches; default 3.  With fp32 operands
 *   the kernel alone is no faster than the column-per-thread kernel of rounds 1-5 (profiles/round6/wgrad_check.log: one term 112 vs
 *   98 us without / 84 vs 102 us with the SiLU; three terms 67.9 vs 64.8 us at 57 616 x 256 x 256, bit-identical results without SiLU); inside the
 *   step the one-term form gains 1.2 % at cfg5 (profiles/round6/ab_wgrad_ldma_fp32.log), the three-term form nothing.  0 = the
 *   column-per-thread kernel everywhere. */
#define NLAM_TUNE_WGRAD_LDMA 9
/*   NLAM_TUNE_WGRAD_LDMA_VAR: (rows per stage, ring depth) variant of wgrad_ldma_kernel, 0 = default (A/B runs). */
#define NLAM_TUNE_WGRAD_LDMA_VAR 10
/*   NLAM_TUNE_WBF_EDGE (round 6): the factorised InteractionNet edge layers of width 512 in the one-term matrix mode and of width
 *   256 in the three-term mode on mlp_fwd_edge_kernel / mlp_bwd_edge_kernel (shapes as template constants, software-pipelined across
 *   super tiles); default 1; 0 = the template kernels (mlp_fwd_wbf_kernel / mlp_bwd_wbf_kernel); 3 = as 1 without the three-term
 *   backward. */
#define NLAM_TUNE_WBF_EDGE 11
/*   NLAM_TUNE_WGRAD_MAX_WGS (round 6): most workgroups (row slices x 256 x 256 windows) of a split-bf16 weight gradient with more
 *   than 128 output rows (default 128: half the CUs -- the launch runs beside the data-gradient chain; 256 = one per CU, rounds 2-5;
 *   4 .. 1024). */
#define NLAM_TUNE_WGRAD_MAX_WGS 12
/*   NLAM_TUNE_CHAIN_CUS (round 6): CUs a wide (> 64) fused-MLP launch sizes its persistent grid for (default 256 = all of them;
 *   16 .. 1024: values above 256 oversubscribe the CUs; set before the first launch of a step is recorded -- nlam_mlp_bwd_blocks
 *   follows it.  Measured (profiles/round6/ab_chain_cus.log): 192 .. 240 lose 1.5-5 %, 384 .. 1024 lose 0.5-5 %). */
#define NLAM_TUNE_CHAIN_CUS 13
/*   NLAM_TUNE_WGRAD_DMA_R: 32-row chunks wgrad_dma_kernel (m and every source width <= 64) requests behind one barrier: 1, 2 or
 *   4, clamped to what the LDS holds for the launch's source count (4 with one source, 2 with two or three); 0 (default) = the
 *   built-in choice per source count.  The partial sums are bit-identical for every value: a speed knob for A/B runs. */
#define NLAM_TUNE_WGRAD_DMA_R 14
int32_t nlam_set_tuning(int32_t key, int32_t value);
/* Scratch the wide kernels need for the packed (MFMA A-operand order) weights of this
 * call; 0 when the call runs on the narrow (weights-in-LDS) kernels. */
int64_t nlam_mlp_fwd_wpack_floats(const nlam_mlp_fwd_t* p);
int64_t nlam_mlp_bwd_wpack_floats(const nlam_mlp_bwd_t* p);
/* workgroups nlam_mlp_bwd launches for this call (rows of vec_partials it writes) */
int32_t nlam_mlp_bwd_blocks(const nlam_mlp_bwd_t* p);
/* 1 if this forward launch (every field but z1 / xhat / wpack set) and the backward / weight-gradient launches that belong to it
 * can run with NLAM_F_STORE_BF16 (z1, xhat, dz1, dz2 as bfloat16 rows) */
int32_t nlam_store_bf16_supported(const nlam_mlp_fwd_t* p);
/* row stride the call's dz2 buffer must have (set p->dz2_ld to it); 0 = dout (every shape but a ragged output width) */
int32_t nlam_mlp_bwd_dz2_ld(const nlam_mlp_bwd_t* p);
/* number of row slices (p->nparts) that fills the chip for this weight-gradient shape */
int32_t nlam_wgrad_nparts(const nlam_wgrad_t* p);
/* Kernel family nlam_wgrad launches for this call under the current tuning (host logic, no launch), or the NLAM_EINVAL /
 * NLAM_EUNSUP nlam_wgrad would return.  nlam_wgrad switches on this code, so the two cannot disagree.  Any nparts >= 1 is
 * served: slices without rows write zeros.  The LDS-DMA families (NLAM_WGP_DMA, NLAM_WGP_LDMA_*) fetch 16 bytes per lane: they
 * are taken only when A, every source pointer and every nonzero source batch stride (in bytes) are 16-byte aligned and, for
 * the bf16 LDS-DMA kernel, m and a bf16 source's width are multiples of 8; otherwise the call falls back to NLAM_WGP_NARROW /
 * the wgrad_wbf_kernel code of the same flags.  bf16 operands need 4-byte aligned rows (NLAM_EINVAL otherwise) and the
 * split-bf16 wide family (NLAM_EUNSUP otherwise). */
#define NLAM_WGP_SMALLN     1   /* wgrad_smalln_kernel: one source of width <= 8, m % 4 == 0                        */
#define NLAM_WGP_DMA        2   /* wgrad_dma_kernel: m and every width <= 64 and % 4                               */
#define NLAM_WGP_NARROW     3   /* wgrad_kernel: m or a width not % 4 (blockIdx.y windows above 12 blocks)          */
#define NLAM_WGP_WIDE       4   /* wgrad_wide_kernel: fp32 MFMA (no NLAM_F_MM_* bits), 128 x 128 windows           */
#define NLAM_WGP_WBF        5   /* wgrad_wbf_kernel, fp32 operands, 128 x 128 windows                              */
#define NLAM_WGP_WBF_BIG    6   /* wgrad_wbf_kernel, fp32 operands, 256 x 256 windows                              */
#define NLAM_WGP_WBF_B      7   /* wgrad_wbf_kernel, bf16 operands, 128 x 128 windows                              */
#define NLAM_WGP_WBF_B_BIG  8   /* wgrad_wbf_kernel, bf16 operands, 256 x 256 windows                              */
#define NLAM_WGP_LDMA_B     9   /* wgrad_ldma_kernel, bf16 operands (NLAM_TUNE_WGRAD_LDMA bit 0)                   */
#define NLAM_WGP_LDMA_1    10   /* wgrad_ldma_kernel, fp32 operands, one term (bit 1)                              */
#define NLAM_WGP_LDMA_3    11   /* wgrad_ldma_kernel, fp32 operands, three terms (bit 2)                           */
int32_t nlam_wgrad_plan(const nlam_wgrad_t* p);

/* Kernel instantiation nlam_mlp_fwd / nlam_mlp_bwd launch for a NARROW call (hid, dout and every source width <= 64:
 * nlam_mlp_*_family == 0), host logic, no launch -- or the NLAM_EINVAL / NLAM_EUNSUP the launch would return.  The narrow
 * launchers switch on this code, so the two cannot disagree.  A wide call gives NLAM_MLPP_NOT_NARROW (0), a call with
 * rows == 0 (which launches nothing and returns 0) NLAM_MLPP_EMPTY.  Otherwise the code is a bit field:
 *   NLAM_MLPP_KERNEL(c)  forward: NLAM_MLPP_FWD_GENERIC  mlp_fwd_kernel, fully generic shapes (fp32 MFMA)
 *                                 NLAM_MLPP_FWD_FAST     mlp_fwd_kernel, FAST shapes (fp32 MFMA)
 *                                 NLAM_MLPP_FWD_BF       mlp_fwd_bf_kernel (split-bf16)
 *                        backward: NLAM_MLPP_BWD_GENERIC mlp_bwd_kernel (fp32 MFMA)
 *                                  NLAM_MLPP_BWD_FAST    mlp_bwd_fast_kernel (fp32 MFMA or split-bf16)
 *   NLAM_MLPP_HB(c), NLAM_MLPP_OB(c)   32-column blocks of the hidden / output width the kernel is instantiated for
 *   NLAM_MLPP_NS(c)      bf16 terms per operand the kernel EXECUTES (0 = fp32 MFMA): a split-bf16 mode the flags ask for runs as
 *                        0 on shapes the split kernels do not cover
 *   NLAM_MLPP_RAG        forward: ragged-input instantiation (a single source of a width that is no multiple of 32, a ragged
 *                        output width, or concatenated pieces); backward: the ragged-output instantiation (dz2 32-padded)
 *   NLAM_MLPP_RES        forward: the residual instantiation (NLAM_F_ADD_SRC0 with `out`, or NLAM_F_ADD_SRC1)
 *   NLAM_MLPP_PRE        forward: the factorised (NLAM_F_PRE_ADD) instantiation
 *   NLAM_MLPP_CAT        forward: the concatenated-pieces (ncat > 0) instantiation */
#define NLAM_MLPP_NOT_NARROW   0
#define NLAM_MLPP_FWD_GENERIC  1
#define NLAM_MLPP_FWD_FAST     2
#define NLAM_MLPP_FWD_BF       3
#define NLAM_MLPP_BWD_GENERIC  1
#define NLAM_MLPP_BWD_FAST     2
#define NLAM_MLPP_KERNEL(c)    ((c) & 3)
#define NLAM_MLPP_HB(c)        (((c) >> 2) & 3)
#define NLAM_MLPP_OB(c)        (((c) >> 4) & 3)
#define NLAM_MLPP_NS(c)        (((c) >> 6) & 3)
#define NLAM_MLPP_RAG          (1 << 8)
#define NLAM_MLPP_RES          (1 << 9)
#define NLAM_MLPP_PRE          (1 << 10)
#define NLAM_MLPP_CAT          (1 << 11)
#define NLAM_MLPP_EMPTY        (1 << 12)
#define NLAM_MLPP_CODE(kernel, hb, ob, ns) ((kernel) | ((hb) << 2) | ((ob) << 4) | ((ns) << 6))
int32_t nlam_mlp_fwd_plan(const nlam_mlp_fwd_t* p);
int32_t nlam_mlp_bwd_plan(const nlam_mlp_bwd_t* p);

/* The same for a WIDE call (hid, dout or a source width above 64: nlam_mlp_*_family != 0): the instantiation nlam_mlp_fwd /
 * nlam_mlp_bwd launch under the current tuning (nlam_set_tuning), host logic, no launch -- or the NLAM_EINVAL / NLAM_EUNSUP the
 * launch would return.  The wide launchers switch on this code, so the two cannot disagree.  A narrow call gives
 * NLAM_MLPW_NOT_WIDE (0), a call with rows == 0 NLAM_MLPW_EMPTY.  Otherwise the code is a bit field:
 *   NLAM_MLPW_KERNEL(c)  NLAM_MLPW_WIDE  mlp_fwd_wide_kernel / mlp_bwd_wide_kernel<NWV, FB> (fp32 MFMA, one tile per workgroup)
 *                        NLAM_MLPW_WBF   mlp_fwd_wbf_kernel / mlp_bwd_wbf_kernel (split-bf16 super-tile template)
 *                        NLAM_MLPW_EDGE  mlp_fwd_edge_kernel / mlp_bwd_edge_kernel<NS, D, SBF> (D = 512 with one term, 256 with three)
 *   NLAM_MLPW_NS(c)      bf16 terms per operand the kernel EXECUTES: 0 (fp32 MFMA), 1 or 3.  Two requested terms run as three; in
 *                        the forward one requested term runs as three when the hidden width has an odd number of 32-column blocks;
 *                        launches below the super-tile threshold (NLAM_TUNE_WBF_MIN_SUPERTILES), widths that are no multiples
 *                        of 4 and, in the forward, an aggregating launch (aggr != NULL) whose dout is no multiple of 4 run as 0
 *                        (with NLAM_F_PRE_ADD, which the fp32 kernels do not have, such a launch is NLAM_EUNSUP)
 *   NLAM_MLPW_PLAN(c)    NLAM_MLPW_WBF only: the launch geometry.  Forward (WbfPlan) 1: d <= 128, 2: d <= 256, 3: d <= 512 on 8-wave
 *                        workgroups; 4: d <= 256 on 64-row super tiles (mid-size launches); 5, 6, 7: the 4-wave half plans
 *                        (NLAM_TUNE_WBF_HALF bits 0 and 2).  Backward (WbfBwdPlan) 1, 2, 3 as in the forward; 5: the 4-wave plan of
 *                        128 < d <= 256 (NLAM_TUNE_WBF_HALF bit 1)
 *   NLAM_MLPW_NWV(c), NLAM_MLPW_FB(c)   NLAM_MLPW_WIDE only: waves per workgroup and 32-feature blocks per wave, <4, 1>, <8, 1> or <8, 2>
 *   NLAM_MLPW_V4         NLAM_MLPW_WBF only: the instantiation with branch-free 16-byte chunk accesses (every width a multiple of 4,
 *                        backward: no padded dz2 either; NLAM_TUNE_WBF_V4)
 *   NLAM_MLPW_SBF        the bf16-storage instantiation (NLAM_F_STORE_BF16).  Stored values are rounded to nearest, ties to even
 *                        (v_cvt_pk_bf16_f32). */
#define NLAM_MLPW_NOT_WIDE     0
#define NLAM_MLPW_WIDE         1
#define NLAM_MLPW_WBF          2
#define NLAM_MLPW_EDGE         3
#define NLAM_MLPW_KERNEL(c)    ((c) & 3)
#define NLAM_MLPW_NS(c)        (((c) >> 2) & 3)
#define NLAM_MLPW_PLAN(c)      (((c) >> 4) & 7)
#define NLAM_MLPW_NWV(c)       (((c) >> 7) & 15)
#define NLAM_MLPW_FB(c)        (((c) >> 11) & 3)
#define NLAM_MLPW_V4           (1 << 13)
#define NLAM_MLPW_SBF          (1 << 14)
#define NLAM_MLPW_EMPTY        (1 << 15)
#define NLAM_MLPW_CODE(kernel, ns, plan, nwv, fb) ((kernel) | ((ns) << 2) | ((plan) << 4) | ((nwv) << 7) | ((fb) << 11))
int32_t nlam_mlp_fwd_wide_plan(const nlam_mlp_fwd_t* p);
int32_t nlam_mlp_bwd_wide_plan(const nlam_mlp_bwd_t* p);

int32_t nlam_mlp_fwd(const nlam_mlp_fwd_t* p, void* hip_stream);
int32_t nlam_mlp_bwd(const nlam_mlp_bwd_t* p, void* hip_stream);

/* Tiled-GEMM family for any width (the widths above nlam_max_width() that nlam_mlp_fwd / nlam_mlp_bwd answer NLAM_EUNSUP for;
 * widths <= 512 are accepted too, for comparisons).  Same structs and semantics as nlam_mlp_fwd / nlam_mlp_bwd -- gathered /
 * concatenated sources (any width >= 1), SiLU or NLAM_F_NO_ACT, LayerNorm, NLAM_F_ADD_SRC0 / _SRC1, out / out_idx, segment
 * aggregation (sum or NLAM_F_MEAN) over the tile schedule, dmode 0-3, z1 / xhat / rstd, dz1 / dz2, vec_partials -- run as a
 * chain of kernels (LDS-tiled split-bf16 GEMMs, LayerNorm row kernels, fixed-order segment sums) over intermediates in `wpack`
 * (wpack_floats >= the workspace query; nothing is packed, the weights are read in nn.Linear layout).  Matrix modes: one bf16
 * term for NLAM_F_MM_BF16X1, three terms for every other mode (f32 and bf16x2 included).  Not served (NLAM_EUNSUP):
 * NLAM_F_PRE_ADD, NLAM_F_STORE_BF16, NLAM_F_ACC_DSRC0, NLAM_F_LEAF_WGRAD, concatenated pieces (ncat > 0).  The backward needs
 * z1, dz1 and dz2 (dz2_ld 0 or dout) and writes nlam_mlp_bwd_gemm_blocks(p) rows of vec_partials (always 256; blocks without
 * rows hold zeros).  Workspace queries return the floats, or the NLAM_EINVAL / NLAM_EUNSUP the launch would return; a forward
 * with z1 == NULL keeps z1 in the workspace (the query grows by batch * rows * hid).  Every sum has a fixed order and the results
 * are bit-identical run to run, EXCEPT over NLAM_TILE_SPLIT tiles: the pieces of such a receiver are added with atomicAdd, in no
 * fixed order, into a destination the caller must have zeroed -- this applies to both `aggr` (forward) and every dmode-3 `dsrc`
 * (backward).  rows == 0 returns 0 without a workspace: `aggr` rows and dmode-3 `dsrc` rows of the receivers the tile list covers
 * and the vec_partials rows are written as zeros, nothing else is written. */
int64_t nlam_mlp_fwd_gemm_workspace_floats(const nlam_mlp_fwd_t* p);
int64_t nlam_mlp_bwd_gemm_workspace_floats(const nlam_mlp_bwd_t* p);
int32_t nlam_mlp_bwd_gemm_blocks(const nlam_mlp_bwd_t* p);
int32_t nlam_mlp_fwd_gemm(const nlam_mlp_fwd_t* p, void* hip_stream);
int32_t nlam_mlp_bwd_gemm(const nlam_mlp_bwd_t* p, void* hip_stream);

/* Pre-packed weights for the narrow (hid, dout <= 64) split-bf16 kernels.  The reference's nn.Linear weights
 * (utils/networks.py:8-40) change once per optimizer step (models/module.py:293-304) but every fused-MLP workgroup of
 * every launch used to re-read them as fp32 and split them into bf16 terms itself.  nlam_mlp_pack writes, for a table of
 * MLPs, the images the kernels lay out in LDS; nlam_mlp_fwd / nlam_mlp_bwd (and the grouped launches) then take such an
 * image in `wpack` (wpack_floats = its size) and fetch it by LDS-DMA.  An image is valid for the (source widths, hid,
 * dout, NLAM_F_PRE_ADD, matrix mode, ldw1) it was packed for and until the weights change; passing NULL keeps the
 * self-staging path.  Launches the images do not serve (fp32 matrix mode, generic shapes) ignore `wpack`; the wide
 * kernels keep their own meaning of `wpack` (scratch they pack per launch), so pass an image to narrow launches only.
 * nlam_mlp_pack_floats: size of the forward (which = 0) / backward (which = 1) image, 0 when the shape is not served. */
typedef struct {
    const float* W1;       /* (hid, ldw1 or sum of widths) */
    const float* W2;       /* (dout, hid) */
    float* fwd_image;      /* >= nlam_mlp_pack_floats(job, 0) floats, 16-byte aligned, or NULL */
    float* bwd_image;      /* >= nlam_mlp_pack_floats(job, 1) floats, 16-byte aligned, or NULL */
    int32_t hid, dout, nsrc;
    int32_t ldw1;          /* floats between rows of W1; 0 = sum of the GEMM sources' widths */
    int32_t width[NLAM_MAX_SRC];
    uint32_t flags;        /* NLAM_F_PRE_ADD | NLAM_F_MM_BF16X1..3 */
} nlam_pack_job_t;
int64_t nlam_mlp_pack_floats(const nlam_pack_job_t* job, int32_t which);
/* The same idea for the WIDE kernels, whose `wpack` scratch is packed per launch by default (a pack kernel in front of every
 * wide forward / backward launch: 184 + 147 launches per Hi-LAM d = 128 step).  nlam_mlp_fwd_pack_records /
 * nlam_mlp_bwd_pack_records describe, as opaque 64-byte records, the pack jobs that fill p->wpack for exactly the launch `p`
 * (same shapes, rows, tiles, batch, flags, dmode: they select the kernel family and with it the layout); they return the
 * number of records (<= 4; 0 for a narrow launch) and the record kind (0: fp32 A-fragment order, 1 / 3: one / three bf16
 * terms).  nlam_pack_records runs a table of records of ONE kind (device memory) in one launch.  A launch whose wpack was
 * filled this way passes NLAM_F_WPACK_READY. */
typedef struct {
    unsigned char bytes[64];
} nlam_pack_rec_t;
int32_t nlam_mlp_fwd_pack_records(const nlam_mlp_fwd_t* p, nlam_pack_rec_t* out, int32_t cap, int32_t* kind);
int32_t nlam_mlp_bwd_pack_records(const nlam_mlp_bwd_t* p, nlam_pack_rec_t* out, int32_t cap, int32_t* kind);
int32_t nlam_pack_records(const nlam_pack_rec_t* recs_device, int32_t n, int32_t kind, void* hip_stream);
/* `jobs_device`: the job table in DEVICE memory (addresses are stable, so it is uploaded once); one launch packs all */
int32_t nlam_mlp_pack(const nlam_pack_job_t* jobs_device, int32_t njobs, void* hip_stream);

/* GROUPED launches: n <= NLAM_MAX_GROUP independent fused MLPs of the same kernel shape in ONE grid (every workgroup is
 * bound to one member, the 256 workgroups are dealt in proportion to the members' tile counts).  For the embedders of
 * the static grid / mesh / edge features (utils.make_mlp blocks called back to back at graph/base.py:286-295,
 * hierarchical.py:195-231): as separate launches each is a latency-bound chain link.  Covered: single-source members
 * without residual / aggregation whose widths share the 32-column block counts, split-bf16 matrix modes, hid and dout
 * <= 64 (NLAM_EUNSUP otherwise: launch the members one by one).  nlam_mlp_group_blocks gives the workgroups each
 * member gets: member k of the backward writes blocks[k] rows of its vec_partials. */
#define NLAM_MAX_GROUP 8
int32_t nlam_mlp_group_blocks(const int64_t* tiles, int32_t n, int32_t* blocks);
int32_t nlam_mlp_fwd_group(const nlam_mlp_fwd_t* ps, int32_t n, void* hip_stream);
int32_t nlam_mlp_bwd_group(const nlam_mlp_bwd_t* ps, int32_t n, void* hip_stream);
/* Round 4: the grouped entry points also take members of the fp32 WIDE family (a width in 65 .. 128 columns below the
 * split-bf16 super-tile threshold, or matrix mode 0): the chunks of a `SplitMLPs` layer (gnn_layers.py:274-324 called from
 * hi_lam_parallel.py:127-143 -- 3 .. 206 tiles each at the bench size) and the static-feature embedders at d = 128; any
 * source / residual / aggregation set the single launch takes, one kernel shape (hid, dout, flags, LayerNorm or not; source
 * counts and widths may differ) for all members, each with its own `wpack` scratch.  nlam_mlp_*_family says which
 * kernel family a launch runs on (0 narrow, 1 fp32 wide, 2 split-bf16 wide: members of family 2 are launched one by one);
 * nlam_mlp_bwd_group_blocks gives the workgroups (= vec_partials rows written) per member of a grouped backward of either
 * family, checking the members as the launch would. */
int32_t nlam_mlp_fwd_family(const nlam_mlp_fwd_t* p);
int32_t nlam_mlp_bwd_family(const nlam_mlp_bwd_t* p);
int32_t nlam_mlp_bwd_group_blocks(const nlam_mlp_bwd_t* ps, int32_t n, int32_t* blocks);
int32_t nlam_wgrad(const nlam_wgrad_t* p, void* hip_stream);
/* n <= NLAM_MAX_GROUP weight gradients of one shape (m, source widths, flags) in ONE grid, each member with its own rows and
 * `partials` (nparts = nlam_wgrad_nparts of that member): the chunks of a `SplitMLPs` layer (gnn_layers.py:311-324).  Members of
 * the split-bf16 wide family with fp32 operands; NLAM_EUNSUP otherwise (launch them one by one). */
int32_t nlam_wgrad_group(const nlam_wgrad_t* ps, int32_t n, void* hip_stream);
/* The same for the NARROW fp32 family (plan NLAM_WGP_DMA: m and every source width <= 64 and % 4): the dW1 -- or the dW2 --
 * launches of several small MLPs (the node MLPs on a 6 561-node mesh: one or two 32-row chunks per workgroup, 12-15 us a launch
 * that is nearly all fixed cost) in ONE grid.  Member k runs on workgroups first[k] .. first[k] + nparts_k with the body of its
 * own nlam_wgrad launch -- same nparts, same chunks per workgroup, same order of sums -- so its `partials` are bit-identical to
 * that launch's, whatever the other members and their order.  Up to NLAM_MAX_GROUP members (passed by value: 8 x 120 bytes).
 *   NLAM_EINVAL: ps NULL, n < 1, n > NLAM_MAX_GROUP, a member nlam_wgrad_plan calls invalid (NULL A / partials, n != sum of
 *                the widths, ..), a NULL source, rows or batch < 1, or nparts != nlam_wgrad_nparts(member);
 *   NLAM_EUNSUP: a member whose plan is not NLAM_WGP_DMA or whose shape nlam_wgrad_dma_group_supported refuses, or members that
 *                differ in m, n, nsrc, a source width or flags.
 * Members may differ in rows, batch, pointers, gather indices, batch strides and nparts.  On any error nothing is launched.
 * nlam_wgrad_dma_group_supported: 1 when the SHAPE of `p` (m, source count and widths, flags; no pointer is read) is one the
 * grouped kernel is built for -- the (32-column blocks per wave, sources) pairs (1, 1) with or without NLAM_F_SILU_B, (2, 2)
 * and (3, 3) without --, else 0.  The alignment half of the plan (16-byte aligned A, sources and batch strides) is checked by
 * the launch. */
int32_t nlam_wgrad_dma_group_supported(const nlam_wgrad_t* p);
int32_t nlam_wgrad_dma_group(const nlam_wgrad_t* ps, int32_t n, void* hip_stream);

/* out[b, s, :] = scale(s) * sum_{q in [ptr[s], ptr[s+1])} in[b, order[q], :]   (order NULL = q, scale NULL = 1; `order` may name a
 * row more than once; an empty segment is written as zeros).  Which of the three fp32 kernels runs -- it decides the summation
 * order, not the contract -- is what nlam_segment_sum_groups answers: the lane groups that share a segment.  With
 * rows = in_bstride / width (0 when in_bstride is 0: a shared input's row count is not known),
 *   width % 4 == 0, width / 4 a divisor of 64 of at most 32 (width 4, 8, 16, 32, 64 or 128) and rows >= 16 * nseg (segments of
 *   16+ rows on average): segment_sum_split_kernel<S>, S = 4 lane groups for width <= 64, S = 2 for width 128 -- group g sums rows
 *   g, g + S, ... of the segment, eight in flight, and the groups are combined in a fixed order;
 *   everything else: 1 = segment_sum_kernel, one thread per (segment, 4 columns), 16-byte accesses when width % 4 == 0.
 * nlam_segment_sum, _acc and _add take the same kernel for the same (in_bstride, nseg, width).  NLAM_EINVAL for width < 1 or nseg < 0. */
int32_t nlam_segment_sum_groups(int64_t in_bstride, int32_t nseg, int32_t width);
int32_t nlam_segment_sum(const float* in, int64_t in_bstride, const int32_t* ptr, const int32_t* order,
                         const float* scale, float* out, int32_t nseg, int32_t width, int32_t batch,
                         void* hip_stream);
/* same, added onto what `out` already holds (out += ...): lets the sender-side gradient of a layer whose senders
 * and receivers are the same nodes (mesh <-> mesh) land in the receiver-side gradient buffer instead of a second
 * tensor that autograd would add with one more launch */
int32_t nlam_segment_sum_acc(const float* in, int64_t in_bstride, const int32_t* ptr, const int32_t* order,
                         const float* scale, float* out, int32_t nseg, int32_t width, int32_t batch,
                         void* hip_stream);
/* out[b, s] += extra[b, s] + scale[s] * sum_{q in ptr[s]:ptr[s+1]} in[b, order[q]]   (round 6: a layer's sender-side gradient, its
 * receiver-side gradient `extra` and the node MLP's gradient already in `out` meet in ONE pass -- the torch add launch behind
 * every mesh <-> mesh layer's backward (gnn_layers.py:110-157: send_rep is rec_rep) is gone). */
int32_t nlam_segment_sum_add(const float* in, int64_t in_bstride, const int32_t* ptr, const int32_t* order, const float* scale,
                             const float* extra, float* out, int32_t nseg, int32_t width, int32_t batch, void* hip_stream);

/* nlam_segment_sum over input rows stored as bfloat16 (width % 8 == 0; out is float): the dz1 rows of a backward launch that ran with
 * NLAM_F_STORE_BF16 */
int32_t nlam_segment_sum_bf16(const uint16_t* in, int64_t in_bstride, const int32_t* ptr, const int32_t* order,
                              const float* scale, float* out, int32_t nseg, int32_t width, int32_t batch, void* hip_stream);

/* buf[b, dst[s], :] = sum_{q in [ptr[s], ptr[s+1])} buf[b, src[q], :], q ascending, for s < n; rows of `width` floats, batch
 * stride `bstride` floats.  Second pass of the DETERMINISTIC reduction of receivers with more in-edges than a 32-row tile
 * (reference: PyG's scatter under Trainer(deterministic=True), gnn_layers.py:175-189, train_model.py:566): the tile schedule
 * gives every piece of such a receiver a virtual segment behind the real ones (rowptr / inv_deg are extended accordingly, the
 * kernels see ordinary one-receiver tiles and use plain stores), and this sums the pieces into the receiver's row.  The
 * one-pass alternative -- NLAM_TILE_SPLIT tiles, atomic adds into a zeroed buffer -- stays available to ABI users. */
int32_t nlam_split_combine(float* buf, int64_t bstride, const int32_t* ptr, const int32_t* src, const int32_t* dst, int32_t n,
                           int32_t width, int32_t batch, void* hip_stream);

/* out[i] (+)= sum_p partials[p * stride + i], i < n ; accumulate != 0 adds into out */
int32_t nlam_reduce_partials(const float* partials, int32_t nparts, int64_t stride, int32_t n, float* out,
                             int32_t accumulate, void* hip_stream);

/* Up to NLAM_MAX_REDUCE_JOBS reductions of the nlam_reduce_partials kind in ONE launch: the dW1, dW2,
 * db1, db2, dgamma, dbeta of one fused-MLP backward (autograd's AccumulateGrad `grad += new`, folded in
 * when accumulate != 0 and out points into the gradient buffer). */
#define NLAM_MAX_REDUCE_JOBS 40   /* e.g. the 4 x 9 reductions of the four static-feature embedders of one grouped backward */
typedef struct {
    const float* partials;
    float* out;
    int64_t stride;        /* elements between partials */
    int32_t nparts;
    int32_t n;
    int32_t accumulate;
    int32_t ncols;         /* > 0: element i of the reduction goes to out[(i / ncols) * ld + i % ncols] (a column block */
    int32_t ld;            /*      of a wider row-major matrix: one source's slice of W1.grad); 0: out[i]                */
    int32_t _pad;
} nlam_reduce_job_t;
typedef struct {
    nlam_reduce_job_t job[NLAM_MAX_REDUCE_JOBS];
    int32_t njobs;
    int32_t _pad;
} nlam_reduce_jobs_t;
int32_t nlam_reduce_jobs(const nlam_reduce_jobs_t* jobs, void* hip_stream);
/* waves per nlam_reduce_jobs workgroup (NLAM_RED_WAVES of the build): job element i sums parts [w per, (w + 1) per) in wave w,
 * per = ceil(nparts / waves), and the waves' sums are added in wave order -- the summation order the results depend on */
int32_t nlam_reduce_jobs_waves(void);

/* Node-level product of the factorised edge MLP (NLAM_F_PRE_ADD) and its data gradient:
 *   out[r][h] (+)= sum_c x[r][c] * W[h * ldn + c * ldk],   r < rows, h < n, c < k
 * (forward: W = W1 + column offset, ldn = row stride of W1, ldk = 1; backward: the transposed product with
 * ldn = 1, ldk = row stride of W1).  x (rows, k) and out (rows, n) are contiguous and 16-byte aligned; k, n multiples of 32 up to
 * 64, or multiples of 64 (n % 128 == 0: k a multiple of 32) up to nlam_max_width(), see nlam_linear_plan; rows of out past
 * `rows` are not written; matrix mode from flags (NLAM_F_MM_BF16X1..3; the fp32-MFMA mode is not instantiated: NLAM_EUNSUP). */
typedef struct {
    const float* x;
    const float* W;
    float* out;
    int64_t rows;
    int64_t ldn;
    int64_t ldk;
    int32_t k;
    int32_t n;
    int32_t accumulate;    /* != 0: out += */
    uint32_t flags;
    const float* W2;       /* optional second product over the same x (widths above 64 only): out2 = x . A2^T, same shapes and */
    float* out2;           /* strides (the sender- and the receiver-side product of a layer whose senders are its receivers)   */
} nlam_linear_t;
int32_t nlam_linear(const nlam_linear_t* p, void* hip_stream);
/* Which kernel instantiation nlam_linear launches for *p under the current tuning (nlam_set_tuning), host logic, no launch -- or the
 * NLAM_EINVAL / NLAM_EUNSUP the launch would return.  nlam_linear switches on this code, so the two cannot disagree.  rows == 0
 * gives NLAM_LINP_EMPTY (the launch returns 0 and writes nothing).  Otherwise the code is a bit field:
 *   NLAM_LINP_KERNEL(c)  NLAM_LINP_BF    linear_bf_kernel<KB, MB, NS>: k, n <= 64, W staged once per persistent workgroup, one wave =
 *                                        one 32-row tile, any ldn / ldk and any 4-byte alignment of W
 *                        NLAM_LINP_BFW   linear_bfw_kernel<NS>: k, n multiples of 64 up to nlam_max_width(), 64 x 64 weight blocks,
 *                                        any ldn / ldk and any 4-byte alignment of W (the strip kernel)
 *                        NLAM_LINP_GEMM  linear_gemm_kernel<NS, WN, TA, SK>: n % 128 == 0, k % 32 == 0, both up to nlam_max_width(),
 *                                        and a layout it can read: ldk == 1 with ldn % 4 == 0 and W (and W2) 16-byte aligned, or
 *                                        ldn == 1 (NLAM_LINP_TA); taken where NLAM_TUNE_LIN_GEMM says so.  A shape only this
 *                                        kernel serves (k % 64 != 0) in a layout it cannot read is NLAM_EUNSUP
 *   NLAM_LINP_NS(c)      bf16 terms per operand the kernel EXECUTES: always the 1, 2 or 3 that flags request
 *   NLAM_LINP_KB(c), NLAM_LINP_MB(c)   NLAM_LINP_BF only: k / 32 and n / 32, 1 or 2
 *   NLAM_LINP_RESIDENT   NLAM_LINP_BFW only: k <= 256 and NLAM_TUNE_LIN_WGS > 0 -- an output pair's whole weight strip stays in LDS and
 *                        at most NLAM_TUNE_LIN_WGS workgroups walk rounds of eight 32-row tiles; otherwise the strip is streamed
 *                        through two LDS buffers
 *   NLAM_LINP_WN(c)      NLAM_LINP_GEMM only: 2 = 128-row tiles (rows >= the threshold of NLAM_TUNE_LIN_GEMM, default 32 768), 1 = 64-row
 *                        tiles.  Row tiles are padded to a multiple of eight; the workgroups of the padding return at once
 *   NLAM_LINP_SK(c)      NLAM_LINP_GEMM only: K = 16 steps per staged chunk, 4 (one term, 64-row tiles, k % 64 == 0) or 2
 *   NLAM_LINP_TA         NLAM_LINP_GEMM only: the transposed layout (ldn == 1)
 *   NLAM_LINP_DUAL       the launch also computes out2 from W2 (NLAM_LINP_BFW and NLAM_LINP_GEMM) */
#define NLAM_LINP_BF           1
#define NLAM_LINP_BFW          2
#define NLAM_LINP_GEMM         3
#define NLAM_LINP_KERNEL(c)    ((c) & 3)
#define NLAM_LINP_NS(c)        (((c) >> 2) & 3)
#define NLAM_LINP_KB(c)        (((c) >> 4) & 3)
#define NLAM_LINP_MB(c)        (((c) >> 6) & 3)
#define NLAM_LINP_RESIDENT     (1 << 8)
#define NLAM_LINP_WN(c)        (((c) >> 9) & 3)
#define NLAM_LINP_SK(c)        (((c) >> 11) & 7)
#define NLAM_LINP_TA           (1 << 14)
#define NLAM_LINP_DUAL         (1 << 15)
#define NLAM_LINP_EMPTY        (1 << 16)
#define NLAM_LINP_CODE(kernel, ns)     ((kernel) | ((ns) << 2))
#define NLAM_LINP_BF_SHAPE(kb, mb)     (((kb) << 4) | ((mb) << 6))
#define NLAM_LINP_GEMM_SHAPE(wn, sk)   (((wn) << 9) | ((sk) << 11))
int32_t nlam_linear_plan(const nlam_linear_t* p);
/* 1 when nlam_mlp_fwd / nlam_mlp_bwd / nlam_linear have a factorised (NLAM_F_PRE_ADD) kernel for this problem, else 0
 * (only nsrc, the source widths, hid, dout, flags, ntiles and batch of *p are read) */
int32_t nlam_pre_add_supported(const nlam_mlp_fwd_t* p);

/* Training loss of ForecasterModule.training_step (models/module.py:463-510) with metrics.wmse /
 * mask_and_reduce_metric (metrics.py:37-137) for a per-variable std:
 *   loss = scale * sum_{row, v} row_weight[row % nodes] * inv_var[v] * (pred - target)^2,
 * row_weight = interior mask / #interior nodes, scale = 1 / (batch * ar_steps).  The forward writes one
 * partial per block (nparts blocks; finish with nlam_reduce_partials, fixed order); the backward takes the
 * upstream scalar gradient from device memory. */
int32_t nlam_wmse_fwd(const float* pred, const float* target, const float* inv_var, const float* row_weight, int64_t rows,
                      int32_t nodes, int32_t nvars, float scale, float* partials, int32_t nparts, void* hip_stream);
int32_t nlam_wmse_bwd(const float* pred, const float* target, const float* inv_var, const float* row_weight,
                      const float* gscalar, int64_t rows, int32_t nodes, int32_t nvars, float scale, float* dpred,
                      void* hip_stream);

/* State update of one autoregressive step, all optional terms in one pass over (rows, width) fp32 rows:
 *   out[r][f] = a[r % nodes] * x[r][f]  +  c[r % nodes] * ( y[r][f] + z[r][f] * s[f] + m[f] )
 * NULL x (with a), y, z (with s), m drop their term; NULL c means 1.  Replaces the elementwise chains
 *   prev_state + (delta * diff_std + diff_mean)                step_predictors/graph/base.py:331-343, base.py:335-396 (no clamp)
 *   boundary_mask * true_state + interior_mask * pred_state    forecasters/autoregressive.py:128-131
 * and, with the roles of the operands permuted, their backward (g * interior_mask, g * diff_std). */
int32_t nlam_affine_mix(const float* x, const float* a, const float* y, const float* c, const float* z, const float* s,
                        const float* m, float* out, int64_t rows, int32_t nodes, int32_t width, void* hip_stream);

/* ForecasterModule.on_after_batch_transfer (models/module.py:326-367): up to NLAM_MAX_STD_JOBS tensors
 * standardised in ONE launch,  out[r][c] = (x[r][c] - mean[c / rep]) / std[c / rep].  `rep` = 1 for the states;
 * for the forcing it is the window size: the per-feature statistics are tiled feature-major over the window
 * (repeat_interleave, module.py:352-358).  IEEE subtraction and division: bit-equal to the reference's formula. */
#define NLAM_MAX_STD_JOBS 4
typedef struct {
    const float* x;
    float* out;
    const float* mean;     /* (width / rep) */
    const float* std;      /* (width / rep), already clamped to >= eps by the caller (module.py:306-324) */
    int64_t rows;
    int32_t width;
    int32_t rep;
} nlam_std_job_t;
typedef struct {
    nlam_std_job_t job[NLAM_MAX_STD_JOBS];
    int32_t njobs;
    int32_t _pad;
} nlam_std_jobs_t;
int32_t nlam_standardize(const nlam_std_jobs_t* jobs, void* hip_stream);

/* The elementwise tail of ONE autoregressive step in one pass (forward) and one pass (backward):
 *   new   = prev + delta * dstd[f] + dmean[f]          step_predictors/graph/base.py:331-343 (no clamping configured)
 *   pred  = bmask[n] * truth + (1 - bmask[n]) * new     forecasters/autoregressive.py:128-131
 *   loss += scale * row_weight[n] * inv_var[f] * (pred - target)^2    metrics.py:37-137 + module.py:463-510
 * rows = batch * nodes rows of `width` state variables; dstd / dmean may be NULL (1 / 0).  The forward writes one loss
 * partial per block (`nparts` blocks; finish with nlam_reduce_partials).  The backward takes the gradient of `pred` that
 * later AR steps produced (g_pred, NULL for the last step) and the scalar gradient of the loss from device memory:
 *   G = g_pred + 2 * scale * gloss * row_weight[n] * inv_var[f] * (pred - target)
 *   d_delta = (1 - bmask[n]) * dstd[f] * G ,   d_prev = (1 - bmask[n]) * G   (either output may be NULL). */
int32_t nlam_step_tail_fwd(const float* delta, const float* prev, const float* truth, const float* target, const float* dstd,
                           const float* dmean, const float* bmask, const float* inv_var, const float* row_weight, float scale,
                           float* pred, float* partials, int32_t nparts, int64_t rows, int32_t nodes, int32_t width,
                           void* hip_stream);
int32_t nlam_step_tail_bwd(const float* g_pred, const float* gloss, const float* pred, const float* target, const float* dstd,
                           const float* bmask, const float* inv_var, const float* row_weight, float scale, float* d_delta,
                           float* d_prev, int64_t rows, int32_t nodes, int32_t width, void* hip_stream);

/* The training losses the reference selects with --loss (train_model.py:271-276, metrics.DEFINED_METRICS, metrics.py:87-386).
 * With d = pred - target, s the std and z = (target - pred) / s, the entry of each kind is
 *   NLAM_LOSS_MSE         d^2                     (s ignored: the reference replaces it with ones)
 *   NLAM_LOSS_MAE         |d|                     (s ignored)
 *   NLAM_LOSS_WMSE        d^2 / s^2
 *   NLAM_LOSS_WMAE        |d| / s
 *   NLAM_LOSS_NLL         d^2 / (2 s^2) + log s + log(2 pi) / 2
 *   NLAM_LOSS_CRPS_GAUSS  s * (z * (2 Phi(z) - 1) + 2 phi(z) - pi^-1/2)
 * and the reduction is that of nlam_wmse_fwd:  loss = scale * sum_{row, v} row_weight[row % nodes] * entry.  sign(0) = 0 in the
 * gradients of the absolute errors (torch.l1_loss).  The std is not validated on the device (s > 0 is the caller's contract). */
#define NLAM_LOSS_MSE        1
#define NLAM_LOSS_MAE        2
#define NLAM_LOSS_WMSE       3
#define NLAM_LOSS_WMAE       4
#define NLAM_LOSS_NLL        5
#define NLAM_LOSS_CRPS_GAUSS 6
#define NLAM_LOSS_MAX_VARS   4096   /* nvars of a per-variable std (its constants live in LDS); NLAM_EUNSUP above */
/* One masked loss pass over (rows, nvars) fp32 rows, rows = batch * ar_steps * nodes.  The std is per entry (`std`, the
 * rollout's pred_std of an output_std model) or, with std == NULL, per variable (`var_std`, module.py:157-178); mse / mae read
 * neither.  nlam_loss_fwd writes one partial per block into partials[0 .. nparts) (finish with nlam_reduce_partials, fixed
 * order: bit-identical run to run); nlam_loss_bwd takes the upstream scalar gradient from gscalar (device memory: capturable)
 * and writes dpred and, when dstd != NULL (per-entry std only), dstd; both are 0 on rows of weight 0.  NLAM_EINVAL for an
 * unknown kind, null pointers or sizes that do not fit together (rows % nodes != 0), before anything is launched. */
typedef struct {
    const float* pred;         /* (rows, nvars) */
    const float* target;       /* (rows, nvars) */
    const float* std;          /* (rows, nvars) per-entry std, or NULL */
    const float* var_std;      /* (nvars) per-variable std, read when std == NULL */
    const float* row_weight;   /* (nodes) interior mask / #interior nodes */
    const float* gscalar;      /* backward: the scalar gradient of the loss (device) */
    float* partials;           /* forward: (nparts) */
    float* dpred;              /* backward: (rows, nvars) */
    float* dstd;               /* backward: (rows, nvars) or NULL */
    int64_t rows;
    int32_t nodes;
    int32_t nvars;
    int32_t kind;              /* NLAM_LOSS_* */
    int32_t nparts;
    float scale;               /* 1 / (batch * ar_steps) */
    int32_t _pad;
} nlam_loss_t;
int32_t nlam_loss_fwd(const nlam_loss_t* p, void* hip_stream);
int32_t nlam_loss_bwd(const nlam_loss_t* p, void* hip_stream);
/* nlam_step_tail_fwd / _bwd with the loss term of any NLAM_LOSS_* kind for a per-variable std (`var_std`, may be NULL for mse /
 * mae) instead of inv_var:  loss += scale * row_weight[n] * entry(pred - target, var_std[f]),
 *   G = g_pred + scale * gloss * row_weight[n] * d entry / d pred.  Still one pass each way per AR step: one kernel template
 * serves both pairs.  This pair asks for rows % nodes == 0 and width <= NLAM_LOSS_MAX_VARS (NLAM_EUNSUP above). */
int32_t nlam_step_tail_loss_fwd(int32_t kind, const float* delta, const float* prev, const float* truth, const float* target,
                                const float* dstd, const float* dmean, const float* bmask, const float* var_std,
                                const float* row_weight, float scale, float* pred, float* partials, int32_t nparts, int64_t rows,
                                int32_t nodes, int32_t width, void* hip_stream);
int32_t nlam_step_tail_loss_bwd(int32_t kind, const float* g_pred, const float* gloss, const float* pred, const float* target,
                                const float* dstd, const float* bmask, const float* var_std, const float* row_weight, float scale,
                                float* d_delta, float* d_prev, int64_t rows, int32_t nodes, int32_t width, void* hip_stream);

/* The step tail with the two options of a step predictor that the pair above leaves out, still one pass each way:
 * output clamping (StepPredictor.get_clamped_new_state, step_predictors/base.py) and a predicted std (output_std).
 * Per element (row, f), n = row % nodes, F = nvars, ld = delta_ld (F, or 2 F with a std head):
 *   r    = delta[row * ld + f] * dstd[f] + dmean[f]
 *   new  = prev + r                                                                   NLAM_CLAMP_NONE
 *        = lo + (hi - lo) * sigmoid(log(u / (1 - u)) + r), u = clamp((prev - lo) / (hi - lo), 1e-6, 1 - 1e-6)   NLAM_CLAMP_BOTH
 *        = lo + softplus(inv_softplus(prev - lo) + r)                                 NLAM_CLAMP_LOWER
 *        = hi - softplus(inv_softplus(hi - prev) - r)                                 NLAM_CLAMP_UPPER
 *   pred = bmask[n] * truth + (1 - bmask[n]) * new
 *   std  = softplus(delta[row * ld + F + f])        -> pred_std (rows, F), with a std head
 *   loss += scale * row_weight[n] * entry(pred - target; consts[f], or this element's std)
 * The clamp of u is at the fp32 values float32(1e-6) and float32(1 - 1e-6) = 1 - 17 * 2^-24, as torch clamps an fp32 tensor: beyond
 * the upper one 1 - u is 1.3 % above 1e-6, so a float64 evaluation with the decimal constants differs there by that much.
 * softplus (beta 1, threshold 20) and inv_softplus (utils/tensor.py, lower clamp log(float32(1 + 1e-6))) are torch's, and the
 * backward gives the derivatives autograd gives that formulation (0 through a clamp outside its bounds).  lo / hi are the
 * standardised limits, lo < hi is the caller's contract; entries of variables without that limit are not read.
 * Forward: target == NULL and partials == NULL means no loss term (inference); otherwise one partial per block as above.
 * Backward: writes d_prev (may be NULL) and the whole d_delta (rows, ld): the mean half G * d new / d r * dstd[f] with
 * G = (1 - bmask[n]) * (g_pred + scale * gloss * row_weight[n] * d entry / d pred), and the std half
 * (g_std + scale * gloss * row_weight[n] * d entry / d std) * softplus'(raw), written also where it is zero.  g_pred and
 * g_std may be NULL; with target == NULL the loss took no part and gloss is not read.
 * clamp_mode_host is HOST memory, read during the call (a captured launch keeps its values): the library checks it and hands the
 * modes to the kernel with its arguments.  Every other pointer is device memory.  NLAM_EINVAL / NLAM_EUNSUP before any launch. */
#define NLAM_CLAMP_NONE  0
#define NLAM_CLAMP_BOTH  1
#define NLAM_CLAMP_LOWER 2
#define NLAM_CLAMP_UPPER 3
typedef struct {
    const float* delta;          /* (rows, delta_ld) the network output */
    const float* prev;           /* (rows, nvars) */
    const float* truth;          /* forward: (rows, nvars) the boundary forcing */
    const float* target;         /* (rows, nvars), or NULL: no loss term */
    const float* dstd;           /* (nvars) or NULL (1) */
    const float* dmean;          /* (nvars) or NULL (0) */
    const float* bmask;          /* (nodes) */
    const float* row_weight;     /* (nodes), read with a loss term */
    const float* consts;         /* (nvars) the per-variable std; NULL with a std head or for mse / mae */
    const int32_t* clamp_mode_host;   /* HOST (nvars) NLAM_CLAMP_*, or NULL: none */
    const float* clamp_lo;       /* (nvars) */
    const float* clamp_hi;       /* (nvars) */
    float* pred;                 /* (rows, nvars): written by the forward, read by the backward (with a loss term) */
    float* pred_std;             /* (rows, nvars) likewise; non-NULL exactly when delta_ld == 2 * nvars */
    float* partials;             /* forward: (nparts), NULL exactly when target is */
    const float* g_pred;         /* backward: (rows, nvars) or NULL */
    const float* g_std;          /* backward: (rows, nvars) or NULL (std head only) */
    const float* gloss;          /* backward: the scalar gradient of the loss (device), read with a loss term */
    float* d_delta;              /* backward: (rows, delta_ld) */
    float* d_prev;               /* backward: (rows, nvars) or NULL */
    int64_t rows;
    int32_t nodes;
    int32_t nvars;               /* <= NLAM_LOSS_MAX_VARS */
    int32_t delta_ld;            /* nvars or 2 * nvars */
    int32_t kind;                /* NLAM_LOSS_* (a valid one also without a loss term) */
    int32_t nparts;
    float scale;
} nlam_step_tail_t;
int32_t nlam_step_tail_ext_fwd(const nlam_step_tail_t* p, void* hip_stream);
int32_t nlam_step_tail_ext_bwd(const nlam_step_tail_t* p, void* hip_stream);

/* The evaluation metrics of validation_step / test_step (models/module.py:491-504, :546-576, :607-681) over a rollout,
 * pred / target / std (batch * steps * nodes, nvars) fp32, with "masked grid mean" = sum_n row_weight[n] * x (row_weight =
 * interior / #interior: mask_and_reduce_metric, metrics.py:37-84).  The entry of `kind` is that of nlam_loss_fwd, with the
 * same std rules (mse / mae read no std; `std` per entry, else `var_std` per variable).  Every output may be NULL:
 *   step_loss (batch, steps)        masked grid mean of sum_v entry                 (the time_step_loss before its batch mean)
 *   sq        (batch, steps, nvars) masked grid mean of (pred - target)^2           (metrics.mse, sum_vars=False)
 *   ab        (batch, steps, nvars) masked grid mean of |pred - target|             (metrics.mae, sum_vars=False)
 *   std_mean  (batch, steps, nvars) masked grid mean of the per-entry std           (needs `std`)
 *   maps      (batch, nmaps, nodes) sum_v entry at lead time map_steps[s], NaN where row_weight[n] == 0 (the spatial loss)
 * Two launches: workgroups own (batch, step, node chunk) and write per-variable partial sums into `workspace` (at least
 * nlam_eval_workspace_floats(batch, steps, nodes, nvars) floats) and the maps directly; a second kernel adds the chunks in a
 * fixed order (bit-identical run to run).  No allocation, no host synchronisation.  NLAM_EINVAL (before any launch) for null
 * required pointers, sizes < 1, an unknown kind, a missing std, map steps outside [0, steps) or a short workspace;
 * NLAM_EUNSUP for nvars > NLAM_EVAL_MAX_VARS or nmaps > NLAM_EVAL_MAX_MAPS. */
#define NLAM_EVAL_MAX_MAPS 32
#define NLAM_EVAL_MAX_VARS 256   /* a workgroup keeps every variable's sums in registers (4 per thread, period 4 * nvars) */
typedef struct {
    const float* pred;         /* (batch * steps * nodes, nvars) */
    const float* target;       /* (batch * steps * nodes, nvars) */
    const float* std;          /* (batch * steps * nodes, nvars) per-entry std, or NULL */
    const float* var_std;      /* (nvars) per-variable std, read when std == NULL (may be NULL for mse / mae) */
    const float* row_weight;   /* (nodes) interior mask / #interior nodes */
    float* workspace;          /* (workspace_floats) */
    float* step_loss;          /* (batch, steps) or NULL */
    float* sq;                 /* (batch, steps, nvars) or NULL */
    float* ab;                 /* (batch, steps, nvars) or NULL */
    float* std_mean;           /* (batch, steps, nvars) or NULL */
    float* maps;               /* (batch, nmaps, nodes), or NULL when nmaps == 0 */
    int64_t workspace_floats;
    int32_t batch;
    int32_t steps;
    int32_t nodes;
    int32_t nvars;
    int32_t kind;              /* NLAM_LOSS_* */
    int32_t nmaps;
    int32_t map_steps[NLAM_EVAL_MAX_MAPS];   /* 0-based lead-time indices, [0, nmaps) used */
} nlam_eval_t;
int32_t nlam_eval_metrics(const nlam_eval_t* p, void* hip_stream);
/* floats of nlam_eval_t.workspace for these sizes; -1 (NLAM_EINVAL) for sizes < 1 */
int64_t nlam_eval_workspace_floats(int32_t batch, int32_t steps, int32_t nodes, int32_t nvars);

/* Row-wise concatenation of up to NLAM_MAX_CAT sources into out (rows, sum of widths): the torch.cat of the grid input
 * features (prev_state, prev_prev_state, forcing, static features; step_predictors/graph/base.py:275-283).  A source
 * with bstride 0 is shared by all batch items (expand_to_batch, step_predictors/base.py:122-139). */
typedef struct {
    const float* ptr[NLAM_MAX_CAT];
    int64_t bstride[NLAM_MAX_CAT];   /* floats between batch items of the source; 0 = shared */
    int32_t width[NLAM_MAX_CAT];
    int32_t nsrc;
    int32_t batch;
    int32_t nodes;                   /* rows per batch item */
    int32_t _pad;
    float* out;                      /* (batch, nodes, sum of widths) */
} nlam_cat_t;
int32_t nlam_concat(const nlam_cat_t* p, void* hip_stream);

/* The data path: WeatherDataset.__getitem__ (weather_dataset.py:467-533) for a BATCH of sample indices, cut straight out
 * of analysis time series that are resident in HBM -- _slice_state_time (:199-262, analysis branch :255-261),
 * _slice_forcing_time (:264-361, analysis branch :330-359), the feature-major / window-minor stacking of the forcing
 * window (:443-445) -- optionally followed, in the same pass, by ForecasterModule.on_after_batch_transfer
 * (models/module.py:326-367: (x - mean) / std, forcing statistics tiled over the window, IEEE sub + div).
 *   sample i = sample_idx[b]:  state rows  [i + max(0, past - 2), i + max(2, past) + ar_steps)  -> 2 init + ar_steps target
 *                              forcing of step t, window slot w:  time  i + max(2, past) + t - past + w
 *                              forcing_windowed[b][t][n][f * window + w],  window = past + future + 1
 * Sample indices are read on the device (a resident permutation drives an epoch without host traffic); they must lie
 * in [0, nlam_window_len): the kernel clamps the time index instead of faulting, the Python wrapper validates host
 * indices (IndexError as weather_dataset.py:497-503).  HBM-bound: every output float is read once and written once. */
typedef struct {
    const float* state;          /* (n_times, nodes, d_state) */
    const float* forcing;        /* (n_times, nodes, d_forcing) or NULL when d_forcing == 0 */
    const int64_t* times;        /* (n_times) time stamps (ns) or NULL */
    const int64_t* sample_idx;   /* device, (batch) */
    float* init_states;          /* (batch, 2, nodes, d_state) */
    float* target_states;        /* (batch, ar_steps, nodes, d_state) */
    float* forcing_windowed;     /* (batch, ar_steps, nodes, d_forcing * window) or NULL when d_forcing == 0 */
    int64_t* target_times;       /* (batch, ar_steps) or NULL; with times == NULL it receives the (clamped) time index */
    const float* state_mean;     /* (d_state)   all four NULL: raw values, as the reference's dataset returns them */
    const float* state_std;      /* (d_state) */
    const float* forcing_mean;   /* (d_forcing) */
    const float* forcing_std;    /* (d_forcing) */
    int64_t n_times;
    int32_t nodes, d_state, d_forcing, batch;
    int32_t ar_steps, num_past_forcing_steps, num_future_forcing_steps, _pad;
} nlam_window_t;
/* len(WeatherDataset) for analysis data (weather_dataset.py:179-194); n_forcing_times < 0: no forcing */
int64_t nlam_window_len(int64_t n_state_times, int64_t n_forcing_times, int32_t ar_steps, int32_t num_past_forcing_steps,
                        int32_t num_future_forcing_steps);
int32_t nlam_window_batch(const nlam_window_t* p, void* hip_stream);

/* A forecast to any lead time as replays of ONE recorded AR step (neural_lam_amd/forecast.py).  A captured launch cannot change its
 * pointers between replays, so everything that depends on the lead time is addressed on the device through a counter:
 *   start (batch) int64   the time index t0 of the LATEST initial state of each forecast
 *   lead  (1)     int32   k, the number of lead times already produced
 * Lead k + 1 is valid at time index t0 + k + 1: its forcing window reads times t0 + k + 1 - past .. t0 + k + 1 + future
 * (feature-major / window-minor, forcing_windowed[b][n][f * window + w], as nlam_window_batch), its boundary truth is the state
 * at t0 + k + 1.  Time indices are clamped into [0, n_times) instead of faulting, as in nlam_window_batch.  The series are those of
 * nlam_window_t; the state statistics are required (the outputs are de-standardised with them), the forcing pair with d_forcing > 0.
 *   nlam_forecast_init    prev_prev = standardised state at t0 - 1, prev = at t0 (both (batch, nodes, d_state)); *lead = 0.
 *   nlam_forecast_head    reads *lead; writes this lead's standardised forcing_windowed (batch, nodes, d_forcing * window) and
 *                         truth (batch, nodes, d_state): (x - mean) / std, IEEE sub + div -- the bits of nlam_window_batch.
 *   nlam_forecast_tail    reads *lead; one pass per element over the network output delta (batch * nodes, delta_ld), delta_ld =
 *                         d_state or 2 * d_state with a std head, with dstd / dmean / bmask / clamp_* as in nlam_step_tail_t:
 *                           new = the pred of nlam_step_tail_ext_fwd(target = NULL) on (delta, prev, truth): the same device
 *                                 function, the same bits
 *                           prev_prev[e] = prev[e];  prev[e] = new                       the state rotates in place
 *                           out_state[b][k][n][f] = new * state_std[f] + state_mean[f]   physical units
 *                           out_std[b][k][n][f]   = softplus(raw) * state_std[f]         with a std head
 *                           valid_times[b][k]     = times[t0 + k + 1], or that (clamped) index when times == NULL
 *                           sq / ab given: per-workgroup partial sums of row_weight[n] * (new - truth)^2 and
 *                                 row_weight[n] * |new - truth| into workspace (standardised units: the sq / ab of nlam_eval_metrics)
 *                         If *lead >= max_lead the kernel writes nothing at all.
 *   nlam_forecast_finish  one small launch, always: adds the partials in a fixed order into sq[b][k][f] / ab[b][k][f] (bit-identical
 *                         run to run), then increments *lead (not beyond max_lead).  One thread reads the counter and writes it; no
 *                         other launch writes it (nlam_forecast_init aside, which does not read it).
 * No allocation, no host synchronisation.  clamp_mode_host is HOST memory, read during the call.  NLAM_EINVAL (before any launch)
 * for null required pointers, sizes < 1, delta_ld not in {d_state, 2 * d_state}, out_std given exactly when there is no std head,
 * a short workspace; NLAM_EUNSUP for d_state > NLAM_LOSS_MAX_VARS, with sq / ab for d_state > NLAM_EVAL_MAX_VARS, and for a
 * (nodes x row) block of 2^31 floats or more. */
typedef struct {
    const float* state;          /* (n_times, nodes, d_state) */
    const float* forcing;        /* (n_times, nodes, d_forcing) or NULL when d_forcing == 0 */
    const int64_t* times;        /* (n_times) time stamps (ns) or NULL */
    const int64_t* start;        /* device (batch): t0 */
    int32_t* lead;               /* device (1): k */
    const float* state_mean;     /* (d_state) */
    const float* state_std;      /* (d_state) */
    const float* forcing_mean;   /* (d_forcing), required when d_forcing > 0 */
    const float* forcing_std;    /* (d_forcing) */
    float* prev;                 /* (batch, nodes, d_state) standardised state at the latest lead: init writes, tail rotates */
    float* prev_prev;            /* (batch, nodes, d_state) the one before */
    float* forcing_windowed;     /* head: (batch, nodes, d_forcing * window), or NULL when d_forcing == 0 */
    float* truth;                /* head writes, tail reads: (batch, nodes, d_state) */
    const float* delta;          /* tail: (batch * nodes, delta_ld) the network output */
    const float* dstd;           /* tail: (d_state) or NULL (1) */
    const float* dmean;          /* tail: (d_state) or NULL (0) */
    const float* bmask;          /* tail: (nodes) */
    const float* row_weight;     /* tail: (nodes) interior mask / #interior nodes, read with sq / ab */
    const int32_t* clamp_mode_host;   /* tail: HOST (d_state) NLAM_CLAMP_*, or NULL: none */
    const float* clamp_lo;       /* (d_state) */
    const float* clamp_hi;       /* (d_state) */
    float* out_state;            /* tail: (batch, max_lead, nodes, d_state) physical units */
    float* out_std;              /* tail: (batch, max_lead, nodes, d_state); non-NULL exactly when delta_ld == 2 * d_state */
    int64_t* valid_times;        /* tail: (batch, max_lead) or NULL */
    float* sq;                   /* tail + finish: (batch, max_lead, d_state) or NULL */
    float* ab;                   /* tail + finish: (batch, max_lead, d_state) or NULL */
    float* workspace;            /* tail + finish, with sq / ab: nlam_forecast_workspace_floats(batch, nodes, d_state) floats */
    int64_t workspace_floats;
    int64_t n_times;
    int32_t nodes, d_state, d_forcing, batch;
    int32_t max_lead, num_past_forcing_steps, num_future_forcing_steps, delta_ld;
} nlam_forecast_t;
int32_t nlam_forecast_init(const nlam_forecast_t* p, void* hip_stream);
int32_t nlam_forecast_head(const nlam_forecast_t* p, void* hip_stream);
int32_t nlam_forecast_tail(const nlam_forecast_t* p, void* hip_stream);
int32_t nlam_forecast_finish(const nlam_forecast_t* p, void* hip_stream);
/* floats of nlam_forecast_t.workspace for these sizes; NLAM_EINVAL for sizes < 1, NLAM_EUNSUP for nvars > NLAM_EVAL_MAX_VARS */
int64_t nlam_forecast_workspace_floats(int32_t batch, int32_t nodes, int32_t nvars);

/* nlam_forecast_init / _head over STRIDED series: forecast-type and ensemble datastores, addressed as nlam_window_ens_t addresses
 * them.  Element (sample s, member m, row j) of a series -- one contiguous (nodes x d) block -- sits at
 *   base + s * stride_sample + j * stride_step + m * stride_member      (floats, 64-bit)
 *   analysis data (is_forecast = 0): stride_sample == stride_step, the time stride (NLAM_EINVAL otherwise); n_times = time steps
 *   forecast data (is_forecast = 1): stride_sample = analysis stride, stride_step = lead-time stride; n_times = analysis times
 *   forcing without a member axis: forcing_stride_member = 0
 * sample_idx[b] is the flat sample index of forecast b, read on the device and clamped into [0, base_len * members) instead of
 * faulting; (s, m) = divmod(idx, members), time-major.  base_len is that of nlam_window_batch_ens at ar_steps = max_lead:
 * nlam_window_len over n_times for analysis data (at least 1), n_times for forecast data.  With off = max(2, past) and k = *lead:
 *   nlam_forecast_init_strided   prev_prev = row off - 2, prev = row off - 1; *lead = 0
 *   nlam_forecast_head_strided   truth = row off + k; slot w of the forcing window = row off + k - past + w
 * Rows are clamped as well: forecast data into [0, state_steps) and [0, forcing_steps), analysis data the time index s + j into
 * [0, n_times).  Output layout, standardisation and the guard on *lead are those of the plain pair; each block takes the 16-byte
 * path when that block, its destination and its size allow it (strides may break the alignment from one member to the next).  The
 * outputs have the bits of nlam_window_batch_ens at ar_steps = max_lead with statistics.
 * Of nlam_forecast_t the destinations, statistics, counter and sizes are read; its state, forcing, times, start and n_times are
 * ignored.  nlam_forecast_tail (valid_times = NULL: its time arithmetic is that of a plain series) and nlam_forecast_finish serve
 * both kinds of source.  NLAM_EINVAL (before any launch) for null required pointers, sizes < 1, negative strides, members < 1,
 * is_forecast not in {0, 1}, and on forecast data state_steps < off + max_lead or, with d_forcing > 0, forcing_steps <
 * off + max_lead + future; NLAM_EUNSUP as the plain pair. */
typedef struct {
    const float* state;
    const float* forcing;            /* NULL when d_forcing == 0 */
    const int64_t* sample_idx;       /* device (batch): flat sample indices */
    int64_t state_stride_sample, state_stride_step, state_stride_member;
    int64_t forcing_stride_sample, forcing_stride_step, forcing_stride_member;
    int64_t n_times;
    int32_t state_steps, forcing_steps;   /* forecast data: lead times per analysis time (ignored for analysis data) */
    int32_t is_forecast, members;
} nlam_forecast_src_t;
int32_t nlam_forecast_init_strided(const nlam_forecast_t* p, const nlam_forecast_src_t* src, void* hip_stream);
int32_t nlam_forecast_head_strided(const nlam_forecast_t* p, const nlam_forecast_src_t* src, void* hip_stream);

/* Sampled ensembles inside the recorded forecast step (neural_lam_amd/forecast.py, EnsembleForecast): batch = starts * members,
 * batch item b = s * members + m (member-minor), every start repeated `members` times in nlam_forecast_t.start.
 *
 * The generator is Philox4x32-10 (Salmon et al. 2011, the constants of Random123): counter (c0, c1, c2, c3), key = (low, high)
 * word of a 64-bit seed.  The four output words x become four standard normals z by two Box-Muller pairs:
 *   u_i = ((x_i >> 9) + 0.5) * 2^-23            exact in fp32, never 0 or 1
 *   r = sqrtf(-2 logf(u_0)), z_0 = r cospif(2 u_1), z_1 = r sinpif(2 u_1); (z_2, z_3) the same from (u_2, u_3)
 *   nlam_philox_normal_fill   out[i], i < n: element i % 4 of counter (i / 4, c1, c2, c3).  NLAM_EINVAL for out == NULL or
 *                             n < 0, NLAM_EUNSUP for n > 2^34; n == 0 launches nothing.
 *   nlam_latent_sample        reads *lead = k (nothing is written once k >= max_lead).  params (batch, rows, P) are the
 *                             parameters of the prior: P = latent_dim with diagonal = 0 (std 1), P = 2 latent_dim with
 *                             diagonal = 1 (mean | std_raw, std = 1e-4 + softplus(std_raw)).
 *                               latent[b][e] = mean + std * z          e < rows * latent_dim
 *                             noise_in == NULL: z is element e % 4 of counter (e / 4, k, b % members, low word of start[b])
 *                             under *seed, and goes to noise_out[k][b][e] when noise_out is given; noise_in given: z =
 *                             noise_in[k][b][e] (both (max_lead, batch, rows, latent_dim)).  NLAM_EINVAL for null required
 *                             pointers, sizes < 1, batch not a multiple of members, diagonal outside {0, 1}; NLAM_EUNSUP for
 *                             batch > 65535 or rows * latent_dim >= 2^31.
 *   nlam_ens_scores           after nlam_forecast_tail, before nlam_forecast_finish; reads *lead = k (nothing is written once
 *                             k >= max_lead) and never writes it.  prev / truth (starts * members, nodes, d_state) are the
 *                             standardised new states and the analysis (the truth of member 0 is used); w_n = row_weight[n],
 *                             M = members, xbar the member mean, y the truth:
 *                               ens_sq[s][k][f]   = sum_n w_n (xbar - y)^2
 *                               ens_var[s][k][f]  = sum_n w_n / (M - 1) sum_m (x_m - xbar)^2            0 for M = 1
 *                               ens_abs[s][k][f]  = sum_n w_n / M sum_m |x_m - y|
 *                               ens_pair[s][k][f] = sum_n w_n / (M (M - 1)) sum_{i<j} |x_i - x_j|       0 for M = 1
 *                                                   (fair CRPS = ens_abs - ens_pair)
 *                               rank_hist[s][k][f][r], r = 0 .. M: the nodes with w_n != 0 whose truth has exactly r
 *                                                   members strictly below it (a member equal to the truth is not below)
 *                               out_mean[s][k][n][f]   = xbar * state_std[f] + state_mean[f]
 *                               out_spread[s][k][n][f] = sqrt(sum_m (x_m - xbar)^2 / (M - 1)) * state_std[f]
 *                             Per-workgroup partial sums in the workspace, one finishing launch that adds them in a fixed
 *                             order: no floating-point atomics, bit-identical from run to run.  NLAM_EINVAL for null
 *                             pointers (all are required), sizes < 1, a short workspace; NLAM_EUNSUP for members >
 *                             NLAM_ENS_MAX_MEMBERS, d_state > NLAM_EVAL_MAX_VARS, starts > 65535, nodes * d_state >= 2^31.
 * Every check comes before any launch; no allocation, no host synchronisation. */
#define NLAM_ENS_MAX_MEMBERS 64
typedef struct {
    const float* params;      /* (batch, rows, P) */
    const float* noise_in;    /* (max_lead, batch, rows, latent_dim) or NULL: draw */
    float* noise_out;         /* (max_lead, batch, rows, latent_dim) or NULL */
    float* latent;            /* (batch, rows, latent_dim) */
    const int64_t* start;     /* device (batch): t0, as nlam_forecast_t.start */
    const int32_t* lead;      /* device (1): k, only read */
    const uint64_t* seed;     /* device (1): required when noise_in == NULL */
    int32_t batch, members, rows, latent_dim;
    int32_t diagonal, max_lead;
} nlam_latent_sample_t;
int32_t nlam_philox_normal_fill(float* out, int64_t n, uint64_t seed, uint32_t c1, uint32_t c2, uint32_t c3, void* hip_stream);
int32_t nlam_latent_sample(const nlam_latent_sample_t* p, void* hip_stream);
typedef struct {
    const float* prev;         /* (starts * members, nodes, d_state) standardised states of this lead */
    const float* truth;        /* (starts * members, nodes, d_state) standardised analysis */
    const float* row_weight;   /* (nodes) */
    const float* state_mean;   /* (d_state) */
    const float* state_std;    /* (d_state) */
    const int32_t* lead;       /* device (1): k, only read */
    float* ens_sq;             /* (starts, max_lead, d_state) */
    float* ens_var;            /* (starts, max_lead, d_state) */
    float* ens_abs;            /* (starts, max_lead, d_state) */
    float* ens_pair;           /* (starts, max_lead, d_state) */
    int32_t* rank_hist;        /* (starts, max_lead, d_state, members + 1) */
    float* out_mean;           /* (starts, max_lead, nodes, d_state) physical units */
    float* out_spread;         /* (starts, max_lead, nodes, d_state) physical units */
    float* workspace;          /* nlam_ens_scores_workspace_floats(starts, members, nodes, d_state) floats */
    int64_t workspace_floats;
    int32_t starts, members, nodes, d_state;
    int32_t max_lead, _pad;
} nlam_ens_scores_t;
int32_t nlam_ens_scores(const nlam_ens_scores_t* p, void* hip_stream);
/* floats of nlam_ens_scores_t.workspace; NLAM_EINVAL for sizes < 1, NLAM_EUNSUP for members > NLAM_ENS_MAX_MEMBERS or
 * nvars > NLAM_EVAL_MAX_VARS */
int64_t nlam_ens_scores_workspace_floats(int32_t starts, int32_t members, int32_t nodes, int32_t nvars);

/* Exceedance probabilities and quantile fields of the same ensemble, and their scores, for lead slot k = *lead (only read; nothing
 * is written once k >= max_lead): after nlam_ens_scores, before nlam_forecast_finish.  prev / truth / row_weight / state_mean /
 * state_std as in nlam_ens_scores_t; truth may be NULL.  E = events, Q = quantiles, M = members, x_(0) <= ... <= x_(M-1) the
 * sorted members of one element, y its truth, w_n = row_weight[n], "live" = w_n != 0.  Every table is device memory, read by the
 * launch: a replay sees new values.
 *   event e     variable event_var[e]; x is in the event when x > event_thr[e] (event_sense[e] = 0) or x < event_thr[e]
 *               (event_sense[e] = 1); equality never counts.  Thresholds are in standardised units.
 *   quantile j  level q = q_level[j] with i = q_index[j] = floor(q (M - 1)) and g = q_frac[j] = q (M - 1) - i, both computed by
 *               the caller in float64: the launch does no arithmetic on q but the 1 - q of the pinball loss.
 *                 Q_j = x_(i) + g (x_(min(i + 1, M - 1)) - x_(i))                 numpy's default (linear) quantile
 *               The members are ordered as sign-magnitude bit patterns: -0 below +0, a NaN member at the end its sign puts it,
 *               so the quantiles that reach it are NaN.
 *   prob[s][k][e][n]      = (float)c / (float)M, c = the members of variable event_var[e] at node n in the event
 *   quant[s][k][j][n][f]  = Q_j * state_std[f] + state_mean[f]
 * and with truth given, o = 1 when the truth is in the event, else 0:
 *   brier[s][k][e]        = sum_n w_n (c / M - o)^2
 *   rel_count[s][k][e][c] = the live nodes with exactly c members in the event, c = 0 .. M;  rel_obs: those of them with o = 1
 *   pinball[s][k][j][f]   = sum_n w_n rho,  rho = q (y - Q_j) for y >= Q_j, else (1 - q) (Q_j - y)        standardised units
 *   below[s][k][j][f]     = the live nodes with y < Q_j
 * With truth == NULL the five score pointers must be NULL and only prob and quant are written.  Per-(start, chunk) partial sums
 * in the workspace, one finishing launch (with truth only) that adds them in a fixed order: no floating-point atomics,
 * bit-identical from run to run.  The ranges of event_var ([0, d_state)), event_sense ({0, 1}) and q_index ([0, members)) are the
 * caller's to check: the launch clamps the two indices into range and treats any non-zero sense as 1.
 * NLAM_EINVAL for null required pointers (prev, row_weight, state_mean, state_std, lead, workspace), sizes < 1, events or
 * quantiles < 0 or both 0, events > 0 without its three tables and prob, quantiles > 0 without its three tables and quant, a short
 * workspace, a score pointer without truth, truth without brier / rel_count / rel_obs (events > 0) or pinball / below
 * (quantiles > 0); NLAM_EUNSUP for members > NLAM_ENS_MAX_MEMBERS, d_state > NLAM_EVAL_MAX_VARS, events > NLAM_ENS_MAX_EVENTS,
 * quantiles > NLAM_ENS_MAX_QUANTILES, starts > 65535, nodes * d_state >= 2^31.  Every check comes before any launch; no
 * allocation, no host synchronisation. */
#define NLAM_ENS_MAX_EVENTS 32
#define NLAM_ENS_MAX_QUANTILES 16
typedef struct {
    const float* prev;            /* (starts * members, nodes, d_state) standardised states of this lead */
    const float* truth;           /* (starts * members, nodes, d_state) standardised analysis, or NULL: no scores */
    const float* row_weight;      /* (nodes) */
    const float* state_mean;      /* (d_state) */
    const float* state_std;       /* (d_state) */
    const int32_t* lead;          /* device (1): k, only read */
    const int32_t* event_var;     /* device (events) */
    const int32_t* event_sense;   /* device (events): 0 above, 1 below */
    const float* event_thr;       /* device (events): standardised units */
    const int32_t* q_index;       /* device (quantiles) */
    const float* q_frac;          /* device (quantiles) */
    const float* q_level;         /* device (quantiles) */
    float* prob;                  /* (starts, max_lead, events, nodes) */
    float* quant;                 /* (starts, max_lead, quantiles, nodes, d_state) physical units */
    float* brier;                 /* (starts, max_lead, events) */
    int32_t* rel_count;           /* (starts, max_lead, events, members + 1) */
    int32_t* rel_obs;             /* (starts, max_lead, events, members + 1) */
    float* pinball;               /* (starts, max_lead, quantiles, d_state) */
    int32_t* below;               /* (starts, max_lead, quantiles, d_state) */
    float* workspace;             /* nlam_ens_products_workspace_floats(starts, members, nodes, d_state, events, quantiles) floats */
    int64_t workspace_floats;
    int32_t starts, members, nodes, d_state;
    int32_t max_lead, events, quantiles, _pad;
} nlam_ens_products_t;
int32_t nlam_ens_products(const nlam_ens_products_t* p, void* hip_stream);
/* floats of nlam_ens_products_t.workspace; NLAM_EINVAL for sizes < 1, events or quantiles < 0 or both 0, NLAM_EUNSUP for members >
 * NLAM_ENS_MAX_MEMBERS, nvars > NLAM_EVAL_MAX_VARS, events > NLAM_ENS_MAX_EVENTS or quantiles > NLAM_ENS_MAX_QUANTILES */
int64_t nlam_ens_products_workspace_floats(int32_t starts, int32_t members, int32_t nodes, int32_t nvars, int32_t events,
                                           int32_t quantiles);

/* Neighbourhood probabilities of the same events and the sums of the fractions skill score (FSS, Roberts and Lean 2008), for
 * lead slot k = *lead (only read; nothing is written once k >= max_lead): after nlam_ens_products, before nlam_forecast_finish.
 * prev / truth / row_weight / lead and the three event tables as in nlam_ens_products_t (the same device tables; truth may be
 * NULL).  The grid is nx x ny, node n = i * ny + j; N = nx * ny, M = members, W = scales, w_n = row_weight[n], "live" =
 * w_n != 0.  C(n) = the members of variable event_var[e] at node n in event e, O(n) = 1 when the truth is in it, else 0.
 * radius is device memory, read by the launch: a replay sees new values.  With r = radius[w], the window W_r(n) is the nodes
 * (i', j') of the grid with |i' - i| <= r and |j' - j| <= r: no wrap, no padding, a negative radius acts as 0 and one larger than
 * the grid gives the whole grid.  Three integers per (event, scale, node):
 *   A  = the live nodes of W_r(n),   SC = sum of C over them,   SO = sum of O over them
 *   nprob[s][k][e][w][n] = (float)SC / (float)(M A), NaN where A = 0; written for every node, live or not
 * and with truth given, of = (float)SO / (float)A:
 *   fbs[s][k][e][w]      = sum over live n of w_n (nprob - of)^2
 *   fbs_ref[s][k][e][w]  = sum over live n of w_n (nprob^2 + of^2)              FSS = 1 - sum_s fbs / sum_s fbs_ref
 * members * nx * ny <= 2^24 is required: both conversions are then exact and nprob is one correctly rounded division; at r = 0
 * nprob of a live node is prob of nlam_ens_products bit for bit.  The window sums come from int32 summed-area tables in the
 * workspace (exact in any order; the cost does not depend on the radii); fbs and fbs_ref from per-workgroup partial sums in the
 * workspace and one finishing launch that adds them in a fixed order: no floating-point atomics, bit-identical from run to run.
 * Five launches with truth, four without, for every size.  The launch clamps event_var into [0, d_state) and treats any
 * non-zero sense as 1.
 * NLAM_EINVAL for null required pointers (prev, row_weight, lead, the three event tables, radius, nprob, workspace), sizes < 1,
 * a short workspace, fbs or fbs_ref without truth, truth without both; NLAM_EUNSUP for members > NLAM_ENS_MAX_MEMBERS, d_state >
 * NLAM_EVAL_MAX_VARS, events > NLAM_ENS_MAX_EVENTS, scales > NLAM_NBR_MAX_SCALES, starts > 65535, members * nx * ny > 2^24.
 * Every check comes before any launch; no allocation, no host synchronisation. */
#define NLAM_NBR_MAX_SCALES 8
typedef struct {
    const float* prev;            /* (starts * members, nx * ny, d_state) standardised states of this lead */
    const float* truth;           /* (starts * members, nx * ny, d_state) standardised analysis, or NULL: no scores */
    const float* row_weight;      /* (nx * ny) */
    const int32_t* lead;          /* device (1): k, only read */
    const int32_t* event_var;     /* device (events) */
    const int32_t* event_sense;   /* device (events): 0 above, 1 below */
    const float* event_thr;       /* device (events): standardised units */
    const int32_t* radius;        /* device (scales): cells */
    float* nprob;                 /* (starts, max_lead, events, scales, nx * ny) */
    float* fbs;                   /* (starts, max_lead, events, scales) */
    float* fbs_ref;               /* (starts, max_lead, events, scales) */
    float* workspace;             /* nlam_ens_neighbourhood_workspace_floats(starts, members, nx, ny, d_state, events, scales) floats */
    int64_t workspace_floats;
    int32_t starts, members, nx, ny;
    int32_t d_state, max_lead, events, scales;
} nlam_ens_neighbourhood_t;
int32_t nlam_ens_neighbourhood(const nlam_ens_neighbourhood_t* p, void* hip_stream);
/* floats of nlam_ens_neighbourhood_t.workspace: nx ny (1 + 2 starts events) table words and 2 starts events scales words per 256
 * nodes; NLAM_EINVAL for sizes < 1, NLAM_EUNSUP as nlam_ens_neighbourhood */
int64_t nlam_ens_neighbourhood_workspace_floats(int32_t starts, int32_t members, int32_t nx, int32_t ny, int32_t nvars, int32_t events,
                                                int32_t scales);

/* Variance spectra of lattice fields from a 2-D discrete cosine transform (Denis, Cote and Laprise 2002), for lead slot
 * k = *lead (only read; nothing is written once k >= max_lead): inside the recorded forecast step, before nlam_forecast_finish.
 * Grid and window: the grid is nx x ny, node n = i * ny + j; the window i0 <= i < i0 + cx, j0 <= j < j0 + cy has cx >= 2 and
 *   cy >= 2 (they size the launches) and its origin (i0, j0) = origin[0 .. 1] in device memory, read by the launch and clamped
 *   into [0, nx - cx] x [0, ny - cy]: a replay sees a moved window, and nothing outside the grid is ever read.  One field (item b
 *   of a source, variable v with f = var[v]) is g(i, j) = x[b][(i0 + i) * ny + (j0 + j)][f].
 * Basis: C_n[k][i] = beta_k cos(pi k (2 i + 1) / (2 n)), beta_0 = sqrt(1 / n), beta_k = sqrt(2 / n): the orthonormal DCT-II,
 *   computed by the host in float64 and rounded once to fp32; basis_x = C_cx (cx, cx), basis_y = C_cy (cy, cy), row-major [k][i].
 * Coefficients: G(m, n) = sum_i sum_j basis_x[m][i] g(i, j) basis_y[n][j], as two passes of fp32 dot products in ascending index
 *   order, first along j, then along i, on v_mfma_f32_16x16x4_f32 (bitwise an fp32 fmaf chain).
 * Variance array: s2(m, n) = G(m, n)^2 / (cx cy); by Parseval the sum over (m, n) != (0, 0) is the population variance of g.
 * Bins: the launch knows no binning convention.  The host passes the coefficients of every bin as a CSR list: bin b owns
 *   bin_idx[bin_ptr[b] .. bin_ptr[b + 1]), each entry a coefficient m * cy + n; a coefficient that is in no list is dropped (the
 *   host leaves (0, 0), the mean, out).  bin_ptr has bins + 1 words inside [0, bin_entries] (clamped as they are read), bin_idx
 *   has bin_entries <= cx cy words (clamped into [0, cx cy)).
 * Output: spec[b][k][v][bin] = scale_v / (cx cy) * sum over the bin's list, in list order, of G^2; scale_v = state_std[f]^2 for
 *   a standardised source (physical units squared), 1 for a source with physical = 1; 0 for an empty bin.  The sum is added in
 *   a fixed order, without floating-point atomics: two runs give the same bits.
 * Sources: up to NLAM_SPEC_MAX_SOURCES per call, each (batch, nx * ny, d_state) floats with its own batch stride and a lead
 *   stride multiplied by *lead (0 for the state of the step; nx * ny * d_state for per-lead slots such as out_mean of
 *   nlam_ens_scores).  var, the bases, the bin lists and state_std are device memory, read by the launches: a replay sees new values.
 *   var is clamped into [0, d_state).
 * Three launches for every size.  Indices inside one item are 32-bit, offsets between items, sources and leads 64-bit.
 * NLAM_EINVAL for null required pointers (lead, origin, both bases, var, bin_ptr, bin_idx, workspace, every source's x and spec,
 * state_std with a standardised source), sizes < 1, sources outside [1, NLAM_SPEC_MAX_SOURCES], a source batch < 1 or a negative
 * stride, a window larger than the grid or with cx or cy < 2, bin_entries outside [0, cx cy], a short workspace; NLAM_EUNSUP for
 * d_state > NLAM_EVAL_MAX_VARS, vars > d_state, a source batch above 65535, nx * ny * d_state >= 2^31 or cx * cy * vars >= 2^31.
 * Every check comes before any launch; no allocation, no host synchronisation. */
#define NLAM_SPEC_MAX_SOURCES 3
typedef struct {
    const float* x;               /* (batch, nx * ny, d_state) */
    float* spec;                  /* (batch, max_lead, vars, bins) */
    int64_t batch_stride;         /* floats between two items */
    int64_t lead_stride;          /* floats, multiplied by *lead */
    int32_t batch;
    int32_t physical;             /* 0: standardised, scale_v = state_std[f]^2; 1: scale_v = 1 */
} nlam_dct_spectra_src_t;
typedef struct {
    nlam_dct_spectra_src_t src[NLAM_SPEC_MAX_SOURCES];
    const int32_t* origin;        /* device (2): i0, j0 */
    const float* basis_x;         /* device (cx, cx) */
    const float* basis_y;         /* device (cy, cy) */
    const int32_t* var;           /* device (vars) */
    const int32_t* bin_ptr;       /* device (bins + 1) */
    const int32_t* bin_idx;       /* device (bin_entries): m * cy + n, ascending inside a bin */
    const float* state_std;       /* device (d_state) */
    const int32_t* lead;          /* device (1): k, only read */
    float* workspace;             /* nlam_dct_spectra_workspace_floats(items, cx, cy, vars) floats, items = the sum of the batches */
    int64_t workspace_floats;
    int32_t sources, nx, ny, d_state;
    int32_t vars, bins, bin_entries, max_lead;
    int32_t cx, cy;
} nlam_dct_spectra_t;
int32_t nlam_dct_spectra(const nlam_dct_spectra_t* p, void* hip_stream);
/* floats of nlam_dct_spectra_t.workspace: the pass along j and the coefficients, 2 items cx cy vars; NLAM_EINVAL for items or
 * vars < 1 and cx or cy < 2, NLAM_EUNSUP for items > 3 * 65535, vars > NLAM_EVAL_MAX_VARS or cx * cy * vars >= 2^31 */
int64_t nlam_dct_spectra_workspace_floats(int32_t items, int32_t cx, int32_t cy, int32_t vars);

/* The posterior draw and the KL term of the Graph-EFM training objective (Oskarsson et al. 2024, section 3; models.EFMForecaster)
 * inside the recorded training step.  With D = latent_dim, u = 1e-4, pq (batch, rows, 2 D) the encoder's parameters (always
 * diagonal) and pp (batch, rows, P) the prior's -- P = D with diagonal = 0 (std 1), P = 2 D with diagonal = 1 -- per element
 * e < rows * D of batch item b:
 *     mu_q = pq[.., :D], s_q = u + softplus(pq[.., D:]);   mu_p = pp[.., :D], s_p = u + softplus(pp[.., D:]) or 1
 *   nlam_latent_kl_fwd        latent[b][e] = mu_q + s_q eps,   eps[b][e] = eps
 *                             kl[b]   = sum_e log(s_p / s_q) + (s_q^2 + (mu_q - mu_p)^2) / (2 s_p^2) - 1/2
 *                                       (evaluated as 1/2 (r^2 + n^2) - 1/2 - log r, r = s_q / s_p, n = (mu_q - mu_p) / s_p:
 *                                       exactly 0 where q == p)
 *                             kl_term = *kl_weight * sum_b kl[b]
 *                             noise_in == NULL: eps is element e % 4 of the Philox counter (e / 4, t, b, low word of *draw)
 *                             under *seed (the generator and the Box-Muller pairs of nlam_latent_sample); *draw is only read.
 *                             noise_in given: eps = noise_in[b][e].  Per-workgroup partial sums in the workspace and one
 *                             finishing workgroup that adds them in a fixed order (an item's partials in block order, then the
 *                             items): no floating-point atomics, bit-identical from run to run.
 *   nlam_latent_kl_bwd        elementwise, from the same pq, pp and the eps the forward wrote; g = g_latent[b][e] (0 for
 *                             g_latent == NULL), w = *g_kl_term * *kl_weight, dlt = mu_q - mu_p:
 *                               g_pq[.., :D] = g + w dlt / s_p^2
 *                               g_pq[.., D:] = (g eps + w (s_q / s_p^2 - 1 / s_q)) softplus'(pq[.., D:])
 *                               g_pp[.., :D] = -w dlt / s_p^2                                             unless g_pp == NULL
 *                               g_pp[.., D:] = w (1 / s_p - (s_q^2 + dlt^2) / s_p^3) softplus'(pp[.., D:])   diagonal = 1
 *                             softplus and its derivative are those of the step tails (beta 1, threshold 20, derivative 1 above).
 * Both: 16-byte accesses where the buffers involved are 16-byte aligned (the parameter matrices also need D % 4 == 0), single
 * elements otherwise; every check before any launch; no allocation, no host synchronisation.  NLAM_EINVAL for null required
 * pointers (fwd: pq, pp, eps, kl_weight, latent, kl, kl_term, workspace, and seed and draw when noise_in == NULL; bwd: pq, pp,
 * eps, kl_weight, g_kl_term, g_pq), sizes < 1, diagonal outside {0, 1}, t < 0, a short workspace; NLAM_EUNSUP for
 * batch > 65535 or rows * latent_dim >= 2^31. */
typedef struct {
    const float* pq;           /* (batch, rows, 2 latent_dim) */
    const float* pp;           /* (batch, rows, P) */
    const float* noise_in;     /* (batch, rows, latent_dim) or NULL: draw */
    const float* kl_weight;    /* device (1) */
    const uint64_t* seed;      /* device (1): required when noise_in == NULL; the 64 bits of the key (a signed word carries the same) */
    const int64_t* draw;       /* device (1): required when noise_in == NULL; only read */
    float* eps;                /* (batch, rows, latent_dim): written by fwd, read by bwd */
    float* latent;             /* fwd: (batch, rows, latent_dim) */
    float* kl;                 /* fwd: (batch) */
    float* kl_term;            /* fwd: device (1) */
    float* workspace;          /* fwd: nlam_latent_kl_workspace_floats(batch, rows, latent_dim) floats */
    int64_t workspace_floats;
    const float* g_latent;     /* bwd: (batch, rows, latent_dim) or NULL: zero */
    const float* g_kl_term;    /* bwd: device (1) */
    float* g_pq;               /* bwd: (batch, rows, 2 latent_dim) */
    float* g_pp;               /* bwd: (batch, rows, P) or NULL */
    int32_t batch, rows, latent_dim, diagonal;
    int32_t t, _pad;           /* t: the AR step, word 1 of the counter */
} nlam_latent_kl_t;
int32_t nlam_latent_kl_fwd(const nlam_latent_kl_t* p, void* hip_stream);
int32_t nlam_latent_kl_bwd(const nlam_latent_kl_t* p, void* hip_stream);
/* floats of nlam_latent_kl_t.workspace: one per workgroup; NLAM_EINVAL for sizes < 1 */
int64_t nlam_latent_kl_workspace_floats(int32_t batch, int32_t rows, int32_t latent_dim);

/* The ensemble CRPS fine-tuning term of the Graph-EFM training schedule (Oskarsson et al. 2024, section 3: L_Var + lambda_CRPS
 * L_CRPS; models.EFMForecasterStep(crps_members = M)) inside the recorded training step.
 *
 * The prior draw with a gradient.  params (batch, rows, P): P = D = latent_dim with diagonal = 0 (std 1), P = 2 D with
 * diagonal = 1 (std = 1e-4 + softplus(params[.., D:])), as nlam_latent_sample reads them; per element e < rows * D of item b:
 *   nlam_latent_draw_fwd      latent[b][e] = mean + std eps,   eps[b][e] = eps
 *                             noise_in == NULL: eps is element e % 4 of the Philox counter (e / 4, t, b, low word of *draw)
 *                             under *seed (the generator, the Box-Muller pairs and the quad layout of nlam_latent_kl_fwd; the
 *                             caller keeps the keys of the two apart); *draw is only read.  noise_in given: eps = noise_in[b][e].
 *   nlam_latent_draw_bwd      elementwise, from params and the eps the forward wrote, g = g_latent[b][e]:
 *                               g_params[.., :D] = g
 *                               g_params[.., D:] = g eps softplus'(params[.., D:])          diagonal = 1
 *                             g_params == NULL (a constant prior): nothing is launched.  softplus and its derivative are those
 *                             of the step tails (beta 1, threshold 20, derivative 1 above).
 * Both: 16-byte accesses where the buffers involved are 16-byte aligned (the parameter matrices also need D % 4 == 0), single
 * elements otherwise.  NLAM_EINVAL for null required pointers (fwd: params, eps, latent, and seed and draw when noise_in == NULL;
 * bwd: params, eps, g_latent), sizes < 1, diagonal outside {0, 1}, t < 0; NLAM_EUNSUP for batch > 65535 or rows * latent_dim >= 2^31.
 *
 * The term.  pred (batch * members, nodes, nvars): item b * M + m is member m of batch item b (the member-minor layout of
 * nlam_ens_scores); target (batch, nodes, nvars).  With M = members, x_m the members and y the target of one element, w_n =
 * row_weight[n], c_f = var_weight[f] (1 for var_weight == NULL):
 *   nlam_crps_ens_fwd         crps[b] = sum_n,f (w_n c_f) [ 1/M sum_m |x_m - y|  -  1/(M (M - 1)) sum_{i<j} |x_i - x_j| ]
 *                             term    = *weight * sum_b crps[b]
 *                             (the bracket is ens_abs - ens_pair of nlam_ens_scores per element: the fair / unbiased ensemble
 *                             CRPS; M = 2 is the paper's estimator).  One thread per quad of four consecutive elements of an
 *                             item, the members in registers; per-workgroup partial sums in the workspace and one finishing
 *                             workgroup that adds them in a fixed order (an item's partials in block order, then the items):
 *                             no floating-point atomics, bit-identical from run to run.  A zero row weight is a weight like any
 *                             other.
 *   nlam_crps_ens_bwd         elementwise, recomputed from pred and target; g = (*g_term * *weight) (w_n c_f):
 *                               g_pred[b M + m][n][f] = g ( sgn(x_m - y) / M  -  1/(M (M - 1)) sum_{j != m} sgn(x_m - x_j) )
 *                             sgn(a - b) = (a > b) - (a < b), by comparison: a tie gives exactly 0 (the subgradient torch.abs
 *                             takes) and the sign sums are exact integers.
 * Both: 16-byte accesses where pred, target (and g_pred) are 16-byte aligned and nodes * nvars % 4 == 0, single elements
 * otherwise; var_weight is staged in LDS.  NLAM_EINVAL for null required pointers (fwd: pred, target, row_weight, weight, crps,
 * term, workspace; bwd: pred, target, row_weight, weight, g_term, g_pred), sizes < 1, members < 2, a short workspace; NLAM_EUNSUP
 * for members > NLAM_CRPS_MAX_MEMBERS, batch > 65535, nvars > NLAM_LOSS_MAX_VARS, nodes * nvars >= 2^31.
 * All four: every check before any launch; no allocation, no host synchronisation. */
#define NLAM_CRPS_MAX_MEMBERS 16
typedef struct {
    const float* params;       /* (batch, rows, P) */
    const float* noise_in;     /* (batch, rows, latent_dim) or NULL: draw */
    const uint64_t* seed;      /* device (1): required when noise_in == NULL; the 64 bits of the key */
    const int64_t* draw;       /* device (1): required when noise_in == NULL; only read */
    float* eps;                /* (batch, rows, latent_dim): written by fwd, read by bwd */
    float* latent;             /* fwd: (batch, rows, latent_dim) */
    const float* g_latent;     /* bwd: (batch, rows, latent_dim) */
    float* g_params;           /* bwd: (batch, rows, P) or NULL */
    int32_t batch, rows, latent_dim, diagonal;
    int32_t t, _pad;           /* t: the AR step, word 1 of the counter */
} nlam_latent_draw_t;
int32_t nlam_latent_draw_fwd(const nlam_latent_draw_t* p, void* hip_stream);
int32_t nlam_latent_draw_bwd(const nlam_latent_draw_t* p, void* hip_stream);
typedef struct {
    const float* pred;         /* (batch * members, nodes, nvars) */
    const float* target;       /* (batch, nodes, nvars) */
    const float* row_weight;   /* (nodes) */
    const float* var_weight;   /* (nvars) or NULL: ones */
    const float* weight;       /* device (1) */
    float* crps;               /* fwd: (batch), unweighted */
    float* term;               /* fwd: device (1) */
    float* workspace;          /* fwd: nlam_crps_ens_workspace_floats(batch, members, nodes, nvars) floats */
    int64_t workspace_floats;
    const float* g_term;       /* bwd: device (1) */
    float* g_pred;             /* bwd: (batch * members, nodes, nvars) */
    int32_t batch, members, nodes, nvars;
} nlam_crps_ens_t;
int32_t nlam_crps_ens_fwd(const nlam_crps_ens_t* p, void* hip_stream);
int32_t nlam_crps_ens_bwd(const nlam_crps_ens_t* p, void* hip_stream);
/* floats of nlam_crps_ens_t.workspace: one per workgroup; NLAM_EINVAL for sizes < 1 or members < 2, NLAM_EUNSUP for members >
 * NLAM_CRPS_MAX_MEMBERS, nvars > NLAM_LOSS_MAX_VARS or nodes * nvars >= 2^31 */
int64_t nlam_crps_ens_workspace_floats(int32_t batch, int32_t members, int32_t nodes, int32_t nvars);

/* The same batch launch over STRIDED series: forecast-type and ensemble datastores (weather_dataset.py:135-200, :235-254,
 * :303-342, :399-418).  Element (sample s, member m, step j) of a series -- one contiguous (nodes x d) block -- sits at
 *   base + s * stride_sample + j * stride_step + m * stride_member      (floats, 64-bit)
 *   analysis data (is_forecast = 0): stride_sample = stride_step = the time stride; n_times = time steps
 *   forecast data (is_forecast = 1): stride_sample = analysis stride, stride_step = lead-time stride; n_times = analysis times
 *   forcing without a member axis: forcing_stride_member = 0 (every member reads the same forcing)
 * Flat sample index idx (read on the device, clamped to [0, base_len * members) instead of faulting) -> (s, m) =
 * divmod(idx, members), time-major as the reference; members = 1 under load_single_member.  base_len: as
 * nlam_window_len over n_times for analysis data, n_times for forecast data.  With off = max(2, past):
 *   state rows j = max(0, past - 2) ... off + ar_steps - 1  -> 2 init + ar_steps target
 *   forcing of step k, window slot w: j = off + k - past + w (window = past + future + 1, feature-major / window-minor)
 *   target_times[b][k], j = off + k:  analysis: times[s + j], or the time index s + j when times == NULL
 *                                     forecast: times[s] + elapsed[j], or the lead-time index j when both are NULL
 * Forecast data needs state_steps >= off + ar_steps and, with forcing, forcing_steps >= off + ar_steps + future lead
 * times per analysis time (both are ignored for analysis data).  Standardisation as nlam_window_t. */
typedef struct {
    const float* state;
    const float* forcing;            /* NULL when d_forcing == 0 */
    const int64_t* times;            /* analysis: (n_times) valid times; forecast: (n_times) analysis times; or NULL */
    const int64_t* elapsed;          /* forecast: (state_steps) lead times, with times; NULL otherwise */
    const int64_t* sample_idx;       /* device, (batch) flat indices */
    float* init_states;              /* (batch, 2, nodes, d_state) */
    float* target_states;            /* (batch, ar_steps, nodes, d_state) */
    float* forcing_windowed;         /* (batch, ar_steps, nodes, d_forcing * window) or NULL when d_forcing == 0 */
    int64_t* target_times;           /* (batch, ar_steps) or NULL */
    const float* state_mean;
    const float* state_std;
    const float* forcing_mean;
    const float* forcing_std;
    int64_t state_stride_sample, state_stride_step, state_stride_member;
    int64_t forcing_stride_sample, forcing_stride_step, forcing_stride_member;
    int64_t n_times;
    int32_t state_steps, forcing_steps;
    int32_t is_forecast, members;
    int32_t nodes, d_state, d_forcing, batch;
    int32_t ar_steps, num_past_forcing_steps, num_future_forcing_steps, _pad;
} nlam_window_ens_t;
int32_t nlam_window_batch_ens(const nlam_window_ens_t* p, void* hip_stream);

/* Per-sample moments of a resident series, read in place (the standardization statistics of
 * neural_lam/datastore/npyfilesmeps/compute_standardization_stats.py; no batch is materialised).  Addressing as
 * nlam_window_ens_t: element (sample s, member m, row j) is the contiguous (nodes x nvars) block at
 *   series + s * stride_sample + j * stride_step + m * stride_member      (floats, 64-bit)
 * for the flat samples idx = first ... first + count - 1, (s, m) = divmod(idx, members), all inside [0, base_len * members):
 * a range that leaves it is refused, no index is clamped
 * (base_len: n_times - (row_begin + nrows) + 1 for analysis data -- nlam_window_len with past = future = 0 when
 * row_begin + nrows = 2 + ar_steps, sample s reading time steps s + j -- and n_times for forecast data).  The
 * rows of a sample are j = row_begin ... row_begin + nrows - 1 (the state: 0 ... ar_steps + 1; the forcing with no past /
 * future window: 2 ... ar_steps + 1).  Two modes, per feature f:
 *   step == 0 (values): out_mean[i][f] = mean of x, out_sq[i][f] = mean of x^2 over the nrows rows and the nodes of
 *     sample first + i; count output rows.
 *   step >= 1 (standardized one-step differences): used = (nrows / step) * step; sub-offset k in [0, step) takes rows
 *     row_begin + k, row_begin + k + step, ... < row_begin + used; for consecutive pairs (a, b) of them
 *     d = (x[b] - mean) / std - (x[a] - mean) / std in fp32 (IEEE sub, div, sub, in this order); out_mean / out_sq are the
 *     means of d and d^2 over pairs and nodes.  Output row i * step + k (sample-major); count * step rows.  Needs at least
 *     one pair (nrows / step >= 2).
 * Accumulation is fp64 from the first element: a workgroup owns a fixed span of the elements of one output row's
 * (nodes x nvars) blocks (whole chunks of 8 * lanes elements, lanes = (256 / nvars) * nvars; not whole nodes); its partial sums
 * go to `workspace` and a second launch adds them in a fixed order (bit-identical run to run; the split depends on nodes
 * and nvars only, so a sample's row does not depend on first / count).  No atomics, no allocation, no host
 * synchronisation.  NLAM_EINVAL (before any launch) for null pointers, sizes < 1, negative strides, samples outside
 * [0, base_len * members), too short a lead-time axis (forecast: steps < row_begin + nrows), no pair to difference or a
 * short workspace; NLAM_EUNSUP for nvars > NLAM_MOMENTS_MAX_VARS or a (nodes x nvars) block of 2^31 floats or more. */
#define NLAM_MOMENTS_MAX_VARS 256   /* a workgroup's lanes keep fixed features: 4 * lanes elements per stride, lanes a multiple of nvars */
typedef struct {
    const float* series;
    const float* mean;               /* (nvars) for step >= 1; NULL for step == 0 */
    const float* std;                /* (nvars) for step >= 1; NULL for step == 0 */
    double* workspace;               /* nlam_moments_workspace_doubles(nodes, nvars, count, step) doubles */
    double* out_mean;                /* (count * max(step, 1), nvars) */
    double* out_sq;                  /* (count * max(step, 1), nvars) */
    int64_t workspace_doubles;
    int64_t stride_sample, stride_step, stride_member;
    int64_t n_times;                 /* analysis: time steps of the common axis; forecast: analysis times */
    int64_t first, count;            /* flat sample range */
    int32_t is_forecast, members;
    int32_t steps;                   /* forecast: lead times of the resident series (ignored for analysis data) */
    int32_t nodes, nvars;
    int32_t row_begin, nrows;
    int32_t step;                    /* 0: values; >= 1: standardized differences with this stride */
} nlam_moments_t;
int32_t nlam_window_moments(const nlam_moments_t* p, void* hip_stream);
/* doubles of nlam_moments_t.workspace for these sizes; -1 (NLAM_EINVAL) for sizes out of range */
int64_t nlam_moments_workspace_doubles(int32_t nodes, int32_t nvars, int64_t count, int32_t step);

/* Resident series as PACKED int16.  Every series has per-feature fp32 tables scale[f] > 0 and offset[f]:
 *   decode  x = fadd_rn(fmul_rn((float)q, scale[f]), offset[f])       two separately rounded fp32 operations, never one fma
 *           (contraction is switched off around them; numpy on float32 arrays: q.astype(float32) * scale + offset)
 *   encode  q = clamp(rintf(fdiv_rn(fsub_rn(x, offset[f]), scale[f])), -32767, 32767)   round to nearest even; -32768 is never
 *           produced and has no special meaning on decode
 * Standardisation, where an entry applies it, follows on the decoded value exactly as in the fp32 entries (IEEE sub, then div);
 * the two affine maps are not folded.  Every _q16 entry therefore gives the bits of its fp32 entry on a series of the decoded
 * values: it launches the kernel of that fp32 entry, instantiated for int16 elements where a series is packed (the fp32 entries
 * launch the float instantiations).  Strides of a packed series are counted in int16 ELEMENTS; a (nodes x d) block may start at any 2-byte-aligned
 * address and is read four codes (8 bytes) per lane when it starts on an 8-byte boundary, its destination on a 16-byte
 * boundary and its length is a multiple of 4, code by code otherwise (the fp32 entries' 16-byte test).
 *
 * nlam_series_range: per-feature minimum, maximum and count of non-finite values of a contiguous fp32 chunk (rows, nvars),
 *   MERGED into the running device tables run_min / run_max (nvars floats, initialised by the caller to +inf / -inf) and
 *   run_bad (nvars int64, initialised to 0): a series uploaded in chunks is reduced chunk by chunk.  Non-finite values are
 *   counted and take no part in the extrema.  min and max are exact and order-independent; no atomics: per-workgroup
 *   partial tables in `workspace` (nlam_series_range_workspace_words(rows, nvars) 32-bit words, monotone in rows), folded by
 *   a second launch.  NLAM_EINVAL for null pointers, rows or nvars < 1, a short workspace; NLAM_EUNSUP for nvars >
 *   NLAM_MOMENTS_MAX_VARS.
 * nlam_series_pack_q16: encodes the contiguous fp32 chunk (rows, nvars) into dst[dst_offset ... dst_offset + rows * nvars)
 *   (elements).  16-byte loads and 8-byte stores where the chunk is 16-byte and the destination 8-byte aligned, single
 *   elements otherwise and on the last partial quad.  NLAM_EINVAL for null pointers, rows or nvars < 1, dst_offset < 0;
 *   NLAM_EUNSUP for chunks of 2^31 elements or more.
 * Both: no allocation, no host synchronisation. */
int64_t nlam_series_range_workspace_words(int64_t rows, int32_t nvars);
int32_t nlam_series_range(const float* x, int64_t rows, int32_t nvars, float* run_min, float* run_max, int64_t* run_bad,
                          uint32_t* workspace, int64_t workspace_words, void* hip_stream);
int32_t nlam_series_pack_q16(const float* x, int64_t rows, int32_t nvars, const float* scale, const float* offset, int16_t* dst,
                             int64_t dst_offset, void* hip_stream);

/* The packed source of a _q16 entry, passed beside the entry's parameter struct.  A series whose pointer is set here is read
 * from it, with the strides of the parameter struct counted in int16 elements, and the float pointer of that series in the
 * parameter struct is ignored.  A series whose pointer is NULL here is not packed: it is read as fp32 through the float
 * pointer and float strides of the parameter struct (state packed and forcing fp32, or the reverse).  NLAM_EINVAL when the
 * state is in neither place, when d_forcing > 0 and the forcing is in neither place, or when a packed series comes without
 * one of its two tables. */
typedef struct {
    const int16_t* state;           /* packed state series or NULL */
    const int16_t* forcing;         /* packed forcing series or NULL */
    const float* state_scale;       /* (d_state) */
    const float* state_offset;      /* (d_state) */
    const float* forcing_scale;     /* (d_forcing) */
    const float* forcing_offset;    /* (d_forcing) */
} nlam_q16_src_t;

/* nlam_window_batch_ens over packed series: the same launch shape, clamp of the flat index, (s, m) = divmod(idx, members), rows,
 * forcing-window transpose, target_times and optional standardisation.  A plain analysis series is the case
 * state_stride_sample == state_stride_step with members = 1.  Checks and return codes as nlam_window_batch_ens, with the
 * series pointers checked as nlam_q16_src_t describes. */
int32_t nlam_window_batch_q16(const nlam_window_ens_t* p, const nlam_q16_src_t* src, void* hip_stream);

/* nlam_window_moments over a packed series (`series`, strides of nlam_moments_t in int16 elements; nlam_moments_t.series is
 * ignored), both modes: the same node split, the same fp64 sums from the first decoded element in the same order, the same
 * second launch; out_mean / out_sq are bit-identical to nlam_window_moments on the decoded series.  Checks and return codes
 * as nlam_window_moments; NLAM_EINVAL also for a null series, scale or offset. */
int32_t nlam_window_moments_q16(const nlam_moments_t* p, const int16_t* series, const float* scale, const float* offset,
                                void* hip_stream);

/* nlam_forecast_init_strided / _head_strided over packed series: the same launch shapes, sample arithmetic, row clamps, guard on
 * *lead and standardisation; nlam_forecast_tail / _finish read what the head wrote and serve this source as well.  Of
 * nlam_forecast_src_t the strides of a packed series are counted in int16 elements.  Checks and return codes as the strided
 * pair, with the series pointers checked as nlam_q16_src_t describes. */
int32_t nlam_forecast_init_q16(const nlam_forecast_t* p, const nlam_forecast_src_t* src, const nlam_q16_src_t* packed,
                               void* hip_stream);
int32_t nlam_forecast_head_q16(const nlam_forecast_t* p, const nlam_forecast_src_t* src, const nlam_q16_src_t* packed,
                               void* hip_stream);

/* decoupled-weight-decay Adam on flat buffers; step_count is the 1-based step */
int32_t nlam_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                        float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step_count,
                        float grad_scale, void* hip_stream);
/* the same update with the step count RESIDENT on the device: a one-thread launch advances *step_count_dev (int32, starts at
 * 0) and leaves the bias corrections 1 - beta1^t, sqrt(1 - beta2^t) in bias_corr_dev[0..1] for the update launch behind it.
 * No launch argument depends on the step, so the optimizer can be part of a captured HIP graph that is replayed per step. */
int32_t nlam_adamw_step_resident(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                                 float beta1, float beta2, float eps, float weight_decay, int32_t* step_count_dev,
                                 float* bias_corr_dev, float grad_scale, void* hip_stream);

/* Sum of squares of `n` floats (the flat gradient): one pass with 16-byte loads, fp64 from the first element, a fixed-order
 * reduction to one fp64 partial per workgroup in partials[0 .. nlam_grad_sumsq_workspace_doubles(n)) -- no atomics, so the
 * same buffer gives the same bits on every run.  With `norm` non-null a one-wave launch behind it adds the partials in a
 * fixed order and writes norm[0] = (float)(scale * sqrt(sum)). */
int64_t nlam_grad_sumsq_workspace_doubles(int64_t n);
int32_t nlam_grad_sumsq(const float* grad, int64_t n, double* partials, int64_t workspace_doubles, float scale, float* norm,
                        void* hip_stream);

/* nlam_adamw_step_resident with the decisions about the update taken on the device, in three launches none of whose
 * arguments depends on the step (so they can be captured and replayed):
 *   1. nlam_grad_sumsq's first launch over `grad`;
 *   2. one wave: norm = grad_scale * sqrt(sum) (the norm of the averaged gradient).  Not finite and skip_nonfinite set: the
 *      step count and bias corrections stay, control[3] = 1, control[4] += 1.  Otherwise the step count advances, the bias
 *      corrections are left as nlam_adamw_step_resident leaves them, lr_t = lr * f(s) for s = step count - 1, and
 *      coefficient = min(1, max_grad_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_);
 *   3. the update of nlam_adamw_step_resident with lr_t and grad * grad_scale * coefficient; nothing is touched on a skip.
 * Schedule (torch.optim.lr_scheduler.LambdaLR stepped after every optimizer step), W = warmup_steps, T = total_steps,
 * r = min_ratio: f(s) = (s + 1) / W for s < W; otherwise with p = min(1, (s - W) / max(1, T - W)):
 *   NLAM_SCHED_CONSTANT 1;  NLAM_SCHED_WARMUP_COSINE r + (1 - r) (1 + cos(pi p)) / 2;  NLAM_SCHED_WARMUP_LINEAR r + (1 - r)(1 - p)
 * evaluated in fp64 and rounded once.  NLAM_SCHED_NONE: lr_t = lr.  max_grad_norm <= 0: no clipping (coefficient 1).
 * control: NLAM_OPTCTL_WORDS 4-byte words, zero before the first step:
 *   [0] float lr_t  [1] float coefficient (0 on a skip)  [2] float norm  [3] int32 skip flag  [4] int32 skipped steps */
#define NLAM_SCHED_NONE 0
#define NLAM_SCHED_CONSTANT 1
#define NLAM_SCHED_WARMUP_COSINE 2
#define NLAM_SCHED_WARMUP_LINEAR 3
#define NLAM_OPTCTL_WORDS 8
typedef struct {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int32_t* step_count_dev;
    float* bias_corr_dev;
    double* partials;                /* nlam_grad_sumsq_workspace_doubles(n) doubles */
    void* control;
    int64_t n;
    int64_t partials_doubles;
    float lr, beta1, beta2, eps, weight_decay, grad_scale;
    float max_grad_norm;
    float min_ratio;
    int32_t schedule;                /* NLAM_SCHED_* */
    int32_t warmup_steps, total_steps;
    int32_t skip_nonfinite;
} nlam_optctl_t;
int32_t nlam_adamw_step_controlled(const nlam_optctl_t* p, void* hip_stream);

/* Gradient accumulation over K micro-batches with ONE recorded step: the head and the tail of the step decide on the device
 * whether a call opens or closes a window, so no launch argument depends on the micro-step.
 * accum: NLAM_ACCUM_WORDS 4-byte words, zero before the first step:
 *   [0] int32 index of the next micro-batch in the window (0 .. K-1)   [1] int32 hold flag (1: the last call only accumulated)
 *   [2] float running loss sum of the open window                      [3] float mean loss of the last completed window
 * nlam_accum_begin: the zero of the flat gradient in front of forward + backward, in place of a memset: `grad[0 .. n)` is
 *   zeroed when accum[0] == 0 and left alone otherwise.  Any 4-byte aligned `grad`, any n >= 0 (16-byte stores on the aligned
 *   interior, single elements in front of and behind it).
 * nlam_adamw_step_accum: the three launches of nlam_adamw_step_controlled, each gated:
 *   1. the sum of squares runs only when accum[0] == steps - 1 (the micro-batch that completes the window);
 *   2. one wave adds loss[0] (0 for a null `loss`) to the running sum -- restarted at accum[0] == 0, fp32, in call order --
 *      and, the window not being complete, advances accum[0], raises the hold flag and stops: the control block keeps the
 *      values of the last completed window.  Otherwise accum[0] = 0, the hold flag is cleared, accum[3] = sum / (float)steps
 *      and the decisions of nlam_adamw_step_controlled follow, from the same code (grad_scale should hold the 1 / steps of
 *      the mean).  A window whose norm is not finite is skipped as there and is closed all the same, so the next
 *      nlam_accum_begin clears the gradient;
 *   3. the update touches nothing while the hold flag or the skip flag is up.
 * steps == 1 gives the bits of nlam_adamw_step_controlled.  NLAM_EINVAL: null or misaligned accum, steps < 1, and whatever
 * nlam_adamw_step_controlled rejects. */
#define NLAM_ACCUM_WORDS 4
typedef struct {
    int32_t* accum;                  /* NLAM_ACCUM_WORDS words on the device */
    const float* loss;               /* this micro-batch's loss on the device, or null */
    int32_t steps;                   /* K >= 1 */
} nlam_accum_t;
int32_t nlam_accum_begin(float* grad, int64_t n, const int32_t* accum, void* hip_stream);
int32_t nlam_adamw_step_accum(const nlam_optctl_t* p, const nlam_accum_t* a, void* hip_stream);

/* An exponential moving average of the parameters, kept by the launch that writes them (no launch more; `ema` is read
 * and written once per update, 8 bytes per parameter): AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay)) stepped
 * after every optimizer step, started as EMAWeightAveraging(update_starting_at_step=start_step) starts it.  With u the
 * 1-based count of APPLIED updates (*step_count_dev once this call's first launches have advanced it), for every element,
 * p being the new parameter value:
 *   u < start_step: ema is not touched;   u == start_step: ema = p;   u > start_step: ema = ema + w * (p - ema)
 * with w = 1.0f - decay computed once on the host, and the last form evaluated as one subtract, one multiply and one add,
 * each rounded to fp32 (never contracted): every kernel that carries it gives the same bits.  The decision is read on the
 * device, so no launch argument depends on the step.  ema is not touched where the parameters are not: a step refused for
 * a non-finite norm, a micro-batch inside an accumulation window, n == 0.  Parameters, moments, step count and bias
 * corrections get the bits of the entry without `_ema`.
 * nlam_adamw_step_resident_ema: the two launches of nlam_adamw_step_resident.
 * nlam_adamw_step_controlled_ema: a == NULL: the three launches of nlam_adamw_step_controlled; otherwise those of
 *   nlam_adamw_step_accum, with the same gates.
 * NLAM_EINVAL: null e or e->ema, ema not 4-byte aligned (16-byte accesses are used only where param, grad, both moments
 * and ema all sit on a 16-byte boundary), decay outside [0, 1) or NaN, start_step < 1, and whatever the entry without
 * `_ema` rejects. */
typedef struct {
    float* ema;                      /* n floats */
    float decay;                     /* in [0, 1) */
    int32_t start_step;              /* >= 1: the applied update at which ema becomes a copy of the parameters */
} nlam_ema_t;
int32_t nlam_adamw_step_resident_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                                     float beta1, float beta2, float eps, float weight_decay, int32_t* step_count_dev,
                                     float* bias_corr_dev, float grad_scale, void* hip_stream, const nlam_ema_t* e);
int32_t nlam_adamw_step_controlled_ema(const nlam_optctl_t* p, const nlam_accum_t* a, const nlam_ema_t* e, void* hip_stream);
/* a[0 .. n) <-> b[0 .. n), in place, one launch (evaluation under the averaged weights without rebinding a buffer that
 * captured graphs hold).  Any 4-byte aligned a and b, any n >= 0: 16-byte accesses on the interior that is 16-byte aligned
 * in BOTH buffers (none when their offsets within 16 bytes differ), single elements around it.  The ranges must not
 * overlap.  NLAM_EINVAL: null or misaligned buffers, n < 0. */
int32_t nlam_flat_swap(float* a, float* b, int64_t n, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* NLAM_HIP_H */
