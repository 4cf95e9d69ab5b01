/* simclr_hip.h -- C ABI of libsimclr_hip.so: the MI355X (gfx950) SimCLR pretraining hot path.
 *
 * The reference (google-research/simclr, tf2/) has no native/FFI boundary: the hot path sits
 * behind Python callables that hand everything to TensorFlow ops.  This header is the boundary a
 * maintainer binds instead (ctypes stub in INTEGRATION.md); every entry point names the reference
 * lines whose arithmetic it replaces.  Paths are relative to /root/reference/.
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes, no torch / framework types.
 *   - every pointer is a DEVICE pointer owned by the caller unless stated otherwise; the library
 *     never allocates, frees or synchronises; work is enqueued on `stream` (a hipStream_t).
 *   - returns 0 on success; nonzero = error (1 bad argument, 2 launch failure) with a message in
 *     simclr_last_error() (thread-local).  Re-entrant across streams.
 *   - `dtype`: SIMCLR_DT_F32 (0) or SIMCLR_DT_BF16 (1) = storage type of activations / compute
 *     weights ("T" below).  Accumulation, statistics, losses and optimizer state are fp32/fp64.
 *   - layouts: activations NHWC, master conv weights HWIO fp32, dense weights [in,out] fp32
 *     (tf2/resnet.py:196-203, tf2/model.py:143-146).
 *   - `dtype` may carry OPTION FIELDS above the low byte (fp32 storage only; entry points that
 *     accept them say so):
 *       SIMCLR_FMT_TERMS(t)  bits 12..19: the matrix arithmetic of THIS call (t = 0 exact fp32 MFMA,
 *                            3 | 6 bf16-piece terms, 13 = three fp16-piece terms, forward only) -- the
 *                            process-wide default of simclr_set_f32_matmul is then not consulted, so
 *                            calls on different streams / threads can run different modes;
 *       SIMCLR_FMT_PS_IN     the gradient operand (dy) of simclr_conv2d_dgrad / _dgrad_bn / _wgrad is
 *                            in the PRE-SPLIT BLOCK FORMAT: same 4 bytes per element, but every 128-byte
 *                            block of 32 channels holds eight 16-byte chunks of bf16 pieces -- chunk g
 *                            (g < 4) = hi = bf16(x) of channels {4g..4g+3, 16+4g..16+4g+3}, chunk 4 + g =
 *                            lo = bf16(x - hi) of the same channels -- so that the three-term GEMMs read
 *                            their operand pieces without splitting anything in the k-loop;
 *       SIMCLR_FMT_PS_OUT    simclr_bn_bwd_apply / simclr_bn_bwd_apply_pool write dx in that format (channels % 32 == 0);
 *       SIMCLR_FMT_PS_W      the WEIGHT operand of simclr_conv2d_fwd / _fwd_pivoted / _fwd_bn_apply (terms 13) or of
 *                            simclr_conv2d_dgrad / _dgrad_bn (terms 3) is the pre-split copy simclr_presplit_weights_multi
 *                            made of it (once per optimizer step instead of once per launch inside the library).
 */
#ifndef SIMCLR_HIP_H_
#define SIMCLR_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMCLR_DT_F32 0
#define SIMCLR_DT_BF16 1
#define SIMCLR_FMT_PS_IN 0x100
#define SIMCLR_FMT_PS_OUT 0x200
#define SIMCLR_FMT_TERMS(t) (((t) + 1) << 12)
#define SIMCLR_FMT_PS_W 0x100000

typedef struct ihipStream_t* simclr_stream_t; /* == hipStream_t */

/* ---- runtime ---------------------------------------------------------------------------------- */
const char* simclr_last_error(void);
int simclr_abi_version(void);
/* lane-layout probes used by the GPU tests (0 mfma bf16 16x16x32, 1 mfma f32 16x16x4, 2 ds_read_tr16, 3 mfma f16 16x16x32 incl. subnormal inputs) */
int simclr_probe(int which, const void* a, const void* b, void* out, simclr_stream_t stream);

/* ---- NT-Xent contrastive loss: tf2/objective.py:35-89 (add_contrastive_loss) ------------------ */
/* tf.math.l2_normalize, objective.py:53-54.  z = x*rsqrt(max(sum x^2,1e-12)); inv[row] kept for bwd. */
int simclr_l2norm_fwd(const float* x, float* z, float* inv, int rows, int D, simclr_stream_t stream);
int simclr_l2norm_bwd(const float* z, const float* inv, const float* dz, float* dx, int rows, int D,
                      simclr_stream_t stream);
/* Matrix arithmetic of the sweeps (round 6, opt-in): the D argument of simclr_ntxent_fwd / _bwd may carry SIMCLR_FMT_TERMS(13) --
 * every fp32 product of S = Q K^T and of dF += T^T dS then runs as three fp16-piece MFMA terms (~2^-22 per product, i.e.
 * ~2^-22 / T on the logits) instead of the fp32-input MFMA (1/16 of the 16-bit rate).  Only for l2-NORMALISED rows (|z| <= 1 lies
 * in fp16's range; tf2/objective.py:53-54 hidden_norm=True); both calls of one loss must use the same setting. */
size_t simclr_ntxent_workspace_bytes(int n, int N, int D);
/* objective.py:55-87 + metrics.py:28-31.  z_local [2n,D] = [hidden1;hidden2] of this replica,
 * z_all [2N,D] = [hidden1_large;hidden2_large] (objective.py:60-61), N = R*n, rank = replica id
 * (objective.py:64-67).  out[0] = loss, out[1] = contrast_acc.  row_stats [2n,2] feeds the bwd. */
int simclr_ntxent_fwd(const float* z_local, const float* z_all, int n, int N, int D, int rank,
                      float temperature, float* out, float* row_stats, void* workspace,
                      simclr_stream_t stream);
/* What tape.gradient (tf2/run.py:621) derives for objective.py:76-87.  dz_local [2n,D]: gradient
 * through the local (query) rows; dz_all [2N,D]: gradient through the gathered rows, to be
 * reduce-scattered (SUM) across replicas = transpose of objective.py:114-122.  grad_scale = the
 * upstream factor (1/R, tf2/run.py:617).  out[2] = contrast_entropy (metrics.py:33-35). */
int simclr_ntxent_bwd(const float* z_local, const float* z_all, int n, int N, int D, int rank,
                      float temperature, const float* row_stats, float grad_scale, float* dz_local,
                      float* dz_all, float* out, void* workspace, simclr_stream_t stream);
/* dense logits_ab [n,N] (objective.py:80,89) for API parity only; not on the hot path. */
int simclr_ntxent_logits_ab(const float* z_local, const float* z_all, int n, int N, int D,
                            float temperature, float* logits_ab, simclr_stream_t stream);
/* Wide NT-Xent: the same three computations for ANY width D (proj_out_dim > 256; proj_head_mode=none feeds the encoder's
 * 512 ... 8192-wide output), as LDS-tiled GEMMs with a k-loop over D.  D is a plain width (no option bits); `terms` is the matrix
 * arithmetic, and only 0 = exact fp32-input MFMA is implemented (anything else returns an error).  The backward writes dS once
 * into the workspace ([2n, 2N] fp32, padded to the tile) and runs dz_local = dS z_all and dz_all = dS^T z_local as two GEMMs:
 * no atomics, bitwise run-to-run deterministic.  A workspace holds one fwd/bwd pair, as for simclr_ntxent_fwd. */
size_t simclr_ntxent_wide_workspace_bytes(int n, int N, int D);
/* objective.py:55-87 + metrics.py:28-31, arguments and outputs as simclr_ntxent_fwd. */
int simclr_ntxent_wide_fwd(const float* z_local, const float* z_all, int n, int N, int D, int terms, int rank,
                           float temperature, float* out, float* row_stats, void* workspace, simclr_stream_t stream);
/* tape.gradient of objective.py:76-87 + metrics.py:33-35, arguments and outputs as simclr_ntxent_bwd. */
int simclr_ntxent_wide_bwd(const float* z_local, const float* z_all, int n, int N, int D, int terms, int rank,
                           float temperature, const float* row_stats, float grad_scale, float* dz_local,
                           float* dz_all, float* out, void* workspace, simclr_stream_t stream);
/* dense logits_ab [n,N] (objective.py:80,89) on the matrix cores. */
int simclr_ntxent_wide_logits_ab(const float* z_local, const float* z_all, int n, int N, int D, int terms,
                                 float temperature, float* logits_ab, simclr_stream_t stream);

/* ---- generalized contrastive loss (csrc/gcl.hip): colabs/intriguing_properties/generalized_contrastive_loss.ipynb ----
 * loss = loss_scaling * (align + lambda_weight * dist_match), the notebook's `generalized_contrastive_loss` cell.
 * z_local [2n, D] = this replica's two views stacked, z_all [2N, D] = every replica's view-1 rows, then every replica's view-2 rows
 * (the NT-Xent layout), N = R*n.  D in {64, 128, 256}, any n >= 1.  No atomics: bitwise run-to-run deterministic. */
size_t simclr_gcl_lse_workspace_bytes(int n, int N, int D);    /* 0 for a shape the kernels refuse */
/* dist='logsumexp' (the cell's `get_logsumexp_loss` + the alignment term): out[0] = loss, out[1] = align = mean((z1 - z2)^2) / 2,
 * out[2] = dist_match = mean_i(logsumexp_j(z_i.z_j / T) - log D) over the 2n local rows and ALL 2N columns (self column included,
 * nothing masked; the constant is the log of the hidden width, as the cell takes shape(states)[1]).  row_stats [2n] is kept for the
 * backward; the workspace holds one fwd/bwd pair. */
int simclr_gcl_lse_fwd(const float* z_local, const float* z_all, int n, int N, int D, float temperature, float lambda_weight,
                       float loss_scaling, float* out, float* row_stats, void* workspace, simclr_stream_t stream);
/* tape.gradient of that cell: dz_local [2n, D] = query-side gradient + the alignment gradient, dz_all [2N, D] = key-side gradient
 * (to be reduce-scattered like simclr_ntxent_bwd's), both times grad_scale.  rank = replica id (where the local rows sit in z_all).
 * skip_self != 0 leaves out the term of every local row's OWN column, 2 coeff softmax_ii z_i in total: for l2-normalised rows it is
 * radial, the normalisation backward (simclr_l2norm_bwd) annihilates it, and next to it (softmax_ii ~ 1 at small temperatures) the
 * tangential gradient would lose its low bits in fp32.  Pass 0 when the rows are not normalised: there the term is part of the gradient. */
int simclr_gcl_lse_bwd(const float* z_local, const float* z_all, int n, int N, int D, float temperature, float lambda_weight,
                       float loss_scaling, int rank, int skip_self, const float* row_stats, float grad_scale, float* dz_local,
                       float* dz_all, void* workspace, simclr_stream_t stream);
/* dist='normal' / 'uniform' (the cell's `get_swd_loss`, its O(M^2) one-hot `sort` replaced by a sort): Pt, Qt [D, M] fp32 = the
 * projected hiddens / prior, one contiguous row per projected dimension, M <= 8192.  Every row of both is sorted ascending (equal keys of
 * Pt by row index: numpy.argsort(kind='stable')); dP[perm[k], c] = coeff * (P_sorted[c, k] - Q_sorted[c, k]) into a [M, D] row-major
 * tensor, col_loss[c] = sum_k (Q_sorted - P_sorted)^2, perm [D, M] int32 (may be null) = the sorting permutation of Pt's rows. */
int simclr_swd_sort_match(const float* Pt, const float* Qt, int M, int D, float coeff, float* dP, float* col_loss, int* perm,
                          simclr_stream_t stream);
/* The rest of `get_swd_loss` + the cell's last lines: out[0] = loss, out[1] = align, out[2] = dist_match = sum_c col_loss[c] / (D M)
 * (reduce_mean over [D, M]), summed in a fixed order. */
int simclr_gcl_swd_out(const float* col_loss, const float* z_local, int n, int M, int D, float lambda_weight, float loss_scaling, float* out,
                       simclr_stream_t stream);
/* tape.gradient of the SWD cell wrt the local rows: g_all [2N, D] = d dist_match / d z_all (every replica computes the identical
 * global term, so no collective follows); dz_local [2n, D] = lambda_weight * loss_scaling * grad_scale * R * (own rows of g_all) + the
 * alignment gradient +-(z1 - z2) / (n D) * loss_scaling * grad_scale. */
int simclr_gcl_swd_bwd(const float* g_all, const float* z_local, int n, int N, int D, int rank, float lambda_weight, float loss_scaling,
                       float grad_scale, float* dz_local, simclr_stream_t stream);
/* C [M, N] = A [M, K] B [N, K]^T, fp32 row-major, any M and N, K a multiple of 16, exact f32 MFMA: the cell's two
 * matmul(., rand_w) projections and their transposes (simclr_small_gemm_nt_f32 needs M and N multiples of 16). */
int simclr_gcl_gemm_nt(const float* A, const float* B, float* C, int M, int N, int K, simclr_stream_t stream);

/* ---- supervised contrastive loss (Khosla et al. 2020, Supervised Contrastive Learning, the L_out^sup form), csrc/supcon.hip ----
 * NT-Xent with every same-class row of the global batch as a positive.  Layout as simclr_ntxent_fwd: z_local [2n, D] = this replica's
 * [view-1 rows; view-2 rows], z_all [2N, D] = every replica's view-1 rows, then every replica's view-2 rows, N = R*n.  labels_all [N]
 * int32 = the class ids of the global batch in z_all's sample order: column j has label labels_all[j mod N].  Local row i (view
 * v = i / n, sample s = i % n) is global column self(i) = v*N + rank*n + s.
 *   A(i) = all 2N columns except self(i);  P(i) = {p in A(i): label(p) == label(i)}  (the other view of the image: |P(i)| >= 1)
 *   l_i  = logsumexp_{a in A(i)}(z_i.z_a / T) - (1 / |P(i)|) sum_{p in P(i)} z_i.z_p / T
 * The temperature / base_temperature factor of the paper's code is left out: with all labels distinct this is simclr_ntxent_fwd's loss.
 * D in {64, 128, 256}, any n >= 1; exact fp32-input MFMA, the [2n, 2N] matrix never written, no atomics: bitwise run-to-run
 * deterministic.  Labels are only compared for equality.  The workspace holds one fwd/bwd pair. */
size_t simclr_supcon_workspace_bytes(int n, int N, int D);     /* 0 for a shape the kernels refuse */
/* out[0] = loss = (1 / n) sum_{i < 2n} l_i (the sum of the two per-view means), out[1] = contrast_acc = the share of the 2n rows with
 * max_{p in P(i)} s_ip >= max_{a in A(i) \ P(i)} s_ia (a row without a non-positive column is a hit), out[2] = contrast_positives =
 * the mean of |P(i)| over the 2n rows.  row_stats [2n, 2] = {logsumexp over A(i) in the base-2 domain, |P(i)|}, kept for the backward. */
int simclr_supcon_fwd(const float* z_local, const float* z_all, const int* labels_all, int n, int N, int D, int rank, float temperature,
                      float* out, float* row_stats, void* workspace, simclr_stream_t stream);
/* The gradient through the logits: dS_ia = grad_scale / (n T) * (softmax_{A(i)}(s_i)_a - [a in P(i)] / |P(i)|), dS_{i, self(i)} = 0;
 * dz_local [2n, D] = dS z_all, dz_all [2N, D] = dS^T z_local (to be reduce-scattered like simclr_ntxent_bwd's). */
int simclr_supcon_bwd(const float* z_local, const float* z_all, const int* labels_all, int n, int N, int D, int rank, float temperature,
                      const float* row_stats, float grad_scale, float* dz_local, float* dz_all, void* workspace, simclr_stream_t stream);

/* ---- hard-negative and debiased NT-Xent (Robinson et al. 2021, Contrastive Learning with Hard Negative Samples: beta; Chuang et al.
 * 2020, Debiased Contrastive Learning: tau_plus), csrc/hcl.hip ----
 * The formulas are this project's definition of the two corrections, not a parity claim with either paper's code.  Layout as
 * simclr_ntxent_fwd.  Local row i (view v = i / n, sample s = i % n) has the own column self(i) = v*N + rank*n + s and the positive
 * column pos(i) = (1 - v)*N + rank*n + s; Neg(i) = the other M = 2N - 2 columns.  With a = 1 / T and s_ik = z_i.z_k:
 *   p_i = exp(a s_i,pos),  A_i = sum_{k in Neg(i)} exp((1 + beta) a s_ik),  B_i = sum_{k in Neg(i)} exp(beta a s_ik)
 *   G_raw_i = (M A_i / B_i - tau_plus M p_i) / (1 - tau_plus),  G_i = max(G_raw_i, M exp(-a))  (the floor)
 *   l_i = log(p_i + G_i) - a s_i,pos
 * At beta = 0 and tau_plus = 0 this is simclr_ntxent_fwd's loss.  D in {64, 128, 256}, any n >= 1 with N = R*n >= 2; T > 0 and finite,
 * beta >= 0 and finite, tau_plus in [0, 1); z_local, z_all, row_stats, dz_local, dz_all and the workspace 16-byte aligned.  Anything else
 * returns 1 and launches nothing.  Exact fp32-input MFMA, the [2n, 2N] matrix never written, the row finalize in double, no atomics:
 * bitwise run-to-run deterministic.  The workspace holds one fwd/bwd pair. */
size_t simclr_hcl_workspace_bytes(int n, int N, int D);        /* 0 for a shape the kernels refuse */
/* out[0] = loss = (1 / n) sum_{i < 2n} l_i (the sum of the two per-view means), out[1] = the share of the 2n local rows on the floor.
 * row_stats [2n, 4] = {log2 A_i, log2 B_i, the row's negative coefficient a w_i (0 on the floor), its positive coefficient}, kept for
 * the backward, which reads the forward's decision about the floor and never re-decides. */
int simclr_hcl_fwd(const float* z_local, const float* z_all, int n, int N, int D, int rank, float temperature, float beta, float tau_plus,
                   float* out, float* row_stats, void* workspace, simclr_stream_t stream);
/* The gradient through the logits, times grad_scale / n: above the floor dS_ik = a w_i ((1 + beta) P1_ik - beta P0_ik) for k in Neg(i),
 * w_i = (M A_i / B_i) / ((1 - tau_plus)(p_i + G_i)), P1 / P0 the softmaxes over Neg(i) at scales (1 + beta) a / beta a, and
 * dS_i,pos = a (p_i (1 - tau_plus M / (1 - tau_plus)) / (p_i + G_i) - 1); on the floor dS_ik = 0 and dS_i,pos = a (p_i / (p_i + G_i) - 1);
 * dS_{i, self(i)} = 0.  dz_local [2n, D] = dS z_all, dz_all [2N, D] = dS^T z_local (to be reduce-scattered like simclr_ntxent_bwd's). */
int simclr_hcl_bwd(const float* z_local, const float* z_all, int n, int N, int D, int rank, float temperature, float beta, float tau_plus,
                   const float* row_stats, float grad_scale, float* dz_local, float* dz_all, void* workspace, simclr_stream_t stream);

/* ---- NNCLR: nearest-neighbour positives for NT-Xent (after Dwibedi et al. 2021, With a Little Help from My Friends), csrc/nnclr.hip ----
 * This project's definition, written from memory of the paper, not a parity claim.  nn_local [2n, D] = the neighbour row of every
 * local row (view-a rows, then view-b rows; constants), z_local [2n, D] = the local rows themselves (read for nn_sim only), z_all
 * [2N, D] laid out as simclr_ntxent_fwd's.  Local row r (view v = r / n, sample s = r % n) contrasts its neighbour against the N
 * columns of the OTHER view, C(r) = [(1 - v)*N, (1 - v)*N + N), with the positive p(r) = (1 - v)*N + rank*n + s.  With a = 1 / T:
 *   l_r = logsumexp_{c in C(r)}(a nn_r.z_all[c]) - a nn_r.z_all[p(r)]
 * D in {64, 128, 256}, any n >= 1 with N = R*n >= 2; T > 0 and finite; every matrix, row_stats and the workspace 16-byte aligned.
 * Anything else returns 1 and launches nothing.  Exact fp32-input MFMA, the [2n, N] matrix never written, the row finalize in double,
 * no atomics: bitwise run-to-run deterministic.  The workspace holds one fwd/bwd pair. */
size_t simclr_nnclr_workspace_bytes(int n, int N, int D);      /* 0 for a shape the kernels refuse */
/* out[0] = the replica's loss share = (1 / n) sum_{r < 2n} l_r (the sum of the two per-view means), out[1] = the share of the 2n local
 * rows whose positive column is the lowest-index maximum of C(r), out[2] = the mean of z_r.nn_r.  row_stats [2n, 4] = {log2-sum-exp2 of
 * the row's base-2 logits as a float, what the float left of it, 1 - P_r,p(r), z_r.nn_r}; the backward reads the first three. */
int simclr_nnclr_fwd(const float* nn_local, const float* z_local, const float* z_all, int n, int N, int D, int rank, float temperature,
                     float* out, float* row_stats, void* workspace, simclr_stream_t stream);
/* The column gradient, the only one there is: dz_all [2N, D] = (grad_scale a / n) sum_{r : c in C(r)} (P_rc - [c = p(r)]) nn_r, P_r the
 * softmax over C(r) (to be reduce-scattered like simclr_ntxent_bwd's dz_all).  No row-side term: the neighbour rows are constants. */
int simclr_nnclr_bwd(const float* nn_local, const float* z_all, int n, int N, int D, int rank, float temperature, const float* row_stats,
                     float grad_scale, float* dz_all, void* workspace, simclr_stream_t stream);

/* ---- Barlow Twins loss (Zbontar et al. 2021, Barlow Twins: Self-Supervised Learning via Redundancy Reduction), csrc/barlow.hip ----
 * The Gram form: with zhat the per-view, per-dimension standardisation of the gathered block over the GLOBAL batch,
 * C = zhat1^T zhat2 / N ([D, D], never formed), c_i = C_ii, G1 = zhat1 zhat1^T, G2 = zhat2 zhat2^T,
 *   on_diag = sum_i (1 - c_i)^2,   off_diag = sum_{i != j} C_ij^2 = (1 / N^2) sum_{a, b} G1_ab G2_ab - sum_i c_i^2,
 *   L = loss_scaling * (on_diag + lambda_weight * off_diag).
 * Layout as simclr_ntxent_fwd: h_all / zhat_all [2N, D] = every replica's view-1 rows, then every replica's view-2 rows, N = R*n; this
 * replica's rows are rank*n .. rank*n + n - 1 of each view.  D a multiple of 64 in [64, 8192], any n >= 1.  Exact fp32-input MFMA,
 * column statistics and loss sums in double in a fixed order, no atomics: bitwise run-to-run deterministic, and everything computed
 * from the gathered block alone is identical on every replica.  The workspace holds one fwd/bwd pair. */
size_t simclr_bt_workspace_bytes(int n, int N, int D);          /* 0 for a shape the kernels refuse */
/* Where simclr_bt_fwd keeps the Gram blocks of the local rows in the workspace: fp32 [2, rows, pitch] from that byte offset, block v
 * row a column b = zhat_v[rank*n + a] . zhat_v[b]; rows >= n and pitch >= N are padded to the tile with zeros.  0 for a refused shape. */
size_t simclr_bt_gram_offset_bytes(int n, int N, int D);
size_t simclr_bt_gram_rows(int n, int N, int D);
size_t simclr_bt_gram_pitch(int n, int N, int D);
/* zhat = (h - mu) / sqrt(var + eps) per view and column over the N rows (two passes: mean, then the biased variance from centred
 * squares, sums in double); rstd [2, D] = 1 / sqrt(var + eps) is kept for simclr_bt_apply.  N = 1 gives zhat = 0. */
int simclr_bt_standardize(const float* h_all, int N, int D, float eps, float* zhat_all, float* rstd, simclr_stream_t stream);
/* out[0] = this replica's loss value loss_scaling * (on_diag + lambda_weight * off_diag) with off_diag = R / N^2 * sum_{a local, b}
 * G1_ab G2_ab - sum_i c_i^2 (the mean over the replicas is L), out[1] = on_diag, out[2] = off_diag. */
int simclr_bt_fwd(const float* zhat_all, int n, int N, int D, int rank, float lambda_weight, float loss_scaling, float* out,
                  void* workspace, simclr_stream_t stream);
/* g_local [2n, D] = grad_scale * R * dL/dzhat of the local rows of both views:
 *   g1_a = s * (lambda_weight * (2 / N^2) * sum_b G2_ab zhat1_b + d o zhat2_a / N),  d_i = -2 (1 - c_i) - 2 lambda_weight c_i,
 * s = loss_scaling * grad_scale * R (view 2: G1, zhat2_b, zhat1_a), from the Gram blocks simclr_bt_fwd left in the workspace;
 * colsums [2 views, 2, D] doubles = the column sums over the local rows of g and of g o zhat, to be summed over the replicas. */
int simclr_bt_bwd(const float* zhat_all, int n, int N, int D, int rank, float lambda_weight, float loss_scaling, float grad_scale,
                  void* workspace, float* g_local, double* colsums, simclr_stream_t stream);
/* The standardisation backward: dh_a = (g_a - colsums[v][0] / N - zhat_a o colsums[v][1] / N) * rstd[v], colsums summed over the
 * GLOBAL batch; dh [2n, D] = grad_scale * R * dL/dh of the local rows. */
int simclr_bt_apply(const float* g_local, const float* zhat_all, const float* rstd, const double* colsums, int n, int N, int D, int rank,
                    float* dh, simclr_stream_t stream);

/* ---- VICReg loss (Bardes, Ponce, LeCun 2022, VICReg: Variance-Invariance-Covariance Regularization for Self-Supervised Learning),
 * csrc/vicreg.hip ----
 * The Gram form: per view v of the gathered block, xc = h - colmean(h) over the GLOBAL batch, var_i = sum_a xc_ai^2 / (N - 1)
 * (unbiased), std_i = sqrt(var_i + eps), Cov = xc^T xc / (N - 1) ([D, D], never formed), G = xc xc^T ([N, N]),
 *   inv  = (1 / (N D)) sum_{a, i} (h1_ai - h2_ai)^2,
 *   var  = (1 / 2) sum_v (1 / D) sum_i max(0, gamma - std_vi),
 *   cov  = sum_v (1 / D) sum_{i != j} Cov_v,ij^2 = sum_v (1 / D) ((1 / (N-1)^2) sum_{a, b} G_v,ab^2 - sum_i var_vi^2),
 *   L    = sim_coeff * inv + std_coeff * var + cov_coeff * cov.
 * Layout as simclr_bt_fwd: h_all / xc_all [2N, D] = every replica's view-1 rows, then every replica's view-2 rows, N = R*n; this
 * replica's rows are rank*n .. rank*n + n - 1 of each view.  D a multiple of 64 in [64, 8192], n >= 1, N >= 2.  Exact fp32-input MFMA,
 * one view per workgroup; where both views' tiles give fewer than 256 workgroups the k range (D) is split into S parts at multiples
 * of 32 whose partial tiles a merge launch adds in the fixed order ((p0 + p1) + p2) + ... in fp32.  Column statistics, loss sums and the
 * subtraction in double in a fixed order, no atomics: bitwise run-to-run deterministic, and everything computed from the gathered block
 * alone is identical on every replica.  The workspace holds one fwd/bwd pair. */
size_t simclr_vicreg_workspace_bytes(int n, int N, int D);      /* 0 for a shape the kernels refuse */
/* Where simclr_vicreg_fwd keeps the (merged) Gram blocks of the local rows in the workspace: fp32 [2, rows, pitch] from that byte
 * offset, block v row a column b = xc_v[rank*n + a] . xc_v[b]; rows >= n and pitch >= N are padded to the tile with zeros.  0 for a
 * refused shape. */
size_t simclr_vicreg_gram_offset_bytes(int n, int N, int D);
size_t simclr_vicreg_gram_rows(int n, int N, int D);
size_t simclr_vicreg_gram_pitch(int n, int N, int D);
/* S, the number of k parts of the Gram launch (1: no split, no merge launch), and the workgroups of that launch = 2 views x tiles x S.
 * 0 for a refused shape. */
int simclr_vicreg_k_splits(int n, int N, int D);
int simclr_vicreg_fwd_workgroups(int n, int N, int D);
/* xc = fl32(h - mu) per view and column over the N rows (mean in double); stats [2 views, 2, D] doubles = {var, std}: var from the
 * squares of the ROUNDED xc it stores, summed in double, / (N - 1); std = sqrt(var + eps).  N < 2 is refused. */
int simclr_vicreg_center(const float* h_all, int N, int D, float eps, float* xc_all, double* stats, simclr_stream_t stream);
/* out[0] = this replica's loss value sim_coeff * inv + std_coeff * var + cov_coeff * cov, out[1] = inv over its own rows (1 / (n D)),
 * out[2] = var (global), out[3] = cov with R / (N-1)^2 * sum_{a local, b} G_ab^2 in place of the full sum, reported as computed (never
 * clamped at zero).  The mean over the replicas is L. */
int simclr_vicreg_fwd(const float* h_all, const float* xc_all, const double* stats, int n, int N, int D, int rank, float sim_coeff,
                      float std_coeff, float cov_coeff, float gamma, float* out, void* workspace, simclr_stream_t stream);
/* dh_local [2n, D] = grad_scale * R * dL/dh of the local rows of both views, one launch from the Gram blocks simclr_vicreg_fwd left in
 * the workspace.  With x, o the raw rows of this view and of the other one:
 *   dL/dh_a = cov_coeff * (4 / ((N-1)^2 D) * sum_b G_ab xc_b - 4 / ((N-1) D) * var o xc_a)
 *           - std_coeff * (1 / (2 D)) * [std < gamma] o xc_a / ((N-1) std) + sim_coeff * (2 / (N D)) * (x_a - o_a).
 * The centring has no backward (the column sums of the xc-gradient vanish) and no collective follows. */
int simclr_vicreg_bwd(const float* h_all, const float* xc_all, const double* stats, int n, int N, int D, int rank, float sim_coeff,
                      float std_coeff, float cov_coeff, float gamma, float grad_scale, void* workspace, float* dh_local,
                      simclr_stream_t stream);

/* ---- label-free representation diagnostics, csrc/repr.hip ----
 * z_all [2N, D] fp32 = the l2-normalised projections of the gathered global batch, view a in rows [0, N), view b in rows [N, 2N).
 * Per view v: xc = z_v - colmean(z_v), G = xc xc^T ([N, N], never written), r_a = G_aa.  out4 = {align, uniform, std, rank}:
 *   align   = (1 / N) sum_i |z_a,i - z_b,i|^2                                                    in [0, 4]
 *   uniform = (1/2) sum_v log((1 / (N (N-1))) sum_{a != b} exp(-t max(r_a + r_b - 2 G_ab, 0)))   in [-4t, 0]; 0 = one point
 *   std     = (1/2) sum_v sqrt(D) (1 / D) sum_k sqrt(sum_a xc_ak^2 / (N-1))                      about 1 healthy, 0 collapsed
 *   rank    = (1/2) sum_v (sum_a G_aa)^2 / sum_ab G_ab^2 (the participation ratio of the covariance spectrum, in [1, min(D, N-1)]);
 *             a view with sum_a G_aa / (N-1) <= 1e-12 counts 0.
 * D a multiple of 64 in [64, 8192], 2 <= N <= 65536, 0 < t <= 16.  fp32 storage, exact fp32-input MFMA, every sum in double in a fixed
 * order, no atomics: bitwise run-to-run deterministic and identical on every replica that holds the same block.  Reads z_all only;
 * writes the workspace (16-byte aligned, simclr_repr_workspace_bytes) and out4. */
size_t simclr_repr_workspace_bytes(int N, int D);   /* 0 for a shape the kernels refuse */
/* Edge of the tile of G a workgroup of the pairs launch owns: 128 where both views' tiles give >= 256 workgroups (N >= 1409), else 64.
 * 0 for a refused shape. */
int simclr_repr_tile_edge(int N, int D);
int simclr_repr_stats(const float* z_all, int N, int D, float t, void* ws, float* out4, simclr_stream_t stream);

/* ---- cached-feature linear probe: l2-regularised multinomial logistic regression, csrc/logreg.hip ----
 * x [n, D] fp32 = a slab of standardised features, w [C, D], b [C], labels [n] int32 in [0, C) (the CALLER guarantees the range: a label
 * outside matches no class and is never used as an index), weights [n] fp32 (0 = a padding row), inv_S = 1 / the weight total of the
 * whole bank.  s_nc = x_n . w_c + b_c on the exact fp32-input MFMA, k in a fixed order.
 * simclr_logreg_fwd: lse [n] double = logsumexp_c s_nc; out3 = {sum_n w_n (lse_n - s_n,y_n), sum of w_n over the rows whose label is the
 *   lowest-index maximum, sum_n w_n} as three doubles (NOT scaled by inv_S).  mode 0: nothing else is written.  mode 1: store [n, pitch]
 *   fp32 (pitch = simclr_logreg_store_pitch(C) = C rounded up to 4; columns >= C are never written; the column sum of the backward reads them with their
 *   16-byte quad and ignores them) receives
 *   G_nc = (w_n inv_S) (softmax_c(s_n) - [c = y_n]).  mode 2: store receives the raw logits s_nc.
 * simclr_logreg_bwd: dw [C, D] (+)= G^T X, db [C] (+)= colsum(G) of a slab (accumulate != 0 adds to what dw / db hold).  The slab's rows
 *   are cut into simclr_logreg_row_splits parts (a multiple of 32 rows each, the last one ragged) where the C x D grid alone would leave
 *   CUs idle; the parts are added as ((p0 + p1) + p2) + ... in fp32.
 * D a multiple of 64 in [64, 8192], 2 <= C <= 4096, 1 <= n <= 65536, every pointer 16-byte aligned.  No atomics, every reduction in a
 * fixed order: repeat calls are bitwise equal.  Both calls share one workspace of simclr_logreg_workspace_bytes. */
size_t simclr_logreg_workspace_bytes(int n, int D, int C);   /* 0 for a shape the kernels refuse */
int simclr_logreg_row_splits(int n, int D, int C);           /* row parts of the backward product; 0 for a refused shape */
int simclr_logreg_tile_edge(int n, int D, int C);            /* edge (64 or 128) of the forward's logit tile; 0 for a refused shape */
int simclr_logreg_bwd_tile_edge(int n, int D, int C);        /* edge (64 or 128) of the backward's dW tile; 0 for a refused shape */
int simclr_logreg_store_pitch(int C);                        /* floats per row of store; 0 for a refused C */
int simclr_logreg_fwd(const float* x, const float* w, const float* b, const int* labels, const float* weights, int n, int D, int C,
                      double inv_S, int mode, float* store, double* lse, double* out3, void* workspace, simclr_stream_t stream);
int simclr_logreg_bwd(const float* g, const float* x, int n, int D, int C, float* dw, float* db, int accumulate, void* workspace,
                      simclr_stream_t stream);

/* ---- spherical k-means on frozen features: assignment, segmented sums and the centroid finish, csrc/kmeans.hip ----
 * x [n, D] fp32 = a slab of unit rows, c [K, D] fp32 = unit centroids, weights [n] fp32 (0 = a padding row).  A score x_n . c_k runs on
 * the exact fp32-input MFMA, k in a fixed order that depends on neither the tile's position nor n nor K: it is a function of the two rows.
 * simclr_kmeans_assign: assign [n] int32 = argmax_k x_n . c_k (ties to the lowest k, a NaN score below every number; a row whose scores
 *   are all NaN gets 0 and best = NaN), best [n] fp32 = that score, out3 = {sum_n w_n (1 - best_n), sum_n w_n, the number of rows with
 *   w_n > 0 whose assignment differs from the value assign held ON ENTRY} as three doubles; only rows with w_n > 0 enter them.  assign is
 *   read before it is written: the first call passes it filled with -1.  The [n, K] scores are never written.
 * simclr_kmeans_update: sums [K, D] double (+)= sum_j w_r x_r over r = order[j], offsets[k] <= j < offsets[k+1], in ascending j;
 *   wsum [K] double (+)= the same sum of w_r (accumulate != 0 adds to what they hold).  order [n] int32 = the slab's rows sorted by
 *   assignment (stable), offsets [K + 1] int32 = the segment starts.  No index read from memory is dereferenced unchecked: an order
 *   entry outside [0, n) is skipped, an offsets entry is clamped to [0, n].
 * simclr_kmeans_finish: c_new_k = fp32(sums_k / |sums_k|), normalised in double; a cluster with wsum_k <= 0 or |sums_k|^2 <= 1e-24 (or
 *   not finite) keeps c_prev_k.  out2 = {number of kept clusters, max_k (1 - c_new_k . c_prev_k)} as two doubles.  c_new may not alias
 *   c_prev.  Its workspace is the head (2 K doubles) of any workspace of simclr_kmeans_workspace_bytes(n, D, K).
 * D a multiple of 64 in [64, 8192], 2 <= K <= 16384, 1 <= n <= 65536, every pointer 16-byte aligned.  No atomics, every reduction in a
 * fixed order: repeat calls are bitwise equal. */
size_t simclr_kmeans_workspace_bytes(int n, int D, int K);   /* 0 for a shape the kernels refuse */
int simclr_kmeans_tile_edge(int n, int D, int K);            /* edge (64 or 128) of the assignment's score tile; 0 for a refused shape */
int simclr_kmeans_assign(const float* x, const float* c, const float* weights, int n, int D, int K, int* assign, float* best, double* out3,
                         void* workspace, simclr_stream_t stream);
int simclr_kmeans_update(const float* x, const float* weights, const int* order, const int* offsets, int n, int D, int K, double* sums,
                         double* wsum, int accumulate, simclr_stream_t stream);
int simclr_kmeans_finish(const double* sums, const double* wsum, const float* c_prev, int K, int D, float* c_new, double* out2,
                         void* workspace, simclr_stream_t stream);

/* ---- eigen-spectrum evaluation of frozen features: column sums and the centred covariance, csrc/spectrum.hip ----
 * x [n, D] fp32 = a slab of (unnormalised) rows, weights [n] fp32.  A row is COUNTED when its weight is > 0 and not at all otherwise: the
 * kernels select, they never multiply, and an uncounted row is not read (a NaN or inf in it changes no output bit).
 * simclr_spectrum_colsum: sums [D + 1] double (+)= {the column sums of the counted rows, their number} (accumulate != 0 adds to what
 *   sums holds).
 * simclr_spectrum_cov: cov [D, D] double (+)= sum_counted (x_n - mu32)(x_n - mu32)^T, mu32 [D] fp32 = the caller's mean rounded to
 *   fp32 (the caller applies - S delta delta^T, delta = mu - mu32, in double).  The rows are centred into an fp32 scratch in the
 *   workspace first; the product runs on the exact fp32-input MFMA over the tile pairs (i <= j) only, the slab's rows cut into
 *   simclr_spectrum_row_parts parts (a multiple of 32 rows each, the last one ragged, none longer than 8192 rows).  A part accumulates
 *   in fp32; the parts, then the slab, are added in double in ascending order, and the mirror element is written from the same
 *   register: cov[a, b] and cov[b, a] hold the same bits (with accumulate != 0, provided they did on entry).
 * D a multiple of 64 in [64, 8192], 1 <= n <= 65536, every pointer 16-byte aligned.  No atomics, every reduction in a fixed order:
 * repeat calls are bitwise equal. */
int simclr_spectrum_dim_ok(int D);                           /* 1 for a width the kernels take, else 0 */
size_t simclr_spectrum_workspace_bytes(int n, int D);        /* both entry points; 0 for a shape the kernels refuse */
size_t simclr_spectrum_colsum_workspace_bytes(int n, int D); /* what simclr_spectrum_colsum alone needs (the head of the above); 0 if refused */
int simclr_spectrum_tile_edge(int n, int D);                 /* edge (64 or 128) of the covariance tile; 0 for a refused shape */
int simclr_spectrum_row_parts(int n, int D);                 /* row parts of the covariance product; 0 for a refused shape */
int simclr_spectrum_colsum(const float* x, const float* weights, int n, int D, double* sums, int accumulate, void* workspace,
                           simclr_stream_t stream);
int simclr_spectrum_cov(const float* x, const float* weights, const float* mu32, int n, int D, double* cov, int accumulate,
                        void* workspace, simclr_stream_t stream);

/* ---- weighted k-NN evaluation of frozen features (Wu et al. 2018), csrc/knn.hip ---------------------------------------- */
/* q [Q, D], bank [N, D] fp32 row-major, unpadded.  s(i, j) = sum_d q[i,d] bank[j,d] on the exact fp32-input MFMA, accumulated in a fixed
 * order over d: a function of the two rows alone (not of i, j, Q, N or the tile), so sharding the bank or the queries changes no bit.
 * Row i of top_val [Q, k] fp32 / top_idx [Q, k] int32 = the first k pairs of the total order "similarity descending, bank index
 * ascending", in that order; a NaN similarity orders below every number.  1 <= k <= 256 (a candidate list is sorted in LDS),
 * k <= N < 2^31, D a multiple of 16, Q >= 1.  The [Q, N] matrix is never written: a workgroup keeps the k best of a bank slab of
 * simclr_knn_slab_rows() rows per query, a second launch merges the slabs; workspace = Q * ceil(N / slab) * k * 8 bytes.  No
 * floating-point atomics; bitwise repeatable. */
int simclr_knn_slab_rows(void);
size_t simclr_knn_workspace_bytes(int Q, int N, int D, int k);
int simclr_knn_topk(const float* q, const float* bank, int Q, int N, int D, int k, float* top_val, int* top_idx, void* workspace,
                    simclr_stream_t stream);
/* top_val [Q, k] as written by simclr_knn_topk, top_label [Q, k] int32 = the neighbours' class ids.  w_r = exp((top_val[i,r] -
 * top_val[i,0]) / temperature) in fp32; score_c = the sum of w_r over the neighbours of class c, added in ascending rank order r.
 * pred [Q, 5] int32 / score [Q, 5] fp32 = the five best classes by "score descending, class id ascending" (classes without a neighbour
 * score 0); with fewer than five classes the unused entries are -1 / 0.  The class scores live in LDS: 1 <= num_classes <= 32768. */
int simclr_knn_vote(const float* top_val, const int* top_label, int Q, int k, int num_classes, float temperature, int* pred, float* score,
                    simclr_stream_t stream);

/* ---- LARS: tf2/lars_optimizer.py:83-137 (_resource_apply_dense), all tensors in 2 launches ---- */
/* table: device int64[5*T] = {w ptrs | g ptrs | v ptrs | numel | flags(bit0 use_weight_decay :139-148,
 * bit1 do_layer_adaptation :150-157)}; chunks: device int64[2*num_chunks] = (tensor id, element
 * offset), one per simclr_lars_chunk_elems() elements, a tensor's chunks consecutive and in offset order; norms: device
 * double[2*num_chunks] scratch (per-chunk partial norms, summed in a fixed order: the update is run-to-run deterministic).
 * lr_dev (nullable) overrides lr with a device-resident value (graph replay). */
int simclr_lars_chunk_elems(void);
int simclr_lars_multi_tensor(const long long* table, int num_tensors, const long long* chunks,
                             int num_chunks, const float* lr_dev, float lr, float momentum,
                             float weight_decay, float eeta, int classic_momentum, int use_nesterov,
                             double* norms, simclr_stream_t stream);
/* The other two branches of build_optimizer (tf2/model.py:31-34), same descriptor / chunk tables (row 2 = the slot; flags
 * bit 0 = add l2 * w to the gradient: the derivative of add_weight_decay's loss term, tf2/model.py:62-69).
 * simclr_sgd_multi_tensor: tf.keras.optimizers.SGD(lr, momentum, nesterov): accum = momentum * accum - lr * g;
 * w += nesterov ? momentum * accum - lr * g : accum.  simclr_adam_multi_tensor: tf.keras.optimizers.Adam (the slot holds
 * 2 * numel floats: m, then v); step = 1-based update count of the bias correction. */
int simclr_sgd_multi_tensor(const long long* table, int num_tensors, const long long* chunks, int num_chunks,
                            const float* lr_dev, float lr, float momentum, int use_nesterov, float l2, simclr_stream_t stream);
int simclr_adam_multi_tensor(const long long* table, int num_tensors, const long long* chunks, int num_chunks,
                             const float* lr_dev, float lr, float beta1, float beta2, float epsilon, long long step, float l2,
                             simclr_stream_t stream);

/* ---- convolution / dense: tf2/resnet.py:183-208 (Conv2dFixedPadding), tf2/model.py:143-154 ----- */
/* Matrix arithmetic of the SIMCLR_DT_F32 convolution / dense launches (the reference's tf.nn.conv2d / tf.matmul on float32,
 * resnet.py:196-208, model.py:148-153): number of bf16 terms per fp32 product, for the forward GEMM and for the two backward
 * GEMMs (dgrad, wgrad).  0 (default) = exact fp32 MFMA; 3 = x_hi*w_hi + x_hi*w_lo + x_lo*w_hi (~2^-17 per product);
 * 6 = every term of weight >= 2^-18 of a three-way split (fp32 level).  Storage, accumulation, statistics and every
 * elementwise kernel stay fp32; bf16 launches are unaffected.  fwd_terms = 13 (round 6): three FP16-piece terms
 * (11-bit pieces: ~2^-22 per product, the accuracy of six bf16 terms at half the MFMA work; operands must lie within fp16's
 * range -- BatchNorm outputs, images, weights do; an out-of-range operand gives inf / NaN, never a silently wrong value; the
 * stem keeps six bf16 terms).  This call sets the process-wide DEFAULT only: a convolution / dense entry point whose `dtype`
 * carries SIMCLR_FMT_TERMS(t) runs with t whatever the default is (the re-entrant form; simclr_amd/ops.py always sends it).
 * The setting is a LOWER bound on accuracy: the non-persistent fallback kernel (more than 64 N-tiles) always runs the exact fp32 MFMA whatever is selected here.
 * simclr_get_f32_matmul(0 | 1) returns the forward | backward setting. */
int simclr_set_f32_matmul(int fwd_terms, int bwd_terms);
int simclr_get_f32_matmul(int which);
/* Scheduling of simclr_conv2d_fwd / _dgrad / _dgrad_bn / _fwd_bn_apply (no reference counterpart: TensorFlow's runtime
 * schedules its own kernels): the persistent grid runs floor(tiles / workgroups) whole output tiles per workgroup and
 * shares every left-over tile between 2..8 workgroups along the reduction ("split tail"); the partial fp32 accumulators
 * meet in a scratch buffer the LIBRARY owns -- the one exception to "never allocates": <= 64 MB per stream, hipMalloc'ed
 * on the first launch that needs it (outside any graph capture), kept for the life of the process.  Results are
 * deterministic (fixed summation order).  Environment SIMCLR_IGEMM_SPLIT=0 disables it.  The hook below returns the
 * number of parts the most recent launch used (0 = whole tiles only); tests use it to prove the path ran. */
int simclr_conv2d_last_split_parts(void);
/* The owner of a shared tile waits for its partners with a BOUNDED spin (a lost partner must not hang the device).  A partner
 * that never arrives is counted in a sticky device word next to the flags; this call copies the counters back (synchronous --
 * call it where the host synchronises anyway: simclr_amd/run.py does at every logging interval) and returns their sum in
 * *host_total: 0 on a healthy device.  The flags are reset by the consumer inside the launch and carry no host-side sequence
 * number, so a launch captured into a hipGraph replays correctly (the scratch must exist before the capture starts). */
int simclr_conv2d_split_tail_timeouts(unsigned* host_total);
/* Which kernel instantiation the most recent forward / dgrad launch of this process selected: the template-argument list as
 * spelled at the launch site plus element size, GEMM role, grid, block, LDS bytes, tile counts and split-tail parts.  With the
 * environment variable SIMCLR_DRY_RUN=1 the convolution entry points take every launch decision and record it here WITHOUT
 * touching the device (pointers are not dereferenced, nothing is allocated or launched): tools/instantiation_table.py dumps the
 * (layer class -> instantiation) table of the benchmark models on a machine without a GPU. */
const char* simclr_conv2d_last_instantiation(void);
/* Three-term data gradient of the SIMCLR_DT_F32 launches (simclr_set_f32_matmul(*, 3)): the weight operand is rewritten once per
 * launch into (hi, lo) bf16 planes in a library-owned per-stream buffer (the second exception to "never allocates": the
 * largest weight matrix, >= 16 MB, hipMalloc'ed on first use), so the k-loop does no splitting work for it; bitwise the
 * same result as the in-register split.  Environment SIMCLR_F32_PRESPLIT=0 disables it.  The hook returns 1 if the most
 * recent fp32 data-gradient launch took that path. */
int simclr_conv2d_last_presplit(void);
/* master HWIO fp32 -> compute copies.  mode 0: [Cout][KH*KW*Cin] (fwd), 1: [Cin][KH*KW*Cout]
 * (dgrad), 2: stem [Cout][KHP][KWP][4] zero padded.  CinP/CoutP (0 = none): zero-padded channel dims. */
int simclr_prep_weights(const float* w_hwio, void* dst, int KH, int KW, int Cin, int Cout, int mode,
                        int KHP, int KWP, int CinP, int CoutP, int dtype, simclr_stream_t stream);
/* modes 0 (dst_t) and 1 (dst_d) of the same weight in one launch. */
int simclr_prep_weights_pair(const float* w_hwio, void* dst_t, void* dst_d, int KH, int KW, int Cin, int Cout,
                             int CinP, int CoutP, int dtype, simclr_stream_t stream);
/* The (dst_t, dst_d) pairs of MANY convolutions in one launch: the refresh of every compute copy after an optimizer
 * step (tf2/resnet.py:183-208 has 52 of these layers in ResNet-50).  table: device int64 [T][8] = {w_hwio, dst_t, dst_d,
 * KH*KW, Cin, Cout, CinP, CoutP}; chunks: device int64 [nchunks][2] = {tensor index, tile}: one entry per E x E tile
 * (E = simclr_prep_chunk_elems()) of every tap's padded (CinP, CoutP) plane, tile = (tap * nci + ci_tile) * nco + co_tile,
 * nci = ceil(CinP / E), nco = ceil(CoutP / E). */
int simclr_prep_chunk_elems(void);
int simclr_prep_weights_pair_multi(const long long* table, const long long* chunks, int nchunks, int dtype,
                                   simclr_stream_t stream);
/* Partial-statistics slots.  Every `stats` / `partial` argument below is float [nslot][2][C], zeroed by the caller.
 * With nslot >= the number returned here each producing workgroup stores into its OWN slot (no float atomics) and the
 * slot reduction of simclr_bn_finalize / simclr_bn_bwd_finalize / simclr_bn_reduce_slots adds the slots in a fixed
 * order: BatchNorm statistics are then bit-identical from run to run, like the reference's SyncBatchNormalization
 * (tf2/resnet.py:54-60).  With fewer slots the producers fall back to float atomics into slot (workgroup % nslot). */
int simclr_conv2d_stats_slots(long long M, int C);      /* simclr_conv2d_fwd, simclr_conv2d_dgrad_bn: M output rows x C channels */
int simclr_stem_stats_slots(long long M);               /* simclr_stem_conv_fwd: M = V*OH*OW */
int simclr_bn_bwd_reduce_slots(long long rows, int C, int dtype);

/* y[V,OH,OW,Cout] = conv(x[V,IH,IW,Cin], w), explicit symmetric padding `pad` (resnet.py:167-180).
 * stats (nullable) float[nslot][2][Cout], zeroed by caller: per-channel partial (sum, sum sq) of y
 * for BatchNorm (resnet.py:50-78) -- of the fp32 accumulators (128-wide tiles, eight-phase 256-wide tile); the 256 x 256
 * instantiation of the persistent kernel (SIMCLR_IGEMM_TILE=256 / K-extended dgrad classes) takes them over the bf16-ROUNDED
 * outputs, the tensor the reference's moments see: the two differ by the output rounding (<= 2^-9 relative per element,
 * ~1e-5 sigma on the mean at 10^5 rows).  Cin % 64 == 0 (bf16) / 32 (f32); Cout % 4 == 0 (bf16 with Cout % 8 != 0 runs the
 * non-persistent kernel, like Cout > 8192: the persistent kernels store bf16 rows in 16-byte chunks of 8 channels).
 * y == NULL (bf16, stats required, Cout % 8 == 0, Cout <= 8192): statistics-only pass -- the convolution is computed, nothing is stored. */
int simclr_conv2d_fwd(const void* x, const void* w_t, void* y, float* stats, int nslot, int V, int IH,
                      int IW, int Cin, int OH, int OW, int Cout, int KH, int KW, int stride, int pad,
                      int dtype, simclr_stream_t stream);
/* simclr_conv2d_fwd for SIMCLR_DT_F32 with PIVOTED BatchNorm statistics (resnet.py:50-78: the moments of the convolution
 * output).  pivot float[Cout] (out): the convolution output at one interior pixel (image 0, OH/2, OW/2); the slots receive
 * sum(y - pivot[n]) and sum((y - pivot[n])^2) over the valid rows, and simclr_bn_reduce_slots_pivoted(count = V*OH*OW) turns
 * them into the raw fp64 moments simclr_bn_finalize(sums) takes.  Raw fp32 moments lose (mean / sigma)^2 * 2^-24 of the
 * variance; about a pivot the sums stay at the scale of the spread.  y, stats and pivot are required. */
int simclr_conv2d_fwd_pivoted(const void* x, const void* w_t, void* y, float* stats, int nslot, float* pivot, int V,
                              int IH, int IW, int Cin, int OH, int OW, int Cout, int KH, int KW, int stride, int pad,
                              int dtype, simclr_stream_t stream);
/* The same convolution with its consumer's BatchNorm apply in the epilogue (bf16 only; resnet.py:470-487, conv3 -> bn3 ->
 * + shortcut -> relu):  y = act(bf16(conv(x)) * scale + shift + r), r = res or res * rscale + rshift (projection shortcut
 * whose BatchNorm is applied here too, resnet.py:411-421);  relu_bits[i] bit e = (y[8 i + e] > 0).
 * Bitwise equal to simclr_conv2d_fwd followed by simclr_bn_apply; the convolution output never reaches memory.
 * scale / shift [Cout]: from simclr_bn_finalize over the statistics of a first simclr_conv2d_fwd(y = NULL) pass.
 * res (nullable) [V,OH,OW,Cout]; rscale / rshift (nullable, both or none) [Cout]; relu: 0 | 1; relu_bits (nullable)
 * uint8 [V*OH*OW*Cout/8]. */
int simclr_conv2d_fwd_bn_apply(const void* x, const void* w_t, void* y, const float* scale, const float* shift,
                               const void* res, const float* rscale, const float* rshift, int relu,
                               unsigned char* relu_bits, int V, int IH, int IW, int Cin,
                               int OH, int OW, int Cout, int KH, int KW, int stride, int pad, int dtype,
                               simclr_stream_t stream);
/* dx[V,IH,IW,Cin] (+)= conv_transpose(dy[V,OH,OW,Cout], w); autodiff of the above (run.py:621). */
int simclr_conv2d_dgrad(const void* dy, const void* w_d, void* dx, int accumulate, int V, int IH, int IW,
                        int Cin, int OH, int OW, int Cout, int KH, int KW, int stride, int pad, int dtype,
                        simclr_stream_t stream);
/* dgrad whose output is the gradient wrt a BatchNormRelu output (tf2/resnet.py:74-78): the ReLU mask and
 * the BatchNorm-backward reductions sum(dm), sum(dm*x^) are fused into the epilogue; dx receives
 * dm = dx*mask.  stats float[nslot][2][Cin] zeroed by the caller.  mask_mode 1: bn_mask>0 (tensor after the
 * ReLU, e.g. the block output of resnet.py:487); 2: bn_x*scale+shift>0; 3: bn_mask = the bit tensor written by
 * simclr_bn_apply(relu_bits) (16x less traffic than mode 1); 4: as 3 but ONLY sum(dm) is produced and bn_x / bn_mean /
 * bn_rstd are not read (may be NULL) -- sum(dm*x^) then comes from simclr_bn_fold_s2.  stride 1 only; Cin % 8 == 0 (bf16) / 4 (f32). */
int simclr_conv2d_dgrad_bn(const void* dy, const void* w_d, void* dx, int accumulate, const void* bn_x,
                           const void* bn_mask, const float* bn_scale, const float* bn_shift,
                           const float* bn_mean, const float* bn_rstd, int mask_mode, float* stats, int nslot,
                           int V, int IH, int IW, int Cin, int OH, int OW, int Cout, int KH, int KW,
                           int stride, int pad, int dtype, simclr_stream_t stream);
size_t simclr_conv2d_wgrad_workspace_bytes(int V, int OH, int OW, int Cin, int Cout, int KH, int KW,
                                           int dtype);
/* dw[KH*KW*Cin][Cout] fp32 (HWIO) (+)= x^T * dy.  `pixpitch` = elements between neighbouring pixels
 * of x (== Cin except for the packed stem input). */
int simclr_conv2d_wgrad(const void* x, const void* dy, float* dw, int accumulate, void* workspace, int V,
                        int IH, int IW, int Cin, int pixpitch, int OH, int OW, int Cout, int KH, int KW,
                        int stride, int pad, int dtype, simclr_stream_t stream);
/* stem conv (Cin=3; resnet.py:593-599 7x7 s2, :551-556 CIFAR 3x3 s1) on the packed input */
int simclr_stem_conv_fwd(const void* xp, const void* w_s, void* y, float* stats, int nslot, int V, int HP,
                         int WP, int OH, int OW, int Cout, int KHP, int KWP, int stride, int dtype,
                         simclr_stream_t stream);
int simclr_unpack_stem_dw(const float* src, float* dst, int KH, int KW, int Cin, int Cout, int KWP,
                          int accumulate, simclr_stream_t stream);
/* Stem weight gradient of the three-term parity mode (fp32 storage, three bf16-piece backward terms) from PRE-SPLIT operands
   (tf2/resnet.py:593-599 under tape.gradient): xq = simclr_presplit_packed(xp) -- every packed pixel [4] fp32 becomes four bf16 hi
   pieces followed by four bf16 lo pieces, same 16 bytes --, dy_ps [V*OH*OW][64] in the pre-split block format
   (simclr_bn_bwd_apply with SIMCLR_FMT_PS_OUT).  dw_kn: fp32 [KH*KWP*4][64], the layout simclr_unpack_stem_dw reads; workspace:
   simclr_stem_wgrad_ps_workspace_bytes.  Only the 7x7 / stride-2 stem with 64 output channels (simclr_stem_wgrad_ps_supported);
   every other stem keeps simclr_conv2d_wgrad on the packed input. */
int simclr_presplit_packed(const void* xp, void* xq, long long npix, simclr_stream_t stream);
/* Pre-split copies of n compute-weight matrices in ONE launch (what the three-term forward / data-gradient launches otherwise make of
   their weight operand per call): table [n][4] int64 on the device = (source fp32 [rows][K], K % 32 == 0; destination, same size;
   128-byte k-blocks = rows * K / 32; pieces: 0 = bf16 -- a data-gradient call's w_d --, 1 = fp16 of 2^8 * w -- a forward call's w_t);
   max_blocks = the largest block count in the table.  Pass the destination as the weight argument together with SIMCLR_FMT_PS_W. */
int simclr_presplit_weights_multi(const long long* table, int n, long long max_blocks, simclr_stream_t stream);
int simclr_stem_wgrad_ps_supported(int KH, int KWP, int stride, int Cout);
size_t simclr_stem_wgrad_ps_workspace_bytes(int V, int OH, int OW, int KH);
int simclr_stem_wgrad_ps(const void* xq, const void* dy_ps, float* dw_kn, int accumulate, void* workspace, int V, int HP,
                         int WP, int OH, int OW, int Cout, int KH, int KWP, int stride, simclr_stream_t stream);

/* ---- BatchNorm: tf2/resnet.py:31-78 (BatchNormRelu), residual tail :382/:487 ------------------- */
int simclr_bn_reduce_slots(const float* partial, int nslot, int C, double* sums, simclr_stream_t stream);
/* slots of simclr_conv2d_fwd_pivoted -> raw moments: sums[c] = S1 + count p, sums[C + c] = S2 + 2 p S1 + count p^2 (fp64) */
int simclr_bn_reduce_slots_pivoted(const float* partial, int nslot, int C, const float* pivot, double count, double* sums,
                                   simclr_stream_t stream);
/* BatchNorm statistics of c = h W (1x1 convolution, tf2/resnet.py:470-474 conv3 -> bn3) without forming c:
 * sums[0][n] = sum_k colsum(h)[k] W[k][n], sums[1][n] = sum_k GW[k][n] W[k][n] with GW = (h^T h) W [K][N] (fp32, from
 * simclr_conv2d_gram + simclr_small_gemm_nt_f32), w_kn = the weights as multiplied, fp32 [K][N]; colsum(h) as fp64
 * (cs64) or fp32 (cs32), exactly one non-NULL.  sums: double [2][N], the operand of simclr_bn_finalize. */
int simclr_bn_sums_from_gram(const float* gw, const float* w_kn, const double* cs64, const float* cs32, int K, int N,
                             double* sums, simclr_stream_t stream);
/* sums [2][C] fp64 (after the cross-replica all-reduce) OR partial [nslot][2][C] fp32 (single replica). */
int simclr_bn_finalize(const double* sums, const float* partial, int nslot, double count, int C,
                       const float* gamma, const float* beta, float* moving_mean, float* moving_var,
                       float decay, float eps, float* mean, float* rstd, float* scale, float* shift,
                       simclr_stream_t stream);
/* y = [relu]( x*scale+shift [+ res | + res*rscale+rshift] ).  relu_bits (nullable): receives the ReLU mask
 * (y > 0) as one byte per 16-byte chunk of y (bit e = element e of the chunk: 8 channels bf16, 4 channels f32),
 * i.e. unsigned char [rows][C/8] (bf16) or [rows][C/4] (f32) -- what simclr_conv2d_dgrad_bn mask_mode 3 reads
 * instead of the whole block output. */
int simclr_bn_apply(const void* x, const float* scale, const float* shift, const void* res,
                    const float* rscale, const float* rshift, void* y, unsigned char* relu_bits,
                    long long rows, int C, int relu, int dtype, simclr_stream_t stream);
/* mask_mode: 0 none, 1 (mask_src > 0), 2 (x*scale+shift > 0)  -- the ReLU gradient */
int simclr_bn_bwd_reduce(const void* dy, const void* x, const void* mask_src, const float* scale,
                         const float* shift, const float* mean, const float* rstd, long long rows, int C,
                         int mask_mode, float* partial, int nslot, int dtype, simclr_stream_t stream);
int simclr_bn_bwd_finalize(const double* local_sums, const double* global_sums, const float* partial,
                           int nslot, double count, int C, float* dgamma, float* dbeta, int accumulate,
                           float* c1, float* c2, simclr_stream_t stream);
int simclr_bn_bwd_apply(const void* dy, const void* x, const void* mask_src, const float* scale,
                        const float* shift, const float* mean, const float* rstd, const float* c1,
                        const float* c2, long long rows, int C, int mask_mode, void* dx, void* dmasked,
                        int dtype, simclr_stream_t stream);

/* ---- view packing / pooling: tf2/model.py:250-259, tf2/resnet.py:602-611, :693-696 ------------- */
int simclr_pack_views(const float* images, void* xp, int b, int H, int W, int k, int HP, int WP, int pad,
                      int dtype, simclr_stream_t stream);
/* the same with the pre-split copy of the packed pixels (simclr_presplit_packed) written in the same pass; fp32 only */
int simclr_pack_views_ps(const float* images, void* xp, void* xq, int b, int H, int W, int k, int HP, int WP, int pad,
                         simclr_stream_t stream);
int simclr_bnrelu_maxpool_fwd(const void* x, const float* scale, const float* shift, void* y,
                              unsigned char* arg, int V, int H, int W, int C, int OH, int OW, int ksz,
                              int stride, int pad_t, int pad_l, int dtype, simclr_stream_t stream);
int simclr_maxpool_bwd(const void* dy, const unsigned char* arg, void* dx, int V, int H, int W, int C,
                       int OH, int OW, int ksz, int stride, int pad_t, int pad_l, int dtype,
                       simclr_stream_t stream);
/* Stem backward with the max-pool backward fused in (the gradient wrt the BN+ReLU output is never written): BN-backward
 * reduce and apply straight from the pooled gradient + arg-max taps (tf2/resnet.py:602-611 under tape.gradient). */
int simclr_bn_bwd_pool_slots(long long rows, int C, int dtype);
int simclr_bn_bwd_reduce_pool(const void* dy, const unsigned char* arg, const void* x, const float* scale,
                              const float* shift, const float* mean, const float* rstd, int V, int H, int W, int C,
                              int OH, int OW, int ksz, int stride, int pad_t, int pad_l, float* partial, int nslot,
                              int dtype, simclr_stream_t stream);
int simclr_bn_bwd_apply_pool(const void* dy, const unsigned char* arg, const void* x, const float* scale,
                             const float* shift, const float* mean, const float* rstd, const float* c1, const float* c2,
                             void* dx, int V, int H, int W, int C, int OH, int OW, int ksz, int stride, int pad_t, int pad_l,
                             int dtype, simclr_stream_t stream);
int simclr_global_avgpool_fwd(const void* x, void* y, int V, int HW, int C, int dtype,
                              simclr_stream_t stream);
int simclr_global_avgpool_fwd_f32(const void* x, float* y32, int V, int HW, int C, int dtype,
                                  simclr_stream_t stream);   /* same mean, float32 output (input of fp32 heads) */
int simclr_global_avgpool_bwd(const void* dy, const void* mask_src, void* dx, int V, int HW, int C,
                              int dtype, simclr_stream_t stream);

/* ---- on-device augmentation: batch_random_blur, tf2/data_util.py:323-361,413-440 (tf2/model.py:255-258) ---- */
int simclr_batch_blur(const float* images, float* tmp, float* out, const float* filt, const float* selector,
                      int b, int H, int W, int nviews, int K, simclr_stream_t stream);
/* the same followed by solarization in the blur's last pass: solarize [nviews][b] in {0,1} (laid out like selector); after the
 * clip an element v of a (view, image) whose coin is set becomes v >= threshold ? 1 - v : v.  Unselected images are copied,
 * clipped and solarized; K = 1 with an all-zero selector is copy + clip + solarize.  All coins 0: bitwise simclr_batch_blur.
 * Error code for a null pointer, a non-positive size, an even or non-positive K, a threshold outside [0, 1] or NaN. */
int simclr_batch_blur_solarize(const float* images, float* tmp, float* out, const float* filt, const float* selector,
                               const float* solarize, float threshold, int b, int H, int W, int nviews, int K,
                               simclr_stream_t stream);

/* ---- ResNet-D shortcut pool (tf2/resnet.py:330-338,400-408) and selective-kernel unit (:266-277) ---- */
int simclr_avgpool2_fwd(const void* x, void* y, int V, int H, int W, int C, int stride, int dtype,
                        simclr_stream_t stream);
int simclr_avgpool2_bwd(const void* dy, void* dx, int V, int H, int W, int C, int stride, int dtype,
                        simclr_stream_t stream);
int simclr_sk_pool_fwd(const void* a, void* g, int V, int HW, int f, int gpitch, int dtype, simclr_stream_t stream);
int simclr_sk_mix_fwd(const void* a, const void* l, void* out, int V, int HW, int f, int lpitch, int dtype,
                      simclr_stream_t stream);
int simclr_sk_mix_bwd_logits(const void* a, const void* l, const void* dout, void* dl, int V, int HW, int f,
                             int lpitch, int dtype, simclr_stream_t stream);
int simclr_sk_mix_bwd_streams(const void* l, const void* dout, const void* dg, void* da, int V, int HW, int f,
                              int lpitch, int gpitch, int dtype, simclr_stream_t stream);

/* ---- supervised (linear-eval) head tail: tf2/objective.py:27-32, tf2/metrics.py:49-55 ---------- */
int simclr_bias_softmax_xent(const void* z, const float* bias, const int* labels, int rows,
                             int label_rows, int nclass, int cpad, float gscale, void* dlogits,
                             float* out, int dtype, simclr_stream_t stream);
int simclr_colsum(const void* x, int rows, int C, int cvalid, float* out, int accumulate, int dtype,
                  simclr_stream_t stream);

/* ---- distillation (self-training) tail: add_kd_loss, tf2/colabs/distillation_self_training.ipynb:803-808, with the teacher
 * agreement of the step at :908-919.  s = zs + bias_s (student), t = zt + bias_t (teacher), T = temperature:
 *   out[0] += T^2 * mean_rows(-sum_c softmax(t/T)_c log softmax(s/T)_c);  out[1] += share of rows with argmax s == argmax t (first
 *   maximum wins); dlogits[row][c] = T * (softmax(s/T)_c - softmax(t/T)_c) * gscale / rows in the student's dtype, 0 for
 *   nclass <= c < cpad_s.  Row pitches cpad_s, cpad_t >= nclass and storage dtypes dtype_s, dtype_t are independent; pad columns of
 *   the inputs are never read; either bias may be NULL; fp32 arithmetic with both row maxima subtracted.  out is added to: the caller
 *   zeroes it (as for simclr_bias_softmax_xent). */
int simclr_kd_softmax_xent(const void* zs, const float* bias_s, const void* zt, const float* bias_t, int rows, int nclass,
                           int cpad_s, int cpad_t, float temperature, float gscale, void* dlogits, float* out,
                           int dtype_s, int dtype_t, simclr_stream_t stream);

/* ---- small helpers ------------------------------------------------------------------------------ */
/* dtype hand-over between the fp32 heads / loss and the T-typed encoder (tf2/model.py:262-266) */
int simclr_cast(const void* x, void* y, long long n, int dtype_in, int dtype_out, simclr_stream_t stream);
/* y += a*x: gradient of the supervised head's L2 term (tf2/model.py:49-60, run.py:609-612) */
int simclr_axpy_f32(float a, const float* x, float* y, long long n, simclr_stream_t stream);
/* Metric bookkeeping of one step in one launch (tf2/run.py:587-613: update_pretrain_metrics_train, update_finetune_metrics_train,
 * weight_decay, total_loss = the sum of the loss terms).  src: HOST array of n <= 16 device scalar pointers, scale: host array
 * of n factors (NULL = 1): dst[i] += scale[i] * *src[i] (dst NULL: skipped); total (nullable) receives the sum of the scaled
 * terms whose bit is set in total_mask; copy (nullable, n floats) receives the scaled terms themselves -- the step's
 * scalars live in a per-step arena that the next step reuses, the copy is what a caller may keep. */
int simclr_accumulate_scalars(const float* const* src, const float* scale, int n, float* dst, float* total,
                              int total_mask, float* copy, simclr_stream_t stream);
int simclr_l2_loss_f32(const float* x, long long n, float* out, simclr_stream_t stream); /* tf.nn.l2_loss, model.py:49-60 */

/* ---- BatchNorm backward FOLDED into the convolution that produced the BN's input (1x1 expand convs, K <= N): what
 * tape.gradient (tf2/run.py:621) yields for conv -> BatchNormalization (tf2/resnet.py:460-467, the block's last conv + BN)
 * without ever forming the gradient wrt the conv output.  With c = h W, dh = a*dm + b*c + d per channel:
 *   dW = (h^T dm)*a + ((h^T h) W)*b + colsum(h) (x) d ;   d(h) = dm (a*W)^T + h (W diag(b) W^T) + W d.
 * simclr_bn_fold_pre -> a, b, d, W*b (fp32), the first N columns of the extended dgrad weights and the bias W d
 * (simclr_bn_fold_coeffs: a, b, d alone);  [GEMMs h^T dm, h^T h via simclr_conv2d_wgrad; (h^T h) W and (W*b) W^T via simclr_conv2d_fwd];
 * simclr_bn_fold_post -> dW and the last K columns of the extended weights (dW alone with wext = q = NULL);  simclr_conv2d_dgrad_bn_ext -> d(h) with the fused
 * BN-backward reduce of the producer BN, reading dm and h (K-extended reduction) instead of a materialised dh. ---- */
int simclr_bn_fold_coeffs(const float* scale, const float* mean, const float* rstd, const float* c1, const float* c2,
                          float* a, float* b, float* d, int C, simclr_stream_t stream);
int simclr_bn_fold_pre(const void* w, const float* scale, const float* mean, const float* rstd, const float* c1,
                       const float* c2, float* a, float* b, float* d, float* wb, void* wext, float* e, int K, int N,
                       int dtype, simclr_stream_t stream);
int simclr_bn_fold_post(const float* t1, const float* gw, const double* cs, const float* cs32, const float* a, const float* b,
                        const float* d, const float* q, float* dw, void* wext, int K, int N, int accumulate, int dtype,
                        simclr_stream_t stream);
int simclr_conv2d_dgrad_ext(const void* dm, const void* h, const void* w_ext, const float* bias, void* dx, int accumulate,
                            int V, int H, int W, int Cin, int Cout, int dtype, simclr_stream_t stream);  /* plain epilogue */
/* sum(dm * x^) of the folded BatchNorm from t1 = h^T dm (no pass over the conv output): sums [2][N] fp64, sums[0] = sum dm given */
int simclr_bn_fold_s2(const float* t1, const void* w, const float* mean, const float* rstd, double* sums, int K, int N,
                      int dtype, simclr_stream_t stream);
/* h^T h [K*K] followed by colsum(h) [K] for h [M][K] (T), K in {64, 128, 256(bf16)}: the activation is streamed once.
 * fp32 storage: dtype may carry SIMCLR_FMT_TERMS of the forward pass the statistics serve -- exact arithmetic (or no field and an exact
 * process default) = exact fp32 MFMA; any split mode = six bf16-piece terms (fp32-level products), column sums by exact fp32 MFMA */
size_t simclr_conv2d_gram_workspace_bytes(long long M, int K, int dtype);
int simclr_conv2d_gram(const void* h, float* out, void* workspace, long long M, int K, int dtype, simclr_stream_t stream);
/* C [M][N] = A [M][K] B[N][K]^T, fp32 on the matrix cores (the small K x K / K x N products of the folded form);
 * M, N multiples of 16, K of 32 */
int simclr_small_gemm_nt_f32(const float* A, const float* B, float* C, int M, int N, int K, simclr_stream_t stream);
int simclr_conv2d_dgrad_bn_ext(const void* dm, const void* h, const void* w_ext, const float* bias, void* dx,
                               int accumulate, const void* bn_x, const void* bn_mask, const float* bn_scale,
                               const float* bn_shift, const float* bn_mean, const float* bn_rstd, int mask_mode,
                               float* stats, int nslot, int V, int H, int W, int Cin, int Cout, int dtype,
                               simclr_stream_t stream);

/* ---- two-view training augmentation on the device: tf2/data_util.py:443-475 (preprocess_for_train: random-resized-crop
 * with bicubic resize :246-320/:362-377, random flip :463, colour jitter in random order :54-173/:380-389, random grayscale
 * :48-52, clip :473-474) for every image and both views of tf2/data.py:52-62.  The random draws come from the caller as
 * params [b][views][16] = {crop_y, crop_x, crop_h, crop_w, flip, jitter_on, perm[4], brightness, contrast, saturation,
 * hue_delta, gray_on, 0}; src [b,Hs,Ws,3] float32 in [0,1] (src_dtype 0) or uint8 (src_dtype 2); out [b,H,W,3*views]
 * float32 in [0,1], the layout Model.__call__ (tf2/model.py:241-259) consumes. ---- */
size_t simclr_augment_workspace_bytes(int b, int views, int H, int W);
int simclr_augment_views(const void* src, int src_dtype, const float* params, void* workspace, float* out, int b,
                         int views, int Hs, int Ws, int H, int W, simclr_stream_t stream);
/* The same pipeline from PACKED variable-size records (the on-disk array format of simclr_amd/data.py): `packed` holds
 * packed_bytes bytes of uint8 RGB images, HWC, tightly packed, back to back; table is a DEVICE array [b][3] = {byte offset,
 * height, width} of image i, read at packed + offset with row pitch 3 * width.  params, workspace
 * (simclr_augment_workspace_bytes) and out as above; out is bitwise what simclr_augment_views writes for the same pixels and
 * draws.  A record that does not lie inside packed_bytes yields zeros and a crop box is clamped into its image: no table or
 * parameter content causes a read outside the buffer. */
int simclr_augment_views_ragged(const unsigned char* packed, long long packed_bytes, const long long* table,
                                const float* params, void* workspace, float* out, int b, int views, int H, int W,
                                simclr_stream_t stream);

/* ---- collective C without a collective library: tf2/resnet.py:50-60 (SyncBatchNormalization moment all-reduce) -------
 * One-shot exchange over peer-mapped memory (csrc/comm.hip): every rank owns a mailbox all peers map through hipIpc;
 * an exchange is ONE single-workgroup launch per rank that writes its block into every peer's mailbox, publishes a
 * sequence flag, waits (bounded) for the R flags of its own mailbox and adds the R blocks in rank order (bit-identical
 * on every replica).  The 64-byte handles travel between processes by the caller's means (simclr_amd/comm.py:
 * torch.distributed.all_gather_object).  RCCL remains the fallback (FLAGS / SIMCLR_PEER_STATS) and carries A and B. */
size_t simclr_comm_mailbox_bytes(int world, int max_doubles);
/* allocates (library-owned, uncached where available) + zeroes the mailbox; ipc_handle_64: 64 bytes out; 3 = no hipIpc */
int simclr_comm_create(int world, int max_doubles, void** mailbox, void* ipc_handle_64);
int simclr_comm_open(const void* ipc_handle_64, void** mapped);
int simclr_comm_close(void* mapped);
/* Wall-clock bound (seconds) of the arrival wait of the exchanges launched after this call; <= 0 restores the default (600 s or
 * SIMCLR_PEER_STATS_TIMEOUT_S).  Process-wide; used for the short-bounded set-up self-test. */
int simclr_comm_set_timeout(double seconds);
int simclr_comm_destroy(void* mailbox);
/* out[i] = sum_r in_r[i] (rank order), count <= max_doubles fp64 values; peers: HOST array of `world` mapped mailboxes
 * (peers[rank] = own); seq = 1, 2, ... identical on all ranks per exchange; status (nullable device int, zeroed once by the
 * caller) = STICKY count of peer arrivals that timed out (never cleared by the library); an exchange that timed out returns NaN
 * in `out`.  Refuses a capturing stream (seq is a kernel argument: a hipGraph replay would carry a stale sequence number). */
int simclr_comm_stats_allreduce(const double* in, double* out, int count, void* const* peers, int rank, int world,
                                int max_doubles, unsigned seq, int* status, simclr_stream_t stream);

/* ---- BYOL on a momentum target network (csrc/byol.hip): Grill et al. 2020, Bootstrap Your Own Latent ----
 * Exponential moving average of every target tensor towards its online tensor in ONE launch, on the descriptor / chunk tables of
 * simclr_lars_multi_tensor: table = device int64 [3 * num_tensors], row 0 = target pointers, row 1 = online pointers, row 2 = element
 * counts (fp32 tensors); chunks[2c] = tensor id, chunks[2c + 1] = element offset, a multiple of simclr_lars_chunk_elems().
 * t = t + one_minus_tau * (o - t): subtract, multiply and add are rounded separately (no fma), so float32 numpy restates it bit for
 * bit.  16-byte accesses where both pointers of a chunk are 16-byte aligned, scalar ones otherwise; any element count.
 * Refused: empty / null tables, one_minus_tau outside [0, 1]. */
int simclr_ema_multi_tensor(const long long* table, int num_tensors, const long long* chunks, int num_chunks, float one_minus_tau,
                            simclr_stream_t stream);
/* q [2b, D] = the online predictor's output, t [2b, D] = the target network's projection, fp32, 16-byte aligned; row r of q pairs with
 * row p = (r + b) mod 2b of t.  With xhat = x / sqrt(max(sum x^2, 1e-12)) (tf.math.l2_normalize) and l_r = sum_j (qhat_rj - that_pj)^2
 * (the difference is summed in double; 2 - 2 cos is never formed):
 *   out[0] = (1 / b) sum_r l_r (the sum of the two per-view means, the convention of NT-Xent here), out[1] = mean_r qhat_r . that_p.
 * Rows are summed in double in a fixed order: two calls are bitwise equal.  row_stats: device double [2b, 4], kept for simclr_byol_bwd;
 * row_out: device double [2b, 2] scratch.  Refused (nothing launched): null / misaligned pointers, b < 1, D not a multiple of 64 in
 * [64, 8192]. */
int simclr_byol_fwd(const float* q, const float* t, int b, int D, float* out, double* row_stats, double* row_out,
                    simclr_stream_t stream);
/* dq [2b, D] fp32 = (grad_scale / b) * d(sum_r l_r) / dq, from the row_stats of simclr_byol_fwd on the same q, t.  A row with
 * sum q^2 < 1e-12 has the constant norm 1e-6 (the gradient of tf.maximum goes to the epsilon): dq_r = (grad_scale / b) * 2e6 *
 * (qhat_r - that_p).  t gets no gradient.  Refusals as simclr_byol_fwd. */
int simclr_byol_bwd(const float* q, const float* t, int b, int D, const double* row_stats, float grad_scale, float* dq,
                    simclr_stream_t stream);

/* ---- MoCo v2 on a queue of momentum keys (csrc/moco.hip): He et al. 2020, Momentum Contrast; Chen et al. 2020, Improved Baselines ----
 * q [two_n, D] = the l2-normalised online projections, [view-a rows; view-b rows]; t [two_n, D] = the l2-normalised momentum keys of
 * the same rows; queue [K, D] = keys of earlier steps; all fp32, 16-byte aligned, D in {64, 128, 256}.  The pairing is formed inside:
 * row r's positive key is t_p, p = (r + two_n / 2) mod two_n (BYOL's pairing; pass t as the target network returned it).  The
 * negatives of a row are the K queue rows and nothing else.  With n = two_n / 2:
 *   s_r+ = q_r . t_p / T,  s_rj = q_r . queue_j / T,  l_r = logsumexp([s_r+, s_r0 .. s_r,K-1]) - s_r+
 *   out[0] = (1 / n) sum_r l_r (the sum of the two per-view means, the convention of NT-Xent here),
 *   out[1] = share of the rows with q_r . t_p >= max_j q_r . queue_j (equality is a hit).
 * Exact-fp32 MFMA sweep over 64-row queue tiles, online log-sum-exp on the rounded logit, key splits merged in a fixed order, the
 * [two_n, K] matrix never written, no atomics: two calls are bitwise equal.  The negatives' sum stays apart from the positive term
 * until the row finalize, which forms l_r in double (log1p of the negatives' sum when the positive is the maximum): logsumexp - s+ is
 * never formed in fp32.  row_stats: device float [two_n, 2] = {logsumexp over the K + 1 logits in the base-2 domain, 1 - P_r+ formed as
 * the negatives' share of the softmax sum}, kept for simclr_moco_bwd.  workspace: simclr_moco_workspace_bytes(two_n, K, D) bytes, shared
 * by both calls (0 for a refused shape).  simclr_moco_key_splits: the number of key splits of the forward sweep (0 for a refused shape).
 * Refused (1 returned, nothing launched): null / misaligned pointers, another D, two_n < 2 or odd, K < 1, temperature <= 0 or NaN. */
size_t simclr_moco_workspace_bytes(int two_n, int K, int D);
int simclr_moco_key_splits(int two_n, int K);
int simclr_moco_fwd(const float* q, const float* t, const float* queue, int two_n, int K, int D, float temperature, float* out,
                    float* row_stats, void* workspace, simclr_stream_t stream);
/* dq [two_n, D] fp32 = grad_scale * d out[0] / dq = (grad_scale / (n T)) (sum_j P_rj queue_j - (1 - P_r+) t_p), P the softmax over the
 * K + 1 logits, from the row_stats of simclr_moco_fwd on the same arguments.  One query-side sweep that recomputes S; t and the queue
 * get no gradient.  Refusals as simclr_moco_fwd. */
int simclr_moco_bwd(const float* q, const float* t, const float* queue, int two_n, int K, int D, float temperature,
                    const float* row_stats, float grad_scale, float* dq, void* workspace, simclr_stream_t stream);

/* ---- DINO self-distillation (csrc/dino.hip): Caron et al. 2021, Emerging Properties in Self-Supervised Vision Transformers ----
 * q [two_n, D] = the l2-normalised online projections, [view-a rows; view-b rows]; k [two_n, D] = the l2-normalised target projections
 * of the same rows; ws / wt [K, D] = the row-normalised prototypes of the online / the target network; center [K]; all fp32, the
 * matrices 16-byte aligned, D in {64, 128, 256}, K >= 2 (a ragged last tile is fine), two_n even.  The pairing is formed inside:
 * p(r) = (r + two_n / 2) mod two_n.  With s_rj = q_r . ws_j / Ts, t_rj = (k_r . wt_j - center_j) / Tt, Ps / Pt their row softmaxes:
 *   l_r = logsumexp_j(s_r) - sum_j Pt[p(r), j] s_rj,   out[0] = (1 / two_n) sum_r l_r (the mean over the two cross-view terms),
 *   out[1] = (1 / two_n) sum_r H(Pt[r]), the mean teacher entropy in nats,
 *   u [two_n, D] = sum_j Pt[r, j] ws_j (the positive term of row r is q_r . u_p(r) / Ts; kept for simclr_dino_bwd_q).
 * Two-pass form: a statistics sweep of both sides (one launch), the merge of their key splits, the teacher expectation sweep (wt and
 * ws tiles side by side in LDS), the row finalize in double, a one-workgroup reduce.  Exact-fp32 MFMA sweeps over 64-row tiles, online
 * statistics on the rounded logit, splits merged in a fixed order, no [two_n, K] matrix ever written, no atomics: two calls are
 * bitwise equal.  The statistics keep the non-maximum mass apart (log1p) and the entropy is log(sum) - sum e^(t-m)(t-m) / sum with
 * every term <= 0.  row_stats: device float [two_n, 2] = {logsumexp of s_r, logsumexp of t_r} in the base-2 domain, kept for the two
 * backward calls.  workspace: simclr_dino_workspace_bytes(two_n, K, D) bytes, shared by the three calls (0 for a refused shape).
 * simclr_dino_key_splits: key splits of the statistics sweeps; simclr_dino_row_splits: row splits of the key-side sweep (0 for a
 * refused shape).  Refused (1 returned, nothing launched): null / misaligned pointers, another D, two_n < 2 or odd, K < 2, a
 * temperature <= 0 or NaN. */
size_t simclr_dino_workspace_bytes(int two_n, int K, int D);
int simclr_dino_key_splits(int two_n, int K);
int simclr_dino_row_splits(int two_n, int K);
int simclr_dino_fwd(const float* q, const float* k, const float* ws, const float* wt, const float* center, int two_n, int K, int D,
                    float student_temp, float teacher_temp, float* out, float* row_stats, float* u, void* workspace,
                    simclr_stream_t stream);
/* dq [two_n, D] = grad_scale * d out[0] / dq = (grad_scale / (two_n Ts)) (sum_j Ps[r, j] ws_j - u_p(r)) from the row_stats and u of
 * simclr_dino_fwd on the same arguments: one query-side sweep that recomputes s. */
int simclr_dino_bwd_q(const float* q, const float* ws, const float* u, int two_n, int K, int D, float student_temp,
                      const float* row_stats, float grad_scale, float* dq, void* workspace, simclr_stream_t stream);
/* dws [K, D] = grad_scale * d out[0] / dws = (grad_scale / (two_n Ts)) sum_r (Ps[r, j] - Pt[p(r), j]) q_r: the key-side sweep.  A
 * workgroup owns 64 prototypes and streams 64-row tiles of q and of the paired rows k_p(r); it recomputes BOTH logits, so center and
 * wt must still be the ones simclr_dino_fwd read.  Row splits are merged in a fixed order.  k, wt and center get no gradient. */
int simclr_dino_bwd_w(const float* q, const float* k, const float* ws, const float* wt, const float* center, int two_n, int K, int D,
                      float student_temp, float teacher_temp, const float* row_stats, float grad_scale, float* dws, void* workspace,
                      simclr_stream_t stream);
/* kbar [D] (device double) = scale * sum_r k[r][d] over the rows of k [rows, D] fp32, accumulated in double in a fixed order: with
 * scale = 1 / (global rows) and a SUM all-reduce over the replicas it is the global mean of the normalised target projections, the
 * one vector the DINO centre needs.  Refused: null / misaligned pointers, another D, rows < 1. */
int simclr_dino_key_mean(const float* k, int rows, int D, double scale, double* kbar, simclr_stream_t stream);
/* center_j <- center_j + (1 - momentum) (wt_j . kbar - center_j), kbar = device double [D], the mean of the l2-normalised target
 * projections over all rows of the global batch.  The dot product accumulates in double and is rounded to fp32 once; the blend's three
 * fp32 roundings are separate, (1 - momentum) is formed in double and cast once.  Refused: null / misaligned pointers, another D,
 * K < 2, a momentum outside [0, 1] or NaN. */
int simclr_dino_center(const float* wt, const double* kbar, float* center, int K, int D, float momentum, simclr_stream_t stream);

/* ---- SwAV (csrc/swav.hip): Caron et al. 2020, Unsupervised Learning of Visual Features by Contrasting Cluster Assignments ----
 * q [two_n, D] = the l2-normalised online projections, [view-a rows; view-b rows]; w [K, D] = the row-normalised prototypes; z_all
 * [rows_all, D] = the gathered global batch, view-major (rows < rows_all / 2 are view a); alpha [2, K] = the per-view column potentials
 * in nats; all fp32, the matrices 16-byte aligned, D in {64, 128, 256}, K in [2, 1048576] (a ragged last tile is fine), row counts even.
 * simclr_swav_sinkhorn: the Sinkhorn-Knopp assignment of the official distributed_sinkhorn, per view on the global batch, as scaling
 * potentials.  With L_gj = z_g . w_j / epsilon, beta = 0 at the start, N = rows_all / 2 and it = 1 .. iters:
 *   alpha[v][j] = -ln K - logsumexp_{g in view v}(L_gj + beta_g);   for it < iters: beta_g = -ln N - logsumexp_j(L_gj + alpha[v(g)][j]).
 * The code of row g is softmax_j(L_gj + alpha[v(g)][j]); no [rows_all, K] matrix is written.  The column sweep fixes 64 prototypes and
 * streams 64-row tiles (a tile may straddle the view boundary: every element counts for its own row's view), the row sweep fixes 64
 * rows and streams prototype tiles; splits are merged in a fixed order and finalized in double; no atomics: two calls are bitwise equal.
 * iters in [1, 16].  workspace: simclr_swav_workspace_bytes(rows, K, D) bytes serve the Sinkhorn on `rows` rows as well as the three
 * loss calls on `rows` rows (0 for a refused shape).  simclr_swav_key_splits / simclr_swav_row_splits: key splits of the query-side
 * statistics sweeps / row splits of the key-side sweeps (the Sinkhorn's column sweep and simclr_swav_bwd_w) at that shape.
 * simclr_swav_fwd: with p(r) = (r + two_n / 2) mod two_n, v(r) = the view of row r, s_rj = q_r . w_j / temperature,
 * t_rj = q_r . w_j / epsilon + alpha[v(r)][j], Ps / Pt their row softmaxes (Pt is the code):
 *   l_r = logsumexp_j(s_r) - sum_j Pt[p(r), j] s_rj,   out[0] = (1 / two_n) sum_r l_r,   out[1] = (1 / two_n) sum_r H(Pt[r]) in nats,
 *   u [two_n, D] = sum_j Pt[r, j] w_j (kept for simclr_swav_bwd_q),  row_stats [two_n, 2] = {logsumexp of s_r, of t_r}, base 2.
 * One statistics sweep pushes both statistics from one dot product; then the code expectation sweep, the row finalize in double and a
 * one-workgroup reduce.  The non-maximum mass stays apart (log1p) and the entropy is formed from two non-negative terms.
 * Refused (1 returned, nothing launched): null / misaligned pointers, another D, a row count < 2 or odd, K outside [2, 1048576], a
 * temperature or epsilon <= 0 or NaN, iters outside [1, 16]. */
size_t simclr_swav_workspace_bytes(int rows, int K, int D);
int simclr_swav_key_splits(int rows, int K);
int simclr_swav_row_splits(int rows, int K);
int simclr_swav_sinkhorn(const float* z_all, const float* w, int rows_all, int K, int D, float epsilon, int iters, float* alpha,
                         void* workspace, simclr_stream_t stream);
int simclr_swav_fwd(const float* q, const float* w, const float* alpha, int two_n, int K, int D, float temperature, float epsilon,
                    float* out, float* row_stats, float* u, void* workspace, simclr_stream_t stream);
/* dq [two_n, D] = grad_scale * d out[0] / dq = (grad_scale / (two_n T)) (sum_j Ps[r, j] w_j - u_p(r)) from the row_stats and u of
 * simclr_swav_fwd on the same arguments.  The codes are stop-gradient: alpha gets none. */
int simclr_swav_bwd_q(const float* q, const float* w, const float* u, int two_n, int K, int D, float temperature,
                      const float* row_stats, float grad_scale, float* dq, void* workspace, simclr_stream_t stream);
/* dw [K, D] = grad_scale * d out[0] / dw = (grad_scale / (two_n T)) sum_r (Ps[r, j] - Pt[p(r), j]) q_r: the key-side sweep.  A
 * workgroup owns 64 prototypes and streams 64-row tiles of q and of the paired rows q_p(r); alpha is read for the view of the PAIRED
 * row.  Row splits are merged in a fixed order. */
int simclr_swav_bwd_w(const float* q, const float* w, const float* alpha, int two_n, int K, int D, float temperature, float epsilon,
                      const float* row_stats, float grad_scale, float* dw, void* workspace, simclr_stream_t stream);

/* ---- SwAV multi-crop (csrc/swav_multicrop.hip): Caron et al. 2020 section 4, the official loss with crops_for_assign = [0, 1] ----
 * x [L b, D] = the l2-normalised LOCAL rows, view-major (row v b + i = local view v of image i); z [2b, D], u [2b, D], alpha [2, K] and
 * global_row_stats [2b, 2] = the global rows handed to simclr_swav_fwd, and what it read / returned for them; w [K, D] as there.  All
 * fp32, the matrices 16-byte aligned, D in {64, 128, 256}, K in [2, 1048576], L in [1, 8], b >= 1 (L b may be odd and ragged).
 * With s_rj = x_r . w_j / temperature, Ps its row softmax, i = r mod b and c = 1 / (2 (L + 1) b):
 *   simclr_swav_local_fwd:   out[0] = c sum_r (2 logsumexp_j(s_r) - x_r . (u_i + u_{b+i}) / temperature),
 *                            row_stats [L b] = logsumexp_j(s_r), base 2.  A statistics sweep, a row finalize in double, a reduce.
 *   simclr_swav_local_bwd_x: dx [L b, D] = grad_scale (c / temperature) (2 sum_j Ps[r, j] w_j - u_i - u_{b+i}).
 *   simclr_swav_local_bwd_w: dw [K, D] = grad_scale (c / temperature) (sum_r 2 Ps[r, j] x_r - sum_{g < 2b} Pt[g, j] m_{g mod b}),
 *                            m_i = sum_v x_{v b + i} (views added in the order 0, 1, ...), Pt[g] = the code of global row g
 *                            recomputed from z, alpha of the row's own view and the lse_t of global_row_stats: two key-side sweeps
 *                            (64 prototypes per workgroup), the second streaming z for the logits and m as the multiplier tile.
 * The codes are stop-gradient and the local rows take no part in the Sinkhorn.  Splits are merged in a fixed order, no atomics: two
 * calls are bitwise equal.  workspace: simclr_swav_local_workspace_bytes(b, L, K, D) bytes serve the three calls (0 for a refused
 * shape).  simclr_swav_local_key_splits: key splits of the statistics sweep; _row_splits / _code_row_splits: row splits of the student
 * / code key-side sweep.  Refused (1 returned, nothing launched): null / misaligned pointers, another D, K outside [2, 1048576], L
 * outside [1, 8], b < 1, a temperature or epsilon <= 0 or NaN. */
size_t simclr_swav_local_workspace_bytes(int b, int L, int K, int D);
int simclr_swav_local_key_splits(int b, int L, int K);
int simclr_swav_local_row_splits(int b, int L, int K);
int simclr_swav_local_code_row_splits(int b, int L, int K);
int simclr_swav_local_fwd(const float* x, const float* w, const float* u, int b, int L, int K, int D, float temperature, float* out,
                          float* row_stats, void* workspace, simclr_stream_t stream);
int simclr_swav_local_bwd_x(const float* x, const float* w, const float* u, int b, int L, int K, int D, float temperature,
                            const float* row_stats, float grad_scale, float* dx, void* workspace, simclr_stream_t stream);
int simclr_swav_local_bwd_w(const float* x, const float* z, const float* w, const float* alpha, int b, int L, int K, int D,
                            float temperature, float epsilon, const float* row_stats, const float* global_row_stats, float grad_scale,
                            float* dw, void* workspace, simclr_stream_t stream);

/* ---- DINO multi-crop (csrc/dino_multicrop.hip): Caron et al. 2021, the official loss with ncrops = 2 + L ----
 * The L local views of the b images against the teacher rows of BOTH global views.  x [L b, D] = the l2-normalised local rows,
 * view-major; k [2b, D], ws / wt [K, D], center [K], u [2b, D] and global_row_stats [2b, 2] = what simclr_dino_fwd read / returned
 * for the two global views of the same images.  A logit is linear in the prototype, sum_j Pt[g, j] s_rj = x_r . u_g / Ts, so the
 * value and the query-side backward of the local term are simclr_swav_local_fwd / simclr_swav_local_bwd_x on (x, ws, u, L, Ts) as
 * they stand; their row_stats [L b] (logsumexp_j of x_r . ws_j / Ts, base 2) is local_row_stats here.  The key-side backward is
 * this family: with c = 1 / (2 (L + 1) b), Ps the student softmax of the local rows and Pt[g] = softmax_j((k_g . wt_j - center_j)
 * / Tt) the teacher row of global row g ITSELF (normalised by global_row_stats[2 g + 1], not by the paired row's entry that
 * simclr_dino_bwd_w reads),
 *   simclr_dino_local_bwd_w: dws [K, D] = grad_scale (c / Ts) (2 sum_r Ps[r, j] x_r - sum_{g < 2b} Pt[g, j] m_{g mod b}),
 *                            m_i = sum_v x_{v b + i} (views added in the order 0, 1, ...): the build of m, two key-side sweeps
 *                            (64 prototypes per workgroup; the second holds wt and center_j and streams k beside the wrapped m
 *                            tile), a combine.  center, wt and k must still be the ones simclr_dino_fwd read.
 * All fp32, the matrices 16-byte aligned, D in {64, 128, 256}, K in [2, 1048576], L in [1, 8], b >= 1.  Row splits are merged in a
 * fixed order, no atomics: two calls are bitwise equal.  workspace: simclr_dino_local_workspace_bytes(b, L, K, D) bytes, this
 * family's own (0 for a refused shape).  simclr_dino_local_row_splits / _teacher_row_splits: row splits of the student sweep over the
 * L b local rows / of the teacher sweep over the 2b global rows.  Refused (1 returned, nothing launched): null / misaligned
 * pointers, another D, K outside [2, 1048576], L outside [1, 8], b < 1, a temperature <= 0 or NaN. */
size_t simclr_dino_local_workspace_bytes(int b, int L, int K, int D);
int simclr_dino_local_row_splits(int b, int L, int K);
int simclr_dino_local_teacher_row_splits(int b, int L, int K);
int simclr_dino_local_bwd_w(const float* x, const float* k, const float* ws, const float* wt, const float* center, int b, int L, int K,
                            int D, float student_temp, float teacher_temp, const float* local_row_stats,
                            const float* global_row_stats, float grad_scale, float* dws, void* workspace, simclr_stream_t stream);

/* ---- DropBlock (csrc/dropblock.hip): tf2/resnet.py:81-157, the four sites of a bottleneck block (:424-487) ----
 * A site's block pattern is a BIT tensor packed along C: unsigned char [V,H,W,C/8], bit j of a byte = channel 8*byte + j (C % 8 == 0,
 * so it is also the linear bit string of the NHWC elements), with its `count`: device uint64 [2] = {ones, size} of the pattern in the
 * reference's units -- elements, or (image, channel) planes when min(dropblock_size, W) == W, where the pattern is [V,1,1,C] and is
 * written broadcast over the plane.  percent_ones = float(count[0]) / float(count[1]) is formed on the device by the consumers. */
/* tf2/resnet.py:111-153.  keep_thresh = fp32(1 - gamma) (gamma = seed_drop_rate, :113-114, computed by the caller in double): a valid
 * block centre keeps its seed bit iff fp32(keep_thresh + u) >= 1.  noise (nullable): the uniform [0,1) fp32 tensor [V,H,W,C] to read u
 * from (tests); NULL: u of element i (linear NHWC index) = (32 bits >> 8) * 2^-24 with the 32 bits = the low (i even) / high (i odd)
 * half of splitmix64's output function applied to key + (i/2 + 1) * 0x9E3779B97F4A7C15 -- no state, nothing read.  The count is an
 * integer sum: bitwise repeatable.  Refused: H != W, C % 8 != 0, H = W > 178 (one workgroup stages an (image, 8- or 32-channel)
 * plane twice in LDS, 2 x 32000 bytes: every map of the network up to image_size 448, 112 x 112, fits), null bits / count. */
int simclr_dropblock_mask(const float* noise, long long key, int V, int H, int W, int C, int dropblock_size, float keep_thresh,
                          unsigned char* bits, void* count, simclr_stream_t stream);
/* tf2/resnet.py:155-156: y = x / percent_ones * pattern (true division, then the multiply; fp32 arithmetic on fp32 or bf16 storage),
 * x, y [rows, C].  Applied to dy it is the gradient (pattern and percent_ones are constants to tape.gradient).  percent_ones == 0
 * gives NaN / inf as in the reference. */
int simclr_dropblock_apply(const void* x, const unsigned char* bits, const void* count, void* y, long long rows, int C, int dtype,
                           simclr_stream_t stream);
/* tf2/resnet.py:482-487 with the DropBlock sites of :468-472 (a = bn3's output) and :424-427 (b = the shortcut) in front of the add:
 * out = relu(a / pa * ma + b / pb * mb), relu(o) = o < 0 ? 0 : o (NaN passes).  relu_bits (nullable): the ReLU mask in the format
 * simclr_bn_apply(relu_bits) writes (one byte per 16-byte chunk of out). */
int simclr_dropblock_tail_fwd(const void* a, const unsigned char* bits_a, const void* count_a, const void* b, const unsigned char* bits_b,
                              const void* count_b, void* out, unsigned char* relu_bits, long long rows, int C, int dtype,
                              simclr_stream_t stream);
/* tape.gradient of the above: g = relu bit ? dout : 0;  da = g / pa * ma;  db = g / pb * mb, both written in one pass. */
int simclr_dropblock_tail_bwd(const void* dout, const unsigned char* relu_bits, const unsigned char* bits_a, const void* count_a,
                              const unsigned char* bits_b, const void* count_b, void* da, void* db, long long rows, int C, int dtype,
                              simclr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIMCLR_HIP_H_ */
