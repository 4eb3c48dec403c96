/*
 * mcgra.h - C ABI of the MI355X-native MC-GRA adjacency-optimisation hot path.
 *
 * Drop-in boundary for the inner loop of MC-GRA/topology_attack.py
 * (PGDAttack.attack, lines 161-298) and the functions it calls.  The reference
 * is Python/PyTorch, so the binding a maintainer adds is a ctypes stub
 * (INTEGRATION.md); every entry point takes plain device pointers, sizes and a
 * hipStream_t passed as void*.  No torch types cross this boundary.
 *
 * Conventions
 *   - all matrices are row-major fp32 in device (HBM) memory unless stated;
 *   - "ld" arguments are leading dimensions in elements;
 *   - every function returns 0 on success, a negative MCGRA_E* code otherwise;
 *     mcgra_last_error() returns a static description of the last failure on
 *     the calling thread;
 *   - functions enqueue on `stream` and do not synchronise unless documented;
 *   - threads: standalone ops may be called from any thread.  An attack engine
 *     (mcgra_attack_t) is driven by one thread at a time, and the engines of one
 *     device in a process share their side streams (the N x N x N product, the
 *     small-operand terms and the decode run beside the caller's stream): steps of
 *     different engines of one device, issued from different host threads or on
 *     different streams, are correct but serialise on those side streams.
 *
 * Reference citations are relative to /root/reference/MC-GRA.
 */
#ifndef MCGRA_H
#define MCGRA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCGRA_OK 0
#define MCGRA_EINVAL (-1)  /* bad argument */
#define MCGRA_EHIP (-2)    /* HIP runtime error */
#define MCGRA_ENOSUP (-3)  /* valid in the reference, not implemented on this path yet */
#define MCGRA_ENOMEM (-4)

#define MCGRA_MAX_LAYERS 8

/* args.measure (main.py:109, topology_attack.py:190-208) */
enum mcgra_measure {
  MCGRA_MEASURE_HSIC = 0, /* CudaCKA.linear_HSIC utils.py:1085 */
  MCGRA_MEASURE_MSE = 1,  /* torch.nn.MSELoss  topology_attack.py:194 */
  MCGRA_MEASURE_KL = 2,   /* PGDAttack.calc_kl topology_attack.py:483 */
  MCGRA_MEASURE_CKA = 3,  /* CudaCKA.linear_CKA utils.py:1091 */
  MCGRA_MEASURE_DP = 4,   /* PGDAttack.dot_product topology_attack.py:480 */
  MCGRA_MEASURE_KDE = 5   /* utils.MutualInformation(sigma=0.4, num_bins=<operand width>, normalize=True) utils.py:980,
                             topology_attack.py:199-201, :244-246, :261-263.  Entry (i, j) of an operand meets bin j only
                             (utils.py:995) and exp(-((v - b_j) / 0.32)^2 / 2) is exactly 0 in float32 once b_j - v > 4.6, so the
                             N x N terms live on the first floor(max(feature_adj) + 4.7) + 1 columns (8 for the operands the
                             reference builds, all <= 1): mcgra_attack_set_graph measures max |feature_adj|, widens the
                             column count up to 32 and returns MCGRA_ENOSUP beyond (values > 27.3) */
};

const char* mcgra_version(void);
const char* mcgra_last_error(void);
/* number of HIP devices visible, or a negative error */
int mcgra_device_count(void);

/* ------------------------------------------------------------------ GEMM --
 * C[m x n] = alpha * op(A)[m x k] * op(B)[k x n] + beta * C, fp32 MFMA
 * (v_mfma_f32_32x32x2_f32), row-major.  ta/tb: 0 = as stored, 1 = transposed.
 * This is the torch.mm / torch.matmul the reference calls at models/gcn.py:41-42,
 * utils.py:1086-1087 and topology_attack.py:416. */
int mcgra_sgemm(void* stream, int ta, int tb, int m, int n, int k, float alpha,
                const float* A, int lda, const float* B, int ldb, float beta,
                float* C, int ldc);

/* Symmetric variants used for the Gram matrices of linear_HSIC (utils.py:1086-1089).
 * "Lower tile storage": element (i,j) of an n x n symmetric matrix is valid iff
 * j < (i/128 + 1) * 128, i.e. the 128 x 128 tiles on or below the diagonal.
 *   mcgra_ssyrk_lower: C = alpha A A^T + beta C, A [n x k]; writes lower tile storage only.
 *   mcgra_ssymm_lower: C[n x m] = alpha S B + beta C, S [n x n] read from lower tile storage. */
int mcgra_ssyrk_lower(void* stream, int n, int k, float alpha, const float* A, int lda,
                      float beta, float* C, int ldc);
int mcgra_ssymm_lower(void* stream, int n, int m, float alpha, const float* S, int lds,
                      const float* B, int ldb, float beta, float* C, int ldc);

/* C[n x n] = S (X - rowsub 1^T)^T for a symmetric S given in lower tile storage (or in full), i.e. C[m][j] = sum_k
 * S[m][k] (X[j][k] - rowsub[j]) (rowsub may be NULL), evaluated as the 3-plane bf16 split of DESIGN.md section 3:
 * operands as x0 + x1 + x2 in bf16, the six plane products with i + j <= 2 in the fp32 accumulator of the bf16 MFMA
 * (fp32-level error).  With X = adj_norm (symmetric) and rowsub its column means this is (H Kf H) Xc, the N x N x N
 * product torch.mm performs inside CudaCKA.linear_HSIC's backward (utils.py:1085-1089).  Synchronous; packs both
 * operands itself (the engine keeps S packed across steps). */
int mcgra_ssymm_split_bf16(void* stream, int n, const float* S, int lds, const float* X, int ldx, const float* rowsub,
                           float* C, int ldc);
/* The same product as the 2-plane fp16 split (the engine's default for n >= 1024): each operand scaled by an exact
 * power of two that puts its largest magnitude in [2^14, 2^15), written as x0 + x1 in fp16, the three products x0 y0 +
 * x0 y1 + x1 y0 in the fp32 accumulator of the fp16 MFMA, scales undone exactly in the epilogue.  Half the
 * matrix-core work of the 3-plane form; fp32-level error for elements within 2^18 of their operand's maximum. */
int mcgra_ssymm_split_f16(void* stream, int n, const float* S, int lds, const float* X, int ldx, const float* rowsub,
                          float* C, int ldc);
/* Y[n x nc] = M[n x n] V[n x nc] (nc <= 48; ldm >= n a multiple of 4, M 16-byte aligned) on the kernel the fused step's
 * forward runs beside the N x N x N product: both operands split exactly into three bf16 planes, the six plane products
 * with i + j <= 2 in the fp32 accumulator of the bf16 MFMA (fp32-level error, fp32 exponent range).  Synchronous. */
int mcgra_sgemm_skinny_x3(void* stream, int n, const float* M, int ldm, const float* V, int ldv, int nc, float* Y, int ldy);

/* ------------------------------------------------------- standalone ops --
 * Each mirrors one reference function on its own inputs; the attack engine
 * below runs fused forms of the same kernels. */

/* PGDAttack.get_modified_adj (topology_attack.py:365-379):
 * out = (1 - I) * sym(tril^-1(adj_changes)) + ori_adj; ori_adj may be NULL (zeros).
 * adj_changes has n(n-1)/2 entries in torch.tril_indices(n, n, -1) order. */
int mcgra_get_modified_adj(void* stream, int n, const float* adj_changes,
                           const float* ori_adj, float* out);

/* inverse data movement: out[p(i,j)] = M[i][j], i > j */
int mcgra_pack_tril(void* stream, int n, const float* M, int ld, float* out);

/* utils.normalize_adj_tensor dense branch (utils.py:211-230):
 * out = D^-1/2 (adj + I) D^-1/2, D = rowsum(adj + I), inf -> 0. */
int mcgra_normalize_adj(void* stream, int n, const float* adj, float* out);

/* Info_entropy (topology_attack.py:44-47): *out (device scalar) =
 * -mean(q log2 q), q = clamp(p, 1e-4, 1 - 1e-4) over an n x n matrix. */
int mcgra_info_entropy(void* stream, int n, const float* prob, float* out);

/* PGDAttack.dot_product_decode (topology_attack.py:414-419):
 * out[p(i,j)] = relu(<Z_i, Z_j> / (max(|Z_i|,1e-12) max(|Z_j|,1e-12))), i > j. */
int mcgra_dot_product_decode(void* stream, int n, int d, const float* Z, float* out);

/* PGDAttack.dot_product_decode2 (topology_attack.py:421-467): out [n x n] for
 * Z [n x d].  mode selects the reference's dataset branch:
 *   0 cora / AIDS      sigmoid(relu(Z Z^T - I))                                (:422-425)
 *   1 citeseer         the same after F.normalize(Z, p=2, dim=1)               (:427-431)
 *   2 brazil           relu(Z Z^T - I)                                         (:433-435)
 *   3 polblogs / usair default: relu(F.normalize(Z Z^T, p=2, dim=1) - I)       (:438-442, :459-462)
 *   4 / 5 / 6 usair    relu(Zn Zn^T - I), Zn = F.normalize(Z, p = 2 / 3 / 5)   (:444-458)
 * (mc-gra_amd/topology_attack.py:_decode_mode maps args.dataset / useH_A /
 * useY_A / useY to the mode; mcgra_attack_finalize takes the same number.) */
int mcgra_dot_product_decode2(void* stream, int n, int d, const float* Z, int mode, float* out);

/* utils.MutualInformation(sigma=0.4, num_bins=c, normalize=True)(X, Y)[0] (utils.py:980-1049) for X, Y [m x c]: the
 * operand's width is the number of bins (topology_attack.py:199-201, :244-246, :261-263), entry (i, j) meets bin j
 * (utils.py:995).  *out = the value; gX, gY (optional, [m x c]) = d value / dX, d value / dY.  c > 32: square operands
 * (m == c) whose values keep at most 32 bins within reach of a float32 kernel value; MCGRA_ENOSUP otherwise, and
 * MCGRA_EINVAL for such an operand with an infinite entry.  A refusal writes nothing to out, gX or gY. */
int mcgra_mutual_information(void* stream, int m, int c, const float* X, const float* Y, float* out, float* gX, float* gY);

/* CudaCKA.linear_HSIC (utils.py:1085-1089) for X [m x dx], Y [m x dy]:
 * *out = sum(center(X X^T) * center(Y Y^T)).  Evaluated as |Xc^T Yc|_F^2. */
int mcgra_linear_hsic(void* stream, int m, int dx, int dy, const float* X,
                      const float* Y, float* out);

/* hsic.py (Gaussian-kernel HSIC; not called by the attack loop, named by the task's north_star):
 * hsic_regular (hsic.py:117-124) = mean(Kxc * Kyc^T) with K = exp(-distmat / (2 sigma^2)) (:20-38), Kc = K H (:46);
 * hsic_normalized (:127-135) = Pxy / (sqrt(Pxx) sqrt(Pyy)).  X [m x dx], Y [m x dy]; sigma > 0 (for sigma=None, the
 * median heuristic of :5-17, see mcgra_hsic_regular2 below).  *out device scalar; synchronises. */
int mcgra_hsic_regular(void* stream, int m, int dx, int dy, const float* X, const float* Y,
                       float sigma, float* out);
int mcgra_hsic_normalized(void* stream, int m, int dx, int dy, const float* X, const float* Y,
                          float sigma, float* out);

/* The rest of hsic.py.  sigma=None (median heuristic, hsic.py:5-17) is estimated by the host mirror
 * (mc-gra_amd/hsic.py: mcgra_distmat on the device, the median on the host, as the reference does with numpy) and
 * arrives here as explicit per-operand sigmas. */
int mcgra_hsic_regular2(void* stream, int m, int dx, int dy, const float* X, const float* Y, float sigma_x, float sigma_y,
                        int normalized, float* out);               /* hsic_regular / hsic_normalized, one sigma per operand */
/* hsic.py:138-151 (= utils.py:732-743 with sigma 5): sum(Rx o Ry^T), R = Kc (Kc + 1e-5 m I)^-1.  fp64 throughout
 * (kernel matrices from the fp32 inputs, Gauss-Jordan inverses with partial pivoting): the reference's fp32
 * torch.inverse leaves up to 1e-2 of error on these matrices, this path is the exact value to fp32 output rounding. */
int mcgra_hsic_normalized_cca(void* stream, int m, int dx, int dy, const float* X, const float* Y, float sigma_x, float sigma_y,
                              float* out);
int mcgra_distmat(void* stream, int m, int d, const float* X, float* out);                      /* hsic.py:20-27 */
int mcgra_mmd(void* stream, int mx, int my, int d, const float* X, const float* Y, float sx, float sy, float sxy,
              float* out);                                                                     /* hsic.py:68-89 */
int mcgra_mmd_pxpy_pxy(void* stream, int m, int dx, int dy, const float* X, const float* Y, float sx, float sy,
                       float* out);                                                            /* hsic.py:92-114 */

/* torch.nn.MSELoss()(X, Y) over `count` elements, *out device scalar. */
int mcgra_mse(void* stream, int64_t count, const float* X, const float* Y, float* out);

/* main.metric_pool (main.py:66-75): roc_curve + auc of labels[idx][:, idx] (the true adjacency) against
 * scores[idx][:, idx] (the inference adjacency), without gathering the submatrix.  labels, scores: n x n fp32 with
 * leading dimensions ld_labels, ld_scores >= n; idx: n_idx device int64 node ids (repeats allowed: the gathered matrix
 * holds repeated rows and columns), or NULL for all n nodes once.  *out (host memory) = U / (P N), 2U = the sum over
 * positives of 2 #negatives with a lower score + #negatives with an equal score; synchronises `stream`.
 *   - ties are float32 equality (-0.0 == +0.0; subnormals and negative scores are ordinary values);
 *   - exact: P, N and 2U are 64-bit integers, the one rounding is the final division (nearest double), and the result
 *     is the same bits on every call;
 *   - a selected score that is NaN or +-inf, or a selected label other than 0 or 1: MCGRA_EINVAL (sklearn raises
 *     ValueError); an id outside [0, n): MCGRA_EINVAL;
 *   - P == 0 or N == 0: *out = NaN (what roc_curve + auc return);
 *   - n_idx (n when idx is NULL) up to 65 535, the largest for which 2 P N fits 64 bits; MCGRA_ENOSUP beyond.
 * Device scratch: two 4-byte keys per selected entry plus about 3 MB. */
int mcgra_roc_auc(void* stream, int n, const float* labels, int ld_labels, const float* scores, int ld_scores,
                  const int64_t* idx, int64_t n_idx, double* out);

/* The AUC above and the average precision of the same ranking,
 * sklearn.metrics.average_precision_score(labels[idx][:, idx].reshape(-1), scores[idx][:, idx].reshape(-1)), from one
 * classify, one emit and one sort of the selected entries.  auc, ap: host doubles; either may be NULL (not computed), not
 * both (MCGRA_EINVAL).  Arguments, checks, error codes and the n_idx limit as mcgra_roc_auc; *auc is bit for bit what
 * mcgra_roc_auc returns.
 *   AP = (1 / P) sum over selected positives i of TP(s_i) / (TP(s_i) + FP(s_i)),
 *   TP(s) = #selected positives with score >= s, FP(s) = #selected negatives with score >= s
 *   - ties as above (float32 equality, -0.0 == +0.0): all positives of one score share one term;
 *   - TP + FP < 2^33, so each term is one correctly rounded float64 division; the terms are added in a fixed order (no
 *     floating-point atomics; per lane in index order, a fixed tree over lanes, waves and blocks, the grid a function of
 *     P alone), so *ap is the same bits on every call and under any permutation of a repeat-free idx.  With T =
 *     ceil(P / 2^20) terms per lane the relative error is at most (T + 32) 2^-53: 3.7e-15 up to P = 2^20, 4.6e-13 at
 *     the n_idx limit;
 *   - N == 0: *ap = 1.0 exactly (every term is 1; sklearn gives the same), *auc = NaN;
 *   - P == 0: *ap = NaN, a mean over no positives, as *auc is NaN for an absent class.  (sklearn 1.7 returns 0.0 here
 *     and warns "No positive class found"; older versions return NaN.) */
int mcgra_rank_metrics(void* stream, int n, const float* labels, int ld_labels, const float* scores, int ld_scores,
                       const int64_t* idx, int64_t n_idx, double* auc, double* ap);

/* The curves behind those two numbers: what sklearn.metrics.roc_curve(..., drop_intermediate=) and
 * precision_recall_curve(..., drop_intermediate=) return for labels[idx][:, idx].reshape(-1) against
 * scores[idx][:, idx].reshape(-1), as exact integer counts per kept threshold.  Selection, ties, checks, error codes and the
 * n_idx limit as mcgra_roc_auc (repeats allowed; NaN / +-inf scores and labels other than 0 / 1: MCGRA_EINVAL).
 *   - a LEVEL is a distinct selected score; levels are numbered by descending score.  Level l carries tps[l] = #selected
 *     positives with score >= its value, fps[l] = the same for negatives, and its threshold (the score; -0.0 is reported
 *     as +0.0): sklearn's _binary_clf_curve;
 *   - ROC points (roc_tps, roc_fps, roc_thr: device [cap], all three or none): point 0 is (0, 0, +inf), then the levels
 *     roc_curve keeps, in descending-threshold order: all of them when drop_intermediate == 0 or levels <= 2, otherwise the
 *     first, the last and every interior l with fps[l-1] - 2 fps[l] + fps[l+1] != 0 or the same expression in tps != 0.
 *     fpr = roc_fps / N and tpr = roc_tps / P are left to the caller;
 *   - PR points (pr_tps, pr_fps, pr_thr: device [cap], all three or none), in descending-threshold order (the caller
 *     reverses and appends sklearn's (1, 0)): all levels when drop_intermediate == 0 or levels <= 2, otherwise the first, the
 *     last and every interior l with tps[l] != tps[l-1] or tps[l+1] != tps[l];
 *   - counts (host int64[5]) = {P, N, levels, ROC points (len(fpr) of sklearn), PR points (len(thresholds) of sklearn)},
 *     written whenever the checks pass;
 *   - best (host int64[3], may be NULL) = {tp, fp, level index} of the level that maximises F1 = 2 tp / (tp + fp + P) over
 *     ALL levels, compared exactly (128-bit cross-multiplication), ties to the higher threshold; *best_thr (host, may be
 *     NULL) its threshold.  P == 0: neither is written;
 *   - capacity: the point counts depend on the data (no bound below levels + 1 holds a priori).  A requested curve with more
 *     points than cap: nothing is written to the six buffers, the call returns MCGRA_ENOMEM, counts holds what is needed
 *     and mcgra_last_error() names it;
 *   - counts NULL, cap < 0, a curve with some but not all of its three buffers, or nothing asked for (all six buffers and
 *     best NULL): MCGRA_EINVAL, decided before any HIP call;
 *   - P == 0 or N == 0 still gives the integer curves (the NaN rates of sklearn are the caller's business).
 * Every result is an integer count or the copied bits of a score: no floating-point arithmetic, per-tile counts merged by
 * scans, so the same bits on every call.  Synchronises `stream`.
 * Device scratch: 8 bytes per selected entry (the sort's two key buffers) + 12 bytes per level + about 6 MB. */
int mcgra_rank_curves(void* stream, int n, const float* labels, int ld_labels, const float* scores, int ld_scores,
                      const int64_t* idx, int64_t n_idx, int drop_intermediate, int64_t cap,
                      int64_t* roc_tps, int64_t* roc_fps, float* roc_thr,   /* device [cap]; all three NULL: no ROC */
                      int64_t* pr_tps, int64_t* pr_fps, float* pr_thr,      /* device [cap]; all three NULL: no PR  */
                      int64_t* counts   /* host[5]: P, N, levels, ROC points, PR points */,
                      int64_t* best     /* host[3]: tp, fp, level index of the best-F1 level; may be NULL */,
                      float* best_thr   /* host; may be NULL */);

/* The same AUC for scores that are never stored: s_ij = dot_product_decode2(Z)_ij of the thin factor Z [n x d] (leading
 * dimension ldz >= d), computed pair by pair over idx x idx (main.py:412-437, notrain_test: how much of the graph a prior
 * leaks on its own).  labels, idx, n_idx, *out, exactness, NaN and error codes as mcgra_roc_auc.
 *   - mode 0, 1, 2, 4 of the table above (main.dot_product_decode, main.py:44-55, is modes 0 and 4); 3, 5, 6: MCGRA_ENOSUP;
 *   - d <= 128; wider: MCGRA_ENOSUP (mcgra_decode_scores + mcgra_roc_auc take any width);
 *   - modes 1, 4: rows normalised once, z / max(|z|_2, 1e-12), into an n x d scratch;
 *   - s_ij = <z_i, z_j> accumulated k ascending in fp32 (one fma per k), - 1 where i == j, relu, sigmoid for modes 0, 1:
 *     s_ij and s_ji are the same bits, and the result is bit for bit mcgra_roc_auc on what mcgra_decode_scores writes;
 *   - an entry of Z (any row) that is NaN or +-inf, or a selected score that is: MCGRA_EINVAL.
 * Device scratch: two 4-byte keys per selected pair, the normalised copy, about 3 MB. */
int mcgra_decode_auc(void* stream, int n, int d, const float* Z, int ldz, int mode, const float* labels, int ld_labels,
                     const int64_t* idx, int64_t n_idx, double* out);
/* mcgra_rank_metrics on the scores mcgra_decode_auc ranks: mode and width rules, checks and error codes as
 * mcgra_decode_auc, auc / ap as mcgra_rank_metrics; *auc is bit for bit mcgra_decode_auc's, and both are bit for bit
 * mcgra_rank_metrics on what mcgra_decode_scores writes. */
int mcgra_decode_rank_metrics(void* stream, int n, int d, const float* Z, int ldz, int mode, const float* labels,
                              int ld_labels, const int64_t* idx, int64_t n_idx, double* auc, double* ap);
/* out [n x n] (leading dimension ld_out >= n) = the same s_ij, materialised; any d.  Not the bits of
 * mcgra_dot_product_decode2, whose product runs on the MFMA GEMM.  Synchronises. */
int mcgra_decode_scores(void* stream, int n, int d, const float* Z, int ldz, int mode, float* out, int ld_out);

/* Link-stealing distance baselines: Attack-0 of He et al., "Stealing Links from Graph Neural Networks" (USENIX Security
 * 2021) scores a node pair by a distance between the two nodes' rows of a thin matrix Z [n x d] (leading dimension
 * ldz >= d; any d >= 1, the kernels stream it in chunks) -- posteriors, embeddings or features.  The metric ids, in the
 * paper's order; mcgra_pair_metric_name(id) is the one table of their names (NULL outside 0 .. 7). */
#define MCGRA_PAIR_COSINE 0
#define MCGRA_PAIR_EUCLIDEAN 1
#define MCGRA_PAIR_CORRELATION 2
#define MCGRA_PAIR_CHEBYSHEV 3
#define MCGRA_PAIR_BRAYCURTIS 4
#define MCGRA_PAIR_CANBERRA 5
#define MCGRA_PAIR_CITYBLOCK 6
#define MCGRA_PAIR_SQEUCLIDEAN 7
#define MCGRA_PAIR_METRICS 8
const char* mcgra_pair_metric_name(int metric);
/* The score of a pair is s_ij = 0.0f - dist(z_i, z_j): higher means more like an edge.  With a = z_ik, b = z_jk, every
 * distance is accumulated k ascending in fp32, one defined operation chain per k (scipy.spatial.distance's definitions):
 *     cityblock     sum |a - b|                               sqeuclidean   sum fma(a - b, a - b, .)
 *     euclidean     sqrtf(sqeuclidean)                        chebyshev     max |a - b|
 *     braycurtis    (sum |a - b|) / (sum |a + b|); a zero denominator gives 0
 *     canberra      sum |a - b| / (|a| + |b|); a term whose denominator is zero is 0 (scipy's rule)
 *     cosine        max(0, 1 - <zn_i, zn_j>), <., .> one fma per k, zn = z / max(|z|_2, 1e-12) computed once into an
 *                   n x d scratch.  A zero row is therefore at distance 1 from every row, itself included (scipy: NaN)
 *     correlation   cosine on the rows minus their own mean, mean = (sum of the row) / d.  A row whose entries are all
 *                   equal is centred to exact zeros whatever its sum rounds to, so it is at distance 1 from every row
 *                   (scipy: NaN), and d == 1 makes all pairs tie at distance 1.  The row sums are taken in a fixed order
 *                   (entry l, l + 64, ... per lane, then a fixed tree over the 64 lanes): the same bits on every call
 *   - |a - b|, |a + b|, |a| + |b|, (a - b)^2 and a b give the same bits with a and b swapped, so s_ij and s_ji are the same
 *     bits; the diagonal is the pair (i, i)'s own score (0 for the six difference metrics, about 1e-7 at most for cosine
 *     and correlation, whose rows are normalised in fp32);
 *   - the library is built -O3 without fast-math; hipcc then gives IEEE division and square root
 *     (-fhip-fp32-correctly-rounded-divide-sqrt is its default).  Nothing here relies on either being correctly
 *     rounded: both are functions of their operands' bits alone, which is all the symmetry and the repeatability need;
 *   - a NaN or +-inf anywhere in Z (any row), or for cosine / correlation a row whose sum of squares overflows
 *     float32: MCGRA_EINVAL;
 *   - metric outside 0 .. 7, n < 1, d < 1, Z NULL, ldz < d, out NULL or ld_out < n: MCGRA_EINVAL before any HIP call.
 * mcgra_pair_distance_scores materialises out [n x n] (leading dimension ld_out >= n), bitwise symmetric; after a
 * refusal nothing has been written.  Synchronises `stream`. */
int mcgra_pair_distance_scores(void* stream, int n, int d, const float* Z, int ldz, int metric, float* out, int ld_out);
/* The same scores, ranked without being stored.  The population is that of mcgra_auc_delong / mcgra_topk_metrics, NOT
 * mcgra_roc_auc's ordered entries with the diagonal: idx, n_idx REPEAT-FREE device int64 node ids, or NULL for all n nodes;
 * the candidates are the m = n_idx (n_idx - 1) / 2 unordered pairs of positions a > b, score s of (idx[a], idx[b]), label
 * labels[idx[a]][idx[b]] (labels n x n, ld_labels >= n).  n_idx from 2 to 65 535.
 *   - counts (host int64[4]) = {m, P, N, T}, T twice the Mann-Whitney U as defined for mcgra_auc_delong: bit for bit
 *     mcgra_auc_delong's integers on what mcgra_pair_distance_scores writes, and the same under any permutation of idx;
 *   - *auc = the nearest double of T / (2 P N); *ap follows mcgra_rank_metrics' definition and fixed summation order on
 *     these pairs.  auc, ap: host doubles; either may be NULL, not both.  P == 0 or N == 0: *auc = NaN (T = 0); P == 0:
 *     *ap = NaN; N == 0: *ap = 1.0 exactly;
 *   - before any HIP call: the argument errors above, ld_labels < n, labels NULL, n_idx < 2, auc and ap both NULL or counts
 *     NULL: MCGRA_EINVAL; n_idx > 65 535: MCGRA_ENOSUP;
 *   - the refusals of Z above; a selected score that overflows to a non-finite value, a selected label other than 0 or 1,
 *     a repeated or out-of-range id: MCGRA_EINVAL.  After a refusal nothing has been written.
 * Synchronises `stream`.  Device scratch: two 4-byte keys per selected pair, the normalised copy, about 3 MB. */
int mcgra_pair_distance_rank_metrics(void* stream, int n, int d, const float* Z, int ldz, int metric, const float* labels,
                                     int ld_labels, const int64_t* idx, int64_t n_idx, double* auc, double* ap,
                                     int64_t* counts /* host[4]: m, P, N, T */);

/* The recovered graph: the k best-scored node pairs of `scores` within idx, and how many of them are edges of `labels`.
 *   - the selection: idx, n_idx REPEAT-FREE device int64 node ids (a repeated or out-of-range id: MCGRA_EINVAL), or NULL
 *     for all n nodes in order.  The candidates are the m = n_idx (n_idx - 1) / 2 unordered pairs of positions a > b; pair
 *     (a, b) is nodes u = idx[a], v = idx[b], its score scores[u][v] and its label labels[u][v]: the strict lower triangle
 *     of the gathered submatrix -- for an asymmetric matrix that entry, not [v][u], is the one read.  Its packed position
 *     is p = a (a - 1) / 2 + b (torch.tril_indices(offset=-1); adj_changes).  Unlike mcgra_roc_auc / mcgra_rank_metrics,
 *     which range over all ordered entries of idx x idx, diagonal included, this ranges over unordered off-diagonal pairs;
 *   - the ranking: score descending as float32 values (-0.0 == +0.0; subnormals and negative scores are ordinary values),
 *     ties by ascending packed position; the k best are its first k: np.argsort(-s, kind="stable")[:k] over the scores in
 *     packed order;
 *   - counts (host int64[4]) = {k used, P, TP, m}: P the candidates with label 1, TP those among the k best.  precision =
 *     TP / k, recall = TP / P, F1 = 2 TP / (k + P) are left to the caller (exact integers);
 *   - k == 0 means k = P, the true graph's own edge count in the selection (then precision = recall = F1); with P == 0
 *     counts = {0, 0, 0, m} and *threshold is not written.  k < 0 or k > m: MCGRA_EINVAL;
 *   - *threshold (host, may be NULL) = the score of the k-th pair of the ranking, its bits as stored;
 *   - a selected score that is NaN or +-inf, or a selected label other than 0 or 1: MCGRA_EINVAL; entries outside the
 *     selected lower triangle are not looked at;
 *   - n_idx (n when idx is NULL) from 2 (MCGRA_EINVAL below) up to 65 535, so that p fits 32 bits; MCGRA_ENOSUP beyond;
 *   - exact and the same bits on every call: a radix select on order-preserving keys (no sort of the m candidates),
 *     integer counts, and threshold ties ranked in packed order whatever order the blocks run in.
 * Argument checks that need no device run before any HIP call.  Synchronises `stream`.
 * Device scratch: 5 bytes per candidate pair (a 4-byte key and the label) plus about 3 MB. */
int mcgra_topk_metrics(void* stream, int n, const float* labels, int ld_labels, const float* scores, int ld_scores,
                       const int64_t* idx, int64_t n_idx, int64_t k, int64_t* counts /* host[4]: k used, P, TP, m */,
                       float* threshold /* host, score of the k-th pair; may be NULL */);

/* The same k best pairs as an edge list in RANKING ORDER (best first, ties by ascending packed position), so that the
 * first k' <= k rows are the answer for k'.  Selection, ranking, checks, limits and error codes as mcgra_topk_metrics;
 * 1 <= k <= m.  pairs (device int64 [k x 2]) = the node ids u = idx[a], v = idx[b] (a > b) of each pair; pair_scores
 * (device [k], may be NULL) = scores[u][v], the bits as stored; hits (device uint8 [k], may be NULL; needs labels) = 1
 * where labels[u][v] is 1.  labels may be NULL (then nothing is said about edges; given, every selected label is checked).
 * Synchronises `stream`.
 * Device scratch: 4 bytes per candidate pair, 16 bytes per returned pair (the records and the second buffer of their
 * stable radix sort by descending key), about 3 MB. */
int mcgra_top_pairs(void* stream, int n, const float* scores, int ld_scores, const int64_t* idx, int64_t n_idx, int64_t k,
                    const float* labels /* may be NULL */, int ld_labels,
                    int64_t* pairs /* device [k x 2]: u, v */, float* pair_scores /* device [k], may be NULL */,
                    uint8_t* hits /* device [k], may be NULL; needs labels */);

/* The recovered graph WITHOUT the truth: which candidates are edges, decided from the scores alone by a 2-means split (the
 * reference's PGDAttack.kmeans, baseline.py:88-109, which starts from two random entries, sums float32 in an unspecified
 * order and stops after 20 rounds; this is a defined, exact and repeatable version of it).
 *   - candidates, selection, packed position, checks and limits as mcgra_topk_metrics: idx, n_idx REPEAT-FREE device int64
 *     node ids or NULL for all n nodes; the m = n_idx (n_idx - 1) / 2 pairs of positions a > b with score
 *     scores[idx[a]][idx[b]] and label labels[idx[a]][idx[b]], p = a (a - 1) / 2 + b; nothing outside the selected strict
 *     lower triangle is looked at; n_idx from 2 (MCGRA_EINVAL below) to 65 535 (MCGRA_ENOSUP beyond);
 *   - quantisation: q = rint(s 2^28), round half to even, as an unsigned integer (the product is exact in float32).  A
 *     selected score must satisfy 0 <= s < 16 (-0.0 counts as 0), so q < 2^32 and any sum of m < 2^31 of them fits 63 bits;
 *     the range holds the ensemble of up to eight [0, 1] matrices of topology_attack.py:314-320.  A selected score that is
 *     NaN or +-inf: MCGRA_EINVAL; a finite one below 0 or >= 16: MCGRA_ENOSUP.  Scores of at most 2^-29 (subnormals among
 *     them) collapse to q = 0: the split does not tell them from 0;
 *   - the split is Lloyd's iteration on the q, in integers.  lo = min q, hi = max q.  lo == hi (one value): the result is
 *     DEGENERATE -- iterations = 0, converged = 1, no edges (t = lo + 1, n_high = 0, c0 = c1 = lo, TP = 0) and the thresholds
 *     are not written.  Otherwise t_0 = floor((lo + hi) / 2) + 1, and round k counts the partition of t_k: the low cluster
 *     is {q < t_k}, the high cluster {q >= t_k}; c0 = floor(sum_low / n_low), c1 = floor(sum_high / n_high),
 *     t_{k+1} = floor((c0 + c1) / 2) + 1, so a value equidistant from the two centres goes low (the reference's argmin).
 *     Both clusters are non-empty in every round (c0 < t_{k+1} <= c1).  iterations = k + 1; the iteration stops when
 *     t_{k+1} == t_k (converged = 1) or when iterations == max_iter (converged = 0).  What is reported is always the
 *     partition that was counted, that of t_k;
 *   - out (host int64[10]) = {m, iterations, converged, t, n_high, c0, c1, P, TP, degenerate}: t, c0, c1 in units of 2^-28;
 *     P the candidates with label 1 and TP those of them in the high cluster, both -1 when labels is NULL (given, every
 *     selected label is checked: other than 0 or 1 is MCGRA_EINVAL).  precision = TP / n_high, recall = TP / P,
 *     F1 = 2 TP / (n_high + P) are left to the caller;
 *   - *thr_high (host, may be NULL) = the smallest selected score of the high cluster, *thr_low (host, may be NULL) = the
 *     largest of the low cluster: the bits as stored, -0.0 reported as +0.0.  rint is monotone, so the high cluster is
 *     exactly {s >= *thr_high} as float32 values: mcgra_threshold_pairs with threshold = *thr_high returns the high cluster;
 *   - max_iter < 1 and the other argument errors that need no device: MCGRA_EINVAL before any HIP call.  After any refusal
 *     nothing has been written to out or the thresholds;
 *   - everything is integer arithmetic merged by integer atomics: the same result whatever order the blocks run in.
 * Synchronises `stream` (once per four rounds; no kernel waits for another one's progress).
 * Device scratch: 5 bytes per candidate pair (the 4-byte q and, with labels, the label) plus a few KB. */
int mcgra_two_means_split(void* stream, int n, const float* scores, int ld_scores,
                          const float* labels /* may be NULL */, int ld_labels,
                          const int64_t* idx, int64_t n_idx, int max_iter,
                          int64_t* out      /* host[10]: m, iterations, converged, t, n_high, c0, c1, P, TP, degenerate */,
                          float* thr_high   /* host, may be NULL */,
                          float* thr_low    /* host, may be NULL */);

/* Every candidate with score >= threshold as an edge list in ASCENDING PACKED POSITION: np.nonzero(s >= threshold) over the
 * scores in packed order.  One entry for three thresholds: *thr_high of mcgra_two_means_split, the reference's filter() cut
 * (0.9, baseline.py:106-109) and best_thr of mcgra_rank_curves.  Candidates, selection, checks and limits as
 * mcgra_topk_metrics / mcgra_top_pairs: any finite score, negatives included; a selected NaN or +-inf score, or (given
 * labels) a selected label other than 0 or 1: MCGRA_EINVAL.
 *   - the comparison is that of float32 values: -0.0 >= +0.0 holds, subnormals are ordinary values, threshold = +-inf is
 *     allowed (nothing / everything); a NaN threshold: MCGRA_EINVAL;
 *   - pairs (device int64 [cap x 2]) = u = idx[a], v = idx[b] (a > b); pair_scores (device [cap], may be NULL) =
 *     scores[u][v], the bits as stored; hits (device uint8 [cap], may be NULL; needs labels) = 1 where labels[u][v] is 1;
 *   - counts (host int64[3]) = {m, pairs with score >= threshold, hits among them (-1 without labels)}, written whenever
 *     the checks pass;
 *   - capacity, as mcgra_rank_curves: more qualifying pairs than cap: nothing is written to the buffers, the call returns
 *     MCGRA_ENOMEM, counts holds what is needed and mcgra_last_error() names it.  cap == 0 with pairs NULL asks for the
 *     counts alone (returns 0);
 *   - counts NULL, cap < 0, cap > 0 with pairs NULL, hits without labels, a NaN threshold: MCGRA_EINVAL before any HIP call;
 *   - the order is decided by per-range counts and one scan, never by atomics: the same bits on every call.
 * Synchronises `stream`.  Device scratch: about 16 KB, and 4 bytes per node of the graph when idx is given. */
int mcgra_threshold_pairs(void* stream, int n, const float* scores, int ld_scores,
                          const float* labels /* may be NULL */, int ld_labels,
                          const int64_t* idx, int64_t n_idx, float threshold, int64_t cap,
                          int64_t* pairs /* device [cap x 2]: u, v */, float* pair_scores /* device [cap], may be NULL */,
                          uint8_t* hits  /* device [cap], may be NULL; needs labels */,
                          int64_t* counts /* host[3]: m, pairs with score >= threshold, hits among them (-1 without labels) */);

/* How far an AUC of the recovered graph can be trusted, and whether two of them differ: the exact integers of DeLong's
 * variance of the AUC and of DeLong's covariance of the AUCs of two scorings of the same pairs (DeLong, DeLong and
 * Clarke-Pearson, Biometrics 44, 1988).
 *   - candidates, selection and checks as mcgra_topk_metrics: idx, n_idx REPEAT-FREE device int64 node ids or NULL for all n
 *     nodes; the m = n_idx (n_idx - 1) / 2 unordered pairs of positions a > b with score scores[idx[a]][idx[b]] and label
 *     labels[idx[a]][idx[b]]; nothing outside the selected strict lower triangle is looked at.  This is NOT the population of
 *     mcgra_roc_auc / mcgra_rank_metrics, which range over the ordered entries with the diagonal: every pair appears there
 *     twice, so a variance over it would be too small by about two.  The AUC that belongs to these integers is the AUC of the
 *     unordered pairs, theta = T / (2 P N);
 *   - scores compare as float32 values: -0.0 == +0.0, subnormals and negative scores are ordinary values, ties are float32
 *     equality;
 *   - placements, with P candidates of label 1 and N of label 0:
 *       positive i:  a_i = 2 #{neg: s < s_i} + #{neg: s == s_i}   in [0, 2N]
 *       negative j:  b_j = 2 #{pos: s > s_j} + #{pos: s == s_j}   in [0, 2P]
 *     T = sum a_i = sum b_j (twice the Mann-Whitney U), A2 = sum a_i^2, B2 = sum b_j^2; for two score matrices A and B over
 *     the same labels and selection also A_ab = sum a_i^A a_i^B and B_ab = sum b_j^A b_j^B.  m < 2^31, so every sum is below
 *     2^95 and leaves as (low, high) 64-bit limbs, value = low + high 2^64;
 *   - what the caller forms from them (exact rationals, one rounding each):
 *       var   = (P A2 - T^2) / (4 N^2 P^2 (P - 1)) + (N B2 - T^2) / (4 P^2 N^2 (N - 1))
 *       cov   = (P A_ab - T_a T_b) / (4 N^2 P^2 (P - 1)) + (N B_ab - T_a T_b) / (4 P^2 N^2 (N - 1))
 *     P == 0 or N == 0: every sum is 0 and theta is undefined; P == 1 or N == 1: the variance is undefined;
 *   - a selected score (of either matrix) that is NaN or +-inf, a selected label other than 0 or 1, a repeated or
 *     out-of-range id: MCGRA_EINVAL;
 *   - n_idx (n when idx is NULL) from 2 (MCGRA_EINVAL below) up to 65 535 (MCGRA_ENOSUP beyond); out NULL, a matrix NULL or an
 *     ld below n: MCGRA_EINVAL.  These run before any HIP call.  After any refusal nothing has been written to out and
 *     mcgra_last_error() names the cause;
 *   - integer counts merged by integer atomics, no floating-point arithmetic on the device: the same bits on every call, and
 *     the same integers under any permutation of idx.
 * Synchronises `stream`.
 * Only the candidates of label 1 are stored and sorted; those of label 0 are streamed from the matrices.
 * Device scratch: nothing per candidate pair; 24 bytes per candidate of label 1 and score matrix (its key, the sorted copy, two
 * 4-byte counts and their 8-byte running sum) + 4 for the sort's second buffer; about 3 MB; 4 bytes per node of the graph when
 * idx is given. */
int mcgra_auc_delong(void* stream, int n, const float* labels, int ld_labels, const float* scores, int ld_scores,
                     const int64_t* idx, int64_t n_idx,
                     uint64_t* out /* host[8]: m, P, N, T, A2 lo, A2 hi, B2 lo, B2 hi */);
int mcgra_auc_delong_paired(void* stream, int n, const float* labels, int ld_labels,
                            const float* scores_a, int ld_a, const float* scores_b, int ld_b,
                            const int64_t* idx, int64_t n_idx,
                            uint64_t* out /* host[17]: m, P, N, T_a, T_b, then lo, hi of A2_a, B2_a, A2_b, B2_b, A_ab, B_ab */);

/* Which nodes carry the AUC, and how far it can be trusted when nodes rather than pairs are the independent units: the exact
 * integers of the delete-one-node jackknife of the AUC of mcgra_auc_delong (Efron and Stein, Ann. Statist. 9, 1981).
 *   - candidates, selection, comparison, placements a_p / b_q and checks as mcgra_auc_delong, for one score matrix.  With
 *     2 psi(p, q) in {0, 1, 2} the doubled win of the candidate p of label 1 over the candidate q of label 0 (2 for a higher
 *     score, 1 for a tie), a_p = sum_q 2 psi(p, q), b_q = sum_p 2 psi(p, q), T = sum_p a_p;
 *   - header (host[4]) = m, P, N, T: the values mcgra_auc_delong gives for the same input;
 *   - out (device uint64 [n_idx][5]), row v = position v of idx (not the node id), over the candidates that contain v:
 *       P_v, N_v   those of label 1 and of label 0; P_v + N_v = n_idx - 1
 *       A_v        sum of a_p over its candidates of label 1
 *       B_v        sum of b_q over its candidates of label 0
 *       C_v        sum of 2 psi(p, q) over its candidates p of label 1 and its candidates q of label 0
 *     The candidates that remain when node v is deleted have T - A_v - B_v + C_v (C_v is part of both sums), P - P_v of
 *     label 1 and N - N_v of label 0, so AUC_-v = (T - A_v - B_v + C_v) / (2 (P - P_v) (N - N_v)) -- left to the caller, with
 *     the jackknife variance (n_idx - 1) / n_idx sum_v (AUC_-v - mean)^2.  sum P_v = 2 P, sum N_v = 2 N, sum A_v = sum B_v = 2 T;
 *   - no overflow: n_idx <= 65 535, so P_v, N_v < 2^16 and P, N < 2^31: A_v <= 2 P_v N < 2^48, B_v <= 2 N_v P < 2^48,
 *     C_v <= 2 P_v N_v < 2^33, T <= 2 P N < 2^61;
 *   - refusals as mcgra_auc_delong: n_idx (n when idx is NULL) from 2 (MCGRA_EINVAL below) up to 65 535 (MCGRA_ENOSUP beyond),
 *     header or out NULL, a matrix NULL, an ld below n: before any HIP call; a selected NaN / +-inf score, a selected label
 *     other than 0 or 1, a repeated or out-of-range id: MCGRA_EINVAL.  No per-node stage bounds the selection further (a
 *     node's candidates of label 1 are sorted in device memory, not in LDS), so MCGRA_NODE_RANK_MAX_NIDX does not apply.  After
 *     any refusal nothing has been written to header or out and mcgra_last_error() names the cause;
 *   - integer counts merged by integer adds, no floating-point arithmetic on the device: the same bits on every call.
 * Synchronises `stream`.  Only the candidates of label 1 are stored; those of label 0 are streamed from the matrices.
 * Device scratch: nothing per candidate pair; 52 bytes per selected node; 64 bytes per candidate of label 1; about 3 MB; 4 bytes
 * per node of the graph when idx is given. */
int mcgra_auc_node_jackknife(void* stream, int n, const float* labels, int ld_labels, const float* scores, int ld_scores,
                             const int64_t* idx, int64_t n_idx, uint64_t* header /* host[4]: m, P, N, T */,
                             uint64_t* out /* device [n_idx][5]: P_v, N_v, A_v, B_v, C_v */);

/* Whether the recovered graph LOOKS like the real one: degrees, triangles and wedges of the graph a threshold cuts out of the
 * scores, of the true graph and of their intersection, as exact integers per node and in total.
 *   - candidates, selection and checks as mcgra_threshold_pairs / mcgra_topk_metrics: idx, n_idx REPEAT-FREE device int64 node
 *     ids or NULL for all n nodes; with m = n_idx the pairs of positions a > b with score scores[idx[a]][idx[b]] and label
 *     labels[idx[a]][idx[b]]; nothing outside the selected strict lower triangle is looked at; n_idx from 2 (MCGRA_EINVAL
 *     below) to 65 535 (MCGRA_ENOSUP beyond);
 *   - R is the undirected graph on the m positions with the edge {a, b} iff score >= threshold.  The comparison is
 *     mcgra_threshold_pairs': float32 values, -0.0 >= +0.0 holds, subnormals are ordinary values, threshold = +-inf is allowed
 *     (nothing / everything); a NaN threshold: MCGRA_EINVAL.  G, when labels are given, has the edge {a, b} iff the label is
 *     1.  C = R & G, the recovered edges that are true;
 *   - for a graph X and a position v: d_X(v) is its degree, t_X(v) the number of triangles through v, i.e. of unordered
 *     {u, w} with vu, vw, uw all in X;
 *   - out (device int64 [n_idx][6]), row v = position v of idx (not the node id) = {d_R, t_R, d_G, t_G, d_C, t_C}; the last
 *     four are -1 without labels;
 *   - header (host int64[9]) = {pairs m (m - 1) / 2, E_R, T_R, W_R, E_G, T_G, W_G, E_C, T_C}: E = sum d / 2 edges,
 *     T = sum t / 3 triangles, W = sum d (d - 1) / 2 wedges (paths of length two); the G and C entries are -1 without labels.
 *     Transitivity 3 T / W, the clustering coefficients 2 t / (d (d - 1)) and the comparisons of R with G are left to the
 *     caller.  E_R and E_C are mcgra_threshold_pairs' counts[1] and counts[2] on the same input;
 *   - no overflow: t_v <= C(65 534, 2) < 2^31, T < 2^46, W < 2^48;
 *   - a selected score that is NaN or +-inf (whatever the threshold), given labels a selected label other than 0 or 1, a
 *     repeated or out-of-range id: MCGRA_EINVAL.  header or out NULL, scores NULL, an ld below n, a NaN threshold and the
 *     n_idx limits are decided before any HIP call.  After any refusal nothing has been written to header or out and
 *     mcgra_last_error() names the cause;
 *   - the device does integer arithmetic only and every output has one writer: the same bits on every call, whatever order
 *     the blocks run in.
 * Synchronises `stream`.
 * Device scratch: each graph as a bit matrix of n_idx rows of ceil(n_idx / 64) 64-bit words -- one graph without labels, three
 * with them: 3 n_idx ceil(n_idx / 64) 8 bytes, 38 MB at n_idx = 10 000 and 1.6 GB at the capacity; MCGRA_ENOMEM when that
 * cannot be allocated.  About 100 bytes more, and 4 bytes per node of the graph when idx is given. */
int mcgra_graph_structure(void* stream, int n, const float* scores, int ld_scores,
                          const float* labels /* may be NULL */, int ld_labels,
                          const int64_t* idx, int64_t n_idx, float threshold,
                          int64_t* header /* host[9]: pairs, E_R, T_R, W_R, E_G, T_G, W_G, E_C, T_C */,
                          int64_t* out    /* device [n_idx][6]: d_R, t_R, d_G, t_G, d_C, t_C */);

/* Where the attack's errors sit: the AUC of the true edges against the non-edges at each distance of the TRUE graph, and the
 * false positives of a cut split by that distance, as exact integers.
 *   - candidates, selection, comparison and checks as mcgra_auc_delong: idx, n_idx REPEAT-FREE device int64 node ids or NULL for
 *     all n nodes; the m = n_idx (n_idx - 1) / 2 unordered pairs of positions a > b with score scores[idx[a]][idx[b]] and label
 *     labels[idx[a]][idx[b]]; nothing outside the selected strict lower triangle is looked at; scores compare as float32 values,
 *     -0.0 == +0.0;
 *   - G is the graph on the selected positions whose edges are the candidates of label 1 (mcgra_graph_structure's G) and
 *     dist(a, b) the shortest-path length in G.  G is the INDUCED subgraph: a path through an unselected node does not exist;
 *   - with H = hops in [1, MCGRA_HOP_MAX] every candidate is of one of H + 1 classes: class d, d = 1 .. H, is dist == d (class
 *     1: the edges, P of them); class H + 1, "beyond", is dist > H or no path.  The classes 2 .. H + 1 are the N non-edges;
 *   - out (host int64 [hops + 1][3]), row c - 1 = {pairs_c, T_c, above_c}:
 *       pairs_c   the candidates of the class; pairs_1 = P, the others sum to N
 *       T_c       c >= 2: the sum over the candidates q of the class of b_q = 2 #{edges that score higher} + #{edges that score
 *                 the same}, mcgra_auc_delong's placement: the doubled Mann-Whitney count of the edges against this class
 *                 alone, whose AUC is T_c / (2 P pairs_c).  T_1 = the sum of the other T_c = mcgra_auc_delong's T on the same
 *                 input, so the pooled AUC T_1 / (2 P N) is the mean of the class AUCs weighted by pairs_c / N
 *       above_c   the candidates of the class with score >= threshold, mcgra_threshold_pairs' comparison (-0.0 >= +0.0 holds,
 *                 +-inf are allowed): above_1 the true positives of the cut, the others its false positives by where they sit;
 *   - no overflow: T_c <= 2 P pairs_c < 2^63 for n_idx <= 65 535;
 *   - out NULL, a matrix NULL, an ld below n, hops outside [1, MCGRA_HOP_MAX], a NaN threshold, n_idx (n when idx is NULL) below 2:
 *     MCGRA_EINVAL; n_idx above 65 535: MCGRA_ENOSUP.  These run before any HIP call.  A selected score that is NaN or +-inf, a
 *     selected label other than 0 or 1, a repeated or out-of-range id: MCGRA_EINVAL.  After any refusal nothing has been
 *     written to out and mcgra_last_error() names the cause;
 *   - integer arithmetic only on the device (bit matrices built by ballots and ORs with one writer per word, integer counts
 *     merged by integer atomics): the same bits on every call, and the same integers under any permutation of idx.
 * Synchronises `stream`.
 * Device scratch: hops bit matrices of n_idx rows of ceil(n_idx / 64) 64-bit words (every level is kept for the one pass that
 * classifies the candidates): hops n_idx ceil(n_idx / 64) 8 bytes, 38 MB at n_idx = 10 000 and 1.6 GB at the capacity for
 * hops = 3; MCGRA_ENOMEM when that cannot be allocated.  8 bytes per candidate of label 1, about 3 MB, and 4 bytes per node
 * of the graph when idx is given. */
#define MCGRA_HOP_MAX 8
int mcgra_hop_auc(void* stream, int n, const float* labels, int ld_labels, const float* scores, int ld_scores,
                  const int64_t* idx, int64_t n_idx, int hops, float threshold,
                  int64_t* out /* host [hops + 1][3]: row c - 1 = {pairs_c, T_c, above_c} */);

/* What the attack knows beyond the node classes: the AUC of the true edges against the non-edges of the SAME stratum of class
 * pairs, and the pairs at or above a cut per stratum, as exact integers.
 *   - candidates, selection, comparison and checks as mcgra_auc_delong: idx, n_idx REPEAT-FREE device int64 node ids or NULL for
 *     all n nodes; the m = n_idx (n_idx - 1) / 2 unordered pairs of positions a > b with score scores[idx[a]][idx[b]] and label
 *     labels[idx[a]][idx[b]]; nothing outside the selected strict lower triangle is looked at; scores compare as float32 values,
 *     -0.0 == +0.0;
 *   - node_class (device int32 [n]) is indexed by node id, not by position: the class of position a is c_a = node_class[idx[a]],
 *     in [0, n_class) for every selected node (the unselected entries are not looked at), n_class = C in [1, MCGRA_CLASS_MAX];
 *   - strata (HOST uint8 [C][C]) is symmetric with every entry below n_strata = G, G in [1, C_max (C_max + 1) / 2 = 136]: the
 *     stratum of a candidate is strata[c_a][c_b].  A stratum that no candidate falls into is legal and gives a zero row;
 *   - out (host int64 [n_strata][5]), row g = {pairs_g, P_g, T_g, above_g, hits_g}:
 *       pairs_g   the candidates of the stratum; they sum to m
 *       P_g       those of label 1; N_g = pairs_g - P_g
 *       T_g       the sum over the non-edges q of the stratum of b_q = 2 #{edges of the same stratum that score higher} +
 *                 #{edges of the same stratum that score the same}: mcgra_auc_delong's placement restricted to the stratum,
 *                 whose AUC is T_g / (2 P_g N_g)
 *       above_g   the candidates of the stratum with score >= threshold, mcgra_threshold_pairs' comparison (-0.0 >= +0.0 holds,
 *                 +-inf are allowed)
 *       hits_g    those of label 1 among them;
 *   - no overflow: T_g <= 2 P_g N_g < 2^63 for n_idx <= 65 535;
 *   - out, node_class, strata or a matrix NULL, an ld below n, n_class or n_strata out of range, an asymmetric table or an entry
 *     >= n_strata, a NaN threshold, n_idx (n when idx is NULL) below 2: MCGRA_EINVAL; n_idx above 65 535: MCGRA_ENOSUP.  These run
 *     before any HIP call.  A selected score that is NaN or +-inf, a selected label other than 0 or 1, a repeated or out-of-range
 *     id, a selected node whose class is outside [0, n_class): MCGRA_EINVAL.  After any refusal nothing has been written to out
 *     and mcgra_last_error() names the cause;
 *   - integer arithmetic only on the device (a radix sort of the edges by stratum and score, searches inside a stratum's
 *     segment, integer counts merged by integer atomics): the same bits on every call, the same integers under any permutation
 *     of idx and under any renaming of the classes with their table.
 * Synchronises `stream`.
 * Device scratch: 16 bytes per candidate of label 1, about 3 MB, one byte per selected node, and 4 bytes per node of the graph
 * when idx is given. */
#define MCGRA_CLASS_MAX 16
int mcgra_class_auc(void* stream, int n, const float* labels, int ld_labels, const float* scores, int ld_scores,
                    const int64_t* idx, int64_t n_idx, const int32_t* node_class, int n_class,
                    const uint8_t* strata /* host [n_class][n_class] */, int n_strata, float threshold,
                    int64_t* out /* host [n_strata][5]: row g = {pairs_g, P_g, T_g, above_g, hits_g} */);

/* Which summand carries an ensemble: mcgra_auc_delong's T of up to 255 subset sums of up to eight components, in one pass.
 *   - candidates, selection, label checks and idx rules as mcgra_auc_delong: idx, n_idx REPEAT-FREE device int64 node ids or NULL
 *     for all n nodes; the m = n_idx (n_idx - 1) / 2 unordered pairs of positions a > b with label labels[idx[a]][idx[b]];
 *   - comps: a HOST array of K device pointers, K in [1, MCGRA_SUBSET_MAX_K], component k an n x n float32 matrix of leading
 *     dimension ld_comps, read at [idx[a]][idx[b]] only;
 *   - masks: a HOST array of n_masks in [1, MCGRA_SUBSET_MAX_MASKS] masks, each in [1, 2^K); bit k selects component k.  Repeats
 *     are allowed and give equal T;
 *   - the score of a pair under mask M is the float32 sum of its components k in M in ascending k: s = c_first; s = s + c_next;
 *     ... (one rounding per add, no fma, no other order);
 *   - out (host uint64 [3 + n_masks]) = {m, P, N, T_0, ..., T_{n_masks - 1}}: P the pairs of label 1, N = m - P, T_s =
 *     mcgra_auc_delong's T (twice the Mann-Whitney count of the edges over the non-edges, ties counted once; -0.0 == +0.0) on the
 *     materialised sum of masks[s], whose AUC is T_s / (2 P N).  T_s <= 2 P N < 2^63 for n_idx <= 65 535;
 *   - out, comps, masks, labels or a component NULL, K or n_masks out of range, a mask outside [1, 2^K), an ld below n, n_idx (n
 *     when idx is NULL) below 2: MCGRA_EINVAL; n_idx above 65 535: MCGRA_ENOSUP.  These run before any HIP call.  A selected
 *     component value or a subset sum (of a mask asked for, or of one of its prefixes in ascending k) that is NaN or +-inf, a
 *     selected label other than 0 or 1, a repeated or out-of-range id: MCGRA_EINVAL.  After any refusal nothing has been
 *     written to out and mcgra_last_error() names the cause;
 *   - integer arithmetic on the device apart from the adds (a radix sort of the edges' sums by mask and score, searches inside a
 *     mask's segment, integer counts merged by integer atomics): the same bits on every call, the same integers under any
 *     permutation of idx.
 * Synchronises `stream`.
 * Device scratch: 16 bytes per candidate of label 1 and distinct mask, about 3 MB, and 4 bytes per node of the graph when idx
 * is given. */
#define MCGRA_SUBSET_MAX_K 8
#define MCGRA_SUBSET_MAX_MASKS 255
int mcgra_subset_auc(void* stream, int n, const float* labels, int ld_labels,
                     const float* const* comps /* host [K] device pointers */, int K, int ld_comps, const int64_t* idx,
                     int64_t n_idx, const uint32_t* masks /* host [n_masks] */, int n_masks,
                     uint64_t* out /* host [3 + n_masks]: {m, P, N, T_0, ...} */);

/* Whose neighbourhood leaked: the ranking of every selected node's own candidates, as exact integer counts per node.
 *   - the selection: idx, n_idx REPEAT-FREE device int64 node ids (a repeated or out-of-range id: MCGRA_EINVAL), or NULL for
 *     all n nodes in order.  For position a of idx the candidates are the n_idx - 1 positions b != a; candidate b has score
 *     scores[idx[a]][idx[b]] and label labels[idx[a]][idx[b]]: row a of the gathered submatrix without its diagonal, so an
 *     asymmetric matrix is ranked by rows;
 *   - scores compare as float32 values (-0.0 == +0.0; subnormals and negative scores are ordinary values); the best-first
 *     ranking of a row is score descending, ties by ascending position b (the position in idx, not the node id);
 *   - out (device int64 [n_idx][5]), row a = {P, wins, ties, hits, first_rank}: P the positive candidates; wins / ties the
 *     (positive, negative) candidate pairs whose positive scores higher / the same; hits the positives among the P best of the
 *     best-first ranking; first_rank = 1 + the candidates that score strictly higher than the best positive, 0 when P == 0.
 *     With N = n_idx - 1 - P: the row's AUC = (2 wins + ties) / (2 P N), its R-precision = hits / P, its reciprocal rank =
 *     1 / first_rank, and the reference's calc_mrr on the row (gcn_parameterized.py:18-26: the mean over the positives of
 *     (1 + the negatives that score strictly higher) / N) = (P N - wins - ties + P) / (P N) -- left to the caller;
 *   - a candidate score that is NaN or +-inf, or a candidate label other than 0 or 1: MCGRA_EINVAL; the diagonal and the
 *     unselected rows and columns are not looked at.  After any refusal nothing has been written to out;
 *   - n_idx (n when idx is NULL) from 2 (MCGRA_EINVAL below) up to MCGRA_NODE_RANK_MAX_NIDX: one workgroup ranks one row
 *     entirely in LDS; MCGRA_ENOSUP beyond;
 *   - no floating-point arithmetic: the same bits on every call, whatever order the workgroups run in.
 * Argument checks that need no device run before any HIP call.  Synchronises `stream`.
 * Device scratch: 40 bytes per selected node, and 4 bytes per node of the graph when idx is given. */
#define MCGRA_NODE_RANK_MAX_NIDX 16384
int mcgra_node_rank_metrics(void* stream, int n, const float* labels, int ld_labels, const float* scores, int ld_scores,
                            const int64_t* idx, int64_t n_idx, int64_t* out /* device [n_idx][5] */);

/* The k-nearest-neighbour graph of the scores: every selected node keeps its own k best-scored partners, and the lists are
 * symmetrised as the union ("either end picks the other") and as the mutual graph ("both do").  A local cut, beside the global
 * cuts of mcgra_topk_metrics and mcgra_threshold_pairs; its in-degrees measure hubness (Radovanovic, Nanopoulos and Ivanovic,
 * JMLR 11, 2010).
 *   - selection, candidates and ranking as mcgra_node_rank_metrics: idx, n_idx REPEAT-FREE device int64 node ids or NULL for
 *     all n nodes in order; m = n_idx positions; for position a the candidates are the positions b != a with score
 *     scores[idx[a]][idx[b]] (row a of the gathered submatrix without its diagonal: an asymmetric matrix is ranked by rows);
 *     float32 comparison, -0.0 == +0.0, subnormals and negative scores ordinary values; best first = score descending, ties by
 *     ascending position b (the position in idx, not the node id);
 *   - L_k(a) = the first k positions of row a's ranking.  D: the arc a -> b iff b is in L_k(a) (every out-degree is k);
 *     U: {a, b} iff a -> b or b -> a; Mu: {a, b} iff both; with labels G: {a, b}, a > b, iff labels[idx[a]][idx[b]] == 1 (the
 *     strict lower triangle, as mcgra_graph_structure reads it);
 *   - header (host int64[8]) = {pairs m (m - 1) / 2, k, E_U, E_M, E_G, H_D, H_U, H_M}: the edge counts of U, Mu and G, the
 *     arcs of D whose pair is an edge of G, the edges of U and of Mu that are edges of G; the last four -1 without labels;
 *   - out (device int64 [m][7]), row a = {in, d_U, d_M, d_G, h_D, h_U, h_M}: in = |{b : b -> a}|, the degrees in U, Mu and G,
 *     h_D = |L_k(a) & N_G(a)|, the neighbours in U / Mu that are neighbours in G; the last four -1 without labels.
 *     sum in = m k, d_M = k + in - d_U, E_U + E_M = m k, H_D = H_U + H_M;
 *   - lists (device int32 [m][k], may be NULL), row a = L_k(a) as positions, in ranking order;
 *   - the edge list of U in ASCENDING PACKED POSITION a (a - 1) / 2 + b (a > b), capacity as mcgra_threshold_pairs: pairs
 *     (device int64 [cap][2]) = u = idx[a], v = idx[b]; pair_scores (device [cap], may be NULL) = scores[u][v], the bits as
 *     stored; kind (device uint8 [cap], may be NULL): bit 0 a -> b, bit 1 b -> a, 3 mutual; hits (device uint8 [cap], may be
 *     NULL; needs labels) = 1 where {a, b} is an edge of G.  cap == 0 with pairs NULL asks for no list.  E_U > cap: MCGRA_ENOMEM
 *     with header, out and lists written, nothing in the four list buffers, and mcgra_last_error() naming what is needed;
 *     cap = m k always suffices.  The order comes from per-node counts and one scan, never from atomics;
 *   - n_idx from 2 (MCGRA_EINVAL below) up to MCGRA_KNN_MAX_NIDX (one workgroup selects one row in LDS; MCGRA_ENOSUP beyond);
 *     1 <= k <= m - 1, else MCGRA_EINVAL; k above MCGRA_KNN_MAX_K: MCGRA_ENOSUP;
 *   - a candidate score that is NaN or +-inf, given labels a selected label (strict lower triangle) other than 0 or 1, a
 *     repeated or out-of-range id: MCGRA_EINVAL; the diagonal and the unselected rows and columns are not looked at.  After any
 *     refusal nothing has been written to header, out, lists or the list buffers;
 *   - header, out or scores NULL, an ld below n, the limits on n_idx and k, cap < 0, cap > 0 with pairs NULL, hits without
 *     labels: refused before any HIP call;
 *   - integer arithmetic and key comparisons only: the same bits on every call, whatever order the workgroups run in.
 * A row is selected (four radix rounds over its keys in LDS), not sorted; only the k winners are sorted, and only for lists.
 * Synchronises `stream`.  Device scratch: two bit matrices of m x ceil(m / 64) 64-bit words and a third with labels (96 MB at
 * the capacity), 12 bytes per selected node, and 4 bytes per node of the graph when idx is given; a failed allocation:
 * MCGRA_ENOMEM. */
#define MCGRA_KNN_MAX_NIDX 16384
#define MCGRA_KNN_MAX_K 1024
int mcgra_knn_graph(void* stream, int n, const float* scores, int ld_scores,
                    const float* labels /* may be NULL */, int ld_labels,
                    const int64_t* idx, int64_t n_idx, int64_t k,
                    int64_t* header /* host[8] */, int64_t* out /* device [n_idx][7] */,
                    int32_t* lists /* device [n_idx][k], may be NULL */, int64_t cap,
                    int64_t* pairs /* device [cap x 2]: u, v */, float* pair_scores /* device [cap], may be NULL */,
                    uint8_t* kind /* device [cap], may be NULL */, uint8_t* hits /* device [cap], may be NULL; needs labels */);

/* Which edges leak: every true edge's own placement among the non-edges, by how deep the edge sits in the TRUE graph -- the
 * common neighbours of its two ends (its embeddedness) and the smaller of their degrees -- as exact integers per stratum and,
 * on request, edge by edge.  The positives' side of what mcgra_hop_auc does for the non-edges.
 *   - candidates, selection, comparison and checks as mcgra_auc_delong: idx, n_idx REPEAT-FREE device int64 node ids or NULL for
 *     all n nodes; the m = n_idx (n_idx - 1) / 2 unordered pairs of positions a > b with score scores[idx[a]][idx[b]] and label
 *     labels[idx[a]][idx[b]]; nothing outside the selected strict lower triangle is looked at; scores compare as float32 values,
 *     -0.0 == +0.0;
 *   - G is the graph on the selected positions whose edges are the candidates of label 1 (mcgra_graph_structure's G), the INDUCED
 *     subgraph: a neighbour that is not selected does not exist.  For every edge e = {a, b} of G:
 *       a_e   2 #{non-edges that score lower} + #{non-edges that score the same}, in [0, 2 N]: mcgra_auc_delong's placement of a
 *             positive against ALL N non-edges of the selection
 *       c_e   |N_G(a) & N_G(b)|, the triangles of G through the edge; its class ec = min(c_e, 15)
 *       d_e   min(deg_G(a), deg_G(b)); its class dc = min(15, bit_length(d_e)): 1, 2-3, 4-7, ..., 16384 and more.  dc >= 1 for
 *             every edge, so the rows dc = 0 stay zero;
 *   - header (host int64[6]) = {m, P, N, T, above_pos, above_neg}: T = the sum of the a_e = mcgra_auc_delong's T on the same
 *     input; above_* = the candidates of label 1 / 0 with score >= threshold, mcgra_threshold_pairs' comparison (-0.0 >= +0.0
 *     holds, +-inf are allowed);
 *   - table (host int64 [16][16][3]), cell (ec, dc) = {P, T, above} over the edges of the cell: the P sum to P, the T to T, the
 *     above to above_pos; an edge class's AUC against all non-edges is T_cell / (2 P_cell N).  P == 0 or N == 0: every T is 0;
 *   - the edges in ASCENDING PACKED POSITION a (a - 1) / 2 + b, capacity as mcgra_threshold_pairs: pairs (device int64 [cap][2])
 *     = u = idx[a], v = idx[b]; and, each of which may be NULL, pair_scores (device [cap]) = scores[u][v], the bits as stored;
 *     placement (device int64 [cap]) = a_e; common (device int32 [cap]) = c_e, uncapped; deg (device int32 [cap][2]) =
 *     deg_G(a), deg_G(b).  cap == 0 with every column NULL asks for the integers alone.  0 < cap < P: MCGRA_ENOMEM with header
 *     and table written, nothing in the columns, and mcgra_last_error() naming what is needed (header[1]); rows past P are not
 *     written.  The order comes from a sort of the edges' positions, never from atomics;
 *   - no overflow: T_cell <= 2 P_cell N < 2^63 for n_idx <= 65 535; c_e, d_e < 2^16;
 *   - header or table NULL, a matrix NULL, an ld below n, a NaN threshold, cap < 0, cap > 0 with pairs NULL, cap == 0 with a
 *     column given, n_idx (n when idx is NULL) below 2: MCGRA_EINVAL; n_idx above 65 535: MCGRA_ENOSUP.  These run before any HIP
 *     call.  A selected score that is NaN or +-inf, a selected label other than 0 or 1, a repeated or out-of-range id:
 *     MCGRA_EINVAL.  After any of these refusals nothing has been written to header, table or the columns and
 *     mcgra_last_error() names the cause;
 *   - integer arithmetic only on the device (a bit matrix built by ballots with one writer per word, AND + popcount, two radix
 *     sorts, integer counts and degrees merged by integer atomics): the same bits on every call; header and table are the same under any
 *     permutation of idx, the columns hold the same rows.
 * Synchronises `stream`.
 * Device scratch: one bit matrix of n_idx rows of ceil(n_idx / 64) 64-bit words (13 MB at n_idx = 10 000, 537 MB at the
 * capacity; MCGRA_ENOMEM when that cannot be allocated), 28 bytes per candidate of label 1 (its key, the sort's second buffer,
 * two 4-byte counts, their 8-byte running sum, its packed ends), 4 bytes per selected node, about 3 MB, and 4 bytes per node of
 * the graph when idx is given. */
#define MCGRA_EXPOSURE_CLASSES 16
int mcgra_edge_exposure(void* stream, int n, const float* labels, int ld_labels, const float* scores, int ld_scores,
                        const int64_t* idx, int64_t n_idx, float threshold, int64_t cap,
                        int64_t* pairs /* device [cap x 2]: u, v */, float* pair_scores /* device [cap], may be NULL */,
                        int64_t* placement /* device [cap], may be NULL */, int32_t* common /* device [cap], may be NULL */,
                        int32_t* deg /* device [cap x 2], may be NULL */,
                        int64_t* header /* host[6]: m, P, N, T, above_pos, above_neg */,
                        int64_t* table /* host [16][16][3]: cell (ec, dc) = {P, T, above} */);

/* A defended victim's graph: the edge-level differential-privacy mechanisms EdgeRand and LapGraph of Wu et al., "LinkTeller:
 * Recovering Private Edges from Graph Neural Networks via Influence Analysis" (IEEE S&P 2022), applied to the graph of adj.
 *   - the pairs: positions a > b of all n nodes, label adj[a][b] (only the strict lower triangle of adj is read; a value there
 *     other than 0 or 1: MCGRA_EINVAL), packed position p = a (a - 1) / 2 + b, m = n (n - 1) / 2, E the pairs of label 1;
 *   - the generator: Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9,
 *     0xBB67AE85), key = (seed & 0xffffffff, seed >> 32), counter = (p, 0, replicate, 0), result words w0 .. w3.  One call per
 *     pair and no state: pair p's draw depends on (seed, replicate, p) alone -- not on n, the grid or the call;
 *   - MCGRA_DP_EDGERAND: randomised response.  T = floor(2^32 / (1 + e^eps) + 1/2) in double on the host; pair p's label is
 *     flipped iff w0 < T: with probability q = T / 2^32, which is LinkTeller's "with probability 2 / (1 + e^eps) replace the
 *     cell by a fair coin".  realised = {q, ln((1 - q) / q)} (inf when T = 0, the identity);
 *   - MCGRA_DP_LAPGRAPH: eps1 = 0.01 eps for the edge count, eps2 = 0.99 eps for the cells.  For a draw, u = ((w0 >> 8) + 1/2)
 *     2^-24 in (0, 1), sigma = +1 iff bit 31 of w1 is clear, Lap(beta) = sigma beta (-ln u), in double throughout.  Cell p:
 *     v_p = float32(label + Lap(1 / eps2)), ONE rounding of the double sum.  The target count = clamp(rint(E + Lap(1 / eps1)), 0, m)
 *     from the draw at counter (m, 0, replicate, 0), on the host.  The result holds the `target` best pairs by v descending
 *     (float32 values), ties by ascending p: mcgra_topk_metrics' ranking, by its radix select.  realised = {the count's noise,
 *     NaN};
 *   - out [n x n] = the perturbed graph: 0 / 1, symmetric, zero diagonal; columns from n to ld_out are not touched.  noisy
 *     (LapGraph only; may be NULL) [n x n] = v mirrored, 0 on the diagonal; with NULL the cells live in scratch of the call;
 *   - counts (host int64[6]) = {m, E, target (EdgeRand: -1), kept, added, removed}: the pairs of label 1 that stay, the pairs of
 *     label 0 that become edges, the pairs of label 1 that do not.  kept + removed = E; kept + added = the edge count of out
 *     (LapGraph: = target).  Integer block sums merged by integer atomics: the same bits on every call; realised may be NULL;
 *   - n < 2 or n > 65 535 (p must fit 32 bits), eps <= 0 or not finite, a mechanism other than the two, noisy with EdgeRand, adj,
 *     out or counts NULL, an ld below n: MCGRA_EINVAL before any HIP call, nothing written.  A label other than 0 or 1, or
 *     (LapGraph, eps below about 1e-37) a cell that overflows float32: MCGRA_EINVAL with counts and realised not written; out
 *     and noisy may hold part of a result then.
 * Synchronises `stream`.  EdgeRand is one pass: it reads 2 n^2 bytes and writes 4 n^2.  Device scratch: none for EdgeRand; for
 * LapGraph 5 bytes per pair (the keys of the select and the selection as bytes), about 3 MB, and 4 n^2 bytes when noisy is
 * NULL; MCGRA_ENOMEM when that cannot be allocated. */
#define MCGRA_DP_EDGERAND 0
#define MCGRA_DP_LAPGRAPH 1
int mcgra_dp_perturb_graph(void* stream, int n, const float* adj, int ld_adj, int mechanism, double eps, uint64_t seed,
                           uint32_t replicate, float* out, int ld_out, float* noisy /* device n x n or NULL */, int ld_noisy,
                           int64_t* counts /* host[6]: m, E, target, kept, added, removed */,
                           double* realised /* host[2], may be NULL */);

/* GCN.forward in eval mode (models/gcn.py:164-174): log_softmax(linear1(
 * relu(adj @ (... relu(adj @ (X @ W0) + b0) ...)))).  X [n x nfeat],
 * W[l] [dims[l] x dims[l+1]], b[l] [dims[l+1]], Wlin [nclass x dims[nlayer]].
 * emb_out (optional, may be NULL) receives embedding_GCN.forward with
 * emb_nlayer layers (models/gcn.py:71-76); out [n x nclass] log-probabilities. */
int mcgra_gcn_forward(void* stream, int n, int nfeat, int nlayer, const int32_t* dims,
                      const float* X, const float* adj, const float* const* W,
                      const float* const* b, const float* Wlin, const float* blin,
                      int nclass, int emb_nlayer, float* emb_out, float* out);

/* The LinkTeller influence attack of Wu et al., "LinkTeller: Recovering Private Edges from Graph Neural Networks via Influence
 * Analysis" (IEEE S&P 2022): how much node u's output moves when node v's features are scaled, for every ordered pair.
 *   - the victim is what mcgra_gcn_forward computes: H^0 = X, P^l = A (H^l W_l) + b_l, H^{l+1} = relu(P^l) for l = 0 .. L-1,
 *     Z = H^L Wlin^T + blin, O = log_softmax(Z).  The model arguments are mcgra_gcn_forward's; A = adj is any dense n x n float32
 *     propagation matrix (row stride ld_adj) whose support is symmetric: a_uw != 0 <=> a_wu != 0;
 *   - for a source v, X^(v) is X with row v multiplied by (1 + Delta), Delta = float32(delta) (the paper's delta is 1e-4).
 *     I[v -> u] = || O(X^(v))_u - O(X)_u ||_2 / Delta.  output = MCGRA_INFLUENCE_LOG_POSTERIORS takes O as the victim returns it,
 *     MCGRA_INFLUENCE_POSTERIORS takes exp(O).  symmetrize = 0: out[v][u] = I[v -> u] (the row is the source; the diagonal is the
 *     self-influence); symmetrize = 1: out[a][b] = max(I[a -> b], I[b -> a]), bitwise symmetric;
 *   - the computed form is never two forwards subtracted in float32 (that carries u |O| / Delta of cancellation noise).  The base
 *     pre-activations P^l are kept and the differences carried:  dT^0 = 0 except row v = Delta (x_v W_0);
 *     dP^l_u = sum over w in F_l(v), ascending w, of a_uw dT^l_w;  dH^{l+1}_u = max(dP, -P) if P > 0 else max(P + dP, 0), which is
 *     relu(P + dP) - relu(P) without cancellation and follows a unit that the perturbation switches on or off;
 *     dT^{l+1} = dH^{l+1} W_{l+1};  dZ = dH^L Wlin^T;  dlogp_k = dZ_k - log1p(sum_j p_j expm1(dZ_j)), p = exp(O);
 *     dp_k = p_k expm1(dlogp_k); the norm is the square root of the sum over k ascending of the squares, divided by Delta;
 *   - the frontier is structural: F_0(v) = {v}, F_{l+1}(v) = {u : a_uw != 0 for some w in F_l(v)}.  Outside F_L(v) the output is
 *     exactly +0.0.  One source costs its L-hop neighbourhood, not n rows; a frontier that reaches all n nodes (a hub, a complete
 *     graph, an EdgeRand graph at small eps) is computed correctly but walks dense row lists: counts[1] tells;
 *   - out: device n x n (row stride ld_out); columns from n to ld_out are not touched.  counts (host int64[3]) = {the non-zero
 *     cells of adj, the reached ordered pairs sum_v |F_L(v)|, max_v |F_L(v)|}: exact integers, the same on every call;
 *   - every sum has a fixed order and no float is merged atomically: the same bits on every call and on every grid (the number of
 *     workgroups follows the device and the scratch budget; MCGRA_INFLUENCE_GROUPS in the environment lowers it);
 *   - MCGRA_EINVAL before any HIP call, nothing written: a NULL pointer (W[l], b[l] included), n, nfeat or nclass < 1, a width
 *     < 1, dims[0] != nfeat, an ld below n, nlayer outside 1 .. MCGRA_MAX_LAYERS, a delta whose float32 is not finite, is 0 or has
 *     |Delta| >= 1, output or symmetrize outside 0 / 1.  MCGRA_ENOSUP: n > 65 535, a hidden width or nclass above
 *     MCGRA_INFLUENCE_MAX_WIDTH (one lane owns one column).  MCGRA_EINVAL with counts not written: an asymmetric support, a NaN
 *     or an infinity in adj, X or the weights, a base output that is not finite (X W_0, a pre-activation, which relu would hide,
 *     or O); out is not written then either.
 * Synchronises `stream`.  Device scratch: the base forward's node buffers ((L + 4) n hm floats and mcgra_gcn_forward's product
 * workspace of 64 n hm floats, hm the widest layer), the row lists (8 bytes per non-zero cell of adj, 8 n bytes of offsets) and
 * two slabs of n x hm floats per workgroup, at most 512 MB of them together; MCGRA_ENOMEM when that cannot be allocated. */
#define MCGRA_INFLUENCE_MAX_WIDTH 64
#define MCGRA_INFLUENCE_LOG_POSTERIORS 0
#define MCGRA_INFLUENCE_POSTERIORS 1
int mcgra_influence_scores(void* stream, int n, int nfeat, int nlayer, const int32_t* dims, const float* X, const float* adj,
                           int ld_adj, const float* const* W, const float* const* b, const float* Wlin, const float* blin,
                           int nclass, double delta, int output, int symmetrize, float* out, int ld_out,
                           int64_t* counts /* host[3]: nnz, reached, max_reach */);

/* -------------------------------------------------------- attack engine --
 * One object per PGDAttack instance.  It owns the learnable adjacency
 * (adj_changes, kept dense-symmetric in HBM), the Adam moments and all
 * per-step workspace. */
typedef struct mcgra_attack mcgra_attack_t;

typedef struct mcgra_attack_config {
  int32_t n;           /* nnodes */
  int32_t nfeat;       /* feature width */
  int32_t nclass;
  int32_t nlayer;      /* len(victim_model.gc) */
  int32_t emb_nlayer;  /* embedding.nlayer at loop entry (main.py:240 leaves 2) */
  int32_t dims[MCGRA_MAX_LAYERS + 1]; /* dims[0] = nfeat, dims[l+1] = out width of gc[l] */
  int32_t measure;     /* enum mcgra_measure */
  int32_t n_attack;    /* len(idx_attack) */
  float weight_sup;    /* weight_supervised */
  float w[10];         /* weight_param (w1..w10), topology_attack.py:151 */
  float lr;            /* Adam lr (lr_ori) */
  float eps;           /* args.eps; != 0 needs noise passed to mcgra_attack_step */
  double num_edges;    /* projection budget (topology_attack.py:338) */
  /* row-block sharding over ranks (one process per GPU, see "row-block sharded step" below).  row_begin/row_end is
     the block of adjacency rows this object owns; a single-GPU object uses [0, n) (row_end 0 = n). */
  int32_t row_begin, row_end;
  /* victim family, unified layer form  P_l = adj @ (H W_l) + H Ws_l + b_l,  H_l = act(P_l):
   *   GCN (models/gcn.py:35-46,164-174)        act 0 (relu), head_act 0, has_self 0
   *   dense GAT (models/gat.py:36-50: the attention product is overwritten by adj @ h; heads concatenated into
   *   W_l, zero bias; head elu(out_att(x)) :206)  act 1 (elu), head_act 1, has_self 0
   *   GraphSAGE (models/graphsage.py:37-50: [x | adj@x] @ weight)   act 0, head_act 0, has_self 1 */
  int32_t act, head_act, has_self;
  /* depths of the H_A1 / H_A2 embedding forwards of the post-loop ensemble (topology_attack.py:304-307):
     {1, 2}; embedding_gat.forward ignores set_layers (gat.py:170-174), so a GAT uses {nlayer, nlayer}. 0 = default */
  int32_t fin_layers[2];
  /* shard_world > 0: this object is rank row_begin / shard_rows of shard_world row-block ranks with shard_rows rows
     each (a multiple of 256; the last ranks may own fewer or no rows: n <= shard_rows * shard_world).  0: unsharded. */
  int32_t shard_world, shard_rows;
} mcgra_attack_config_t;

int mcgra_attack_create(mcgra_attack_t** out, const mcgra_attack_config_t* cfg);
int mcgra_attack_destroy(mcgra_attack_t* h);

/* victim_model / embedding weights (models/gcn.py GCN.gc[l].weight/.bias,
 * GCN.linear1); device pointers, copied. */
int mcgra_attack_set_model(mcgra_attack_t* h, void* stream, const float* const* W,
                           const float* const* b, const float* Wlin, const float* blin,
                           const float* const* Ws /* GraphSAGE self weights, NULL unless has_self */);

/* constant inputs of PGDAttack.attack (topology_attack.py:95-98): ori_features
 * [n x nfeat], adj (true graph, used only for the H_A / Y_A priors :177-182),
 * ori_adj (init_adj [n x n]; NULL = zeros, the only value dataset.py:433 produces),
 * feature_adj [n x n], labels [n] int32, idx_attack [n_attack] int32.
 * Computes T0 = X W0, H_A_cur and Y_A once.  Synchronises.
 * A non-NULL ori_adj takes the general step for every measure (modified_adj =
 * clamp(adj_changes + ori_adj) with its gradient gate :164-165 / :474-478, the embedding
 * on modified_adj - ori_adj :185 in a chain of its own, + ori_adj in modified_adj1 :188 and
 * in the adjacency of the post-loop ensemble :302); not available on a row-block rank. */
int mcgra_attack_set_graph(mcgra_attack_t* h, void* stream, const float* features,
                           const float* adj, const float* ori_adj, const float* feature_adj,
                           const int32_t* labels, const int32_t* idx_attack);

/* adj_changes in the reference's packed order (n(n-1)/2 floats). */
int mcgra_attack_set_adj_changes(mcgra_attack_t* h, void* stream, const float* packed);
int mcgra_attack_get_adj_changes(mcgra_attack_t* h, void* stream, float* packed);

/* One iteration of the loop at topology_attack.py:161-298: forward, losses,
 * backward into adj_changes, Adam step, projection, clamp.  noise (n x n,
 * stands for torch.randn_like at :475) may be NULL when eps == 0.
 * scalars_out (host, may be NULL) receives after a stream sync:
 *   [0] loss  [1] origin_loss  [2] c1 [3] c2 [4] c6 [5] c7 [6] c9 [7] c10
 *   [8] sum(clamp(adj_changes,0,1)) after the update  [9] nll
 * Passing NULL keeps the call asynchronous, except for one 4-byte device-to-host readback per step on HSIC
 * configurations with w2 != 0 (whether the decode found a dead embedding row, which selects the low-rank or the Gram
 * evaluation; the fused step reads it from mapped host memory without emptying the queue).  When the
 * preceding call on this handle was mcgra_attack_monitor (and eps == 0) the step adopts that call's forward instead of
 * recomputing it (same bits). */
int mcgra_attack_step(mcgra_attack_t* h, void* stream, const float* noise,
                      double* scalars_out);

/* ------------------------------------------------ row-block sharded step --
 * One process per GPU; rank r owns rows [row_begin, row_end) of the learnable adjacency and of the Adam moments and
 * does 1/world of every N x N pass of the fused low-rank step:
 *   - skinny products M[rows, :] V, then an all-gather of the n x c result rows (node-level work is replicated);
 *   - the N x N x N product as a COLUMN block P1[:, rows] = (H Kf H) Xc[:, rows] from planes packed from the rank's
 *     own rows (Xc^T rows = adj_norm rows by symmetry), then one all-to-all of tile blocks that hands every rank its
 *     ROW block P1[rows, :] as well (the mirrored gradient needs P1_ij and P1_ji);
 *   - decode, tail reductions and Adam on the rank's rows; n-vectors (r, d, gd, the decode backward) ride in the same
 *     all-gathers as the products where both are ready at the same point, and every scalar that is summed over the ranks
 *     (|adj_changes|^2, the masked-pair and dead-row counts, the loss terms) rides in a two-column "lane" of the gathered array: rank k
 *     leaves its partial in row k * rows_per_rank + q, and behind the gather every rank adds the `world` partials in rank
 *     order -- the same bits on every rank, and no all-reduce.  Per step + monitoring forward at L GCN layers: 2 L + 3
 *     all-gathers and the one all-to-all (8 collectives at L = 2; one more gather when want_scalars is set).
 *   The elementwise measures have no product and no low-rank factors: measure MSELoss exchanges 2 L + 2 all-gathers per step and
 *   no N x N data; measure KL (round 6) 2 L + 3 -- one more gather, of the rows' softmax statistics [logsumexp(adj_norm_i) |
 *   logsumexp(modified_adj1_i)], which the decode backward and the tail need of EVERY row.
 * The step is an ordered table of stages (csrc/attack_fused.hip: FS_STAGES, its forward FW_STAGES); a stage that ends at an
 * exchange describes the collective, mcgra_attack_shard_next returns there and the next call goes on with the next stage.  The
 * host layer (mc-gra_amd/sharded.py) executes it with torch.distributed (backend "nccl" = RCCL) on views of ONE caller-owned device arena:
 *     mcgra_attack_bind_exchange(h, arena, mcgra_attack_exchange_bytes(h));
 *     mcgra_attack_shard_begin(h, stream, MCGRA_SHARD_STEP, want_scalars);
 *     while (mcgra_attack_shard_next(h, stream, &ex) == 0 && ex.kind != MCGRA_XCHG_DONE)  run_collective(ex);
 * All offsets are bytes from the arena base.  The collectives must run on `stream` (or be ordered after it).
 * A step whose decode masks a pair all-gathers M and the Adam moments and is redone, replicated, by the general
 * path on every rank (rare: DESIGN.md 1b).  Supported for the configurations the fused step supports
 * (mcgra_attack_fused_steps); anything else returns MCGRA_ENOSUP from mcgra_attack_create with shard_world > 0. */
#define MCGRA_XCHG_DONE 0
#define MCGRA_XCHG_ALLGATHER 1      /* `world` chunks of chunk_bytes at offset; this rank's chunk (index rank) is filled */
#define MCGRA_XCHG_ALLREDUCE_F64 2  /* sum over ranks of `count` doubles at offset (kept in the protocol; the fused step no longer
                                       asks for it: its scalars ride in the gathers' lane) */
#define MCGRA_XCHG_ALLTOALL 3       /* `world` chunks of chunk_bytes: send from offset, receive into offset2 */
typedef struct mcgra_exchange {
  int32_t kind, count;
  int64_t offset, offset2, chunk_bytes;
} mcgra_exchange_t;
#define MCGRA_SHARD_STEP 0          /* one iteration of the loop (:161-283) */
#define MCGRA_SHARD_MONITOR 1       /* the monitoring forward (:290-296); the next step adopts it */
#define MCGRA_SHARD_MONITOR_LAST 2  /* the same forward behind the LAST iteration of a run: no step follows, so nothing is
                                     * started for one (a row-block rank's forward otherwise forks the next step's pack and
                                     * N x N x N product as soon as the degree vector is complete; a product nobody takes is
                                     * dropped safely, but it is a product's worth of GPU time) */
int64_t mcgra_attack_exchange_bytes(mcgra_attack_t* h);
int mcgra_attack_bind_exchange(mcgra_attack_t* h, void* arena, int64_t bytes);
int mcgra_attack_shard_begin(mcgra_attack_t* h, void* stream, int what, int want_scalars);
int mcgra_attack_shard_next(mcgra_attack_t* h, void* stream, mcgra_exchange_t* ex);
/* after a MCGRA_SHARD_STEP begun with want_scalars: the ten values of mcgra_attack_step's scalars_out (identical on
 * every rank); after MCGRA_SHARD_MONITOR(_LAST): out[0] = mean(modified_adj).  Synchronises. */
int mcgra_attack_shard_scalars(mcgra_attack_t* h, void* stream, double* out);
/* rows [row_begin, row_end) of adj_changes' dense form: out [row_end - row_begin][n] fp32 (tests, checkpoints) */
int mcgra_attack_get_rows(mcgra_attack_t* h, void* stream, float* out);
/* How the one N x N x N product of a low-rank step is evaluated by this engine: 0 = fp32 MFMA SYMM, 2 = 3-plane bf16
 * split, 3 = 2-plane fp16 split (the default for n >= 1024), both by the hand-written kernel of split_symm_bf16.hip at
 * fp32-level error; 1 = the SINGLE plane product x0 y0 of the 2-plane fp16 operands (fp16 accuracy, 2^-11
 * per operand; also the four products of a Gram-evaluation step) -- a named mode, MCGRA_SPLIT_BF16=1, never a default (the
 * reference's CPU path is fp32).  Chosen at create from MCGRA_SPLIT_BF16. */
int mcgra_attack_product_mode(mcgra_attack_t* h);
/* Steps that took the low-rank / the Gram (general) evaluation of the N x N linear_HSIC terms since creation. */
int mcgra_attack_path_stats(mcgra_attack_t* h, long long* lowrank_steps, long long* general_steps);
/* How many of the low-rank steps ran as the fused step that evaluates every N x N quantity from the learnable
 * adjacency and n-vectors (attack_fused.hip: adj_norm, its centred copy, modified_adj1 and d loss / d adj_norm are
 * never stored), the fused MSELoss step (calc = MSELoss: elementwise in the same per-pair quantities, no product) and the fused KL
 * step (calc = calc_kl, topology_attack.py:483-487: + per-row softmax statistics from one more per-pair pass) included; those two do
 * not count as low-rank steps in mcgra_attack_path_stats.  Which configurations take a fused step: mcgra_attack_plan, below. */
long long mcgra_attack_fused_steps(mcgra_attack_t* h);
/* What mcgra_attack_create decides for a configuration, from the configuration and the environment alone: no device is touched
 * and none is needed (the rule itself: csrc/attack_plan.hip: plan_attack, which create runs first).  fused .. product_mode and
 * text describe cfg as given; shardable / why answer whether a row-block rank (shard_world > 0) may run it, whatever
 * shard_world / row_begin / row_end of cfg say.  Returns what mcgra_attack_create would return for the same cfg (the reason in
 * mcgra_last_error), except that the refusal of a row-block rank shows in shardable / why only. */
typedef struct mcgra_attack_plan {
  int32_t fused;        /* 0 none, 1 the fused HSIC step, 2 MSELoss, 3 KL (mcgra_attack_fused_steps) */
  int32_t lowrank;      /* the unfused low-rank step is available (mcgra_attack_path_stats) */
  int32_t product_mode; /* as mcgra_attack_product_mode */
  int32_t shardable;    /* create with shard_world > 0 would accept this configuration */
  char why[256];        /* shardable == 0: the first term of the rule that fails */
  char text[1024];      /* diagnostic: every create-time flag, one "name=value" per line */
} mcgra_attack_plan_t;
int mcgra_attack_plan(const mcgra_attack_config_t* cfg, mcgra_attack_plan_t* out);
/* Fused steps whose decode relu-masked pairs (S_ij <= 0 off the diagonal) while every embedding row was alive: they stand.
 * With a ReLU embedding zn >= 0, so a masked pair has S_ij == 0 exactly: the value of modified_adj1 is still Z Z^T - D, and
 * what relu'(0) = 0 takes out of the decode backward is a multiple of zn_j on row i -- coordinates on which em_i is zero,
 * i.e. which the embedding layer's own ReLU backward masks anyway (measured: bit-identical
 * gradients with and without an explicit correction).  Only a DEAD row (em_i == 0: zn_i == 0, the algebra takes
 * |zn_i| = 1) sends a step to the Gram evaluation.  Rounds 1 - 3 sent every step with a masked pair there (3x slower at
 * N = 10 000). */
long long mcgra_attack_masked_fused_steps(mcgra_attack_t* h);
/* Steps whose N x N x N product was cut in two behind whole rounds of the chip.  Monolithic engine, n >= 8192 (DESIGN.md section
 * 1c): behind ~0.8 of the tiles the first rows of P1 are complete in both orientations, and the tail's first pass over them runs
 * beside the product's last rounds (bit-identical to the uncut step; MCGRA_EARLY_TAIL=0 disables; not when the loss terms are
 * asked for).  Row-block ranks: cut for the all-to-all of P1: the rank computes the row
 * panels of its peers first and its own last, in one linear tile order cut behind the peers' tiles; the MCGRA_XCHG_ALLTOALL
 * exchange point is reached when the first part is done, so the collective runs beside the second part (the engine joins it
 * behind the exchange).  Default: wherever a whole round of the chip ends behind the peers' tiles (the cut is then free), and
 * for 2 <= shard_world <= 4 in any case (a second ragged round); MCGRA_A2A_OVERLAP=0 / 1 forces it off / on. */
long long mcgra_attack_cut_product_steps(mcgra_attack_t* h);
/* Gram-evaluation steps (a dead embedding row, GAT / SAGE chains, CKA, MCGRA_NO_LOWRANK) whose four N x N x N products ran on the
 * 2-plane fp16 kernel instead of fp32 SYMM (n >= 1024, HSIC, eps == 0; MCGRA_GRAM_SPLIT=0 turns it off). */
long long mcgra_attack_gram_split_steps(mcgra_attack_t* h);

/* Monitoring forward of topology_attack.py:290-296 on the current adjacency:
 * out_logp [n x nclass] = victim(features, normalize(get_modified_adj)),
 * *sparsity (host) = mean(modified_adj).  Synchronises if sparsity != NULL. */
int mcgra_attack_monitor(mcgra_attack_t* h, void* stream, float* out_logp, double* sparsity);

/* After the loop (topology_attack.py:300-324): adj_changes <- decode(embedding(
 * features, adj_norm of the last iteration)); modified_adj = get_modified_adj +
 * dd2(H_A1) + dd2(H_A2) + feature_adj + dd2(Y_A2) [+ dd2(H_A)] [+ dd2(Y_A)]
 * [+ label_adj].  decode_mode selects the dot_product_decode2 branch
 * (topology_attack.py:421-467): 0 sigmoid(relu(ZZ^T - I)) (cora, AIDS);
 * 1 same on row-normalised Z (citeseer); 2 relu(ZZ^T - I) (brazil);
 * 3 relu(rownorm(ZZ^T) - I) (polblogs / usair default); 4,5,6 relu(Zn Zn^T - I)
 * with Zn rows normalised in p = 2, 3, 5 (usair prior-specific branches).
 * H_A [n x dims[emb]] / Y_A [n x nclass] / label_adj [n x n] may be NULL when
 * the matching use* flag is 0.  out [n x n]. */
int mcgra_attack_finalize(mcgra_attack_t* h, void* stream, int decode_mode,
                          const float* H_A, const float* Y_A, const float* label_adj,
                          float* out);

/* mcgra_attack_finalize with its summands kept apart: the same carry rule, the same M afterwards.  Component k is written as an
 * n x n matrix (ld = n) at comps + k n n, in the order in which mcgra_attack_finalize adds them: 0 learned (modified_adj of
 * :302, with ori_adj when there is one), 1 feature, 2 H_A1, 3 H_A2, 4 Y_A2, 5 ori_HA (H_A), 6 ori_YA (Y_A), 7 label
 * (MCGRA_ENSEMBLE_COMPONENTS of them; comps holds all eight slots).  A component whose input is NULL is not written and its
 * bit is clear in *present (host; may be NULL).  Each component is the bits mcgra_attack_finalize adds (a decode accumulates
 * into `out` there, into a zeroed matrix here).  out may be NULL; otherwise out [n x n] = the float32 sum of the components of
 * out_mask in ascending k, s = c_first; s = s + c_next; ...: for an out_mask equal to the given inputs, mcgra_attack_finalize's
 * out bit for bit.  Refused (MCGRA_EINVAL, before anything is touched) beside mcgra_attack_finalize's refusals: NULL comps, an
 * out_mask with a bit outside present, out_mask == 0 with a non-NULL out. */
#define MCGRA_ENSEMBLE_COMPONENTS 8
int mcgra_attack_finalize_components(mcgra_attack_t* h, void* stream, int decode_mode,
                                     const float* H_A, const float* Y_A, const float* label_adj,
                                     unsigned out_mask, float* out, float* comps, unsigned* present);

/* Device pointer + shape of a named intermediate of the last step, for parity
 * tests ("adj_norm", "A1", "em", "G_adjn", "G_A1", "G_A", "G_sym", "M", "d",
 * "r", "logp", "sm2", "HA", "YA", "T0", "KFC").  ld receives the leading dimension.  "G_sym" (the mirrored packed
 * gradient of the last step) is kept only when MCGRA_KEEP_GSYM=1 was set at create; on a low-rank step "G_A1" does not
 * hold d loss / d modified_adj1 (it is never materialised there).
 * The call takes no stream and orders nothing: a monitor call may have left work running on a side stream that writes the scratch
 * buffers ("A1", "G_A", ...).  Read the pointer through mcgra_attack_copy_buffer, or on a stream behind the wait that
 * mcgra_attack_copy_buffer enqueues there. */
int mcgra_attack_buffer(mcgra_attack_t* h, const char* name, float** ptr,
                        int* rows, int* cols, int* ld);
/* copy of the same intermediate into a caller buffer dst [rows x cols], leading dimension dst_ld; `stream` first waits for
 * whatever the last call left running on a side stream (no flag of the engine changes) */
int mcgra_attack_copy_buffer(mcgra_attack_t* h, void* stream, const char* name, float* dst, int dst_ld);

/* Timing of the dominant kernel: the engine brackets every launch of the fp32
 * MFMA GEMM with HIP events on the launch stream when profiling is enabled.
 * mcgra_attack_gemm_stats synchronises, then returns launch count, total
 * milliseconds and total flops since the last reset. */
int mcgra_attack_profile(mcgra_attack_t* h, int enable);
/* Measurement aid: `reps` back-to-back launches of the last fused step's N x N x N product (split2_m16_kernel on the
 * operand planes that step packed; results go to scratch) with nothing beside them, timed by HIP events on `stream`;
 * returns the mean launch time.  bench.py's roofline.alone and scripts/power_trace.py's product_alone phase.  No engine
 * state changes.  Needs a preceding fused low-rank step with w1 != 0. */
int mcgra_attack_product_replay(mcgra_attack_t* h, void* stream, int reps, double* ms_per_launch);
/* TEST ONLY -- never call it in a real run.  Arms a deliberate defect in the fused step so that a parity test can prove it
 * would notice one (tests/test_gpu_fullsize.py::test_mutations_turn_the_10k_reference_test_red and
 * ::test_mutations_turn_the_fused_10k_reference_tests_red): what = 1 wipes the result of the N x N x N product before the
 * tail reads it, 2 drops the rank-k terms of the tail, 3 drops the per-pair terms c1 / c2 of a fused MSELoss / KL step from
 * the decode and the tail, 4 wipes the KL row statistics (logsumexp of adj_norm's and modified_adj1's rows) after
 * k_decode_stats, 0 disarms.  Says so on stderr.
 * Arming is refused (MCGRA_EINVAL) unless the engine was created with MCGRA_TESTING=1 in the environment. */
int mcgra_attack_test_mutate(mcgra_attack_t* h, int what);
int mcgra_attack_gemm_stats(mcgra_attack_t* h, int reset, int64_t* launches,
                            double* ms, double* flops);

#ifdef __cplusplus
}
#endif
#endif /* MCGRA_H */
