/*
 * stpy_hip.h -- C ABI of libstpy_hip.so: the MI355X (gfx950) implementation of the dense
 * linear-algebra hot path of Mojusko/stpy (kernel Gram matrices, blocked Cholesky, triangular
 * solves, GP prediction epilogue, log-marginal reductions, random-Fourier-feature embed,
 * pivoted partial Cholesky of an on-the-fly kernel matrix for Nystrom landmarks).
 *
 * The reference has no FFI of its own: the path sits behind Python methods that call torch CPU
 * ops.  Each entry point below replaces the torch/scipy call sequence cited next to it
 * (file:line relative to the reference root); INTEGRATION.md shows the ctypes binding a
 * maintainer would add on the reference side.
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer into caller-owned memory (PyTorch-ROCm storage in the
 *     shipped host code), with ONE exception, the index list `del_host` of stpy_potrf_delete (see there);
 *     matrices are row-major with an explicit leading dimension in ELEMENTS;
 *   - dtype: 0 = float64, 1 = float32 (all operands of one call share it);
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises;
 *   - no allocation of data, no ownership transfer; workspaces are sized by the *_workspace_bytes queries and
 *     passed with their size (`work_bytes`), the inverse-diagonal-block array `winv` with its element count
 *     (`winv_elems`): a buffer smaller than the query's answer for the same arguments is refused (-20 / -21)
 *     instead of being overrun;
 *   - state kept by the library, all of it documented here:
 *       * a thread-local last-error string;
 *       * per (device, caller stream): one high-priority side stream + three events, created on the first
 *         stpy_potrf / stpy_trsm_right_lt call on that stream and kept for the life of the process (the panel
 *         look-ahead).  Host threads that drive DIFFERENT streams may call concurrently; calls that share a
 *         stream must be issued by one thread at a time (they are ordered by the stream, like any HIP work); with them 64 bytes
 *         of device memory (the ticket / counter words of the one-launch vector solve), the library's only allocation;
 *       * the launch profiler's record table (stpy_profile_*), guarded by a mutex, off by default;
 *       * the ten ROUTE switches of stpy_tune (which shipped kernel serves a call where the library normally decides by
 *         size): process-wide integers read at launch time, never written by the shipped host code -- tests/ use them to
 *         reach every shipped path at small sizes; they must not be changed while another thread is inside the library.
 *         Behaviour a caller may legitimately want per call is a `flags` argument instead (STPY_FLAG_*).  The timing
 *         experiments of tools/ (ablation bits, measured-and-dropped kernel variants, in-kernel
 *         stamps) are NOT in this library: they live in the lab build (make EXPERIMENTS=1 -> libstpy_hip_lab.so);
 *       * one sticky device error word per caller stream (part of the 64 bytes above), read by stpy_async_status;
 *   - exported symbols: exactly the functions declared in this header (the build hides everything else);
 *   - return value: 0 = ok, <0 = invalid argument (-(index of the argument), 1-based) or
 *     -1000-hipError for a failed launch; numerical failure of the factorisation is reported
 *     through the device word `info_dev` (0 = ok, j>0 = leading minor j not positive definite),
 *     exactly LAPACK's potrf convention, so the host decides when to synchronise and read it;
 *   - an empty problem (an output with a zero dimension: no test points, no rows) returns 0 without
 *     looking at any pointer -- empty tensors have null data pointers.
 */
#ifndef STPY_HIP_H
#define STPY_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

enum { STPY_F64 = 0, STPY_F32 = 1 };

/* stationary / dot-product kernel families; lengthscales arrive as inv_ls[k] = 1/ell_k */
enum {
	STPY_K_SE = 0,        /* kappa * exp(-r^2/2)                      kernels.py:368-398, :552-583 (ard) */
	STPY_K_MATERN12 = 1,  /* kappa * exp(-r)                          kernels.py:844-845                 */
	STPY_K_MATERN32 = 2,  /* kappa * (1+sqrt3 r) exp(-sqrt3 r)        kernels.py:846-848                 */
	STPY_K_MATERN52 = 3,  /* kappa * (1+sqrt5 r+5r^2/3) exp(-sqrt5 r) kernels.py:849-851, :946-962       */
	STPY_K_LINEAR = 4,    /* kappa * <b_j, a_i> + offset              kernels.py:300-320                 */
	STPY_K_POLY = 5       /* kappa * (<b_j, a_i> + offset)^p          kernels.py:744-761 (offset = 1 there);
	                         the degree p (1..64) rides above the family byte: kind = STPY_K_POLY | (p << 8) */
};

/* per-call flags of stpy_potrf / stpy_trsm_right_lt */
enum {
	STPY_FLAG_BESIDE_UPDATE = 1   /* the call is enqueued while another stream's trailing update occupies the chip
	                                 (multi-GPU panel look-ahead): its small K = 128 products take the 32 KiB-LDS
	                                 kernels that fit on a CU beside one update workgroup, not the 128 KiB one-volley
	                                 kernel that would wait for a whole CU to drain */
};

/* how a kernel evaluation is combined into `out` -- the + and * kernel algebra of kernels.py:146-157 */
enum { STPY_OUT_SET = 0, STPY_OUT_ADD = 1, STPY_OUT_MUL = 2 };

const char* stpy_version(void);
const char* stpy_last_error_string(void);

/*
 * Gram matrix, replaces KernelFunction.kernel(a, b) for one kernel item (kernels.py:136-159):
 *   out[j*ldo + i] (op)= kappa * phi(|| (b_j - a_i)[cols] * inv_ls ||) (+ offset for LINEAR)
 *                        + diag_add * [i == j]
 * a: n x lda, b: q x ldb, out: q x n  (orientation (|b|,|a|) as kernels.py:393).
 * cols: device int32[d] column subset ("group", kernels.py:387-388) or NULL for 0..d-1.
 * inv_ls: device array of d elements of `dtype`.  lower_only != 0 writes only i <= j blocks
 * (used when a == b feeds the Cholesky).  diag_add carries s^2 of gauss_procc.py:151-163.
 * work: NULL, or stpy_gram_workspace_bytes(dtype, n, q, d) bytes of scratch.  With a workspace the
 * inner products run on the MFMA contraction with the kernel function fused into its epilogue
 * (all kinds except MATERN12, which always uses the direct-difference tile kernel).
 * Accuracy.  SE on every route, and MATERN32 / MATERN52 with a workspace, form r^2 = |a'|^2 + |b'|^2 - 2 <a', b'> from the points taken
 * relative to the first row of `a` (a' = (a_i - a_0)[cols] * inv_ls, b' likewise: one common shift per call, read on the device), which
 * a stationary kernel does not see.  The error of such an entry is proportional to the squared DIAMETER of the scaled data, not to its
 * distance from the origin:  |out - exact| <= kappa (c 4 (d + 3) eps D^2 + 8 eps),  D^2 the largest scaled squared distance between two
 * points of a and b, eps the machine epsilon of `dtype`, c = max |d phi / d r^2| = 1/2 (SE), 3/2 (MATERN32), 5/6 (MATERN52).  fp32 on
 * data much wider than the lengthscale loses digits accordingly (about 4e-4 at a scaled diameter of 36).  The direct-difference routes
 * (MATERN12 always, MATERN32 / MATERN52 without a workspace) are good to kappa (d + 8) eps wherever the data lies, and give kappa
 * exactly on coincident points.  LINEAR and POLY are not translation invariant and are evaluated as written.
 */
int64_t stpy_gram_workspace_bytes(int dtype, int64_t n, int64_t q, int d);
int stpy_gram(int kind, int dtype,
              const void* a, int64_t n, int64_t lda,
              const void* b, int64_t q, int64_t ldb,
              int d, const int32_t* cols, const void* inv_ls,
              double kappa, double offset, double diag_add,
              int lower_only, int combine,
              void* out, int64_t ldo, void* work, int64_t work_bytes, void* stream);

/* k(x_i, x_i) for i < m -- replaces the per-point Python loop of gauss_procc.py:347 */
int stpy_gram_diag(int kind, int dtype, const void* x, int64_t m, int64_t ldx,
                   int d, const int32_t* cols, const void* inv_ls,
                   double kappa, double offset, int combine, void* out, void* stream);

/*
 * Blocked right-looking Cholesky, A = L L^T in place in the lower triangle (the strict upper
 * triangle is scratch).  Replaces torch.linalg.cholesky (estimator.py:35) and stands in for
 * lstsq / lu_factor / slogdet (gauss_procc.py:370-378, :634).
 * winv: ceil(n/128) blocks of 128x128 elements (winv_elems >= stpy_potrf_winv_elems(n), else -21); receives
 *       inverse(L_cc) of every 128x128 diagonal block (reused by the triangular solves below).
 * work: stpy_potrf_workspace_bytes(dtype, n, nb) bytes.   nb: outer panel width, multiple of 128
 *       (0 = library default).   info_dev: device int32.
 *       The workspace holds two panel buffers of n x (widest panel) elements.  With nb = 0 the widest panel follows the size:
 *       256 / 512 / 1024 columns up to 2048 / 16 384 / 32 768 rows and 2048 above (since library 0.3: the K = 2048 trailing updates),
 *       i.e. 0.54 GB at n = 32 768, 2.1 GB at n = 65 536 and 4.3 GB at n = 131 072 in fp64 -- on top of the in-place matrix.  In fp32 the
 *       workspace also holds the three bf16 planes of one panel (6 more bytes per panel element: 14 instead of 8; 1.9 GB at n = 65 536).  ALWAYS
 *       size it by the query for the same (dtype, n, nb): a buffer sized by an older build's formula is refused with -20, not overrun.
 */
int64_t stpy_potrf_workspace_bytes(int dtype, int64_t n, int nb);
int64_t stpy_potrf_winv_elems(int64_t n);
int stpy_potrf(int dtype, int64_t n, void* A, int64_t lda, void* winv, int64_t winv_elems,
               void* work, int64_t work_bytes, int nb, int flags, int32_t* info_dev, void* stream);

/*
 * Bordered Cholesky: extend a resident factor by k rows (GaussianProcess.add_data_point(iterative=True); the "iterative" branch of
 * fit_gp, gauss_procc.py:136-177, which the reference leaves a stub).  n1 = n0 + k, n1p = n1 rounded up to a multiple of 128,
 * t0 = 128 * floor(n0 / 128).
 *   on entry: rows [0, n0) of A's lower triangle hold a factor from stpy_potrf (or an earlier append) on the tile-padded layout
 *             (winv: its inverse diagonal blocks); rows [n0, n1), columns [0, n1), lower part: the new rows of K + s^2 I;
 *             z (may be NULL): L11^-1 y_old in [0, n0); y: the k new targets (device, read only when z is given).
 *   on exit:  A[0:n1p, 0:n1p] has the layout stpy_potrf leaves for the bordered matrix -- [L21 L22] in rows [n0, n1), zeros in
 *             columns (r, n1p) of each new row r, identity rows [n1, n1p) -- so every consumer (stpy_trsv, stpy_trsm_right_lt,
 *             stpy_predict, stpy_logdet_quad, stpy_trsm_ln_factor, stpy_potri) runs on it with n = n1p; winv blocks
 *             [t0/128, n1p/128) hold inverse(L_cc); z[n0:n1) = L22^-1 (y - L21 z1), z[n1:n1p) = 0; *info_dev = 0, or the 1-based
 *             global index of the first non-positive pivot.
 * Rows [0, n0) of A and the winv blocks below t0 are not written.  L21 = K21 L11^-T streams L11 once per 8 (fp64) / 16 (fp32) right-hand sides:
 * a one-launch dataflow solve (the hand-off protocol of stpy_trsv, whose sticky error word stpy_async_status reports); more than 32
 * (stpy_tune key 34) on the MFMA block solve of stpy_trsm_right_lt.  S = K22 + s^2 I - L21 L21^T (stpy_gemm_nt, lower tiles) is
 * factored by one workgroup for k <= 128 and by stpy_potrf on a padded copy above.  Every sum has a fixed order: bit-reproducible.
 * lda >= n1p (-5), winv_elems >= stpy_potrf_winv_elems(n1p) (-21), work_bytes >= the query (-20); n0 >= 1, k >= 1.
 */
int64_t stpy_potrf_append_workspace_bytes(int dtype, int64_t n0, int64_t k);
int stpy_potrf_append(int dtype, int64_t n0, int64_t k, void* A, int64_t lda, void* winv, int64_t winv_elems, void* z, const void* y,
                      void* work, int64_t work_bytes, int32_t* info_dev, void* stream);

/*
 * Rank-k update (sign = +1) or downdate (sign = -1) of a resident factor in place: KernelizedFeatures.add_data_point(iterative=True),
 * the feature-space counterpart of the bordered factor above (the reference's rank-one Woodbury step on the explicit inverse,
 * kernelized_features.py:213-218).
 *   on entry: the lower triangle of L (n x n, any n >= 1) holds a factor as stpy_potrf leaves it, winv its inverse 128 x 128 diagonal
 *             blocks; W is n x k row-major, ldw >= k (the (m, k) tensor embed_t returns); sign is +1 or -1.
 *   on exit:  L' L'^T = L L^T + sign W W^T with a positive diagonal; EVERY block of winv is refreshed, in the layout stpy_potrf
 *             leaves for the new matrix (identity on the rows / columns of a ragged last tile), so every consumer -- stpy_trsv,
 *             stpy_trsm_right_lt, stpy_potri, stpy_logdet_quad -- runs on (L', winv) unchanged; W is destroyed; the strict upper
 *             triangle of L is neither read nor written; *info_dev = 0, or the 1-based index of the first column whose pivot is not
 *             positive and finite (sign = -1: l_jj^2 - w_j^2 <= 0) -- L is then undefined from that column on and the caller refits.
 * W^T is eliminated against L^T column by column with plane rotations (hyperbolic for sign = -1), all k columns of a chunk of W
 * against column j before column j + 1, in block columns of 128: one workgroup rotates the diagonal block and writes the table of
 * (c, s, 1/c) into `work`, a second launch applies it to the rows below (one row per lane, staged through LDS).  32 columns of W ride
 * along in one pass over L; a wider W is cut into chunks inside the call, each a pass of its own.  One pass reads and writes the
 * lower triangle once: O(n^2 k) work against the O(n^3) of a refactorisation.  Every sum has a fixed order: bit-reproducible.
 * Refused: dtype (-1), n < 0 (-2), k < 0 (-3), sign (-4), NULL L / winv / W / work / info_dev (-5 / -7 / -9 / -11 / -13), ldl < n (-6),
 * ldw < k (-10), winv_elems < stpy_potrf_winv_elems(n) (-21), work_bytes < the query (-20).  n == 0 or k == 0: returns 0, nothing is
 * read or written.
 */
int64_t stpy_chol_update_workspace_bytes(int dtype, int64_t n, int64_t k);
int stpy_chol_update(int dtype, int64_t n, int64_t k, int sign,
                     void* L, int64_t ldl, void* winv, int64_t winv_elems,
                     void* W, int64_t ldw,
                     void* work, int64_t work_bytes, int32_t* info_dev, void* stream);

/*
 * Row deletion: the factor of K[R,R] + s^2 I from the resident factor of K + s^2 I, R the indices that are kept
 * (GaussianProcess.remove_data_point(iterative=True); the reference can only refit).  n1 = n0 - k, n0p / n1p = n0 / n1 rounded up to a
 * multiple of 128.  With S the deleted indices, L[R,R] is lower triangular (R increases) and
 *     K[R,R] + s^2 I = L[R,R] L[R,R]^T + U U^T,   U = L[R,S]   (n1 x k),
 * a rank-k POSITIVE update of the compacted triangle: the rotations of stpy_chol_update with sign = +1, no downdate, no pivot that can
 * fail on finite data.  Rows of U above the first deleted index are zero, so the block columns left of 128 * floor(S[0] / 128) are
 * copied and not rotated; deleting the last rows costs the copy alone, deleting row 0 one pass over L per 32 deleted rows: O(n^2 k)
 * against the O(n^3) of a refit.
 *   del_host: k strictly increasing indices in [0, n0).  This is the ONE HOST pointer of the ABI: the indices decide which device
 *             addresses the gather reads, so they are validated on the host, before any HIP call -- a bad index is refused (-15) and can
 *             never become an out-of-bounds device read, which a device-resident list could not promise without a round trip.  They
 *             reach the head of `work` as kernel arguments (256 per launch on `stream`): the array has been read when the call
 *             returns and may be freed at once, and the call waits for nothing, like every other entry point.
 *   on entry: A (order n0p, lda >= n0p) holds a factor in the tile-padded layout stpy_potrf / stpy_potrf_append leave.
 *   on exit:  B[0:n1p, 0:n1p] (ldb >= n1p) and winv blocks [0, n1p/128) are as stpy_potrf would leave them for the padded K[R,R] + s^2 I:
 *             lower triangle, diagonal tiles whole with zeros above the diagonal, identity on rows / columns [n1, n1p); tiles strictly
 *             above the diagonal are not written.  A is not written.  *info_dev = 0, or the 1-based first column whose pivot is not
 *             finite (non-finite input only).
 * The compaction is out of place (a workgroup's destination rows are other workgroups' source rows): A and B must not overlap (-16).
 * Every sum has a fixed order: bit-reproducible.
 * Refused, before any HIP call: dtype (-1), n0 < 1 (-2), k < 0 or k >= n0 (-3), NULL del_host / A / B / winv / work / info_dev
 * (-4 / -5 / -7 / -9 / -11 / -13), indices out of range, unsorted or repeated (-15), lda < n0p (-6), ldb < n1p (-8), overlapping A and B
 * (-16), winv_elems below the need of order n1p (-21), work_bytes < the query (-20).  k == 0: returns 0, nothing is read or written.
 */
int64_t stpy_potrf_delete_workspace_bytes(int dtype, int64_t n0, int64_t k);
int stpy_potrf_delete(int dtype, int64_t n0, int64_t k, const int32_t* del_host,
                      const void* A, int64_t lda, void* B, int64_t ldb,
                      void* winv, int64_t winv_elems, void* work, int64_t work_bytes,
                      int32_t* info_dev, void* stream);

/* B <- B L^-T for B: m x n row-major (rows = right-hand sides).  With B = K* (M x N) this is
 * V^T = (L^-1 K*^T)^T of the variance term, gauss_procc.py:378,392.  From 2048 rows on: recursive
 * halving of the column range (one long product per split, no workspace).  Fewer rows: panels of nb
 * columns (nb = 0: library default), right-looking, or left-looking when n >= 32768 and `work`
 * (stpy_trsm_workspace_bytes, may be NULL; 0 bytes when not needed) is given, which lets the long panel
 * products run as several K passes so that the latency-bound diagonal blocks of the next panel overlap them. */
int64_t stpy_trsm_workspace_bytes(int dtype, int64_t m, int64_t n, int nb);
int stpy_trsm_right_lt(int dtype, int64_t m, int64_t n, const void* L, int64_t ldl,
                       const void* winv, int64_t winv_elems, void* B, int64_t ldb, int nb, int flags,
                       void* work, int64_t work_bytes, void* stream);

/*
 * Gradient of the evidence (estimator.py:156-190 drives it through
 * autograd in the reference):  d/dtheta [1/2 y^T K^-1 y + w/2 log det K] = 1/2 tr((w K^-1 - alpha alpha^T) dK/dtheta).
 *
 * stpy_potri: Kinv (n x n, lower triangle written) <- (L L^T)^-1 from the factor; work: n x n
 *   elements of scratch (receives L^-T).  2 n^3/3 flop on the MFMA GEMM.
 * stpy_lml_weight: H <- (weight * Kinv - alpha alpha^T) o F, Kinv the full symmetric K^-1 (n x n; Kinv == NULL or
 *   Kinv == H: in place over H; otherwise Kinv is only read, so several kernel terms share one inverse without a
 *   copy); F_ij is the factor of d k(x_i,x_j) / d lengthscale_m = F_ij u_m^2 / lengthscale_m
 *   (u = scaled coordinate difference) for the kernel family `kind` (SE, MATERN12/32/52).
 *   work: stpy_gram_workspace_bytes(dtype, n, n, d).  The per-coordinate sums sum_ij H_ij u_m^2 then
 *   follow from H [Xs | 1] (one stpy_gemm_nt) -- see stpy_amd/continuous_processes/gauss_procc.py.
 *   F comes from the norm expansion of stpy_gram's workspace route (points relative to x_0, same accuracy of r^2).  MATERN12's
 *   F = exp(-r) / r has no value at r = 0: where r^2 is below the rounding noise of the expansion, 16 eps (|x_i'|^2 + |x_j'|^2), the
 *   pair counts as coincident and F_ij = 0 -- what F multiplies, u_m^2 <= r^2, vanishes to the same accuracy.
 */
int stpy_potri(int dtype, int64_t n, const void* L, int64_t ldl, const void* winv, int64_t winv_elems,
               void* Kinv, int64_t ldk, void* work, int64_t work_bytes, void* stream);
int stpy_lml_weight(int kind, int dtype, const void* x, int64_t n, int64_t ldx, int d,
                    const int32_t* cols, const void* inv_ls, double kappa, double weight,
                    const void* alpha, const void* Kinv, int64_t ldk, void* H, int64_t ldh,
                    void* work, int64_t work_bytes, void* stream);

/* out = L^-1 y (trans = 0) or out = L^-T y (trans = 1); the two together are cholesky_solve,
 * estimator.py:37.  y is used as scratch (destroyed); out must not alias y. */
int stpy_trsv(int dtype, int64_t n, const void* L, int64_t ldl, const void* winv, int64_t winv_elems, void* y,
              void* out, int trans, void* stream);

/* mu[i] = <X_i, z>,  sigma[i] = sqrt(kdiag[i] - <X_i, X_i>)   (X = K* L^-T, z = L^-1 y)
 * gauss_procc.py:381, :391-395.  clamp != 0 clamps the variance at 0 before the sqrt (the
 * reference does not clamp).  clamp == 2: sigma[i] receives the raw <X_i, X_i> instead (partial
 * sums of a column-sharded X, reduced across ranks by the caller).  mu or sigma may be NULL. */
int stpy_predict(int dtype, int64_t m, int64_t n, const void* X, int64_t ldx, const void* z,
                 const void* kdiag, void* mu, void* sigma, int clamp, void* stream);

/* The same epilogue when X is sharded by columns across ranks (multi-GPU): stpy_predict(clamp = 2) yields the local
 * partial sums, the caller all-reduces them, and this finishes in place:  mu[i] *= scale,
 * sigma[i] = sqrt(kdiag[i] - scale * sumsq[i])  (scale = 1 / replicas that took part in the sum).  mu / sigma may be NULL. */
int stpy_predict_finish(int dtype, int64_t m, void* mu, const void* sumsq, const void* kdiag, double scale,
                        void* sigma, int clamp, void* stream);

/* out (op)= src elementwise on an m x n window, then + diag_add on the diagonal: the + / * algebra of kernels.py:146-157
 * for an item that was first summed into scratch (combine: STPY_OUT_SET / _ADD / _MUL).  src == out is allowed (with STPY_OUT_SET:
 * "add diag_add to the diagonal in place"). */
int stpy_combine(int dtype, int64_t m, int64_t n, void* out, int64_t ldo, const void* src, int64_t lds,
                 int combine, double diag_add, void* stream);

/* out2[0] = sum_i log L_ii,  out2[1] = z^T z   (estimator.py:36-38, gauss_procc.py:634-636) */
int stpy_logdet_quad(int dtype, int64_t n, const void* L, int64_t ldl, const void* z,
                     void* out2, void* stream);

/* C (op) A B^T with A: m x k, B: n x k, C: m x n.  mode 0: C = A B^T, 1: C -= A B^T, 2: C += A B^T (slab-wise accumulation
 * of Phi^T Phi in the feature-space normal equations, kernelized_features.py:236-240).
 * lower_only: skip 128x128 tiles strictly above the diagonal (m == n).  ldc must be below 2^25 elements (-10).  This is the MFMA
 * contraction under potrf / trsm; exported for the roofline bench and the full-covariance
 * branch gauss_procc.py:396-399. */
int stpy_gemm_nt(int dtype, int64_t m, int64_t n, int64_t k,
                 const void* A, int64_t lda, const void* B, int64_t ldb,
                 void* C, int64_t ldc, int mode, int lower_only, void* stream);

/* C (op) A A^T on the lower 128x128 tiles (A: n x k; mode as above): the feature-space normal equations V (+)= Phi_slab^T Phi_slab
 * (kernelized_features.py:236-240, torch.mm(Phi.T, Phi)).  Same result as stpy_gemm_nt(A, A, lower_only = 1).  With a
 * workspace of stpy_syrk_workspace_bytes(dtype, n, k) bytes (0 = the shape has no such route: fp64, n < 2048, n % 128, k % 32) an fp32
 * operand is split ONCE into three bf16 planes (6 bytes per element of A) and every output tile reads those, instead of every tile
 * re-splitting its rows (gemm_bf3p.hip); work may be NULL.  Few output tiles with a long K (modes 0 and 2) are also cut along K into chunks that
 * run as one grid and are summed in a fixed order (the query then includes the chunk buffers): those results agree with stpy_gemm_nt to fp32
 * rounding, not bit for bit, and are reproducible from run to run. */
int64_t stpy_syrk_workspace_bytes(int dtype, int64_t n, int64_t k);
int stpy_syrk(int dtype, int64_t n, int64_t k, const void* A, int64_t lda, void* C, int64_t ldc, int mode,
              void* work, int64_t work_bytes, void* stream);

/*
 * The same product when C has few 128x128 tiles but k is long (the left-looking partial sums of the
 * distributed solve, gauss_procc.py:368-378 on a sharded factor): the K range is cut into `passes`
 * pieces that run as separate workgroups into `work` (passes*m*n elements, caller-owned) and are
 * then summed into C in a fixed order.  stpy_gemm_nt_splitk_passes recommends the number of passes
 * (1 = use stpy_gemm_nt).  m <= 8 never needs this: stpy_gemm_nt takes a bandwidth-bound row
 * kernel for such products.
 */
int stpy_gemm_nt_splitk_passes(int64_t m, int64_t n, int64_t k);
int stpy_gemm_nt_splitk(int dtype, int64_t m, int64_t n, int64_t k,
                        const void* A, int64_t lda, const void* B, int64_t ldb,
                        void* C, int64_t ldc, int mode, int passes, void* work, int64_t work_bytes, void* stream);

/*
 * The same contraction on a window of a rank's LOCAL matrix under a 2-D block-cyclic distribution
 * (multi-GPU trailing update): distribution block nb_dist (multiple of 128), process grid pr x pc,
 * this rank (myr, myc); the window starts at local block (i0, j0).  A 128x128 tile in local block
 * (bi, bj) belongs to global block (I, J) = (bi*pr + myr, bj*pc + myc) and is skipped when I < J; inside a diagonal
 * block (I == J) only the tiles on and below that block's own diagonal are touched (the symmetric update needs no more).
 * mode as stpy_gemm_nt (0: C = A B^T, 1: C -= A B^T, 2: C += A B^T; anything else: -11).
 */
int stpy_gemm_nt_bc(int dtype, int64_t m, int64_t n, int64_t k,
                    const void* A, int64_t lda, const void* B, int64_t ldb,
                    void* C, int64_t ldc, int mode,
                    int nb_dist, int pr, int pc, int myr, int myc, int i0, int j0, void* stream);

/* mirror the lower triangle into the upper one (n x n) -- materialises .K after a lower-only Gram */
int stpy_symmetrize_lower(int dtype, int64_t n, void* A, int64_t lda, void* stream);

/* zero the strict upper triangle of A (n x n): the in-place factor of stpy_potrf as a proper lower-triangular operand of
 * stpy_gemm_nt -- L r of the samplers (gauss_procc.py:472-474, kernelized_features.py:328-330) */
int stpy_tril(int dtype, int64_t n, void* A, int64_t lda, void* stream);

/* out2[0] = tr(A) (A: n x n; NULL: 0),  out2[1] = <u, v> (n elements each; u NULL: 0) in a fixed summation order -- the scalar
 * tr(w K^-1) - alpha^T alpha of the noise gradient of the evidence (dK/ds = 2 s I), alpha^T y of GaussianProcess.norm
 * (gauss_procc.py:179-184), tr(V^-1) of KernelizedFeatures.effective_dim (kernelized_features.py:103-106) */
int stpy_trace_dot(int dtype, int64_t n, const void* A, int64_t lda, const void* u, const void* v, void* out2, void* stream);

/* out[k*ldo + i] = x[i*ldx + cols[k]] * inv_ls[k] for k < d (cols NULL: k), and out[d*ldo + i] = 1 when ones_row & 1:
 * [Xs | 1]^T, the "row x K" operand of the evidence gradient's H [Xs | 1] product (see stpy_lml_weight). out: (d + (ones_row & 1)) x n.
 * ones_row & 2: the coordinates are taken relative to the first row of x, out[k*ldo + i] = (x[i*ldx + cols[k]] - x[cols[k]]) * inv_ls[k]
 * (subtracted before the scaling): the operand of stpy_lml_grad_reduce_centred (ones_row = 3). */
int stpy_scaled_points_t(int dtype, const void* x, int64_t n, int64_t ldx, int d, const int32_t* cols, const void* inv_ls,
                         void* out, int64_t ldo, int ones_row, void* stream);

/* The last step of the evidence gradient w.r.t. the lengthscales of one kernel term: with P = H [Xs | 1] (n x (d+1), ldp >= d+1),
 *   acc[pidx[k]] += inv_ls[k] * sum_i ( xs_ik^2 P_id - xs_ik P_ik ),   xs_ik = x[i*ldx + cols[k]] * inv_ls[k],   k < d
 * ( = inv_ls[k]/2 * sum_ij H_ij (xs_ik - xs_jk)^2 for the symmetric H of stpy_lml_weight, which is what is evaluated: the sum is formed
 * about the first point, sum_i t_ik^2 P_id - t_ik (P_ik - xs_0k P_id) with t = xs - xs_0, so that its own terms are of the size of the
 * data's extent and not of its distance from the origin ).  pidx: device int32[d], the parameter slot of coordinate k (all zero for an
 * isotropic 'gamma'; NULL: k); acc is accumulated in coordinate order by one workgroup, so the result is reproducible.
 * stpy_lml_grad_reduce_centred: the same sum from P = H [T | 1], T the coordinates relative to the first point (T^T from
 * stpy_scaled_points_t with ones_row = 3): sum_i t_ik^2 P_id - t_ik P_ik.  P = H Xs carries rounding of the size eps |xs| |H|, which the
 * form above cannot remove; this one is as accurate at any offset of the data as on centred data (what GaussianProcess uses). */
int stpy_lml_grad_reduce(int dtype, const void* x, int64_t n, int64_t ldx, int d, const int32_t* cols, const void* inv_ls,
                         const void* P, int64_t ldp, const int32_t* pidx, void* acc, void* stream);
int stpy_lml_grad_reduce_centred(int dtype, const void* x, int64_t n, int64_t ldx, int d, const int32_t* cols, const void* inv_ls,
                                 const void* P, int64_t ldp, const int32_t* pidx, void* acc, void* stream);

/* The same for a full-covariance item (kernels.py:464-549: z = x[:, cols] cov (n x p), then SE / Matern of |z_i - z_j|; the reference differentiates
 * it by autograd).  With H formed by stpy_lml_weight on the mapped points z (unit lengthscales) and P = H [Z | 1] (n x (p+1)):
 *   out[a * p + m] -= sum_i x[i*ldx + cols[a]] * (P[i][p] * z[i*ldz + m] - P[i][m]),   a < dg, m < p      (= d evidence / d cov[a][m])
 * One workgroup, fixed order. */
int stpy_lml_grad_cov_reduce(int dtype, const void* x, int64_t n, int64_t ldx, int dg, const int32_t* cols,
                             const void* z, int64_t ldz, int p, const void* P, int64_t ldp, void* out, void* stream);

/*
 * Batched evidence: value and gradient of gauss_procc.py:631-638 for `batch` hyper-parameter candidates on the SAME data in one launch,
 * one workgroup per candidate -- the restarts of a hyper-parameter search (optimize_params(parallel=True), gauss_procc.py:642), which the
 * serial path evaluates one after another at ten launches and two host read-backs each.  One kernel term k = kappa phi (SE, MATERN12 / 32 / 52;
 * anything else is refused), float64 only (float32: -2, the caller takes the serial path), n <= stpy_lml_batch_max_n() (512).
 * Candidate b has the inverse lengthscales inv_ls[b*ldi + k] (k < d) and the noise std noise[b]; x (n x ldx, columns cols[k] or k), y (n), kappa
 * and weight are shared.  With K_b = kappa phi(|(x_i - x_j)[cols] o inv_ls_b|) + noise_b^2 I = L L^T, alpha = K_b^-1 y:
 *   value[b]           = 1/2 y^T K_b^-1 y + weight * sum_i log L_ii                       (what stpy_logdet_quad yields on the serial path)
 *   grad[b*ldg + p]    = 1/2 sum_ij (weight K_b^-1 - alpha alpha^T)_ij kappa F_ij sum_{k: pidx[k] = p} u_k^2 inv_ls_b[k],   p < np
 *                        (F, u as for stpy_lml_weight; F_ij = 0 on coincident points for MATERN12; pidx: device int32[d], values in [0, np))
 *   grad[b*ldg + np]   = noise_b (weight tr K_b^-1 - alpha^T alpha)                        (d / d noise std; ldg >= np + 1)
 *   info[b]            = 0, or the 1-based index of the first pivot that is not positive and finite: then value[b] = +inf and the
 *                        gradient row is zero -- a numerical failure of ONE candidate, reported per candidate, the others are unaffected.
 * K_b is filled from direct coordinate differences (kappa (d + 8) eps wherever the data lies: no norm expansion, no common shift), factored
 * by a blocked Cholesky in the candidate's slice of `work` (stpy_lml_batch_workspace_bytes(dtype, n, d, batch) bytes, 16-byte aligned; about
 * 16 n^2 bytes per candidate), inverted through L^-1, and the gradient sums run over K_b^-1 entry by entry.  Every sum has a fixed order
 * and no candidate reads another's data: a candidate's outputs are bit-identical whatever else is in the batch and wherever it sits in it.
 * One launch on `stream`, no host synchronisation, no allocation.
 * Refused before any HIP call: kind (-1), dtype (-2), NULL x / y / inv_ls / noise / pidx / value / grad / info / work (-3), n > the cap (-4),
 * ldx < d (-5), d < 1 (-6), ldi < d (-11), np < 1 (-16), ldg < np + 1 (-19), work_bytes below the query (-20).  n == 0 or batch == 0: returns 0,
 * nothing is read or written.
 */
int64_t stpy_lml_batch_max_n(void);
int64_t stpy_lml_batch_workspace_bytes(int dtype, int64_t n, int d, int64_t batch);
int stpy_lml_batch(int kind, int dtype, const void* x, int64_t n, int64_t ldx, int d, const int32_t* cols,
                   const void* y, int64_t batch, const void* inv_ls, int64_t ldi,
                   const void* noise, double kappa, double weight,
                   const int32_t* pidx, int np,
                   void* value, void* grad, int64_t ldg, int32_t* info,
                   void* work, int64_t work_bytes, void* stream);

/*
 * Local GP experts (LocalExpertsGaussianProcess; Deisenroth and Ng 2015; the reference has no counterpart): E exact GPs on E blocks of the data
 * under ONE hyper-parameter candidate -- the arithmetic of stpy_lml_batch with the roles of data and candidate exchanged, the factor kept for
 * prediction.  One kernel term k = kappa phi (SE, MATERN12 / 32 / 52), float64 only (float32: -2); cols, inv_ls (device, d values), kappa as for
 * stpy_pchol; noise: device, ONE noise std.  With cols the rows of xs AND of xt are the wide rows: coordinate k of a training point is
 * xs[i*ldx + cols[k]], of a test point xt[t*ldt + cols[k]] (ldx, ldt above the largest entry of cols; the other columns are never read).
 * The points are gathered by expert: xs (N x ldx), ys (N), offsets: device int32[E + 1], expert e owns
 * rows offsets[e] .. offsets[e + 1], n_e <= nmax <= stpy_experts_max_n() (512) of them.  nmax is the host's bound on n_e, by which the slices are
 * sized: an expert that violates it (info[e] = -1), or whose offsets leave [0, N] or decrease (info[e] = -2), is reported and nothing is written
 * out of bounds.  With NPM = nmax rounded up to 32, `factor` holds E slices of NPM^2 doubles (stpy_experts_factor_bytes, 16-byte aligned, owned
 * by the caller from the fit to the predictions), `work` of the fit E slices of NPM^2 + 32 NPM doubles, `work` of the prediction 32 NPM doubles
 * per expert and tile of 32 test points.
 *
 * stpy_experts_fit: one workgroup per expert, then one small launch for the totals.  With K_e = kappa phi + noise^2 I = L_e L_e^T on the expert's rows:
 *   factor slice e     = V_e = L_e^-T, upper triangular, row-major with row stride NP_e = n_e rounded up to 32, bordered by an identity; below
 *                      the diagonal only the 32 x 32 diagonal blocks and the blocks just below them are written (zeros), the rest is not touched
 *   alpha[offsets[e]..] = K_e^-1 y_e
 *   value[e]           = 1/2 y_e^T alpha_e + weight * sum_i log (L_e)_ii
 *   grad[e*ldg + p]    (grad != NULL; p < np lengthscale slots by pidx, p = np the noise std; ldg >= np + 1) by the formulas of stpy_lml_batch;
 *                      grad == NULL skips the K_e^-1 and H passes, pidx and np are then unused
 *   info[e]            = 0, or the 1-based index of the first pivot that is not positive and finite: then value[e] = +inf, alpha_e = 0 and the
 *                      gradient row is zero; the other experts are unaffected
 *   total[0]           = sum_e value[e];  total[1 + p] = sum_e grad[e*ldg + p], p <= np (with a gradient; total: np + 2 doubles), in expert order
 * stpy_experts_predict: one launch, one workgroup per (expert, tile of 32 test points xt: M x ldt).  k* from direct coordinate differences with
 * the evaluator of the fit (the same bits on a training point);
 *   mu_e[e*ldm + t]    = k*^T alpha_e
 *   var_e[e*ldm + t]   = kappa - |L_e^-1 k*|^2, L_e^-1 k* on the fp64 MFMA from the stored factor (a variance of the latent f: no noise term)
 * an expert with info[e] != 0 (the array the fit wrote) yields mu_e = 0, var_e = kappa.  ldm >= M.
 * stpy_experts_combine: one thread per test point, sums over experts in expert order; each var_e is first clamped to [kappa 2^-52, kappa];
 * with c_e = 1 / var_e:   mode 0 PoE: beta_e = 1;  1 gPoE: beta_e = 1 / E;  2 BCM: beta_e = 1;  3 rBCM: beta_e = 1/2 (log kappa - log var_e);
 *   1 / var = sum beta_e c_e  (+ (1 - E) / kappa for BCM, + (1 - sum beta_e) / kappa for rBCM),   mu = var * sum beta_e c_e mu_e
 * stpy_experts_predict_grad: stpy_experts_predict with the input gradients of every expert's mean and variance, same grid, one launch.  mu_e and
 * var_e carry the bits stpy_experts_predict writes (the two kernels call one body).  The gradients are compact arrays over the SELECTED
 * coordinates, in cols order: entry (e, t, m) at e*lde + t*ldg + m, m < d, ldg >= d, lde >= M*ldg.  With F the derivative factor of the term
 * (d k / d r^2 = -kappa F / 2: SE exp(-r^2/2), Matern 1/2 exp(-r)/r, 3/2 3 exp(-sqrt3 r), 5/2 5/3 (1 + sqrt5 r) exp(-sqrt5 r)), il = inv_ls
 * and w = K_e^-1 k* = L_e^-T (L_e^-1 k*), the second triangular product on the fp64 MFMA as the first:
 *   gmu_e[e, t, m]     = -kappa il_m^2 sum_k alpha_k F_tk (xt_m - x_km)
 *   gvar_e[e, t, m]    = 2 kappa il_m^2 sum_k w_tk F_tk (xt_m - x_km)          (d k(x, x) / dx = 0: the term is stationary)
 * from direct coordinate differences, subtracted before they are scaled.  Matern 1/2 on a coincident pair (r = 0 exactly) contributes zero, the
 * convention of stpy_gram_grad.  An expert with info[e] != 0 yields mu_e = 0, var_e = kappa and zero gradients.  Rows t >= M are never written.
 * `work`: TWO slices of 32 NPM doubles per expert and tile (the k* tile, over which w is written, and L_e^-1 k*): twice the bytes of the
 * prediction's query.
 * stpy_experts_combine_grad: stpy_experts_combine (the same bits in mu and var) with the chain rule on top, one thread per test point, experts in
 * expert order.  Per selected coordinate, with v_e = clamp(var_e), c_e = 1 / v_e:
 *   dv_e    = gvar_e where kappa 2^-52 <= var_e <= kappa, else 0: the derivative of the function as implemented; on the ties var_e == kappa and
 *             var_e == kappa 2^-52 the clamp counts as inactive
 *   dc_e    = -c_e^2 dv_e;   dbeta_e = -dv_e / (2 v_e) for rBCM, 0 otherwise
 *   dprec   = sum (dbeta_e c_e + beta_e dc_e)  (- sum dbeta_e / kappa for rBCM);   dwm = sum [(dbeta_e c_e + beta_e dc_e) mu_e + beta_e c_e gmu_e]
 *   dvar    = -var^2 dprec;   dmu[t*ldo + m] = dvar wm + var dwm  (wm = sum beta_e c_e mu_e);   dstd[t*ldo + m] = dvar / (2 sqrt(var)),  ldo >= d
 * It reads nothing but its arguments: a pure function of (mode, mu_e, var_e, gmu_e, gvar_e, kappa).
 * Every sum has a fixed order, there are no atomics, spin-waits or cooperative grids, no host synchronisation and no allocation: two calls are
 * bit-identical, and an expert's outputs are bit-identical wherever it sits in whatever batch.
 * Refused before any HIP call: kind (-1), dtype (-2), a NULL array (-3; cols may be NULL, grad may be NULL, pidx with it), nmax above the cap (-4),
 * ldx or ldt < d (-5), d < 1 (-6), N / E / M out of range (-9), combine mode (-10), kappa not positive and finite (-11), ldm < M (-13), np < 1
 * with a gradient (-16), ldg < np + 1 (fit) or ldg < d, ldo < d, lde < M*ldg (the input gradients) (-19), work_bytes below the query (-20),
 * misalignment (-21), factor_bytes below its query (-22).
 * E == 0, N == 0 (or M == 0): returns 0, nothing is read or written.
 */
int64_t stpy_experts_max_n(void);
int64_t stpy_experts_factor_bytes(int dtype, int64_t nmax, int64_t E);
int64_t stpy_experts_fit_workspace_bytes(int dtype, int64_t nmax, int d, int64_t E);
int stpy_experts_fit(int kind, int dtype, const void* xs, int64_t N, int64_t ldx, int d, const int32_t* cols, const void* ys,
                     const int32_t* offsets, int64_t E, int64_t nmax,
                     const void* inv_ls, const void* noise, double kappa, double weight,
                     const int32_t* pidx, int np,
                     void* factor, int64_t factor_bytes, void* alpha, void* value, void* grad, int64_t ldg, void* total, int32_t* info,
                     void* work, int64_t work_bytes, void* stream);
int64_t stpy_experts_predict_workspace_bytes(int dtype, int64_t nmax, int d, int64_t E, int64_t M);
int stpy_experts_predict(int kind, int dtype, const void* xs, int64_t N, int64_t ldx, int d, const int32_t* cols,
                         const int32_t* offsets, int64_t E, int64_t nmax, const void* inv_ls, double kappa,
                         const void* factor, int64_t factor_bytes, const void* alpha, const int32_t* info,
                         const void* xt, int64_t M, int64_t ldt,
                         void* mu_e, void* var_e, int64_t ldm,
                         void* work, int64_t work_bytes, void* stream);
int stpy_experts_combine(int mode, int64_t E, int64_t M, const void* mu_e, const void* var_e, int64_t ldm, double kappa,
                         void* mu, void* var, void* stream);
int64_t stpy_experts_predict_grad_workspace_bytes(int dtype, int64_t nmax, int d, int64_t E, int64_t M);
int stpy_experts_predict_grad(int kind, int dtype, const void* xs, int64_t N, int64_t ldx, int d, const int32_t* cols,
                              const int32_t* offsets, int64_t E, int64_t nmax, const void* inv_ls, double kappa,
                              const void* factor, int64_t factor_bytes, const void* alpha, const int32_t* info,
                              const void* xt, int64_t M, int64_t ldt,
                              void* mu_e, void* var_e, int64_t ldm,
                              void* gmu_e, void* gvar_e, int64_t ldg, int64_t lde,
                              void* work, int64_t work_bytes, void* stream);
int stpy_experts_combine_grad(int mode, int64_t E, int64_t M, int d, const void* mu_e, const void* var_e, int64_t ldm,
                              const void* gmu_e, const void* gvar_e, int64_t ldg, int64_t lde, double kappa,
                              void* mu, void* var, void* dmu, void* dstd, int64_t ldo, void* stream);

/*
 * Local GP experts, routed prediction: every test point asks only its k nearest experts, nearest by the distance to the experts' centroids in
 * scaled coordinates.  The (expert, point) pairs of a prediction drop from E M to k M, whatever N is.  xs, offsets, cols, inv_ls, kappa, factor,
 * alpha, info, xt as for stpy_experts_predict; float64 only.
 *
 * stpy_experts_centroids: one wave per expert,
 *   cent[e*ldc + m]    = (sum over the expert's rows, in row order, of xs[i*ldx + cols[m]] * inv_ls[m]) / n_e,   m < d, ldc >= d
 * An expert without rows, or whose offsets leave [0, N] or decrease, gets +inf in every coordinate: it is never nearer than an expert with rows.
 * stpy_experts_route: one wave per test point.  D_e = sum_m (xt[t*ldt + cols[m]] * inv_ls[m] - cent[e*ldc + m])^2, m ascending, capped at
 * DBL_MAX (a NaN counts as DBL_MAX); D_e = +inf where cent[e*ldc] is +inf.  The k experts with the smallest D_e are selected, ties going to the
 * lower expert id (so experts without rows come last, by id), and written ASCENDING IN EXPERT ID:
 *   sel[t*k + j]       int32, j < k, sel[t*k] < sel[t*k + 1] < ...
 * so that a combination over the k slots keeps the experts' order.  1 <= k <= min(E, stpy_experts_route_max_k()); the cap is 16: a lane of the
 * routing kernel holds its candidates as a sorted list in registers.  E is not bounded by the kernel (lanes stride over the experts).
 * stpy_experts_predict_routed / _predict_routed_grad: stpy_experts_predict / _predict_grad on a WORK LIST of T tiles in place of the grid of
 * E x ceil(M / 32) tiles.  Tile w belongs to expert wexp[w] (device int32[T]) and its column c to pair wpair[32 w + c] = t*k + j (device
 * int32[32 T]): test point t < M, slot j < k of its selection.  wexp[w] outside [0, E): the tile is unused; a pair id outside [0, M k), -1 by
 * convention: the column is empty.  Whatever the two arrays hold, nothing is written out of bounds; a pair listed twice is computed twice, with
 * the same bits.  The caller builds the list from sel on the device (a stable sort of the pair ids by expert, counts, running sums of
 * ceil(count / 32), a scatter); T = floor(M k / 32) + min(E, M k) tiles always suffice.  The results of pair (t, j) go to slot j of point t:
 *   mu_s[j*ldm + t], var_s[j*ldm + t]                         (k x ldm, ldm >= M)
 *   gmu_s[j*lde + t*ldg + m], gvar_s[j*lde + t*ldg + m]       (k x M x d, ldg >= d, lde >= M*ldg)
 * exactly the layout stpy_experts_combine / _combine_grad read with E := k, so those two are the combination of a routed prediction as they
 * stand -- with the consequence that gPoE's beta is 1 / k and BCM's correction (1 - k) / kappa.  Slots of pairs the list does not hold are not
 * written.  An expert with info[e] != 0, without rows or mis-sized puts the prior into its slots (mu 0, var kappa, zero gradients).
 * Bit contract: the four kernels run ONE body, every sum of which runs over an expert's rows for one fixed test point: the entries at (j, t)
 * carry the bits stpy_experts_predict / _predict_grad write at (sel[t*k + j], t); with k = E the routed prediction is the unrouted one.
 * `work`: 32 NPM doubles per tile (T * 32 * NPM in all), twice that with gradients; the queries take T.
 * The gradients are those of the function computed WITH THE SELECTION HELD FIXED: the routed posterior is piecewise smooth and jumps where the
 * k-th and the (k + 1)-th nearest expert of a point swap.
 * No atomics, fixed summation orders: two calls are bit-identical.  Refused before any HIP call, with the codes of the block above, plus: k
 * outside [1, min(E, cap)] (-23); M k or T at or above 2^31 (-9); ldc < d (-5).  E == 0, M == 0, T == 0 (or N == 0 for the predictions):
 * returns 0, nothing is read or written.
 */
int64_t stpy_experts_route_max_k(void);
int stpy_experts_centroids(int dtype, const void* xs, int64_t N, int64_t ldx, int d, const int32_t* cols, const int32_t* offsets, int64_t E,
                           const void* inv_ls, void* cent, int64_t ldc, void* stream);
int stpy_experts_route(int dtype, const void* cent, int64_t ldc, int64_t E, int d, const int32_t* cols, const void* inv_ls,
                       const void* xt, int64_t M, int64_t ldt, int k, int32_t* sel, void* stream);
int64_t stpy_experts_predict_routed_workspace_bytes(int dtype, int64_t nmax, int d, int64_t T);
int stpy_experts_predict_routed(int kind, int dtype, const void* xs, int64_t N, int64_t ldx, int d, const int32_t* cols,
                                const int32_t* offsets, int64_t E, int64_t nmax, const void* inv_ls, double kappa,
                                const void* factor, int64_t factor_bytes, const void* alpha, const int32_t* info,
                                const void* xt, int64_t M, int64_t ldt,
                                int k, const int32_t* wexp, const int32_t* wpair, int64_t T,
                                void* mu_s, void* var_s, int64_t ldm,
                                void* work, int64_t work_bytes, void* stream);
int64_t stpy_experts_predict_routed_grad_workspace_bytes(int dtype, int64_t nmax, int d, int64_t T);
int stpy_experts_predict_routed_grad(int kind, int dtype, const void* xs, int64_t N, int64_t ldx, int d, const int32_t* cols,
                                     const int32_t* offsets, int64_t E, int64_t nmax, const void* inv_ls, double kappa,
                                     const void* factor, int64_t factor_bytes, const void* alpha, const int32_t* info,
                                     const void* xt, int64_t M, int64_t ldt,
                                     int k, const int32_t* wexp, const int32_t* wpair, int64_t T,
                                     void* mu_s, void* var_s, int64_t ldm,
                                     void* gmu_s, void* gvar_s, int64_t ldg, int64_t lde,
                                     void* work, int64_t work_bytes, void* stream);

/*
 * Greedy pivoted partial Cholesky of the kernel matrix K_il = kappa phi(|(x_i - x_l)[cols] o inv_ls|), columns generated on the fly: the landmark
 * choice of NystromFeatures(approx="pivoted") (the reference's nystrom_fea.py has uniform / leverage sampling only).  K is never formed:
 * O(n m) memory, O(n m^2) work.  kind, cols, inv_ls, kappa as for stpy_gram; SE and MATERN12 / 32 / 52 only.  Kernel values come from direct
 * coordinate differences, as in stpy_lml_batch: kappa (d + 8) eps wherever the data lies, exactly kappa on coincident points.
 *   start:   dres[i] = kappa for every i < n.
 *   step j = 0 .. m-1:  p = argmax_i dres[i], ties to the LOWEST index; dres[p] <= tol * kappa or dres[p] <= 0 stops with rank r = j; otherwise
 *            piv[j] = p,  Ft[j*ldf + i] = (K_ip - sum_{l<j} Ft[l*ldf + i] Ft[l*ldf + p]) / sqrt(dres[p]),  dres[i] -= Ft[j*ldf + i]^2,  dres[p] = 0 exactly.
 *   on exit: *rank_dev = r; rows [r, m) of Ft are zero; piv[r:m) = -1; dres (n elements) is the residual diagonal diag(K - F F^T), exactly 0 on the
 *            pivots, whose sum is the trace-norm error of the approximation; the pivots are pairwise distinct.
 * Ft is m x n (ldf >= n): row j is column j of the factor F, the "row x K" operand stpy_syrk and stpy_gemm_nt take.  piv: device int32[m].
 * m <= min(n, 8192).  The cap is the launch count of one call, not a memory budget: a step is one launch, and the values Ft[0:j, p] a step needs
 * pass through LDS in chunks of 1024, so LDS sets no limit on m.
 * One enqueue sequence on `stream` (m + 2 launches), no host synchronisation, no allocation: the stop is the device word *rank_dev, and the
 * launches after it return on reading it.  No workgroup waits for another inside a launch (no spin-waits, no cooperative grid, no atomics):
 * every workgroup owns a tile of points, reduces the per-tile (value, index) argmaxes of the previous launch in `work` -- all arrive at the same
 * p --, streams its tile's rows of Ft with 16-byte loads per lane (when Ft is 16-byte aligned and ldf a multiple of 16 bytes; element-wise
 * otherwise, same results) and writes its own argmax to the other half of `work`.  Every sum has a fixed order: two calls on the same input
 * are bit-identical.  Step j reads j * n elements; a run of rank r reads esz * n * r (r - 1) / 2 bytes, a streaming read whose ceiling is HBM
 * once Ft outgrows the Infinity Cache.
 * Refused before any HIP call: kind (-1), dtype (-2), NULL x / inv_ls / Ft / dres / piv / rank_dev / work (-3), n < 0 or n >= 2^31 (-4), ldx < d (-5),
 * d < 1 (-6), m < 1, m > n or m > 8192 (-10), tol negative or not finite (-11), ldf < n (-13), work not 8-byte aligned (-17), work_bytes below
 * stpy_pchol_workspace_bytes(dtype, n, d, m) (-20).  n == 0: returns 0, nothing is read or written.
 */
int64_t stpy_pchol_workspace_bytes(int dtype, int64_t n, int d, int64_t m);
int stpy_pchol(int kind, int dtype, const void* x, int64_t n, int64_t ldx, int d, const int32_t* cols, const void* inv_ls,
               double kappa, int64_t m, double tol,
               void* Ft, int64_t ldf, void* dres, int32_t* piv, int32_t* rank_dev,
               void* work, int64_t work_bytes, void* stream);

/*
 * Kernel matrix times a block of vectors, the matrix never formed (IterativeGaussianProcess; the reference has no matrix-free route):
 *   Yt[c*ldy + i] = sum_{j<q} kappa phi(|(a_i - b_j)[cols] o inv_ls|) Vt[c*ldv + j] + diag_add Vt[c*ldv + i],     c < t, i < n
 * kind, cols, inv_ls, kappa as for stpy_pchol; SE and MATERN12 / 32 / 52 only.  Block vectors are stored TRANSPOSED, one right-hand side per row
 * (Vt: t x q, Yt: t x n): the orientation KernelFunction._kernel_into writes and the "row x K" operand of stpy_gemm_nt.  Yt must not overlap Vt.
 * Kernel values come from direct coordinate differences with the evaluator of stpy_pchol (the same bits): kappa (d + 8) eps wherever the data
 * lies, exactly kappa on coincident points; with a == b the operator is bitwise symmetric and is the one a stpy_pchol factor was built from.
 * diag_add != 0 needs q == n: the caller states that a and b are the same points.
 * A workgroup owns 64 output points and walks j in a fixed order; on the 16x16x4 MFMA a lane evaluates the one kernel value its B operand
 * wants, and up to 64 right-hand sides share an evaluation.  With too few output tiles to fill the chip the j range is cut into pieces whose
 * partial sums pass through `work` and are added in piece order: no atomics, no spin-waits, no cooperative grid.  Two calls on the same input are
 * bit-identical, and ldv / ldy do not change a bit.  One or two launches, no host synchronisation, no allocation.
 * Refused before any HIP call: kind (-1), dtype (-2), NULL a / b / inv_ls / Vt / Yt (-3), n or q negative or >= 2^31 (-4), lda or ldb < d (-5),
 * d < 1 (-6), t < 1 (-10), kappa or diag_add not finite (-11), diag_add != 0 with q != n (-12), ldv < q or ldy < n (-13), work not 8-byte aligned
 * (-17), work NULL or work_bytes below stpy_kmv_workspace_bytes(dtype, n, q, d, t) (-20; the query does not decrease in n, q or t).
 * n == 0: returns 0, nothing is read or written.  q == 0: Yt = 0.
 */
int64_t stpy_kmv_workspace_bytes(int dtype, int64_t n, int64_t q, int d, int64_t t);
int stpy_kmv(int kind, int dtype,
             const void* a, int64_t n, int64_t lda,
             const void* b, int64_t q, int64_t ldb,
             int d, const int32_t* cols, const void* inv_ls, double kappa, double diag_add,
             const void* Vt, int64_t t, int64_t ldv,
             void* Yt, int64_t ldy,
             void* work, int64_t work_bytes, void* stream);

/*
 * Block preconditioned conjugate gradients on the operator of stpy_kmv: (K(x, x) + diag_add I) X_c = B_c for t independent columns, the rows of
 * Bt / Xt (t x n).  Preconditioner M^-1 = I - G G^T with G (n x r) given as Gn (n x r, ldgn >= r) AND as its transpose Gt (r x n, ldgt >= n), so
 * that both products are NT products on the library's MFMA contraction; with C = s^2 I + F^T F = L L^T and G = F L^-T this is s^2 times the
 * Woodbury inverse of s^2 I + F F^T (F a stpy_pchol factor) -- a constant factor on M^-1 does not change the iterates.  r == 0: plain CG.
 * One call enqueues exactly `iters` iterations (one stpy_kmv, two products, two vector kernels each): no host synchronisation, no allocation.  The
 * state (R, P, Z, Q, the per-column scalars) lives in `work` and persists between calls: init != 0 starts from X = 0, init == 0 continues, and k
 * calls of 10 iterations give the bits of one call of 10 k.  Dot products are accumulated in double in a fixed order, one workgroup per column.
 * A column with |R_c| <= tol |B_c| (recurrence residual) is frozen: its X, R and its[c] never change again.  A zero column: X = 0, its = 0,
 * relres = 0.  A column whose curvature <P_c, A P_c> (or <R_c, M^-1 R_c>) is not positive and finite is frozen with its[c] = -(iteration), X at
 * the last good iterate.  Written after the last iteration of the call (elements of the matrix type): relres[c] = |R_c| / |B_c|, bx[c] = <B_c, X_c>;
 * its[c]: device int32.
 * Refused before any HIP call: as stpy_kmv (kind -1, dtype -2, NULL x / inv_ls / Bt / Xt / relres / bx / its -3, n -4, ldx < d -5, d < 1 -6, t < 1
 * -10, kappa / diag_add -11), ldb or ldxt < n (-13), tol negative or not finite (-14), iters < 0 (-15), r < 0 (-16), r > 0 with NULL Gt / Gn (-3),
 * ldgt < n or ldgn < r (-18), work not 16-byte aligned (-17), work NULL or below stpy_pcg_workspace_bytes(dtype, n, d, t, r) (-20).  n == 0: returns 0.
 */
int64_t stpy_pcg_workspace_bytes(int dtype, int64_t n, int d, int64_t t, int64_t r);
int stpy_pcg(int kind, int dtype, const void* x, int64_t n, int64_t ldx, int d, const int32_t* cols, const void* inv_ls,
             double kappa, double diag_add,
             const void* Gt, int64_t ldgt, const void* Gn, int64_t ldgn, int64_t r,
             const void* Bt, int64_t ldb, void* Xt, int64_t ldxt, int64_t t,
             double tol, int iters, int init,
             void* relres, void* bx, int32_t* its,
             void* work, int64_t work_bytes, void* stream);

/*
 * stpy_pcg that also records what the stochastic Lanczos quadrature of IterativeGaussianProcess.log_marginal_estimate needs: the CG scalars are
 * the Lanczos coefficients of the preconditioned operator.  Same arguments, same workspace query, same kernels, launch sequence and bits in Xt,
 * relres, bx and its as stpy_pcg; in addition, for column c and iteration it (1-based, as counted by its[c]):
 *   coef[(c*cap + it-1)*2 + 0] = the step length as applied (the value cast to the matrix type, stored as a double), written by the step kernel;
 *   coef[(c*cap + it-1)*2 + 1] = the ratio <R, Z>' / <R, Z> applied to the direction AFTER iteration it, written by the direction kernel;
 *   rz0[c] = <B_c, M^-1 B_c>, written by the first direction kernel (init != 0).
 * coef: t * cap * 2 doubles, rz0: t doubles, both on the device.  Slots at and beyond its[c] are left untouched, a frozen column writes nothing
 * (so the ratio after the iteration on which a column converged is not written), and iterations beyond cap write nothing: the host sizes cap =
 * its iteration limit.  init == 0 continues filling, so that blocks of iterations give the coefficients of one long call.
 * With a_j, b_j the two entries of slot j-1 and m = its[c], the Lanczos matrix is the symmetric tridiagonal T (m x m) with T[0,0] = 1 / a_1,
 * T[j,j] = 1 / a_(j+1) + b_j / a_j and T[j,j+1] = sqrt(b_(j+1)) / a_(j+1).
 * Refused before any HIP call: cap < 1 (-19), NULL coef or rz0 (-3), then everything stpy_pcg refuses.
 */
int stpy_pcg_lanczos(int kind, int dtype, const void* x, int64_t n, int64_t ldx, int d, const int32_t* cols, const void* inv_ls,
                     double kappa, double diag_add,
                     const void* Gt, int64_t ldgt, const void* Gn, int64_t ldgn, int64_t r,
                     const void* Bt, int64_t ldb, void* Xt, int64_t ldxt, int64_t t,
                     double tol, int iters, int init,
                     void* relres, void* bx, int32_t* its,
                     double* coef, int64_t cap, double* rz0,
                     void* work, int64_t work_bytes, void* stream);

/*
 * Bilinear forms of the hyper-parameter derivative of the kernel matrix of stpy_kmv (a == b == x), the matrix never formed: for every pair of
 * rows c < t of Ut / Vt (t x n), with e_ijk = (x_i - x_j)[cols[k]] * inv_ls[k] (difference first, scale second), rho_ij = sum_k e_ijk^2 (fma, in
 * coordinate order), phi the kernel profile of stpy_pchol and chi = 2 dphi/drho (SE: -exp(-rho/2); MATERN12: -exp(-r)/r; MATERN32:
 * -3 exp(-sqrt3 r); MATERN52: -(5/3)(1 + sqrt5 r) exp(-sqrt5 r); r = sqrt(rho)):
 *   out[c*ldo + k]     = sum_i sum_j Ut[c,i] Vt[c,j] kappa chi(rho_ij) e_ijk^2      k < d     (d(u^T K v) / d inv_ls[k] = out[c,k] / inv_ls[k])
 *   out[c*ldo + d]     = sum_i sum_j Ut[c,i] Vt[c,j] kappa phi(rho_ij)                        (u^T K v; d / dkappa = out[c,d] / kappa)
 *   out[c*ldo + d + 1] = sum_i Ut[c,i] Vt[c,i]                                                (d(K + s^2 I) / ds = 2 s I)
 * A pair with rho == 0 contributes exactly 0 to the first d outputs (no 0 / 0 for MATERN12).  kind, cols, inv_ls, kappa as for stpy_kmv.
 * A workgroup owns 64 points i and 16 pairs c and walks j in a fixed order; on the 16x16x4 MFMA a lane evaluates rho, phi, chi and the d squares
 * of the one pair (i, j) its B operand wants and issues d + 1 matrix instructions against the same fragment of Vt.  Coordinates stay in
 * registers up to d = 16 (instantiations for 4, 8, 16); beyond, a workgroup owns the outputs of one group of 16 coordinates.  One partial row per
 * workgroup passes through `work`; a second launch adds them in a fixed order (and, with too few workgroups to fill the chip, the pieces the j
 * range was cut into): no atomics, no spin-waits, no cooperative grid.  Two calls give the same bits, and ldu / ldv / ldo do not change a bit.
 * Two launches, no host synchronisation, no allocation.
 * Refused before any HIP call: kind (-1), dtype (-2), NULL x / inv_ls / Ut / Vt / out (-3), n negative or >= 2^31 (-4), ldx < d (-5), d < 1 (-6),
 * t < 1 or more than 65535 blocks of 16 pairs x ceil(d / 16) coordinate groups (-10), kappa not finite (-11), ldu or ldv < n or ldo < d + 2 (-13),
 * work not 8-byte aligned (-17), work NULL or work_bytes below stpy_kmv_dtheta_workspace_bytes(dtype, n, d, t) (-20).
 * n == 0: returns 0, out[c, 0 .. d + 1] = 0 (only out is looked at).
 */
int64_t stpy_kmv_dtheta_workspace_bytes(int dtype, int64_t n, int d, int64_t t);
int stpy_kmv_dtheta(int kind, int dtype, const void* x, int64_t n, int64_t ldx, int d, const int32_t* cols, const void* inv_ls, double kappa,
                    const void* Ut, int64_t ldu, const void* Vt, int64_t ldv, int64_t t,
                    void* out, int64_t ldo, void* work, int64_t work_bytes, void* stream);

/*
 * Values and query-point gradients of kernel sums, the kernel matrix never formed: n query points a (n x lda), q contracted points b (q x ldb) and
 * t coefficient rows Vt (t x q, ldv >= q).  With e_ijk = (a_i - b_j)[cols[k]] * inv_ls[k] (difference first, scale second), rho_ij = sum_k e_ijk^2
 * (fma, in coordinate order), phi and chi = 2 dphi/drho as for stpy_kmv_dtheta:
 *   out[c*ldc + i*ldo + k] = inv_ls[k] * sum_j Vt[c,j] kappa chi(rho_ij) e_ijk        k < d     (d / d a_i[cols[k]] of the next line)
 *   out[c*ldc + i*ldo + d] =             sum_j Vt[c,j] kappa phi(rho_ij)                         (the value stpy_kmv returns, the same kernel bits)
 * ldo >= d + 1 is the stride between query points and ldc >= n * ldo the stride between coefficient rows, both in elements: any (t, n, d + 1)
 * window with a unit last stride.  Gradient columns are compact, in the order of cols (the caller scatters them).  A pair with rho == 0 contributes exactly 0 to the first d outputs
 * (no 0 / 0 for MATERN12).  kind, cols, inv_ls, kappa as for stpy_kmv.  Vt = alpha^T gives the posterior mean and its input gradient; the rows of a
 * pathwise-conditioning solve give the data term of t posterior draws.
 * The launch shape of stpy_kmv_dtheta: a workgroup owns 64 query points and 16 rows c and walks j in a fixed order; on the 16x16x4 MFMA a lane
 * evaluates rho, phi, chi and the d differences of the one pair (i, j) its B operand wants and issues d + 1 matrix instructions against the same
 * fragment of Vt.  Coordinates stay in registers up to d = 16 (instantiations for 4, 8, 16); beyond, a workgroup owns the columns of one group of 8
 * coordinates.  The D tile is stored per query point (no reduction over i).  With too few workgroups to fill the chip the j range is cut into
 * pieces whose tiles pass through `work` and are added in piece order by a second launch: no atomics, no spin-waits, no cooperative grid.  Two
 * calls give the same bits, and lda / ldb / ldv / ldc / ldo do not change a bit.  At most two launches, no host synchronisation, no allocation.
 * Refused before any HIP call: kind (-1), dtype (-2), NULL a / inv_ls / out, or NULL b / Vt with q > 0 (-3), n or q negative or >= 2^31 (-4), lda or
 * ldb < d (-5), d < 1 (-6), t < 1 or more than 65535 blocks of 16 rows x coordinate groups (-10), kappa not finite (-11), ldv < q (-13), work not
 * 8-byte aligned (-17), work NULL or work_bytes below stpy_kmv_dx_workspace_bytes(dtype, n, q, d, t) (-20), ldo < d + 1 (-22), ldc < n * ldo (-23).
 * n == 0: returns 0, nothing is written (no pointer is looked at).  q == 0: out[c, i, 0 .. d] = 0.
 */
int64_t stpy_kmv_dx_workspace_bytes(int dtype, int64_t n, int64_t q, int d, int64_t t);
int stpy_kmv_dx(int kind, int dtype, const void* a, int64_t n, int64_t lda, const void* b, int64_t q, int64_t ldb,
                int d, const int32_t* cols, const void* inv_ls, double kappa,
                const void* Vt, int64_t ldv, int64_t t,
                void* out, int64_t ldc, int64_t ldo, void* work, int64_t work_bytes, void* stream);

/*
 * Values, query-point gradients and query-point Hessians of kernel sums, the kernel matrix never formed: stpy_kmv_dx with the second order added.
 * a, b, Vt, kind, cols, inv_ls, kappa, e_ijk, rho_ij, phi and chi as for stpy_kmv_dx; psi = 2 dchi/drho (SE: exp(-rho / 2); MATERN52:
 * (25 / 3) exp(-sqrt(5 rho))):
 *   out[c*ldc + i*ldo + k]                    = inv_ls[k] * sum_j Vt[c,j] kappa chi e_ijk                                    k < d   (as stpy_kmv_dx)
 *   out[c*ldc + i*ldo + d]                    =             sum_j Vt[c,j] kappa phi                                                   (as stpy_kmv_dx)
 *   out[c*ldc + i*ldo + d + 1 + k(k+1)/2 + l] = inv_ls[k] inv_ls[l] * sum_j Vt[c,j] kappa (psi e_ijk e_ijl + chi [k == l])   l <= k < d
 * the last block being d2 / d a_i[cols[k]] d a_i[cols[l]] of the value.  Only the lower triangle is stored, row by row, compact and in the order of
 * cols (the caller scatters and mirrors).  ldo >= 1 + d + d (d + 1) / 2 is the stride between query points and ldc >= n * ldo the stride between
 * coefficient rows, both in elements.  A pair with rho == 0 contributes exactly 0 to the gradient and kappa chi(0) [k == l] times the scales to the
 * Hessian.  Kinds: SE and MATERN52 only (the second derivative of MATERN12 / MATERN32 is singular at r = 0).  d <= 16 selected coordinates.
 * The launch shape of stpy_kmv_dx: a workgroup owns 64 query points, 16 rows c and ONE GROUP of output columns (the gradient and the value; or
 * Hessian rows g - 1 and d - g, d + 1 columns together) and re-evaluates the pair per group; 1 + ceil(d / 2) groups.  With too few workgroups to
 * fill the chip the j range is cut into pieces whose tiles pass through `work` and are added in piece order by a second launch: no atomics, no
 * spin-waits, no cooperative grid.  Two calls give the same bits, and lda / ldb / ldv / ldc / ldo do not change a bit.  At most two launches, no
 * host synchronisation, no allocation.
 * Refused before any HIP call: kind other than SE / MATERN52 (-1), dtype (-2), NULL a / inv_ls / out, or NULL b / Vt with q > 0 (-3), n or q negative
 * or >= 2^31 (-4), lda or ldb < d (-5), d < 1 or d > 16 (-6), t < 1 or more than 65535 blocks of 16 rows x column groups (-10), kappa not finite
 * (-11), ldv < q (-13), work not 8-byte aligned (-17), work NULL or work_bytes below stpy_kmv_dxx_workspace_bytes(dtype, n, q, d, t) (-20),
 * ldo < 1 + d + d (d + 1) / 2 (-22), ldc < n * ldo (-23).
 * n == 0: returns 0, nothing is written (no pointer is looked at).  q == 0: every output of every point is 0.
 * stpy_kmv_dxx_workspace_bytes does not decrease in n, q or t: a buffer sized for the largest problem of a run serves every smaller one.
 */
int64_t stpy_kmv_dxx_workspace_bytes(int dtype, int64_t n, int64_t q, int d, int64_t t);
int stpy_kmv_dxx(int kind, int dtype, const void* a, int64_t n, int64_t lda, const void* b, int64_t q, int64_t ldb,
                 int d, const int32_t* cols, const void* inv_ls, double kappa,
                 const void* Vt, int64_t ldv, int64_t t,
                 void* out, int64_t ldc, int64_t ldo, void* work, int64_t work_bytes, void* stream);

/*
 * Input gradients of the GP posterior (gauss_procc.py:420-459 mean_gradient_hessian / gradient_mean_var and the
 * autograd of mean_std through a test tensor with requires_grad; ucb_optimize, :918-963).  One kernel term k = kappa phi,
 * test points xt (m x ldt) against training points x (n x ldx), scaled differences e = (xt - x_i)[cols] * inv_ls:
 *   G[t*ldg + cols[k]] (op)= sum_i c_ti d k(xt_t, x_i) / d xt_tk,            c_ti = u_t alpha_i + v_t Wt[t*ldw + i]
 *   order 2 also: H[(t*ldg + cols[k])*ldg + cols[l]] (op)= sum_i c_ti d^2 k / d xt_tk d xt_tl   (H: m blocks of ldg x ldg)
 * For the mean gradient alpha = K^-1 y; for the variance gradient Wt = K* K^-1 (stpy_trsm_right_ln).  alpha or Wt may be
 * NULL (not both); u / v NULL mean 1.  kind, cols, inv_ls, kappa, offset as stpy_gram (the dot-product kinds differentiate
 * kappa phi(<xt, x_i> scaled)); the kernel values are recomputed from the points by direct differences, K* is not read.
 * The coordinates are subtracted BEFORE they are scaled by inv_ls: a translate of x and xt that keeps their differences exact
 * gives the same bits, and a test point equal to a training point has e == 0 exactly (that pair adds exactly 0 to G, also for
 * MATERN12, whose phi'(r) / r is taken as 0 at r == 0).
 * combine: STPY_OUT_SET or STPY_OUT_ADD (the terms of a sum accumulate); cols must not repeat a column.  order 2 is refused
 * for MATERN12 / MATERN32 (no Hessian at r = 0).  The n range is split into chunks whose partial sums land in `work`
 * (stpy_gram_grad_workspace_bytes(dtype, m, n, d, order) bytes) and are summed in a fixed order: results are bit-identical
 * from run to run.  n == 0: nothing is written.
 */
int64_t stpy_gram_grad_workspace_bytes(int dtype, int64_t m, int64_t n, int d, int order);
int stpy_gram_grad(int kind, int dtype, const void* x, int64_t n, int64_t ldx, const void* xt, int64_t m, int64_t ldt,
                   int d, const int32_t* cols, const void* inv_ls, double kappa, double offset,
                   const void* alpha, const void* u, const void* Wt, int64_t ldw, const void* v,
                   int order, int combine, void* G, int64_t ldg, void* H, void* work, int64_t work_bytes, void* stream);

/* B <- B L^-1 (B: m x n rows of right-hand sides), the mirror of stpy_trsm_right_lt: with X = K* L^-T this gives
 * W^T = X L^-1 = K* K^-1 of the variance gradient.  Runs as B L^-1 = (B J) Lr^-T J, J the order reversal, on the tuned
 * solve of stpy_trsm_right_lt, with the REVERSED factor Lr = J L^T J (lower triangular) and its inverse diagonal blocks
 * (block c of winvr = J winv_{nb-1-c}^T J), which stpy_trsm_ln_factor builds once from (L, winv).  The reversed factor is
 * another n x n matrix plus another winv array: 34 GB + 0.5 GB at n = 65 536 in fp64, on top of the factor itself.
 * n must be a multiple of 128 (the tile-padded factor of GaussianProcess); work / nb / flags as stpy_trsm_right_lt
 * (stpy_trsm_workspace_bytes sizes the workspace).  The strict upper triangle of Lr is written as zero. */
int stpy_trsm_ln_factor(int dtype, int64_t n, const void* L, int64_t ldl, const void* winv, int64_t winv_elems,
                        void* Lr, int64_t ldlr, void* winvr, void* stream);
int stpy_trsm_right_ln(int dtype, int64_t m, int64_t n, const void* Lr, int64_t ldlr, const void* winvr, int64_t winv_elems,
                       void* B, int64_t ldb, int nb, int flags, void* work, int64_t work_bytes, void* stream);

/*
 * Random Fourier features, replaces RFFEmbedding.embed (embedding.py:225-241):
 *   bias == NULL: out[i*ldo + j] = scale * cos(<W_j, x_i>)  for j <  m/2
 *                                  scale * sin(<W_j, x_i>)  for j >= m/2
 *   bias != NULL: out[i*ldo + j] = scale * cos(<W_j, x_i> + bias[j])
 * x: n x ldx (d columns used), W: m x ldw, out: n x m;  scale = sqrt(2/m) * sqrt(kappa).
 * feat_scale != NULL: feature j is additionally multiplied by feat_scale[j] (m elements of `dtype`) -- the sqrt of the
 *   quadrature weights of QuadratureEmbedding.embed / HermiteEmbedding (embedding.py:450-466, :573-602), which pairs
 *   cos and sin of the SAME node: pass W stacked twice and scale = sqrt(kappa).  An odd m is accepted with a bias only
 *   (cosine-only grids pass a zero bias).
 * transposed != 0 writes Phi^T instead (out: m x n, out[j*ldo + i]) -- the "row x K" operand the
 * feature-space normal equations Phi^T Phi need (kernelized_features.py:236-240).
 * work (optional, stpy_rff_workspace_bytes; 0 for most shapes): with it the large fp32 d = 64 shapes take the contraction to
 *   the bf16 matrix cores from an EXACT three-way bf16 split of both fp32 operands (six products, fp32 accumulation: the
 *   dropped terms are below one fp32 rounding) -- the fp32 MFMA shares the SIMD's ALUs with the trig work, the bf16 pipe does
 *   not.  The workspace receives the split W (m * 64 * 6 bytes); NULL keeps the fp32-MFMA kernel.  Undersized: -20.
 */
int64_t stpy_rff_workspace_bytes(int dtype, int64_t n, int d, int64_t m);
int stpy_rff_embed(int dtype, const void* x, int64_t n, int64_t ldx, int d,
                   const void* W, int64_t ldw, int64_t m, const void* bias, const void* feat_scale, double scale,
                   void* out, int64_t ldo, int transposed, void* work, int64_t work_bytes, void* stream);

/*
 * Input gradients of a Fourier-feature expansion (QuadratureEmbedding.derivative_1 / derivative_2, embedding.py:268-304, contracted
 * with coefficients; the autograd of KernelizedFeatures.mean_std through a test tensor; sample_and_optimize,
 * kernelized_features.py:501-535).  The feature map is exactly that of stpy_rff_embed (x, W, bias, feat_scale, scale: same meaning,
 * same layout rules; an odd m with a bias only):  phi_tj = a_j cos(<W_j, x_t> + bias_j), or a_j cos | a_j sin of <W_j, x_t> for
 * j < m/2 | j >= m/2 without a bias, a_j = scale * feat_scale[j].  With coefficients C (n x m, ldc >= m; ldc == 0: ONE row of m
 * elements shared by all points -- a sampled theta):
 *   val[t]                    (op)= sum_j C_tj phi_tj                          (n elements; val may be NULL)
 *   G[t*ldg + k]              (op)= sum_j C_tj d phi_tj / d x_tk               = sum_j C_tj a_j (-sin | cos)(.) W_jk
 *   order 2 also: H[(t*ldg + k)*ldg + l] (op)= sum_j C_tj d^2 phi_tj / d x_tk d x_tl = -sum_j C_tj phi_tj W_jk W_jl
 *                                                                              (n blocks of ldg x ldg, the layout of stpy_gram_grad)
 * i.e. G = (C o Phi') W in one pass: neither Phi, Phi' nor the (d, m, n) Jacobian is stored.  combine: STPY_OUT_SET or STPY_OUT_ADD
 * (the parts of a concatenated embedding accumulate).  fp64 uses libm sin / cos, fp32 the hardware functions of the embed's GEMM
 * epilogue, so val agrees with stpy_rff_embed followed by a dot product to rounding.  The feature range is split into chunks whose
 * partial sums land in `work` (stpy_rff_grad_workspace_bytes(dtype, n, d, m, order) bytes; NULL -20, undersized -21) and are added in
 * a fixed order: results are bit-identical from run to run.  Refused: dtype (-1), NULL x / W / C / G (-2 / -6 / -12 / -17), d <= 0
 * (-5), ldx / ldw / ldg < d (-4 / -7 / -18), an odd m without a bias (-8), 0 < ldc < m (-13), order (-14), combine (-15), order 2
 * without H (-19).  n == 0 or m == 0: nothing is written.
 */
int64_t stpy_rff_grad_workspace_bytes(int dtype, int64_t n, int d, int64_t m, int order);
int stpy_rff_grad(int dtype, const void* x, int64_t n, int64_t ldx, int d,
                  const void* W, int64_t ldw, int64_t m, const void* bias, const void* feat_scale, double scale,
                  const void* C, int64_t ldc, int order, int combine, void* val, void* G, int64_t ldg, void* H,
                  void* work, int64_t work_bytes, void* stream);

/*
 * Launch profiler (bench.py's live roofline numbers).  While enabled, HIP events are recorded on
 * the launch stream around every MFMA GEMM / diagonal-block launch.  tag: 0 = trailing SYRK
 * update of potrf, 1 = panel GEMMs of potrf, 2 = GEMMs of stpy_trsm_right_lt, 3 = 128x128
 * diagonal-block kernel, 4 = direct stpy_gemm_nt calls.  read() returns the summed event time
 * (ms), the summed algorithmic flops and the number of launches of that tag.
 */
void stpy_profile_enable(int enable);
/* Errors only the device can detect after a call has returned: waits for `stream`, returns 0, or 1 when a hand-off wait of the
 * one-launch vector solve (stpy_trsv) gave up -- that solve's output is then NaN from the affected block on, so every quantity
 * derived from it is NaN as well -- and clears the word; < 0: the query itself failed. */
int stpy_async_status(void* stream);
/* Route switches (process-wide; see "state kept by the library" at the top -- the shipped host code never writes them).
 * Unknown keys are ignored; stpy_tune_get returns -1 for them.
 *   5  block-solve algorithm: 0 auto (recursive halving with strip leaves), 1 right-looking sweep, 2 left-looking with K passes,
 *      3.. recursive with leaves of 128 << (value - 3) columns
 *   8  K = 128 products with at most this many 64 x 64 tiles take the one-volley kernel (768; 0 never)
 *   9  fp32 RFF route: 1 streaming kernel for large d = 64 shapes (bf16-split form when a workspace is passed) + tile kernel for the
 *      other d = 32 / 64 shapes; 5 the same but always the fp32-MFMA streaming kernel; 2 tile kernel only; 0 GEMM epilogue only
 *   16 vector solves as one dataflow launch for n a multiple of 128 (1; 0: the chain of per-block launches)
 *   17 leaf width of the recursive block solve that runs as one strip launch (1 = the default, 512; 128 / 256 / 512 / 1024; 0 = off)
 *   26 fp32 products: aligned plain / lower-triangular products of at least this many 128 x 128 tiles run on the bf16 matrix cores
 *      from an exact three-way split of both operands (64; 0 = always the fp32 MFMA kernels)
 *   28 fp64 Gram fill: 1 = the dedicated fill kernel for aligned overwriting fills (three small workgroups per CU), 0 = always the
 *      fused epilogue of the MFMA GEMM
 *   30 plain / lower-only products (both types) of at most this many 128 x 128 tiles (and K >= 64) run as 32 x 128 slivers, four
 *      times the workgroups of the tile kernels (3200; 0 = never) -- the small trailing updates at the end of every factorisation
 *   34 bordered factor (stpy_potrf_append): more new rows than this take the MFMA block solve for L21 instead of the dataflow
 *      solve (32; 0 = always the MFMA solve; key 16 = 0 also forces it)
 *   32 fp32 factorisation: 1 = each finished panel is split ONCE into three bf16 planes in the workspace and its trailing updates of
 *      2048 rows and more run from those planes (gemm_bf3p.hip); 0 = every tile of an update splits its operands on the fly (key 26's
 *      kernel).  Both give bit-identical factors.
 * The lab build (libstpy_hip_lab.so) adds the experiment knobs listed in csrc/common.h (STPY_KNOB_LIST). */
void stpy_tune(int key, int value);
/* current value of a switch (-1: unknown key), so a caller can restore what it changed */
int stpy_tune_get(int key);
int stpy_profile_read(int tag, double* total_ms, double* total_flops, int64_t* launches);
/* union of the launch intervals of all tags in tagmask (bit t = tag t): overlapping launches counted once */
int stpy_profile_read_union(int tagmask, double* busy_ms, double* total_flops, int64_t* launches);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
