// Small reductions and layout helpers around the evidence gradient, the samplers and the scalar summaries of the estimator
// (stpy_tril, stpy_trace_dot, stpy_scaled_points_t, stpy_lml_grad_reduce).  None of them is on a roofline: each touches
// O(n^2) bytes once (tril) or O(n d) bytes; they exist so that no arithmetic on device data is left to torch on the product path.
// Every reduction has a fixed summation order (one workgroup, strided partial sums, shuffle tree, 16 wave partials added in
// index order): results are bit-reproducible from run to run.
#include "common.h"
#include "lb_block.h"

namespace stpy {

// ------------------------------------------------------------------------------------------
// zero the strict upper triangle (the in-place Cholesky leaves scratch there): 64 x 64 tiles, tiles below the diagonal untouched
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256)
void tril_kernel(T* __restrict__ A, int64_t lda, int n)
{
	const int ti = blockIdx.y, tj = blockIdx.x;
	if (tj < ti) return;
	const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
	const int gc = tj * 64 + tx;
	if (gc >= n) return;
	for (int r = ty; r < 64; r += 4) {
		const int gr = ti * 64 + r;
		if (gr < n && gc > gr) A[(int64_t)gr * lda + gc] = T(0);
	}
}

template <typename T>
int tril(int64_t n, T* A, int64_t lda, hipStream_t st)
{
	if (n <= 0) return 0;
	if (n > INT32_MAX) { set_error("tril: n exceeds int32"); return -2; }
	const unsigned t = (unsigned)((n + 63) / 64);
	hipLaunchKernelGGL((tril_kernel<T>), dim3(t, t), dim3(256), 0, st, A, lda, (int)n);
	return check_launch("tril");
}

// block-wide sum in a fixed order; valid in thread 0
template <typename T>
__device__ __forceinline__ T block_sum_1024(T v, T* red16)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
	__syncthreads();                                   // (red16 may still be read from the previous call)
	if ((threadIdx.x & 63) == 0) red16[threadIdx.x >> 6] = v;
	__syncthreads();
	T s = T(0);
	if (threadIdx.x == 0)
		for (int w = 0; w < 16; ++w) s += red16[w];
	return s;
}

// out2[0] = sum_i A_ii (A may be null: 0), out2[1] = <u, v> (u may be null: 0)
template <typename T>
__global__ __launch_bounds__(1024)
void trace_dot_kernel(const T* __restrict__ A, int64_t lda, const T* __restrict__ u, const T* __restrict__ v, int n, T* __restrict__ out2)
{
	__shared__ T red[16];
	T s1 = T(0), s2 = T(0);
	for (int i = threadIdx.x; i < n; i += 1024) {
		if (A) s1 += A[(int64_t)i * lda + i];
		if (u) s2 += u[i] * v[i];
	}
	s1 = block_sum_1024(s1, red);
	s2 = block_sum_1024(s2, red);
	if (threadIdx.x == 0) { out2[0] = s1; out2[1] = s2; }
}

template <typename T>
int trace_dot(int64_t n, const T* A, int64_t lda, const T* u, const T* v, T* out2, hipStream_t st)
{
	if (n > INT32_MAX) { set_error("trace_dot: n exceeds int32"); return -2; }
	hipLaunchKernelGGL((trace_dot_kernel<T>), dim3(1), dim3(1024), 0, st, A, lda, u, v, (int)n, out2);
	return check_launch("trace_dot");
}

// out[k*ldo + i] = (x[i*ldx + cols[k]] - [centre] x[cols[k]]) * inv_ls[k]  (k < d),  and out[d*ldo + i] = 1 when ones: the NT operand
// [Xs | 1]^T, with `centre` of the coordinates relative to the first point (subtracted before the scaling)
template <typename T>
__global__ __launch_bounds__(256)
void scaled_points_t_kernel(const T* __restrict__ x, int64_t ldx, int n, int d, const int32_t* __restrict__ cols, const T* __restrict__ inv_ls,
                            T* __restrict__ out, int64_t ldo, int centre)
{
	const int i = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
	if (i >= n) return;
	if (k == d) { out[(int64_t)k * ldo + i] = T(1); return; }
	const int c = cols ? cols[k] : k;
	out[(int64_t)k * ldo + i] = (x[(int64_t)i * ldx + c] - (centre ? x[c] : T(0))) * inv_ls[k];
}

template <typename T>
int scaled_points_t(const T* x, int64_t n, int64_t ldx, int d, const int32_t* cols, const T* inv_ls, T* out, int64_t ldo, int ones_row, hipStream_t st)
{
	if (n <= 0) return 0;
	if (n > INT32_MAX) { set_error("scaled_points_t: n exceeds int32"); return -2; }
	hipLaunchKernelGGL((scaled_points_t_kernel<T>), dim3((unsigned)((n + 255) / 256), (unsigned)(d + (ones_row & 1))), dim3(256), 0, st,
	                   x, ldx, (int)n, d, cols, inv_ls, out, ldo, (ones_row >> 1) & 1);
	return check_launch("scaled_points_t");
}

// With P = H [Xs | 1]  (n x (d+1); column d = h = H 1):
//   S_k = sum_i xs_ik^2 h_i - xs_ik P_ik  ( = 1/2 sum_ij H_ij (xs_ik - xs_jk)^2 for symmetric H ),
//   acc[pidx[k]] += S_k * inv_ls[k]                 -- d/d(lengthscale) of the evidence per coordinate of a kernel term
// The sum does not see a common translation of the points, but formed about the origin its two halves each grow with the square of
// the data's distance from it and then cancel.  So it is formed about the first point: with xs = c0 + t,
//   S_k = sum_i t_i^2 h_i - t_i (H t)_i,     (H t)_i = P_ik - c0 h_i     (H symmetric)
// `centred`: P was formed from t already (stpy_scaled_points_t, ones_row = 3), (H t)_i = P_ik -- P = H Xs carries rounding of the
// size eps |xs| |H| that no later step removes, so this is the form whose accuracy does not depend on where the data lies.
// One workgroup, coordinates in order: several coordinates that share a parameter (an isotropic 'gamma') are added in a fixed order.
template <typename T>
__global__ __launch_bounds__(1024)
void lml_grad_reduce_kernel(const T* __restrict__ x, int64_t ldx, int n, int d, const int32_t* __restrict__ cols, const T* __restrict__ inv_ls,
                            const T* __restrict__ P, int64_t ldp, const int32_t* __restrict__ pidx, T* __restrict__ acc, int centred)
{
	__shared__ T red[16];
	for (int k = 0; k < d; ++k) {
		const int c = cols ? cols[k] : k;
		const T il = inv_ls[k];
		const T x0 = x[c], c0 = centred ? T(0) : x0 * il;
		T s = T(0);
		for (int i = threadIdx.x; i < n; i += 1024) {
			const T t = (x[(int64_t)i * ldx + c] - x0) * il;
			const T* Pi = P + (int64_t)i * ldp;
			s += t * (t * Pi[d] - fma(-c0, Pi[d], Pi[k]));
		}
		s = block_sum_1024(s, red);
		if (threadIdx.x == 0) acc[pidx ? pidx[k] : k] += s * il;
	}
}

template <typename T>
int lml_grad_reduce(const T* x, int64_t n, int64_t ldx, int d, const int32_t* cols, const T* inv_ls, const T* P, int64_t ldp,
                    const int32_t* pidx, T* acc, int centred, hipStream_t st)
{
	if (n > INT32_MAX) { set_error("lml_grad_reduce: n exceeds int32"); return -2; }
	hipLaunchKernelGGL((lml_grad_reduce_kernel<T>), dim3(1), dim3(1024), 0, st, x, ldx, (int)n, d, cols, inv_ls, P, ldp, pidx, acc, centred);
	return check_launch("lml_grad_reduce");
}

// Full-covariance kernel items (kernels.py:464-549: z = x[:, cols] cov, then a stationary kernel of |z_i - z_j|): with P = H [Z | 1]
// (n x (p+1), H = (w K^-1 - alpha alpha^T) o kappa F as stpy_lml_weight forms it for the mapped points Z with unit lengthscales),
//   out[a * p + m] -= sum_i x[i, cols[a]] * (P[i][p] * z[i][m] - P[i][m])       ( = -1/2 sum_ij H_ij (z_i - z_j)_m (x_i - x_j)_a )
// which is d/dcov[a][m] of the evidence.  One workgroup, the dg x p entries in order, fixed summation order.
template <typename T>
__global__ __launch_bounds__(1024)
void lml_grad_cov_reduce_kernel(const T* __restrict__ x, int64_t ldx, int n, int dg, const int32_t* __restrict__ cols,
                                const T* __restrict__ z, int64_t ldz, int pdim, const T* __restrict__ P, int64_t ldp, T* __restrict__ out)
{
	__shared__ T red[16];
	for (int a = 0; a < dg; ++a) {
		const int c = cols ? cols[a] : a;
		for (int m = 0; m < pdim; ++m) {
			T s = T(0);
			for (int i = threadIdx.x; i < n; i += 1024) {
				const T* Pi = P + (int64_t)i * ldp;
				s += x[(int64_t)i * ldx + c] * (Pi[pdim] * z[(int64_t)i * ldz + m] - Pi[m]);
			}
			s = block_sum_1024(s, red);
			if (threadIdx.x == 0) out[a * pdim + m] -= s;
		}
	}
}

template <typename T>
int lml_grad_cov_reduce(const T* x, int64_t n, int64_t ldx, int dg, const int32_t* cols, const T* z, int64_t ldz, int pdim, const T* P, int64_t ldp,
                        T* out, hipStream_t st)
{
	if (n > INT32_MAX) { set_error("lml_grad_cov_reduce: n exceeds int32"); return -2; }
	hipLaunchKernelGGL((lml_grad_cov_reduce_kernel<T>), dim3(1), dim3(1024), 0, st, x, ldx, (int)n, dg, cols, z, ldz, pdim, P, ldp, out);
	return check_launch("lml_grad_cov_reduce");
}

// ------------------------------------------------------------------------------------------
// Batched evidence (stpy_lml_batch): value and gradient of the negative log evidence for `batch` hyper-parameter candidates on the
// same data, ONE workgroup per candidate -- the restarts of a hyper-parameter search, each of which fills a small part of the chip
// and costs ten launches and two host read-backs on the serial path.
//
// Per candidate, in its slice of the workspace (A, V: NP x NP row-major, NP = n rounded up to the block of 32, bordered by an identity;
// dinv: the NP / 32 inverse diagonal blocks):
//   1. A <- lower blocks of K = kappa phi(|(x_i - x_j)[cols] o inv_ls|) + s^2 I from direct coordinate differences;
//   2. blocked left-looking Cholesky in place: panel -= (rows left of it) (its own rows left of it)^T on the fp64 MFMA, the 32 x 32
//      diagonal block factored and inverted by one wave in registers (lane r holds row r; column values travel by v_readlane),
//      the rows below it times the inverse block on the MFMA again;
//   3. V <- L^-T (upper triangular, row-major = W^T for W = L^-1), block column by block column from V's finished part;
//   4. z = W y, alpha = W^T z (LDS), then A <- K^-1 = V V^T (lower blocks), H = (w K^-1 - alpha alpha^T) o kappa F in place over it
//      and the per-coordinate sums over i > j, four coordinates per pass over H.
// Every sum has a fixed order (per-thread partial sums over a fixed set of entries, shuffle tree, four wave partials in index order)
// and no candidate reads what another wrote: a candidate's outputs are bit-identical wherever it sits in whatever batch.
// Barriers: every __syncthreads() below is reached by the whole workgroup -- the loops around them run over workgroup-uniform
// ranges, the single-wave diagonal-block step has no barrier inside, and a failed pivot is published through LDS and read by all
// threads behind a barrier, so the workgroup leaves as a whole.
// ------------------------------------------------------------------------------------------
struct LmlBatchArgs {
	const double* x; int64_t ldx; int n, d; const int32_t* cols; const double* y;
	const double* inv_ls; int64_t ldi; const double* noise; double kappa, weight;
	const int32_t* pidx; int np;
	double* value; double* grad; int64_t ldg; int32_t* info;
	double* work; int64_t slice;         // doubles per candidate
	int kind;
};

inline int64_t lml_batch_slice_elems(int64_t n)
{
	const int64_t np = (n + 31) / 32 * 32;
	return 2 * np * np + 32 * np;
}

__device__ __forceinline__ double lb_r2(const LmlBatchArgs& p, const double* __restrict__ il, int i, int j)
{
	const double* xi = p.x + (int64_t)i * p.ldx;
	const double* xj = p.x + (int64_t)j * p.ldx;
	double s = 0.0;
	for (int k = 0; k < p.d; ++k) {
		const int c = p.cols ? p.cols[k] : k;
		const double u = (xi[c] - xj[c]) * il[k];
		s = fma(u, u, s);
	}
	return s;
}

__global__ __launch_bounds__(256, 2)
void lml_batch_kernel(LmlBatchArgs p)
{
	__shared__ __attribute__((aligned(16))) double As[64 * LB_LDS];
	__shared__ __attribute__((aligned(16))) double Bs[32 * LB_LDS];
	__shared__ double zs[LB_MAX_N], al[LB_MAX_N], red[4];
	__shared__ int s_info;
	const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int n = p.n, NP = (n + 31) & ~31, nblk = NP >> 5, ld = NP;
	double* A = p.work + (int64_t)b * p.slice;
	double* V = A + (int64_t)NP * NP;
	double* dinv = V + (int64_t)NP * NP;
	const double* il = p.inv_ls + (int64_t)b * p.ldi;
	double* grow = p.grad + (int64_t)b * p.ldg;
	const double sd = p.noise[b], s2 = sd * sd, kappa = p.kappa, wgt = p.weight;
	const int ec = tid & 31, er = tid >> 5;              // entry of a 32 x 32 block in the elementwise passes: column, first of 4 rows (8 apart)
	if (tid == 0) {
		s_info = 0;
		for (int k = 0; k <= p.np; ++k) grow[k] = 0.0;
	}

	// ---- 1. lower blocks of K (whole diagonal blocks), identity border; the blocks of V just below its diagonal are read as zero
	for (int bi = 0; bi < nblk; ++bi)
		for (int bj = 0; bj <= bi; ++bj)
#pragma unroll
			for (int q = 0; q < 4; ++q) {
				const int i = 32 * bi + er + 8 * q, j = 32 * bj + ec;
				double v = i == j ? 1.0 : 0.0;
				if (i < n && j < n) v = kappa * lb_phi(p.kind, lb_r2(p, il, i, j)) + (i == j ? s2 : 0.0);
				A[(int64_t)i * ld + j] = v;
				if (bi == bj + 1) V[(int64_t)i * ld + j] = 0.0;
			}

	// ---- 2. Cholesky
	for (int bk = 0; bk < nblk; ++bk) {
		const int j0 = 32 * bk;
		double* Ajj = A + (int64_t)j0 * ld + j0;
		if (bk > 0) lb_panel<1>(Ajj, ld, A + (int64_t)j0 * ld, ld, A + (int64_t)j0 * ld, ld, NP - j0, j0, -1, As, Bs);
		__syncthreads();
		if (wave == 0) {
			const int bad = lb_diag(A, V, ld, j0, dinv + bk * 1024, As);
			if (bad != 0 && lane == 0) s_info = j0 + bad;
		}
		__syncthreads();
		if (s_info != 0) {          // (the same word for every thread: the workgroup leaves as a whole)
			if (tid == 0) {
				p.value[b] = __builtin_huge_val();
				p.info[b] = s_info;
			}
			return;
		}
		if (j0 + 32 < NP) lb_panel<0>(Ajj + (int64_t)32 * ld, ld, Ajj + (int64_t)32 * ld, ld, dinv + bk * 1024, 32, NP - j0 - 32, 32, -1, As, Bs);
	}
	__syncthreads();
	double logdiag = 0.0;
	for (int i = tid; i < n; i += 256) logdiag += log(A[(int64_t)i * ld + i]);
	logdiag = lb_block_sum(logdiag, red);

	// ---- 3. V = L^-T: block column I from the finished columns left of it, V[0:i0, I] = -(V[0:i0, 0:i0] L[I, 0:i0]^T) dinv_I^T
	for (int bk = 1; bk < nblk; ++bk) {
		const int i0 = 32 * bk;
		lb_panel<0>(V + i0, ld, V, ld, A + (int64_t)i0 * ld, ld, i0, i0, 0, As, Bs);
		lb_panel<2>(V + i0, ld, V + i0, ld, dinv + bk * 1024, 32, i0, 32, -1, As, Bs);
	}
	__syncthreads();

	// ---- 4. z = W y (z_i = sum_{k <= i} V[k][i] y_k), alpha = W^T z (alpha_j = sum_{k >= j} V[j][k] z_k)
	for (int i = tid; i < NP; i += 256) {
		const int kend = min(32 * (i / 32 + 1), n);
		double z = 0.0;
#pragma unroll 8
		for (int k = 0; k < kend; ++k) z = fma(V[(int64_t)k * ld + i], p.y[k], z);
		zs[i] = i < n ? z : 0.0;
	}
	__syncthreads();
	for (int j = wave; j < n; j += 4) {
		const double* vr = V + (int64_t)j * ld;
		double s = 0.0;
		for (int k = 32 * (j / 32) + lane; k < NP; k += 64) s = fma(vr[k], zs[k], s);
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
		if (lane == 0) al[j] = s;
	}
	__syncthreads();
	double quad = 0.0, aa = 0.0;
	for (int i = tid; i < n; i += 256) { quad = fma(zs[i], zs[i], quad); aa = fma(al[i], al[i], aa); }
	quad = lb_block_sum(quad, red);
	aa = lb_block_sum(aa, red);

	// ---- K^-1 = V V^T over A's lower blocks (L is no longer needed), then H = (w K^-1 - alpha alpha^T) o kappa F below the diagonal
	for (int bk = 0; bk < nblk; ++bk) {
		const int j0 = 32 * bk;
		lb_panel<0>(A + (int64_t)j0 * ld + j0, ld, V + (int64_t)j0 * ld, ld, V + (int64_t)j0 * ld, ld, NP - j0, NP, j0, As, Bs);
	}
	__syncthreads();
	double tr = 0.0;
	for (int bi = 0; bi < nblk; ++bi)
		for (int bj = 0; bj <= bi; ++bj)
#pragma unroll
			for (int q = 0; q < 4; ++q) {
				const int i = 32 * bi + er + 8 * q, j = 32 * bj + ec;
				double h = 0.0;
				if (i < n && j <= i) {
					const double kv = A[(int64_t)i * ld + j];
					if (i == j) tr += kv;
					else h = (wgt * kv - al[i] * al[j]) * kappa * lb_dfactor(p.kind, lb_r2(p, il, i, j));
				}
				A[(int64_t)i * ld + j] = h;
			}
	tr = lb_block_sum(tr, red);          // (its barriers also order the H stores before the passes below: each entry is re-read by the thread that wrote it anyway)

	// ---- lengthscale sums: 1/2 sum_ij H_ij u_m^2 / l_m = inv_ls_m sum_{i > j} H_ij u_m^2, four coordinates per pass over H
	for (int m0 = 0; m0 < p.d; m0 += 4) {
		double sm[4] = {0.0, 0.0, 0.0, 0.0};
		for (int bi = 0; bi < nblk; ++bi)
			for (int bj = 0; bj <= bi; ++bj)
#pragma unroll
				for (int q = 0; q < 4; ++q) {
					const int i = 32 * bi + er + 8 * q, j = 32 * bj + ec;
					if (i < n && j < i) {
						const double h = A[(int64_t)i * ld + j];
						const double* xi = p.x + (int64_t)i * p.ldx;
						const double* xj = p.x + (int64_t)j * p.ldx;
#pragma unroll
						for (int e = 0; e < 4; ++e)
							if (m0 + e < p.d) {
								const int c = p.cols ? p.cols[m0 + e] : m0 + e;
								const double u = (xi[c] - xj[c]) * il[m0 + e];
								sm[e] = fma(h, u * u, sm[e]);
							}
					}
				}
#pragma unroll
		for (int e = 0; e < 4; ++e) sm[e] = lb_block_sum(sm[e], red);
		if (tid == 0) {
#pragma unroll
			for (int e = 0; e < 4; ++e)
				if (m0 + e < p.d) {
					const int pi = p.pidx[m0 + e];
					if (pi >= 0 && pi < p.np) grow[pi] += sm[e] * il[m0 + e];
				}
		}
	}
	if (tid == 0) {
		p.value[b] = 0.5 * quad + wgt * logdiag;
		grow[p.np] = sd * (wgt * tr - aa);
		p.info[b] = 0;
	}
}

int64_t lml_batch_workspace_bytes(int64_t n, int64_t batch)
{
	return n <= 0 || batch <= 0 ? 0 : batch * lml_batch_slice_elems(n) * (int64_t)sizeof(double);
}

int lml_batch(int kind, const double* x, int64_t n, int64_t ldx, int d, const int32_t* cols, const double* y, int64_t batch,
              const double* inv_ls, int64_t ldi, const double* noise, double kappa, double weight, const int32_t* pidx, int np,
              double* value, double* grad, int64_t ldg, int32_t* info, void* work, hipStream_t st)
{
	LmlBatchArgs p{x, ldx, (int)n, d, cols, y, inv_ls, ldi, noise, kappa, weight, pidx, np, value, grad, ldg, info,
	               (double*)work, lml_batch_slice_elems(n), kind};
	hipLaunchKernelGGL(lml_batch_kernel, dim3((unsigned)batch), dim3(256), 0, st, p);
	return check_launch("lml_batch");
}

#define INST(T) \
	template int lml_grad_cov_reduce<T>(const T*, int64_t, int64_t, int, const int32_t*, const T*, int64_t, int, const T*, int64_t, T*, hipStream_t); \
	template int tril<T>(int64_t, T*, int64_t, hipStream_t); \
	template int trace_dot<T>(int64_t, const T*, int64_t, const T*, const T*, T*, hipStream_t); \
	template int scaled_points_t<T>(const T*, int64_t, int64_t, int, const int32_t*, const T*, T*, int64_t, int, hipStream_t); \
	template int lml_grad_reduce<T>(const T*, int64_t, int64_t, int, const int32_t*, const T*, const T*, int64_t, const int32_t*, T*, int, hipStream_t);
INST(double)
INST(float)

}  // namespace stpy

// ---- C ABI of the batched evidence (include/stpy_hip.h); every refusal below comes before the first HIP call
using namespace stpy;

extern "C" {

int64_t stpy_lml_batch_max_n(void) { return LB_MAX_N; }

int64_t stpy_lml_batch_workspace_bytes(int dtype, int64_t n, int d, int64_t batch)
{
	(void)d;
	return dtype == STPY_F64 ? lml_batch_workspace_bytes(n, batch) : 0;          // (float32 has no batched route)
}

int stpy_lml_batch(int kind, int dtype, const void* x, int64_t n, int64_t ldx, int d, const int32_t* cols, const void* y, int64_t batch,
                   const void* inv_ls, int64_t ldi, const void* noise, double kappa, double weight, const int32_t* pidx, int np,
                   void* value, void* grad, int64_t ldg, int32_t* info, void* work, int64_t work_bytes, void* stream)
{
	if (n == 0 || batch == 0) return 0;          // empty problem: nothing to write
	if (dtype != STPY_F64) { set_error("stpy_lml_batch: dtype %d: the batched evidence is float64 only (0)", dtype); return -2; }
	if (kind < STPY_K_SE || kind > STPY_K_MATERN52) { set_error("stpy_lml_batch: kernel kind %d has no lengthscale gradient (SE, MATERN12/32/52)", kind); return -1; }
	if (n < 0 || n > LB_MAX_N) { set_error("stpy_lml_batch: n=%lld outside [0, %d] (stpy_lml_batch_max_n)", (long long)n, LB_MAX_N); return -4; }
	if (batch < 0 || batch > INT32_MAX) { set_error("stpy_lml_batch: batch=%lld out of range", (long long)batch); return -9; }
	if (d < 1 || np < 1) { set_error("stpy_lml_batch: bad dimensions d=%d np=%d", d, np); return d < 1 ? -6 : -16; }
	if (ldx < d || ldi < d || ldg < (int64_t)np + 1) {
		set_error("stpy_lml_batch: leading dimensions ldx=%lld ldi=%lld (d=%d) ldg=%lld (np+1=%d)", (long long)ldx, (long long)ldi, d, (long long)ldg, np + 1);
		return ldx < d ? -5 : (ldi < d ? -11 : -19);
	}
	if (!x || !y || !inv_ls || !noise || !pidx || !value || !grad || !info || !work) { set_error("stpy_lml_batch: null pointer"); return -3; }
	const int64_t need = lml_batch_workspace_bytes(n, batch);
	if (work_bytes < need) {
		set_error("stpy_lml_batch: workspace of %lld bytes, %lld needed (see the *_workspace_bytes query for these arguments)", (long long)work_bytes, (long long)need);
		return -20;
	}
	if (((uintptr_t)work | (uintptr_t)x) & 7 || ((uintptr_t)work & 15)) { set_error("stpy_lml_batch: work must be 16-byte aligned"); return -21; }
	return lml_batch(kind, (const double*)x, n, ldx, d, cols, (const double*)y, batch, (const double*)inv_ls, ldi, (const double*)noise, kappa, weight,
	                 pidx, np, (double*)value, (double*)grad, ldg, info, work, (hipStream_t)stream);
}

}  // extern "C"
