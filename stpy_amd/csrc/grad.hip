// grad.hip -- input gradients of the GP posterior: the kernel's derivative with respect to the test point summed against
// per-pair coefficients (stpy_gram_grad), and the right solve with L^-1 that gives K*^T-weights W^T = K* K^-1 of the
// variance gradient (stpy_trsm_right_ln, the mirror of stpy_trsm_right_lt through the order reversal J).
//
// stpy_gram_grad: for m test points against n training points
//   out[t][q] = sum_i c_ti * D_q(xt_t, x_i),   c_ti = u_t alpha_i + v_t Wt[t][i]
// with D_q the q-th first (q < d) or second (q = d + k d + l) derivative of one kernel term.  The work is m n d fma-class
// operations plus one exp per pair; the only large operand is Wt (m x n, read once), so the kernel is built to stream Wt
// at HBM rate while the VALU recomputes the kernel from the points:
//   * 256 lanes per workgroup run along the contiguous training index i: the GG_TM rows of Wt a workgroup reads are
//     coalesced, 512 bytes per wave and row;
//   * a workgroup owns GG_TM test points, a chunk of the training points and a block of GG_QB outputs; each lane keeps
//     GG_TM x GG_QB partial sums in registers (64 fp64 = 128 VGPRs) over its strided share of the chunk;
//   * d = 16 (the headline shape) is one output block, so Wt is read once; a larger d loops over output blocks (one more
//     grid dimension) and recomputes r for each -- any d is accepted, the points are read through L1 (they are
//     tiny next to Wt), nothing scales with d in registers or LDS;
//   * the distances are DIRECT differences (xt - x_i) * inv_ls, never the norm expansion: the derivatives need the
//     small differences accurately and Matern 1/2 needs exact zeros.  The raw coordinates are subtracted BEFORE the
//     difference is scaled (as kmv.hip, kmv_pair.h, lb_block.h and reduce.hip do): scaling first rounds x * inv_ls at
//     the magnitude of the data's offset from the origin and loses (offset / spread) eps; subtracting first, a
//     translate of the data by a vector that keeps the differences exact gives the same bits (and a coincident pair
//     has e = 0 exactly: x * inv_ls - x * inv_ls, contracted into one fma, leaves the rounding residual of the product,
//     which Matern 1/2 then divides by).  The dot-product kinds are not translation invariant and keep the product of
//     the two scaled coordinates.  The first derivatives sum w1 * (xt - x_i) of the RAW difference and take both
//     factors inv_ls_k after the sum (one multiply per output and pair less than scaling inside the loop); the
//     Hessian's products e_k e_l are scaled inside the loop.  Subtracting first costs the distance loop one multiply
//     per coordinate and pair that xt * inv_ls - x_i * inv_ls hid in an fma (12.0 against 10.4 ms at the headline
//     shape); with ONE lengthscale for all coordinates r^2 is inv_ls^2 sum (xt - x_i)^2 and the multiply is gone again;
//   * the workgroup's lanes are summed through LDS in a fixed tree, the chunks (split over n so that small m still
//     fills the chip) land in the workspace and a second kernel sums them in chunk order: the result is bit-identical
//     from run to run (no atomics anywhere), and the final scaling by inv_ls and the scatter into the term's columns
//     of G (set or add) happen there.
#include "common.h"

namespace stpy {

constexpr int GG_THREADS = 256, GG_TM = 4, GG_QB = 16;
constexpr int64_t GG_TARGET_WGS = 2048;         // eight workgroups per CU

template <typename T>
struct GradArgs {
	const T* x; const T* xt; const int32_t* cols; const T* inv_ls;
	const T* alpha; const T* u; const T* Wt; const T* v;
	T* part;                         // [nsplit][m][Q] partial sums
	int64_t ldx, ldt, ldw;
	int64_t n, m, chunk;
	int d, Q, nqb, nsplit, ntiles;
	T kappa, offset;
	int kind, degree;
};

// how the n range is cut: enough workgroups to fill the chip, chunks a multiple of the workgroup width
static void grad_plan(int64_t m, int64_t n, int d, int order, int* Q, int* nqb, int64_t* chunk, int* nsplit, int64_t* ntiles)
{
	*Q = d + (order == 2 ? d * d : 0);
	*nqb = (*Q + GG_QB - 1) / GG_QB;
	*ntiles = (m + GG_TM - 1) / GG_TM;
	const int64_t base = (int64_t)(*nqb) * (*ntiles);
	int64_t want = (GG_TARGET_WGS + base - 1) / base;
	const int64_t maxs = (n + GG_THREADS - 1) / GG_THREADS;
	if (want > maxs) want = maxs;
	if (want < 1) want = 1;
	int64_t c = (n + want - 1) / want;
	c = (c + GG_THREADS - 1) / GG_THREADS * GG_THREADS;
	*chunk = c;
	*nsplit = (int)((n + c - 1) / c);
}

template <typename T> __device__ __forceinline__ T ipow(T b, int e)
{
	T r = T(1);
	for (int k = 0; k < e; ++k) r *= b;
	return r;
}

template <typename T, bool HESS>
__global__ __launch_bounds__(GG_THREADS)
void gram_grad_kernel(GradArgs<T> p)
{
	int64_t bid = blockIdx.x;
	const int qb = (int)(bid % p.nqb); bid /= p.nqb;          // output blocks of one tile and chunk are neighbours: they read the same Wt rows
	const int split = (int)(bid % p.nsplit);
	const int64_t tile = bid / p.nsplit;
	const int64_t t0 = tile * GG_TM;
	const int q0 = qb * GG_QB;
	const int tid = threadIdx.x;
	const bool dot = (p.kind == STPY_K_LINEAR || p.kind == STPY_K_POLY);
	const int64_t i_end = min(p.n, (int64_t)(split + 1) * p.chunk);
	// one lengthscale for every coordinate (the isotropic kernels): r^2 = inv_ls^2 sum (xt - x_i)^2, the scaling once per pair, not per coordinate
	const T il0 = p.inv_ls[0];
	bool iso = !dot;
	for (int k = 1; k < p.d; ++k) iso = iso && p.inv_ls[k] == il0;

	int64_t trow[GG_TM];
#pragma unroll
	for (int t = 0; t < GG_TM; ++t) trow[t] = min(t0 + t, p.m - 1);      // rows past m recompute the last one and are never stored
	T us[GG_TM], vs[GG_TM];
#pragma unroll
	for (int t = 0; t < GG_TM; ++t) { us[t] = p.u ? p.u[trow[t]] : T(1); vs[t] = p.v ? p.v[trow[t]] : T(1); }

	// the block's raw test coordinates (first-derivative outputs): read from LDS inside the loop, not held in registers.  The dot-product
	// kinds, whose factor is x_i alone, hold 0 there: one form w1 * (xq - x_i) serves both, and the finish kernel flips their sign
	__shared__ T xq[GG_TM][GG_QB];
	if (tid < GG_TM * GG_QB) {
		const int t = tid / GG_QB, q = q0 + tid % GG_QB;
		xq[t][tid % GG_QB] = (q < p.d && !dot) ? p.xt[min(t0 + t, p.m - 1) * p.ldt + (p.cols ? p.cols[q] : q)] : T(0);
	}
	__syncthreads();

	T acc[GG_TM][GG_QB];
#pragma unroll
	for (int t = 0; t < GG_TM; ++t)
#pragma unroll
		for (int q = 0; q < GG_QB; ++q) acc[t][q] = T(0);

	for (int64_t i = (int64_t)split * p.chunk + tid; i < i_end; i += GG_THREADS) {
		const T* xi = p.x + i * p.ldx;
		// ---- squared scaled distance (stationary: subtract, then scale) or scaled inner product (dot-product kinds)
		T s[GG_TM];
#pragma unroll
		for (int t = 0; t < GG_TM; ++t) s[t] = T(0);
		if (iso) {
			for (int k = 0; k < p.d; ++k) {
				const int c = p.cols ? p.cols[k] : k;
				const T a = xi[c];
#pragma unroll
				for (int t = 0; t < GG_TM; ++t) { const T e = p.xt[trow[t] * p.ldt + c] - a; s[t] += e * e; }
			}
#pragma unroll
			for (int t = 0; t < GG_TM; ++t) s[t] = (s[t] * il0) * il0;
		} else {
			for (int k = 0; k < p.d; ++k) {
				const int c = p.cols ? p.cols[k] : k;
				const T il = p.inv_ls[k];
				const T a = xi[c];
#pragma unroll
				for (int t = 0; t < GG_TM; ++t) {
					const T b = p.xt[trow[t] * p.ldt + c];
					if (dot) s[t] += (a * il) * (b * il);
					else { const T e = (b - a) * il; s[t] += e * e; }
				}
			}
		}
		// ---- coefficient and the two radial factors: first derivatives w1 * e_k, second w2 * e_k e_l (+ w1 on the diagonal)
		T w1[GG_TM], w2[GG_TM];
#pragma unroll
		for (int t = 0; t < GG_TM; ++t) {
			T c = T(0);
			if (p.alpha) c = us[t] * p.alpha[i];
			if (p.Wt) c += vs[t] * p.Wt[trow[t] * p.ldw + i];
			T psi, chi = T(0);
			switch (p.kind) {
			case STPY_K_SE: { const T e = p.kappa * exp(T(-0.5) * s[t]); psi = -e; chi = e; break; }
			case STPY_K_MATERN12: { const T r = sqrt(s[t]); psi = r > T(0) ? -p.kappa * exp(-r) / r : T(0); break; }
			case STPY_K_MATERN32: { const T r = sqrt(s[t]); psi = T(-3) * p.kappa * exp(T(-1.7320508075688772935) * r); break; }
			case STPY_K_MATERN52: {
				const T r = sqrt(s[t]);
				const T e = p.kappa * exp(T(-2.2360679774997896964) * r);
				psi = T(-5.0 / 3.0) * (T(1) + T(2.2360679774997896964) * r) * e;
				chi = T(25.0 / 3.0) * e;
				break;
			}
			case STPY_K_LINEAR: psi = p.kappa; break;
			default: {                   // POLY: kappa p b^(p-1), kappa p (p-1) b^(p-2), b = <xt, x_i> + offset
				const T b = s[t] + p.offset;
				psi = p.kappa * T(p.degree) * ipow(b, p.degree - 1);
				chi = p.degree >= 2 ? p.kappa * T(p.degree) * T(p.degree - 1) * ipow(b, p.degree - 2) : T(0);
			}
			}
			w1[t] = c * psi;
			w2[t] = c * chi;
		}
		// ---- this block's outputs (uniform branches: q, its coordinates and its kind are the same in every lane)
#pragma unroll
		for (int qq = 0; qq < GG_QB; ++qq) {
			const int q = q0 + qq;
			if (q >= p.Q) break;
			int ka = q, kb = -1;
			if (HESS && q >= p.d) { ka = (q - p.d) / p.d; kb = (q - p.d) - ka * p.d; }
			const int ca = p.cols ? p.cols[ka] : ka;
			const T ila = p.inv_ls[ka];
			const T xa = xi[ca];
			if (kb < 0) {
#pragma unroll
				for (int t = 0; t < GG_TM; ++t) {
					acc[t][qq] += w1[t] * (xq[t][qq] - xa);                 // (raw difference: both factors inv_ls in the finish kernel)
				}
			} else if (HESS) {
				const int cb = p.cols ? p.cols[kb] : kb;
				const T ilb = p.inv_ls[kb];
				const T xb = xi[cb];
#pragma unroll
				for (int t = 0; t < GG_TM; ++t) {
					const T ea = dot ? xa * ila : (p.xt[trow[t] * p.ldt + ca] - xa) * ila;
					const T eb = dot ? xb * ilb : (p.xt[trow[t] * p.ldt + cb] - xb) * ilb;
					acc[t][qq] += w2[t] * ea * eb + ((!dot && ka == kb) ? w1[t] : T(0));
				}
			}
		}
	}

	// ---- workgroup sum in a fixed tree: 16 rows of 16 lanes each, then the 16 row sums
	__shared__ T red[GG_THREADS][GG_QB + 1];
	__shared__ T red2[16][GG_QB + 1];
#pragma unroll
	for (int t = 0; t < GG_TM; ++t) {
#pragma unroll
		for (int q = 0; q < GG_QB; ++q) red[tid][q] = acc[t][q];
		__syncthreads();
		{
			const int q = tid & (GG_QB - 1), part = tid / GG_QB;      // 256 threads = 16 parts x 16 outputs
			T sum = T(0);
			for (int r = 0; r < GG_THREADS / 16; ++r) sum += red[part * (GG_THREADS / 16) + r][q];
			red2[part][q] = sum;
		}
		__syncthreads();
		if (tid < GG_QB && t0 + t < p.m && q0 + tid < p.Q) {
			T sum = T(0);
			for (int r = 0; r < 16; ++r) sum += red2[r][tid];
			p.part[((int64_t)split * p.m + t0 + t) * p.Q + q0 + tid] = sum;
		}
		__syncthreads();
	}
}

// chunk partial sums in chunk order, the inv_ls factors left to the end (first derivatives: the one of the scaled difference and
// the one of the chain rule; second derivatives: the two of the chain rule), the scatter into the term's columns
template <typename T>
__global__ __launch_bounds__(256)
void gram_grad_finish_kernel(const T* __restrict__ part, int nsplit, int64_t m, int Q, int d, const int32_t* cols, const T* __restrict__ inv_ls,
                             int combine, T* G, int64_t ldg, T* H, int negate_g)
{
	const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (idx >= m * Q) return;
	const int64_t t = idx / Q;
	const int q = (int)(idx - t * Q);
	T s = T(0);
	for (int sp = 0; sp < nsplit; ++sp) s += part[((int64_t)sp * m + t) * Q + q];
	T* o;
	if (q < d) {
		s = (s * inv_ls[q]) * inv_ls[q];
		if (negate_g) s = -s;                  // dot-product kinds: the sum ran over w1 * (0 - x_i)
		o = G + t * ldg + (cols ? cols[q] : q);
	} else {
		const int ka = (q - d) / d, kb = (q - d) - ka * d;
		s *= inv_ls[ka] * inv_ls[kb];
		o = H + (t * ldg + (cols ? cols[ka] : ka)) * ldg + (cols ? cols[kb] : kb);
	}
	*o = combine == STPY_OUT_ADD ? *o + s : s;
}

int64_t gram_grad_workspace_bytes(int64_t m, int64_t n, int d, int order, size_t esz)
{
	if (m <= 0 || n <= 0 || d <= 0) return 0;
	int Q, nqb, nsplit;
	int64_t chunk, ntiles;
	grad_plan(m, n, d, order, &Q, &nqb, &chunk, &nsplit, &ntiles);
	return (int64_t)nsplit * m * Q * (int64_t)esz;
}

template <typename T>
int gram_grad(int kind, const T* x, int64_t n, int64_t ldx, const T* xt, int64_t m, int64_t ldt, int d, const int32_t* cols, const T* inv_ls,
              double kappa, double offset, const T* alpha, const T* u, const T* Wt, int64_t ldw, const T* v, int order, int combine,
              T* G, int64_t ldg, T* H, void* work, hipStream_t st)
{
	GradArgs<T> p;
	int Q, nqb, nsplit;
	int64_t chunk, ntiles;
	grad_plan(m, n, d, order, &Q, &nqb, &chunk, &nsplit, &ntiles);
	p.x = x; p.xt = xt; p.cols = cols; p.inv_ls = inv_ls;
	p.alpha = alpha; p.u = u; p.Wt = Wt; p.v = v;
	p.part = (T*)work;
	p.ldx = ldx; p.ldt = ldt; p.ldw = ldw;
	p.n = n; p.m = m; p.chunk = chunk;
	p.d = d; p.Q = Q; p.nqb = nqb; p.nsplit = nsplit; p.ntiles = (int)ntiles;
	p.kappa = (T)kappa; p.offset = (T)offset;
	p.kind = kind & 0xff; p.degree = kind >> 8;
	const int64_t wgs = ntiles * nsplit * nqb;
	if (wgs > INT32_MAX) { set_error("stpy_gram_grad: %lld workgroups exceed one launch", (long long)wgs); return -7; }
	if (order == 2) hipLaunchKernelGGL((gram_grad_kernel<T, true>), dim3((unsigned)wgs), dim3(GG_THREADS), 0, st, p);
	else hipLaunchKernelGGL((gram_grad_kernel<T, false>), dim3((unsigned)wgs), dim3(GG_THREADS), 0, st, p);
	int rc = check_launch("stpy_gram_grad");
	if (rc) return rc;
	hipLaunchKernelGGL((gram_grad_finish_kernel<T>), dim3((unsigned)((m * Q + 255) / 256)), dim3(256), 0, st,
	                   (const T*)work, nsplit, m, Q, d, cols, inv_ls, combine, G, ldg, H,
	                   (int)(p.kind == STPY_K_LINEAR || p.kind == STPY_K_POLY));
	return check_launch("stpy_gram_grad finish");
}

// ---- B L^-1 through the order reversal J:  B L^-1 = (B J) Lr^-T J  with  Lr = J L^T J  (lower triangular).  The diagonal
// ---- 128-block c of Lr is J L_c'c'^T J (c' = nb - 1 - c), so its inverse is J W_c'^T J: both come from one anti-transpose.

// dst[i][j] = src[s - 1 - j][s - 1 - i] on an s x s window, one 32 x 32 tile per workgroup through LDS (both sides coalesced).
// blockIdx.z: window index (dst window z <- src window nwin - 1 - z, windows `wstride` elements apart: the winv blocks).
// Tiles of dst strictly above the diagonal are zeroed instead (the strict upper triangle of a factor is never read).
template <typename T>
__global__ __launch_bounds__(256)
void anti_transpose_kernel(const T* __restrict__ src, int64_t lds, T* __restrict__ dst, int64_t ldd, int64_t s, int64_t wstride, int nwin)
{
	__shared__ T tile[32][33];
	const int64_t bi = blockIdx.y, bj = blockIdx.x;         // dst tile (row block, column block)
	const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
	const T* sw = src + (int64_t)(nwin - 1 - (int)blockIdx.z) * wstride;
	T* dw = dst + (int64_t)blockIdx.z * wstride;
	if (bj > bi) {
		for (int r = ty; r < 32; r += 8) {
			const int64_t i = bi * 32 + r, j = bj * 32 + tx;
			if (i < s && j < s) dw[i * ldd + j] = T(0);
		}
		return;
	}
	// dst rows bi*32.. <- src columns s-1-(bi*32+..), dst columns bj*32.. <- src rows s-1-(bj*32+..)
	for (int r = ty; r < 32; r += 8) {
		const int64_t sr = s - 1 - (bj * 32 + r);           // src row for dst column bj*32 + r
		const int64_t sc = s - 32 - bi * 32 + tx;            // src columns of dst rows bi*32 + 31 - tx
		if (sr >= 0 && sc >= 0 && sc < s) tile[r][tx] = sw[sr * lds + sc];
	}
	__syncthreads();
	for (int r = ty; r < 32; r += 8) {
		const int64_t i = bi * 32 + r, j = bj * 32 + tx;
		// dst[i][j] = src[s-1-j][s-1-i]: src row s-1-j = row index (j - bj*32) = tx of the tile, src column s-1-i at tile column 31 - r
		if (i < s && j < s) dw[i * ldd + j] = tile[tx][31 - r];
	}
}

// B[r][c] <-> B[r][n-1-c]
template <typename T>
__global__ __launch_bounds__(256)
void flip_columns_kernel(T* B, int64_t ldb, int64_t row0, int64_t n)
{
	const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (c >= n / 2) return;
	T* row = B + (row0 + blockIdx.y) * ldb;
	const T a = row[c], b = row[n - 1 - c];
	row[c] = b;
	row[n - 1 - c] = a;
}

template <typename T>
static int flip_columns(int64_t m, int64_t n, T* B, int64_t ldb, hipStream_t st)
{
	if (n < 2) return 0;
	for (int64_t r0 = 0; r0 < m; r0 += 65535) {
		const int64_t rows = (m - r0 < 65535) ? (m - r0) : 65535;
		hipLaunchKernelGGL((flip_columns_kernel<T>), dim3((unsigned)((n / 2 + 255) / 256), (unsigned)rows), dim3(256), 0, st, B, ldb, r0, n);
	}
	return check_launch("trsm_right_ln flip");
}

template <typename T>
int reverse_factor(int64_t n, const T* L, int64_t ldl, const T* winv, T* Lr, int64_t ldlr, T* winvr, hipStream_t st)
{
	const int64_t nt = (n + 31) / 32;
	if (nt > 65535) { set_error("stpy_trsm_ln_factor: n too large for one launch"); return -2; }
	hipLaunchKernelGGL((anti_transpose_kernel<T>), dim3((unsigned)nt, (unsigned)nt, 1), dim3(256), 0, st, L, ldl, Lr, ldlr, n, (int64_t)0, 1);
	const int nb = (int)(n / IB);
	hipLaunchKernelGGL((anti_transpose_kernel<T>), dim3(IB / 32, IB / 32, (unsigned)nb), dim3(256), 0, st, winv, (int64_t)IB, winvr, (int64_t)IB,
	                   (int64_t)IB, (int64_t)IB * IB, nb);
	return check_launch("stpy_trsm_ln_factor");
}

template <typename T>
int trsm_right_ln(int64_t m, int64_t n, const T* Lr, int64_t ldlr, const T* winvr, T* B, int64_t ldb, int nb, hipStream_t st, T* work, int gflags)
{
	int rc = flip_columns<T>(m, n, B, ldb, st);
	if (rc) return rc;
	rc = trsm_right_lt<T>(m, n, Lr, ldlr, winvr, B, ldb, nb, st, false, work, gflags);
	if (rc) return rc;
	return flip_columns<T>(m, n, B, ldb, st);
}

}  // namespace stpy

using namespace stpy;

#define GG_DISPATCH(dtype, CALL64, CALL32)                                \
	do {                                                                  \
		if ((dtype) == STPY_F64) return CALL64;                           \
		if ((dtype) == STPY_F32) return CALL32;                           \
		set_error("unknown dtype %d (0 = float64, 1 = float32)", dtype);  \
		return -2;                                                        \
	} while (0)

extern "C" {

int64_t stpy_gram_grad_workspace_bytes(int dtype, int64_t m, int64_t n, int d, int order)
{
	return gram_grad_workspace_bytes(m, n, d, order, dtype == STPY_F32 ? 4 : 8);
}

int stpy_gram_grad(int kind, int dtype, const void* x, int64_t n, int64_t ldx, const void* xt, int64_t m, int64_t ldt,
                   int d, const int32_t* cols, const void* inv_ls, double kappa, double offset,
                   const void* alpha, const void* u, const void* Wt, int64_t ldw, const void* v,
                   int order, int combine, void* G, int64_t ldg, void* H, void* work, int64_t work_bytes, void* stream)
{
	if (m <= 0 || n <= 0) return 0;          // empty problem: nothing is written (empty tensors have null data pointers)
	const int fam = kind & 0xff, degree = kind >> 8;
	if (fam < STPY_K_SE || fam > STPY_K_POLY || (fam == STPY_K_POLY && (degree < 1 || degree > 64)) || (fam != STPY_K_POLY && degree != 0)) {
		set_error("stpy_gram_grad: unknown kernel kind %d", kind); return -1;
	}
	if (dtype != STPY_F64 && dtype != STPY_F32) { set_error("stpy_gram_grad: unknown dtype %d (0 = float64, 1 = float32)", dtype); return -2; }
	if (!x) { set_error("stpy_gram_grad: null pointer x"); return -3; }
	if (!xt) { set_error("stpy_gram_grad: null pointer xt"); return -6; }
	if (d <= 0) { set_error("stpy_gram_grad: d=%d must be positive", d); return -9; }
	if (ldx < 1 || ldt < 1 || (!cols && (ldx < d || ldt < d))) { set_error("stpy_gram_grad: leading dimensions ldx=%lld ldt=%lld below d=%d", (long long)ldx, (long long)ldt, d); return -5; }
	if (!inv_ls) { set_error("stpy_gram_grad: null pointer inv_ls"); return -11; }
	if (!alpha && !Wt) { set_error("stpy_gram_grad: neither alpha nor Wt given (no coefficients)"); return -14; }
	if (Wt && ldw < n) { set_error("stpy_gram_grad: ldw=%lld < n=%lld", (long long)ldw, (long long)n); return -17; }
	if (order != 1 && order != 2) { set_error("stpy_gram_grad: order %d (1 = gradient, 2 = gradient and Hessian)", order); return -19; }
	if (order == 2 && (fam == STPY_K_MATERN12 || fam == STPY_K_MATERN32)) {
		set_error("stpy_gram_grad: the %s kernel has no Hessian (singular at r = 0)", fam == STPY_K_MATERN12 ? "Matern 1/2" : "Matern 3/2"); return -19;
	}
	if (combine != STPY_OUT_SET && combine != STPY_OUT_ADD) { set_error("stpy_gram_grad: combine %d (SET or ADD)", combine); return -20; }
	if (!G) { set_error("stpy_gram_grad: null pointer G"); return -21; }
	if (ldg < 1 || (!cols && ldg < d)) { set_error("stpy_gram_grad: ldg=%lld below d=%d", (long long)ldg, d); return -22; }
	if (order == 2 && !H) { set_error("stpy_gram_grad: order 2 needs H"); return -23; }
	if (!work) { set_error("stpy_gram_grad: null workspace"); return -24; }
	const int64_t need = stpy_gram_grad_workspace_bytes(dtype, m, n, d, order);
	if (work_bytes < need) {
		set_error("stpy_gram_grad: workspace of %lld bytes, %lld needed (stpy_gram_grad_workspace_bytes)", (long long)work_bytes, (long long)need); return -25;
	}
	hipStream_t st = (hipStream_t)stream;
	GG_DISPATCH(dtype,
	            gram_grad<double>(kind, (const double*)x, n, ldx, (const double*)xt, m, ldt, d, cols, (const double*)inv_ls, kappa, offset,
	                              (const double*)alpha, (const double*)u, (const double*)Wt, ldw, (const double*)v, order, combine, (double*)G, ldg, (double*)H, work, st),
	            gram_grad<float>(kind, (const float*)x, n, ldx, (const float*)xt, m, ldt, d, cols, (const float*)inv_ls, kappa, offset,
	                             (const float*)alpha, (const float*)u, (const float*)Wt, ldw, (const float*)v, order, combine, (float*)G, ldg, (float*)H, work, st));
}

int stpy_trsm_ln_factor(int dtype, int64_t n, const void* L, int64_t ldl, const void* winv, int64_t winv_elems,
                        void* Lr, int64_t ldlr, void* winvr, void* stream)
{
	if (n <= 0) return 0;
	if (n % IB != 0) { set_error("stpy_trsm_ln_factor: n=%lld is not a multiple of %d (pad the factor with an identity border)", (long long)n, IB); return -2; }
	if (!L || !winv || !Lr || !winvr) { set_error("stpy_trsm_ln_factor: null pointer"); return -3; }
	if (ldl < n || ldlr < n) { set_error("stpy_trsm_ln_factor: leading dimensions ldl=%lld ldlr=%lld below n=%lld", (long long)ldl, (long long)ldlr, (long long)n); return -4; }
	if (winv_elems < stpy_potrf_winv_elems(n)) { set_error("stpy_trsm_ln_factor: winv holds %lld elements, %lld needed", (long long)winv_elems, (long long)stpy_potrf_winv_elems(n)); return -21; }
	hipStream_t st = (hipStream_t)stream;
	GG_DISPATCH(dtype,
	            reverse_factor<double>(n, (const double*)L, ldl, (const double*)winv, (double*)Lr, ldlr, (double*)winvr, st),
	            reverse_factor<float>(n, (const float*)L, ldl, (const float*)winv, (float*)Lr, ldlr, (float*)winvr, st));
}

int stpy_trsm_right_ln(int dtype, int64_t m, int64_t n, const void* Lr, int64_t ldlr, const void* winvr, int64_t winv_elems,
                       void* B, int64_t ldb, int nb, int flags, void* work, int64_t work_bytes, void* stream)
{
	if (m <= 0 || n <= 0) return 0;
	if (!Lr || !winvr || !B) { set_error("stpy_trsm_right_ln: null pointer"); return -4; }
	if (n % IB != 0) { set_error("stpy_trsm_right_ln: n=%lld is not a multiple of %d", (long long)n, IB); return -3; }
	if (winv_elems < stpy_potrf_winv_elems(n)) { set_error("stpy_trsm_right_ln: winv holds %lld elements, %lld needed", (long long)winv_elems, (long long)stpy_potrf_winv_elems(n)); return -7; }
	if (flags & ~STPY_FLAG_BESIDE_UPDATE) { set_error("stpy_trsm_right_ln: unknown flag bits 0x%x", flags); return -11; }
	if (ldlr < n || ldb < n) { set_error("stpy_trsm_right_ln: bad dimensions"); return -5; }
	if (work) {
		const int64_t need = stpy_trsm_workspace_bytes(dtype, m, n, nb);
		if (work_bytes < need) { set_error("stpy_trsm_right_ln: workspace of %lld bytes, %lld needed (stpy_trsm_workspace_bytes)", (long long)work_bytes, (long long)need); return -20; }
	}
	const int gf = (flags & STPY_FLAG_BESIDE_UPDATE) ? GEMM_BESIDE : 0;
	hipStream_t st = (hipStream_t)stream;
	GG_DISPATCH(dtype,
	            trsm_right_ln<double>(m, n, (const double*)Lr, ldlr, (const double*)winvr, (double*)B, ldb, nb, st, (double*)work, gf),
	            trsm_right_ln<float>(m, n, (const float*)Lr, ldlr, (const float*)winvr, (float*)B, ldb, nb, st, (float*)work, gf));
}

}  // extern "C"
