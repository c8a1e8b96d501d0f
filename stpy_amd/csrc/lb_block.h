// The one-workgroup building blocks of the small batched factorisations: the batched evidence (reduce.hip, lml_batch_kernel) and the local
// experts (experts.hip) -- 256 threads, 32 x 32 blocks, the fp64 MFMA for the panel products, one wave for a diagonal block -- and, built from
// them, the one-workgroup GP fit itself (lb_fit, at the end), which both kernels call.
#pragma once
#include "common.h"

namespace stpy {

constexpr int LB_MAX_N = 512;        // n the kernel accepts (stpy_lml_batch_max_n): z and alpha live in LDS
constexpr int LB_LDS = 34;           // row stride (doubles) of a staged 32-deep tile: rows 4 banks apart, so the 16 rows x 4 k of an MFMA operand
                                     // read (ds_read_b64, banks of 4 bytes, 64 of them) hit 64 different banks

__device__ __forceinline__ double lb_block_sum(double v, double* red4)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
	__syncthreads();                                   // (red4 may still be read from the previous call)
	if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
	__syncthreads();
	return ((red4[0] + red4[1]) + red4[2]) + red4[3];
}

__device__ __forceinline__ double lb_readlane(double v, int lane)
{
	const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
	return __hiloint2double(hi, lo);
}

// kappa-free kernel value and lengthscale-derivative factor F (d k / d l_m = kappa F u_m^2 / l_m) from the scaled squared distance
__device__ __forceinline__ double lb_phi(int kind, double r2)
{
	switch (kind) {
	case STPY_K_SE: return exp(-0.5 * r2);
	case STPY_K_MATERN12: return exp(-sqrt(r2));
	case STPY_K_MATERN32: { const double r = sqrt(r2) * 1.7320508075688772935; return (1.0 + r) * exp(-r); }
	default: { const double r = sqrt(r2) * 2.2360679774997896964; return (1.0 + r + r * r / 3.0) * exp(-r); }
	}
}

__device__ __forceinline__ double lb_dfactor(int kind, double r2)
{
	switch (kind) {
	case STPY_K_SE: return exp(-0.5 * r2);
	case STPY_K_MATERN12: { const double r = sqrt(r2); return r > 0.0 ? exp(-r) / r : 0.0; }          // direct differences: coincident points give r = 0 exactly
	case STPY_K_MATERN32: return 3.0 * exp(-sqrt(r2) * 1.7320508075688772935);
	default: { const double r = sqrt(r2) * 2.2360679774997896964; return (5.0 / 3.0) * (1.0 + r) * exp(-r); }
	}
}

// C[r][c] (r < m, c < 32)  =  (MODE 0)  /  -=  (MODE 1)  /  = -  (MODE 2)   sum_k A[r][k] B[c][k]  over k in [k0, kend) in steps of 32, on the fp64
// MFMA: 64 rows per round, wave w the 16 rows 16 w.. and both 16-column halves.  tri_row0 >= 0: A is upper triangular with its row 0 at column
// tri_row0, and the round that starts at row r0 begins at k0 = tri_row0 + r0 (what lies left of the diagonal block in the round's second 32 rows
// is stored as zero); otherwise k0 = 0.  m, kend multiples of 32; the chunk after the one being multiplied is already on its way into registers.
// C may be the A tile itself when there is ONE chunk (kend = 32): a round's operands are in LDS before its results are stored.
template <int MODE>
__device__ void lb_panel(double* C, int ldc, const double* A, int lda, const double* B, int ldb, int m, int kend, int tri_row0,
                         double* As, double* Bs)
{
	typedef Mfma<double>::v4 v4;
	typedef Mfma<double>::v2 v2;
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	const int ar = tid >> 2, ak = (tid & 3) * 8;          // A tile (64 x 32): this thread's row and the first of its 8 k
	const int br = tid >> 3, bk = (tid & 7) * 4;          // B tile (32 x 32): row, first of 4 k
	const int fr = lane & 15, fk = lane >> 4;             // MFMA operand fragment: row / column of the tile, k within the step of 4
	__syncthreads();                                      // (what the caller's previous step stored is read below; As / Bs are free)
	for (int r0 = 0; r0 < m; r0 += 64) {
		const int k0 = tri_row0 >= 0 ? tri_row0 + r0 : 0;
		const bool arow = r0 + ar < m;
		const double* ap = A + (int64_t)(r0 + ar) * lda + ak;
		const double* bp = B + (int64_t)br * ldb + bk;
		v2 ra[4], rb[2];
		auto fetch = [&](int kc) {
#pragma unroll
			for (int e = 0; e < 4; ++e) ra[e] = arow ? *reinterpret_cast<const v2*>(ap + kc + 2 * e) : v2{0.0, 0.0};
#pragma unroll
			for (int e = 0; e < 2; ++e) rb[e] = *reinterpret_cast<const v2*>(bp + kc + 2 * e);
		};
		v4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
		if (k0 < kend) fetch(k0);
		for (int kc = k0; kc < kend; kc += 32) {
#pragma unroll
			for (int e = 0; e < 4; ++e) *reinterpret_cast<v2*>(As + ar * LB_LDS + ak + 2 * e) = ra[e];
#pragma unroll
			for (int e = 0; e < 2; ++e) *reinterpret_cast<v2*>(Bs + br * LB_LDS + bk + 2 * e) = rb[e];
			__syncthreads();
			if (kc + 32 < kend) fetch(kc + 32);
#pragma unroll
			for (int kk = 0; kk < 8; ++kk) {
				const double a = As[(16 * w + fr) * LB_LDS + 4 * kk + fk];
				const double b0 = Bs[fr * LB_LDS + 4 * kk + fk], b1 = Bs[(16 + fr) * LB_LDS + 4 * kk + fk];
				acc0 = Mfma<double>::mma(a, b0, acc0);
				acc1 = Mfma<double>::mma(a, b1, acc1);
			}
			__syncthreads();
		}
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			const int row = r0 + 16 * w + Mfma<double>::crow(lane, i);
			if (row < m) {
				double* c = C + (int64_t)row * ldc + fr;
				if (MODE == 0) { c[0] = acc0[i]; c[16] = acc1[i]; }
				else if (MODE == 1) { c[0] -= acc0[i]; c[16] -= acc1[i]; }
				else { c[0] = -acc0[i]; c[16] = -acc1[i]; }
			}
		}
	}
}

// One wave: Cholesky of the 32 x 32 diagonal block at (j0, j0) of A (lower triangle read; written back with a zero upper part) and its inverse,
// to dinv (row-major) and, transposed, to the diagonal block of V.  Lane r (and r + 32, which only mirrors it) holds row r in registers;
// column j travels by v_readlane; the inverse is formed in LDS.  Ds: 2 x 32 x 33 doubles of LDS no other wave touches meanwhile.  Returns 0,
// or the 1-based index within the block of the first pivot that is not positive and finite (wave-uniform; nothing is stored then).
__device__ int lb_diag(double* A, double* V, int ld, int j0, double* dinv, double* Ds)
{
	const int lane = threadIdx.x & 63, row = lane & 31;
	double a[32];
	double* blk = A + (int64_t)(j0 + row) * ld + j0;
#pragma unroll
	for (int c = 0; c < 32; ++c) a[c] = blk[c];
	int bad = 0;
#pragma unroll
	for (int j = 0; j < 32; ++j) {
		const double piv = lb_readlane(a[j], j);
		if (bad == 0 && !(piv > 0.0 && piv < __builtin_huge_val())) bad = j + 1;
		const double dj = sqrt(piv), rj = 1.0 / dj;
		a[j] = row > j ? a[j] * rj : (row == j ? dj : 0.0);
#pragma unroll
		for (int c = j + 1; c < 32; ++c) a[c] = fma(-a[j], lb_readlane(a[j], c), a[c]);
	}
	if (bad != 0) return bad;
	// column `row` of the inverse by forward substitution; L[i][k] is read from the copy in LDS (one address per wave: a broadcast)
	if (lane < 32) {
#pragma unroll
		for (int c = 0; c < 32; ++c) {
			blk[c] = a[c];
			Ds[row * 33 + c] = a[c];
		}
	}
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
	// (rolled loops over LDS on purpose: unrolled over a register array the 528 independent reads are all hoisted and spill)
	double* Wl = Ds + 32 * 33;          // the inverse, Wl[i * 33 + c] = (L^-1)[i][c]: lane c owns column c
	for (int i = 0; i < 32; ++i) {
		double s = i == row ? 1.0 : 0.0;
#pragma unroll 4
		for (int k = 0; k < i; ++k) s = fma(-Ds[i * 33 + k], Wl[k * 33 + row], s);
		if (lane < 32) Wl[i * 33 + row] = s / Ds[i * 33 + i];
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
	}
	// dinv[i][c] and V[j0 + c][j0 + i] = (L^-1)[i][c]
	for (int t = lane; t < 1024; t += 64) {
		const int i = t >> 5, c = t & 31;
		const double v = Wl[i * 33 + c];
		dinv[t] = v;
		V[(int64_t)(j0 + c) * ld + j0 + i] = v;
	}
	return 0;
}

// scaled squared distance of two rows from direct coordinate differences: the one evaluator of the fit and of the experts' k*, so a test point
// that is a training point gets the bits the fit saw
__device__ __forceinline__ double lb_r2(const double* __restrict__ xi, const double* __restrict__ xj, const int32_t* __restrict__ cols,
                                        const double* __restrict__ il, int d)
{
	double s = 0.0;
	for (int k = 0; k < d; ++k) {
		const int c = cols ? cols[k] : k;
		const double u = (xi[c] - xj[c]) * il[k];
		s = fma(u, u, s);
	}
	return s;
}

// ------------------------------------------------------------------------------------------
// lb_fit<GRAD, ALPHA>: ONE exact GP fit by ONE workgroup of 256 threads -- the body of lml_batch_kernel (reduce.hip: a candidate's hyper-parameters on
// the shared data) and of experts_fit_kernel<GRAD> (experts.hip: an expert's rows under the shared hyper-parameters).  The two kernels are shells
// that work out whose operands these are; the arithmetic exists here, once.
//
// Operands: n points (rows of x, stride ldx, coordinates cols[0..d) or 0..d), targets y, inverse lengthscales il[d], noise sd, prior variance
// kappa, log-determinant weight wgt; A, V: NP x NP row-major, NP = n rounded up to the block of 32, bordered by an identity (of V only the upper
// triangle, its block diagonal and the blocks just below that are written); dinv: the NP / 32 inverse diagonal blocks.
//   1. A <- lower blocks of K = kappa phi(|(x_i - x_j)[cols] o il|) + sd^2 I from direct coordinate differences;
//   2. blocked left-looking Cholesky in place: panel -= (rows left of it) (its own rows left of it)^T on the fp64 MFMA, the 32 x 32
//      diagonal block factored and inverted by one wave in registers (lb_diag), the rows below it times the inverse block on the MFMA again;
//   3. V <- L^-T (upper triangular, row-major = W^T for W = L^-1), block column by block column from V's finished part;
//   4. z = W y, alpha = W^T z (LDS; with ALPHA also stored to `alpha`), value = 1/2 |z|^2 + wgt sum log L_ii;
//   with GRAD also
//   5. A <- K^-1 = V V^T (lower blocks), H = (wgt K^-1 - alpha alpha^T) o kappa F in place over it, the per-coordinate sums over i > j, four
//      coordinates per pass over H, added into grow[pidx[m]] (slots outside [0, np) dropped), and grow[np] = d/d sd.
// A pivot that is not positive and finite ends the fit: value = +inf, info = its 1-based index, alpha (with ALPHA) zero, grow left as zeroed.
// (ALPHA is a template flag and not a null test: tested at run time the alpha loop is unswitched and its LDS reads change.)
// Every sum has a fixed order (per-thread partial sums over a fixed set of entries, shuffle tree, four wave partials in index order), and the
// fit reads nothing another workgroup writes: its outputs are bit-identical wherever it sits in whatever batch.
// Barriers: every __syncthreads() below is reached by the whole workgroup -- the caller enters with all 256 threads (its own early exits test
// workgroup-uniform words), the loops around the barriers run over workgroup-uniform ranges, the single-wave diagonal-block step has no barrier
// inside, a failed pivot is published through LDS and read by all threads behind a barrier, and GRAD / ALPHA are compile-time: so the
// workgroup leaves as a whole, at the failed pivot, after the value (no GRAD) or at the end.
// The lb_diag call is always_inline: with several instances of this body in one translation unit the inliner would otherwise leave a call, and
// with it a stack (248 VGPRs, 36 bytes of scratch, one workgroup per CU instead of two).
// ------------------------------------------------------------------------------------------
struct LbFit {
	const double* x; int64_t ldx; int n, d; const int32_t* cols; const double* y; const double* il;
	double sd, kappa, wgt; const int32_t* pidx; int np, kind;
	double* A; double* V; double* dinv;
	double* alpha;          // n entries; read only with ALPHA
	double* value; double* grow; int32_t* info;          // this fit's entry / row; grow (np + 1 entries) is read only with GRAD
};

template <bool GRAD, bool ALPHA>
__device__ __forceinline__ void lb_fit(const LbFit& p)
{
	__shared__ __attribute__((aligned(16))) double As[64 * LB_LDS];
	__shared__ __attribute__((aligned(16))) double Bs[32 * LB_LDS];
	__shared__ double zs[LB_MAX_N], al[LB_MAX_N], red[4];
	__shared__ int s_info;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int n = p.n, NP = (n + 31) & ~31, nblk = NP >> 5, ld = NP;
	const double* x = p.x;
	const double* il = p.il;
	double* A = p.A;
	double* V = p.V;
	double* dinv = p.dinv;
	double* grow = p.grow;
	const double sd = p.sd, s2 = sd * sd, kappa = p.kappa, wgt = p.wgt;
	const int ec = tid & 31, er = tid >> 5;              // entry of a 32 x 32 block in the elementwise passes: column, first of 4 rows (8 apart)
	if (tid == 0) {
		s_info = 0;
		if (GRAD)
			for (int k = 0; k <= p.np; ++k) grow[k] = 0.0;
	}

	// ---- 1. lower blocks of K (whole diagonal blocks), identity border; the blocks of V just below its diagonal are stored as zero
	for (int bi = 0; bi < nblk; ++bi)
		for (int bj = 0; bj <= bi; ++bj)
#pragma unroll
			for (int q = 0; q < 4; ++q) {
				const int i = 32 * bi + er + 8 * q, j = 32 * bj + ec;
				double v = i == j ? 1.0 : 0.0;
				if (i < n && j < n) v = kappa * lb_phi(p.kind, lb_r2(x + (int64_t)i * p.ldx, x + (int64_t)j * p.ldx, p.cols, il, p.d)) + (i == j ? s2 : 0.0);
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
			int bad;
			[[clang::always_inline]] bad = lb_diag(A, V, ld, j0, dinv + bk * 1024, As);
			if (bad != 0 && lane == 0) s_info = j0 + bad;
		}
		__syncthreads();
		if (s_info != 0) {          // (the same word for every thread: the workgroup leaves as a whole)
			if (p.alpha)
				for (int i = tid; i < n; i += 256) p.alpha[i] = 0.0;
			if (tid == 0) {
				*p.value = __builtin_huge_val();
				*p.info = s_info;
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
	for (int i = tid; i < n; i += 256) {
		quad = fma(zs[i], zs[i], quad);
		aa = fma(al[i], al[i], aa);
		if (ALPHA) p.alpha[i] = al[i];
	}
	quad = lb_block_sum(quad, red);
	if (!GRAD) {
		if (tid == 0) {
			*p.value = 0.5 * quad + wgt * logdiag;
			*p.info = 0;
		}
		return;
	}
	aa = lb_block_sum(aa, red);

	// ---- 5. K^-1 = V V^T over A's lower blocks (L is no longer needed), then H = (w K^-1 - alpha alpha^T) o kappa F below the diagonal
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
					else h = (wgt * kv - al[i] * al[j]) * kappa * lb_dfactor(p.kind, lb_r2(x + (int64_t)i * p.ldx, x + (int64_t)j * p.ldx, p.cols, il, p.d));
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
						const double* xi = x + (int64_t)i * p.ldx;
						const double* xj = x + (int64_t)j * p.ldx;
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
		*p.value = 0.5 * quad + wgt * logdiag;
		grow[p.np] = sd * (wgt * tr - aa);
		*p.info = 0;
	}
}

}  // namespace stpy
