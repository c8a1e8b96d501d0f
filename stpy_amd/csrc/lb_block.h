// The one-workgroup building blocks of the small batched factorisations: the batched evidence (reduce.hip, lml_batch_kernel) and the local
// experts (experts.hip) -- 256 threads, 32 x 32 blocks, the fp64 MFMA for the panel products, one wave for a diagonal block.
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

}  // namespace stpy
