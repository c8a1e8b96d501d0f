// Values, query-point gradients AND query-point Hessians of kernel sums generated on the fly (stpy_kmv_dxx): for n query points a_i, q contracted
// points b_j and t coefficient rows Vt (t x q), with e_ijk = (a_i - b_j)[cols[k]] * inv_ls[k], rho = sum_k e_k^2, chi = 2 dphi/drho, psi = 2 dchi/drho,
//   out[c, i, k]                     = inv_ls[k] sum_j Vt[c, j] kappa chi e_ijk                                      k < d   (as stpy_kmv_dx)
//   out[c, i, d]                     =           sum_j Vt[c, j] kappa phi                                                     (as stpy_kmv_dx)
//   out[c, i, d + 1 + k(k+1)/2 + l]  = inv_ls[k] inv_ls[l] sum_j Vt[c, j] kappa (psi e_ijk e_ijl + chi [k == l])     l <= k < d
// (out[c, i, p] at c ldc + i ldo + p): the lower triangle of the Hessian with respect to a_i[cols], row by row.  The kernel matrix is never formed.
// With Vt = alpha^T this is the posterior mean, its input gradient and its input Hessian.
//
// A sibling of stpy_kmv_dx (kmvdx.hip) with its launch shape: a workgroup of four waves owns 64 query points i, 16 per wave, ONE block of 16 rows
// c and ONE GROUP of output columns, and walks j in chunks of 64 through LDS.  The 16x16x4 MFMA runs with A = a fragment of Vt (row = c, k = j) and
// B = the ONE value each lane evaluates for the pair (i, j) its operand slot wants.  The 1 + d + d(d+1)/2 columns (153 at d = 16) do not fit the
// register file, so the lane re-evaluates the pair (the d scaled differences, rho, phi, chi, psi: kdd_phi_chi_psi, the evaluator of pchol.hip) once
// per group and issues at most DC + 1 MFMAs against the same A fragment.  The groups (blockIdx.z walks them as well):
//   group 0              the d gradient columns and the value column: the arithmetic of stpy_kmv_dx;
//   group g = 1 .. ceil(d/2)   Hessian rows k1 = g - 1 and k2 = d - g (one row where they meet): (k1 + 1) + (k2 + 1) = d + 1 columns, so every group
//                        carries the same load.  Row k1 accumulates in acc[l], row k2 in acc[DC - l]: the two ranges are disjoint (DC - k2 >= g > k1).
// Coordinates are indexed by compile-time constants (DC = 4, 8, 16 in registers; l <= k is a uniform branch); the ROW's own difference, whose
// index comes from blockIdx, is formed again from LDS with the same two operations (the same bits as the register copy).  Every accumulator is a
// C = D chain on its own, fully live tuple (the fp64 rule of potrf.hip).  d > 16 is refused.
// Epilogue: columns are scaled (inv_ls[k]; inv_ls[k] inv_ls[l]) and the tile is stored.  With too few workgroups to fill the chip the j range is cut
// into blockIdx.y pieces as in stpy_kmv_dx; the pieces' tiles land in `work` unscaled and a second launch adds them in piece order, scales and
// stores.  No atomics, no spin-waits, no cooperative grid, no scratch; the same bits on every call and for every lda / ldb / ldv / ldc / ldo.
// A pair with rho == 0 contributes exactly 0 to the gradient and kappa chi(0) [k == l] (times the scales) to the Hessian: its e_k are 0.
// SE and MATERN52 only: chi of MATERN12 / MATERN32 has no finite derivative at rho = 0.
#ifndef STPY_KMVDXX_HIP
#define STPY_KMVDXX_HIP
#include "common.h"
#include "pchol.hip"          // pc_phi / pc_fma: the one direct-difference evaluator
#include "kmvgrad.hip"        // kd_phi_chi, kd_exp: phi and chi = 2 dphi/drho as stpy_kmv_dtheta evaluates them

#include <math.h>

namespace stpy {

namespace {

constexpr int KXX_THREADS = 256;
constexpr int KXX_TILE = 64;            // query points of a workgroup (16 per wave)
constexpr int KXX_JC = 64;              // contracted points per LDS chunk
constexpr int KXX_PB = 16;              // coefficient rows of a workgroup: one MFMA row block
constexpr int KXX_VS = KXX_PB + 1;      // row stride of the Vt block in LDS
constexpr int KXX_FILL = 256;           // below this many workgroups the j range is cut ...
constexpr int KXX_SPLIT_TARGET = 512;   // ... into pieces, up to this many workgroups
constexpr int KXX_MAX_SPLIT = 512;
constexpr int KXX_SPLIT_MIN_J = 4 * KXX_JC;
constexpr int KXX_MAX_D = 16;
constexpr int KXX_RED_BLOCKS = 1 << 20; // the second launch walks its elements with a grid stride from at most this many workgroups

template <typename T>
struct KxxArgs {
	const T* a; int64_t lda; int n; const T* b; int64_t ldb; int q; int d; const int32_t* cols; const T* inv_ls; T kappa; int kind;
	const T* Vt; int64_t ldv; int t; T* out; int64_t ldc, ldo; T* part; int nsplit, jper, ngroups, ncol;
};

// phi, chi = 2 dphi/drho (kd_phi_chi: the bits of stpy_kmv_dx) and psi = 2 dchi/drho, for SE and MATERN52
template <typename T>
__device__ __forceinline__ void kdd_phi_chi_psi(int kind, T rho, T& phi, T& chi, T& psi)
{
	kd_phi_chi(kind, rho, phi, chi);
	if (kind == STPY_K_SE) {
		psi = phi;
	} else {
		const T r = pc_sqrt(rho) * (T)2.2360679774997896964;
		psi = (T)(25.0 / 3.0) * kd_exp(-r);
	}
}

// output columns of a point: d gradients, the value, the lower triangle row by row
inline int64_t kxx_ncol(int d) { return 1 + (int64_t)d + (int64_t)d * (d + 1) / 2; }
inline int kxx_groups(int d) { return 1 + (d + 1) / 2; }

// DC: coordinates held in registers (d <= DC)
template <typename T, int DC>
__global__ __launch_bounds__(KXX_THREADS)
void kmvxx_kernel(KxxArgs<T> g)
{
	typedef typename Mfma<T>::v4 v4;
	__shared__ T sv[KXX_JC][KXX_VS];
	__shared__ T sb[DC][KXX_JC];
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
	const int64_t i0 = (int64_t)blockIdx.x * KXX_TILE;
	const int64_t i = i0 + 16 * w + li;
	const int grp = (int)blockIdx.z % g.ngroups;                       // column group of the outputs
	const int c0 = ((int)blockIdx.z / g.ngroups) * KXX_PB;
	const int k1 = grp > 0 ? grp - 1 : 0, k2 = grp > 0 ? g.d - grp : 0;       // the group's Hessian rows (k1 <= k2 < d <= DC)
	const bool two = grp > 0 && k2 > k1;
	const int64_t jb64 = (int64_t)blockIdx.y * g.jper;
	const int jb = jb64 < g.q ? (int)jb64 : g.q, je = jb64 + g.jper < g.q ? (int)(jb64 + g.jper) : g.q;
	v4 acc[DC + 1];
#pragma unroll
	for (int k = 0; k <= DC; ++k) acc[k] = v4{(T)0, (T)0, (T)0, (T)0};
	T av[DC], il[DC];
#pragma unroll
	for (int k = 0; k < DC; ++k) {
		const bool in = k < g.d;
		const int c = in ? (g.cols ? g.cols[k] : k) : 0;
		il[k] = in ? g.inv_ls[k] : (T)0;
		av[k] = (in && i < g.n) ? g.a[i * g.lda + c] : (T)0;
	}
	// the rows' own coordinate of a_i and lengthscale: the same loads as av[k1] / il[k1], by a run-time index that registers do not have
	const T il1 = g.inv_ls[k1], il2 = g.inv_ls[k2];
	const T a1 = i < g.n ? g.a[i * g.lda + (g.cols ? g.cols[k1] : k1)] : (T)0;
	const T a2 = i < g.n ? g.a[i * g.lda + (g.cols ? g.cols[k2] : k2)] : (T)0;
	for (int64_t j0 = jb; j0 < je; j0 += KXX_JC) {                        // (64 bits: j0 + 64 may pass 2^31)
		__syncthreads();                                              // (the previous chunk has been read)
		for (int cc = w; cc < KXX_PB; cc += 4) {
			const int c = c0 + cc;
			const int64_t j = j0 + lane;
			sv[lane][cc] = (c < g.t && j < je) ? g.Vt[(int64_t)c * g.ldv + j] : (T)0;
		}
		for (int e = tid; e < DC * KXX_JC; e += KXX_THREADS) {
			const int k = e >> 6, jj = e & 63;
			const int64_t j = j0 + jj;
			sb[k][jj] = (k < g.d && j < je) ? g.b[j * g.ldb + (g.cols ? g.cols[k] : k)] : (T)0;
		}
		__syncthreads();
		if (grp == 0) {
#pragma unroll 1
			for (int s = 0; s < 16; ++s) {
				const int jj = 4 * s + lk;
				T ek[DC], rho = (T)0;
#pragma unroll
				for (int k = 0; k < DC; ++k) {
					const T df = (av[k] - sb[k][jj]) * il[k];
					ek[k] = df;
					rho = pc_fma(df, df, rho);
				}
				T phi, chi;
				kd_phi_chi(g.kind, rho, phi, chi);
				const bool in = j0 + jj < je;
				const T wchi = (in && rho != (T)0) ? g.kappa * chi : (T)0;
				const T wphi = in ? g.kappa * phi : (T)0;
				const T a = sv[jj][li];
#pragma unroll
				for (int k = 0; k < DC; ++k) acc[k] = Mfma<T>::mma(a, wchi * ek[k], acc[k]);
				acc[DC] = Mfma<T>::mma(a, wphi, acc[DC]);
			}
		} else {
#pragma unroll 1
			for (int s = 0; s < 16; ++s) {
				const int jj = 4 * s + lk;
				T ek[DC], rho = (T)0;
#pragma unroll
				for (int k = 0; k < DC; ++k) {
					const T df = (av[k] - sb[k][jj]) * il[k];
					ek[k] = df;
					rho = pc_fma(df, df, rho);
				}
				T phi, chi, psi;
				kdd_phi_chi_psi(g.kind, rho, phi, chi, psi);
				const bool in = j0 + jj < je;
				const T wchi = in ? g.kappa * chi : (T)0;
				const T wpsi = in ? g.kappa * psi : (T)0;
				const T a = sv[jj][li];
				const T p1 = wpsi * ((a1 - sb[k1][jj]) * il1);
#pragma unroll
				for (int l = 0; l < DC; ++l)
					if (l <= k1) acc[l] = Mfma<T>::mma(a, pc_fma(p1, ek[l], l == k1 ? wchi : (T)0), acc[l]);
				if (two) {
					const T p2 = wpsi * ((a2 - sb[k2][jj]) * il2);
#pragma unroll
					for (int l = 0; l < DC; ++l)
						if (l <= k2) acc[DC - l] = Mfma<T>::mma(a, pc_fma(p2, ek[l], l == k2 ? wchi : (T)0), acc[DC - l]);
				}
			}
		}
	}
	// D[row = c][col = i]: the group's columns of (c, i), straight to out (scaled) or, as one of several pieces, to `work` (unscaled)
	if (i >= g.n) return;
	const bool direct = g.nsplit <= 1;
#pragma unroll
	for (int r = 0; r < 4; ++r) {
		const int c = c0 + Mfma<T>::crow(lane, r);
		if (c >= g.t) continue;
		T* dst = direct ? g.out + (int64_t)c * g.ldc + i * g.ldo : g.part + (((int64_t)blockIdx.y * g.t + c) * g.n + i) * g.ncol;
		if (grp == 0) {
#pragma unroll
			for (int k = 0; k < DC; ++k)
				if (k < g.d) dst[k] = direct ? il[k] * acc[k][r] : acc[k][r];
			dst[g.d] = acc[DC][r];
		} else {
			T* h1 = dst + g.d + 1 + k1 * (k1 + 1) / 2;
#pragma unroll
			for (int l = 0; l < DC; ++l)
				if (l <= k1) h1[l] = direct ? (il1 * il[l]) * acc[l][r] : acc[l][r];
			if (two) {
				T* h2 = dst + g.d + 1 + k2 * (k2 + 1) / 2;
#pragma unroll
				for (int l = 0; l < DC; ++l)
					if (l <= k2) h2[l] = direct ? (il2 * il[l]) * acc[DC - l][r] : acc[DC - l][r];
			}
		}
	}
}

// out = the pieces added in piece order, columns scaled as the direct store scales them; with nsplit == 0 (q == 0) the zero fill
template <typename T>
__global__ __launch_bounds__(KXX_THREADS)
void kmvxx_reduce_kernel(KxxArgs<T> g)
{
	const int64_t nc = g.ncol, total = (int64_t)g.t * g.n * nc;
	for (int64_t e = (int64_t)blockIdx.x * KXX_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * KXX_THREADS) {
		const int p = (int)(e % nc);
		const int64_t ci = e / nc, c = ci / g.n, i = ci % g.n;
		T v = (T)0;
		for (int s = 0; s < g.nsplit; ++s) v += g.part[(int64_t)s * total + e];
		if (g.nsplit > 0) {
			if (p < g.d) {
				v = g.inv_ls[p] * v;
			} else if (p > g.d) {
				int k = 0, h = p - g.d - 1;                             // h = k (k + 1) / 2 + l, l <= k
				while ((k + 1) * (k + 2) / 2 <= h) ++k;
				const int l = h - k * (k + 1) / 2;
				v = (g.inv_ls[k] * g.inv_ls[l]) * v;
			}
		}
		g.out[c * g.ldc + i * g.ldo + p] = v;
	}
}

// pieces of the j range for (n, q, d, t): 1 unless the workgroups leave most of the chip idle; 0 for q == 0
inline int kxx_nsplit(int64_t n, int64_t q, int d, int64_t t)
{
	if (q < 1) return 0;
	const int64_t tiles = ((n + KXX_TILE - 1) / KXX_TILE) * ((t + KXX_PB - 1) / KXX_PB) * kxx_groups(d);
	if (tiles >= KXX_FILL) return 1;
	int64_t s = (KXX_SPLIT_TARGET + tiles - 1) / tiles;
	const int64_t by_q = (q + KXX_SPLIT_MIN_J - 1) / KXX_SPLIT_MIN_J;
	if (s > by_q) s = by_q;
	if (s > KXX_MAX_SPLIT) s = KXX_MAX_SPLIT;
	return s < 1 ? 1 : (int)s;
}

// Room for one unscaled (t, n, ncol) tile set per piece of a cut j range, as an envelope that does not decrease in n, q or t (a caller may size one
// buffer for its largest problem): the pieces s are at most S = min(ceil(q / 256), ceil(512 / groups)), and a range is only cut below KXX_FILL
// workgroups, where s t n <= (512 / tiles + 1) t n < 768 * 1024 / groups (t n <= 1024 tiles / groups, tiles < 256).  So min(S t n, that cap) ncol
// elements always suffice; nothing where q <= 256 (never cut).
inline int64_t kxx_workspace_bytes(int dtype, int64_t n, int64_t q, int d, int64_t t)
{
	const int64_t esz = dtype == STPY_F32 ? 4 : 8;
	if (n < 1) n = 1;
	if (t < 1) t = 1;
	if (d < 1) d = 1;
	if (d > KXX_MAX_D) d = KXX_MAX_D;
	const int64_t groups = kxx_groups(d);
	int64_t S = q < 1 ? 0 : (q + KXX_SPLIT_MIN_J - 1) / KXX_SPLIT_MIN_J;
	const int64_t by_groups = (KXX_SPLIT_TARGET + groups - 1) / groups;
	if (S > by_groups) S = by_groups;
	if (S > KXX_MAX_SPLIT) S = KXX_MAX_SPLIT;
	int64_t elems = 0;
	if (S > 1) {
		const int64_t cap = (int64_t)(KXX_SPLIT_TARGET + KXX_FILL) * KXX_TILE * KXX_PB / groups;
		elems = (t <= cap / n && S <= cap / (t * n)) ? S * t * n : cap;
		elems *= kxx_ncol(d);
	}
	return (elems * esz + 255) / 256 * 256 + 256;
}

template <typename T>
int kmv_dxx(int kind, const T* a, int64_t n, int64_t lda, const T* b, int64_t q, int64_t ldb, int d, const int32_t* cols, const T* inv_ls, double kappa,
            const T* Vt, int64_t ldv, int64_t t, T* out, int64_t ldc, int64_t ldo, void* work, hipStream_t st)
{
	const int nsplit = kxx_nsplit(n, q, d, t);
	const int ngroups = kxx_groups(d);
	int64_t jper = q;
	if (nsplit > 1) {
		jper = (q + nsplit - 1) / nsplit;
		jper = (jper + KXX_JC - 1) / KXX_JC * KXX_JC;
	}
	KxxArgs<T> g{a, lda, (int)n, b, ldb, (int)q, d, cols, inv_ls, (T)kappa, kind, Vt, ldv, (int)t, out, ldc, ldo, (T*)work, nsplit, (int)jper, ngroups, (int)kxx_ncol(d)};
	if (nsplit >= 1) {
		const dim3 grid((unsigned)((n + KXX_TILE - 1) / KXX_TILE), (unsigned)nsplit, (unsigned)(((t + KXX_PB - 1) / KXX_PB) * ngroups));
		if (d <= 4) hipLaunchKernelGGL((kmvxx_kernel<T, 4>), grid, dim3(KXX_THREADS), 0, st, g);
		else if (d <= 8) hipLaunchKernelGGL((kmvxx_kernel<T, 8>), grid, dim3(KXX_THREADS), 0, st, g);
		else hipLaunchKernelGGL((kmvxx_kernel<T, 16>), grid, dim3(KXX_THREADS), 0, st, g);
	}
	if (nsplit != 1) {
		const int64_t blocks = (t * n * kxx_ncol(d) + KXX_THREADS - 1) / KXX_THREADS;
		hipLaunchKernelGGL(kmvxx_reduce_kernel<T>, dim3((unsigned)(blocks < KXX_RED_BLOCKS ? blocks : KXX_RED_BLOCKS)), dim3(KXX_THREADS), 0, st, g);
	}
	return check_launch("stpy_kmv_dxx");
}

}  // namespace

}  // namespace stpy

// ---- C ABI (include/stpy_hip.h); every refusal below comes before the first HIP call
using namespace stpy;

extern "C" {

int64_t stpy_kmv_dxx_workspace_bytes(int dtype, int64_t n, int64_t q, int d, int64_t t)
{
	return kxx_workspace_bytes(dtype, n, q, d, t);
}

int stpy_kmv_dxx(int kind, int dtype, const void* a, int64_t n, int64_t lda, const void* b, int64_t q, int64_t ldb,
                 int d, const int32_t* cols, const void* inv_ls, double kappa,
                 const void* Vt, int64_t ldv, int64_t t,
                 void* out, int64_t ldc, int64_t ldo, void* work, int64_t work_bytes, void* stream)
{
	if (kind != STPY_K_SE && kind != STPY_K_MATERN52) {
		set_error("stpy_kmv_dxx: kernel kind %d has no second derivative here (SE and MATERN52 only: MATERN12 / MATERN32 are singular at r = 0)", kind);
		return -1;
	}
	if (dtype != STPY_F64 && dtype != STPY_F32) { set_error("stpy_kmv_dxx: unknown dtype %d (0 = float64, 1 = float32)", dtype); return -2; }
	if (n < 0 || n >= ((int64_t)1 << 31) || q < 0 || q >= ((int64_t)1 << 31)) { set_error("stpy_kmv_dxx: n=%lld or q=%lld outside [0, 2^31)", (long long)n, (long long)q); return -4; }
	if (n == 0) return 0;          // empty output: nothing to write
	if (d < 1 || d > KXX_MAX_D) { set_error("stpy_kmv_dxx: d=%d outside [1, %d]", d, KXX_MAX_D); return -6; }
	const int64_t zblocks = (t < 1 ? 0 : (t + KXX_PB - 1) / KXX_PB) * kxx_groups(d);
	if (t < 1 || zblocks > 65535) { set_error("stpy_kmv_dxx: t=%lld outside [1, 65535 * 16 / groups] (groups = 1 + ceil(d / 2))", (long long)t); return -10; }
	if (lda < d || ldb < d) { set_error("stpy_kmv_dxx: lda=%lld or ldb=%lld below d=%d", (long long)lda, (long long)ldb, d); return -5; }
	if (ldv < q) { set_error("stpy_kmv_dxx: ldv=%lld below q=%lld", (long long)ldv, (long long)q); return -13; }
	const int64_t ncol = kxx_ncol(d);
	if (ldo < ncol) { set_error("stpy_kmv_dxx: ldo=%lld below 1 + d + d (d + 1) / 2 = %lld", (long long)ldo, (long long)ncol); return -22; }
	if (ldo > ((int64_t)1 << 62) / n || ldc < n * ldo) { set_error("stpy_kmv_dxx: ldc=%lld below n * ldo = %lld * %lld", (long long)ldc, (long long)n, (long long)ldo); return -23; }
	if (!kd_finite(kappa)) { set_error("stpy_kmv_dxx: kappa=%g must be finite", kappa); return -11; }
	if (!a || !inv_ls || !out || (q > 0 && (!b || !Vt))) { set_error("stpy_kmv_dxx: null pointer"); return -3; }          // (q == 0 reads neither b nor Vt)
	const int64_t need = kxx_workspace_bytes(dtype, n, q, d, t);
	if (!work || work_bytes < need) {
		set_error("stpy_kmv_dxx: workspace of %lld bytes, %lld needed (see the *_workspace_bytes query for these arguments)", (long long)(work ? work_bytes : 0), (long long)need);
		return -20;
	}
	if ((uintptr_t)work & 7) { set_error("stpy_kmv_dxx: work must be 8-byte aligned"); return -17; }
	hipStream_t st = (hipStream_t)stream;
	if (dtype == STPY_F64)
		return kmv_dxx<double>(kind, (const double*)a, n, lda, (const double*)b, q, ldb, d, cols, (const double*)inv_ls, kappa, (const double*)Vt, ldv, t,
		                       (double*)out, ldc, ldo, work, st);
	return kmv_dxx<float>(kind, (const float*)a, n, lda, (const float*)b, q, ldb, d, cols, (const float*)inv_ls, kappa, (const float*)Vt, ldv, t,
	                      (float*)out, ldc, ldo, work, st);
}

}  // extern "C"

#endif
