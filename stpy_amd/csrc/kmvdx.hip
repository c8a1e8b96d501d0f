// Values and query-point gradients of kernel sums generated on the fly (stpy_kmv_dx): for n query points a_i, q contracted points b_j and t
// coefficient rows Vt (t x q)
//   out[c, i, k] = inv_ls[k] sum_j Vt[c, j] kappa chi(rho_ij) e_ijk (k < d),   out[c, i, d] = sum_j Vt[c, j] kappa phi(rho_ij)   (out[c, i, k] at c ldc + i ldo + k),
// with e_ijk = (a_i - b_j)[cols[k]] * inv_ls[k], rho = sum_k e_k^2 and chi = 2 dphi/drho: out[c, i, k] = d out[c, i, d] / d a_i[cols[k]].  The
// kernel matrix is never formed.  With Vt = alpha^T this is the posterior mean and its input gradient; with the rows of a pathwise
// conditioning solve it is the data term of t posterior draws and their gradients.
//
// A sibling of stpy_kmv_dtheta (kmvgrad.hip) and the same launch shape: a workgroup of four waves owns 64 query points i, 16 per wave, and ONE
// block of 16 rows c, and walks j in chunks of 64 through LDS.  The 16x16x4 MFMA runs with A = a fragment of Vt (row = c, k = j) and B = the
// ONE value each lane evaluates for the pair (i, j) its operand slot wants: the lane forms the d scaled differences once, from them rho, phi
// and chi (kd_phi_chi: the evaluator of pchol.hip, the same bits as stpy_kmv for the value column), and issues d + 1 MFMAs against the same
// A fragment with B = kappa chi e_k and B = kappa phi.  It differs from its sibling in three ways: it is rectangular (a against b), the
// derivative is with respect to the query point (e_k, not e_k^2), and the D tile (row = c, col = i) is STORED per query point instead of
// being reduced over i.  Every accumulator is a C = D chain on its own, fully live tuple (the fp64 rule of potrf.hip).  Coordinates stay in
// registers up to d = 16 (instantiations for 4, 8 and 16); beyond, rho is gathered through LDS 8 coordinates at a time and a workgroup owns
// the columns of ONE group of 8 coordinates (blockIdx.z walks groups as well), so that the register budget does not depend on d.
// Epilogue: the gradient columns are scaled by inv_ls[k] and the tile is stored.  The common case is few queries against a huge q (25 starts
// against 10^6 points: one tile), so the j range is cut into blockIdx.y pieces as in stpy_kmv (up to 512 of them, each at least 256 points
// long); the pieces' tiles land in `work` unscaled and a second launch adds them in piece order, scales and stores.  No atomics, no spin-waits, no cooperative grid, no scratch; the same bits on
// every call and for every lda / ldb / ldv / ldc / ldo.
// A pair with rho == 0 contributes exactly 0 to the first d outputs (its e_k are 0; the guard keeps Matern 1/2, whose chi is -exp(-r) / r, from 0 / 0).
#ifndef STPY_KMVDX_HIP
#define STPY_KMVDX_HIP
#include "common.h"
#include "pchol.hip"          // pc_phi / pc_fma: the one direct-difference evaluator
#include "kmvgrad.hip"        // kd_phi_chi: phi and chi = 2 dphi/drho as stpy_kmv_dtheta evaluates them

#include <math.h>

namespace stpy {

namespace {

constexpr int KX_THREADS = 256;
constexpr int KX_TILE = 64;            // query points of a workgroup (16 per wave)
constexpr int KX_JC = 64;              // contracted points per LDS chunk
constexpr int KX_PB = 16;              // coefficient rows of a workgroup: one MFMA row block
constexpr int KX_VS = KX_PB + 1;       // row stride of the Vt block in LDS
constexpr int KX_FILL = 256;           // below this many workgroups the j range is cut ...
constexpr int KX_SPLIT_TARGET = 512;   // ... into pieces, up to this many workgroups
constexpr int KX_MAX_SPLIT = 512;           // (stpy_kmv stops at 64: here ONE tile of queries against 10^6 points is the common case, and 64 workgroups leave 3/4 of the chip idle)
constexpr int KX_SPLIT_MIN_J = 4 * KX_JC;
constexpr int KX_GC = 8;               // coordinates of an output group beyond d = 16 (the general form)
constexpr int KX_RED_BLOCKS = 1 << 20; // the second launch walks its elements with a grid stride from at most this many workgroups

template <typename T>
struct KxArgs {
	const T* a; int64_t lda; int n; const T* b; int64_t ldb; int q; int d; const int32_t* cols; const T* inv_ls; T kappa; int kind;
	const T* Vt; int64_t ldv; int t; T* out; int64_t ldc, ldo; T* part; int nsplit, jper, nkc;
};

// DC coordinates at a time; ONE: d <= DC, the coordinates of a_i and the lengthscales are loaded once into registers and the workgroup owns
// every output column; otherwise rho is gathered through LDS and the workgroup owns the columns of coordinate group blockIdx.z % nkc
template <typename T, int DC, bool ONE>
__global__ __launch_bounds__(KX_THREADS)
void kmvx_kernel(KxArgs<T> g)
{
	typedef typename Mfma<T>::v4 v4;
	__shared__ T sv[KX_JC][KX_VS];
	__shared__ T sb[DC][KX_JC];
	__shared__ T sa[ONE ? 1 : DC][KX_TILE];
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
	const int64_t i0 = (int64_t)blockIdx.x * KX_TILE;
	const int64_t i = i0 + 16 * w + li;
	const int kc = ONE ? 0 : (int)blockIdx.z % g.nkc;                  // coordinate group of the outputs
	const int c0 = (ONE ? (int)blockIdx.z : (int)blockIdx.z / g.nkc) * KX_PB;
	const int kb = kc * DC;
	const int64_t jb64 = (int64_t)blockIdx.y * g.jper;
	const int jb = jb64 < g.q ? (int)jb64 : g.q, je = jb64 + g.jper < g.q ? (int)(jb64 + g.jper) : g.q;
	v4 acc[DC + 1];
#pragma unroll
	for (int k = 0; k <= DC; ++k) acc[k] = v4{(T)0, (T)0, (T)0, (T)0};
	T av[DC], il[DC];
#pragma unroll
	for (int k = 0; k < DC; ++k) {
		const bool in = kb + k < g.d;
		const int c = in ? (g.cols ? g.cols[kb + k] : kb + k) : 0;
		il[k] = in ? g.inv_ls[kb + k] : (T)0;
		av[k] = (in && i < g.n) ? g.a[i * g.lda + c] : (T)0;
	}
	constexpr int KX_UNROLL = DC <= 8 ? 2 : 1;
	for (int64_t j0 = jb; j0 < je; j0 += KX_JC) {                         // (64 bits: j0 + 64 may pass 2^31)
		__syncthreads();                                              // (the previous chunk has been read)
		for (int cc = w; cc < KX_PB; cc += 4) {
			const int c = c0 + cc;
			const int64_t j = j0 + lane;
			sv[lane][cc] = (c < g.t && j < je) ? g.Vt[(int64_t)c * g.ldv + j] : (T)0;
		}
		if (ONE) {
			for (int e = tid; e < DC * KX_JC; e += KX_THREADS) {
				const int k = e >> 6, jj = e & 63;
				const int64_t j = j0 + jj;
				sb[k][jj] = (k < g.d && j < je) ? g.b[j * g.ldb + (g.cols ? g.cols[k] : k)] : (T)0;
			}
			__syncthreads();
#pragma unroll KX_UNROLL
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
			T rho[16];
#pragma unroll
			for (int s = 0; s < 16; ++s) rho[s] = (T)0;
			for (int k0 = 0; k0 < g.d; k0 += DC) {
				if (k0 > 0) __syncthreads();
				for (int e = tid; e < DC * KX_JC; e += KX_THREADS) {
					const int k = e >> 6, jj = e & 63, kk = k0 + k;
					const int64_t j = j0 + jj;
					const int c = kk < g.d ? (g.cols ? g.cols[kk] : kk) : 0;
					sb[k][jj] = (kk < g.d && j < je) ? g.b[j * g.ldb + c] : (T)0;
					sa[k][jj] = (kk < g.d && i0 + jj < g.n) ? g.a[(i0 + jj) * g.lda + c] : (T)0;
				}
				__syncthreads();
#pragma unroll
				for (int k = 0; k < DC; ++k) {
					const T ak = sa[k][16 * w + li];
					const T ik = k0 + k < g.d ? g.inv_ls[k0 + k] : (T)0;
#pragma unroll
					for (int s = 0; s < 16; ++s) {
						const T df = (ak - sb[k][4 * s + lk]) * ik;
						rho[s] = pc_fma(df, df, rho[s]);
					}
				}
			}
			__syncthreads();                                          // (the last round of rho has been read) the group's own coordinates of j
			for (int e = tid; e < DC * KX_JC; e += KX_THREADS) {
				const int k = e >> 6, jj = e & 63, kk = kb + k;
				const int64_t j = j0 + jj;
				sb[k][jj] = (kk < g.d && j < je) ? g.b[j * g.ldb + (g.cols ? g.cols[kk] : kk)] : (T)0;
			}
			__syncthreads();
#pragma unroll
			for (int s = 0; s < 16; ++s) {
				const int jj = 4 * s + lk;
				T phi, chi;
				kd_phi_chi(g.kind, rho[s], phi, chi);
				const bool in = j0 + jj < je;
				const T wchi = (in && rho[s] != (T)0) ? g.kappa * chi : (T)0;
				const T wphi = in ? g.kappa * phi : (T)0;
				const T a = sv[jj][li];
#pragma unroll
				for (int k = 0; k < DC; ++k) {
					const T df = (av[k] - sb[k][jj]) * il[k];
					acc[k] = Mfma<T>::mma(a, wchi * df, acc[k]);
				}
				acc[DC] = Mfma<T>::mma(a, wphi, acc[DC]);
			}
		}
	}
	// D[row = c][col = i]: one run of d + 1 values per (c, i), straight to out (scaled) or, as one of several pieces, to `work` (unscaled)
	if (i >= g.n) return;
#pragma unroll
	for (int r = 0; r < 4; ++r) {
		const int c = c0 + Mfma<T>::crow(lane, r);
		if (c >= g.t) continue;
		T* dst = g.nsplit > 1 ? g.part + (((int64_t)blockIdx.y * g.t + c) * g.n + i) * (g.d + 1) : g.out + (int64_t)c * g.ldc + i * g.ldo;
#pragma unroll
		for (int k = 0; k < DC; ++k)
			if (kb + k < g.d) dst[kb + k] = g.nsplit > 1 ? acc[k][r] : il[k] * acc[k][r];
		if (kc == 0) dst[g.d] = acc[DC][r];
	}
}

// out = the pieces added in piece order, gradient columns scaled; with nsplit == 0 (q == 0) the zero fill
template <typename T>
__global__ __launch_bounds__(KX_THREADS)
void kmvx_reduce_kernel(KxArgs<T> g)
{
	const int64_t d1 = (int64_t)g.d + 1, total = (int64_t)g.t * g.n * d1;
	for (int64_t e = (int64_t)blockIdx.x * KX_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * KX_THREADS) {
		const int kk = (int)(e % d1);
		const int64_t ci = e / d1, c = ci / g.n, i = ci % g.n;
		T v = (T)0;
		for (int s = 0; s < g.nsplit; ++s) v += g.part[(int64_t)s * total + e];
		if (kk < g.d && g.nsplit > 0) v *= g.inv_ls[kk];
		g.out[c * g.ldc + i * g.ldo + kk] = v;
	}
}

// pieces of the j range for (n, q, d, t): 1 unless the workgroups leave most of the chip idle; 0 for q == 0
inline int kx_nsplit(int64_t n, int64_t q, int d, int64_t t)
{
	if (q < 1) return 0;
	const int64_t groups = d <= 16 ? 1 : ((int64_t)d + KX_GC - 1) / KX_GC;
	const int64_t tiles = ((n + KX_TILE - 1) / KX_TILE) * ((t + KX_PB - 1) / KX_PB) * groups;
	if (tiles >= KX_FILL) return 1;
	int64_t s = (KX_SPLIT_TARGET + tiles - 1) / tiles;
	const int64_t by_q = (q + KX_SPLIT_MIN_J - 1) / KX_SPLIT_MIN_J;
	if (s > by_q) s = by_q;
	if (s > KX_MAX_SPLIT) s = KX_MAX_SPLIT;
	return s < 1 ? 1 : (int)s;
}

// one unscaled (t, n, d + 1) tile set per piece when the j range is cut (fewer than KX_FILL workgroups: n t / 1024 < 256), else nothing
inline int64_t kx_workspace_bytes(int dtype, int64_t n, int64_t q, int d, int64_t t)
{
	const int64_t esz = dtype == STPY_F32 ? 4 : 8;
	if (n < 1) n = 1;
	if (t < 1) t = 1;
	if (d < 1) d = 1;
	const int64_t s = kx_nsplit(n, q, d, t);
	const int64_t elems = s > 1 ? s * t * n * ((int64_t)d + 1) : 0;
	return (elems * esz + 255) / 256 * 256 + 256;
}

template <typename T>
int kmv_dx(int kind, const T* a, int64_t n, int64_t lda, const T* b, int64_t q, int64_t ldb, int d, const int32_t* cols, const T* inv_ls, double kappa,
           const T* Vt, int64_t ldv, int64_t t, T* out, int64_t ldc, int64_t ldo, void* work, hipStream_t st)
{
	const int nsplit = kx_nsplit(n, q, d, t);
	const int nkc = d <= 16 ? 1 : (d + KX_GC - 1) / KX_GC;
	int64_t jper = q;
	if (nsplit > 1) {
		jper = (q + nsplit - 1) / nsplit;
		jper = (jper + KX_JC - 1) / KX_JC * KX_JC;
	}
	KxArgs<T> g{a, lda, (int)n, b, ldb, (int)q, d, cols, inv_ls, (T)kappa, kind, Vt, ldv, (int)t, out, ldc, ldo, (T*)work, nsplit, (int)jper, nkc};
	if (nsplit >= 1) {
		const dim3 grid((unsigned)((n + KX_TILE - 1) / KX_TILE), (unsigned)nsplit, (unsigned)(((t + KX_PB - 1) / KX_PB) * nkc));
		if (d <= 4) hipLaunchKernelGGL((kmvx_kernel<T, 4, true>), grid, dim3(KX_THREADS), 0, st, g);
		else if (d <= 8) hipLaunchKernelGGL((kmvx_kernel<T, 8, true>), grid, dim3(KX_THREADS), 0, st, g);
		else if (d <= 16) hipLaunchKernelGGL((kmvx_kernel<T, 16, true>), grid, dim3(KX_THREADS), 0, st, g);
		else hipLaunchKernelGGL((kmvx_kernel<T, KX_GC, false>), grid, dim3(KX_THREADS), 0, st, g);
	}
	if (nsplit != 1) {
		const int64_t blocks = (t * n * ((int64_t)d + 1) + KX_THREADS - 1) / KX_THREADS;
		hipLaunchKernelGGL(kmvx_reduce_kernel<T>, dim3((unsigned)(blocks < KX_RED_BLOCKS ? blocks : KX_RED_BLOCKS)), dim3(KX_THREADS), 0, st, g);
	}
	return check_launch("stpy_kmv_dx");
}

}  // namespace

}  // namespace stpy

// ---- C ABI (include/stpy_hip.h); every refusal below comes before the first HIP call
using namespace stpy;

extern "C" {

int64_t stpy_kmv_dx_workspace_bytes(int dtype, int64_t n, int64_t q, int d, int64_t t)
{
	return kx_workspace_bytes(dtype, n, q, d, t);
}

int stpy_kmv_dx(int kind, int dtype, const void* a, int64_t n, int64_t lda, const void* b, int64_t q, int64_t ldb,
                int d, const int32_t* cols, const void* inv_ls, double kappa,
                const void* Vt, int64_t ldv, int64_t t,
                void* out, int64_t ldc, int64_t ldo, void* work, int64_t work_bytes, void* stream)
{
	if (kind < STPY_K_SE || kind > STPY_K_MATERN52) { set_error("stpy_kmv_dx: kernel kind %d is not stationary (SE, MATERN12/32/52)", kind); return -1; }
	if (dtype != STPY_F64 && dtype != STPY_F32) { set_error("stpy_kmv_dx: unknown dtype %d (0 = float64, 1 = float32)", dtype); return -2; }
	if (n < 0 || n >= ((int64_t)1 << 31) || q < 0 || q >= ((int64_t)1 << 31)) { set_error("stpy_kmv_dx: n=%lld or q=%lld outside [0, 2^31)", (long long)n, (long long)q); return -4; }
	if (n == 0) return 0;          // empty output: nothing to write
	if (d < 1) { set_error("stpy_kmv_dx: d=%d", d); return -6; }
	const int64_t zblocks = (t < 1 ? 0 : (t + KX_PB - 1) / KX_PB) * (d <= 16 ? 1 : ((int64_t)d + KX_GC - 1) / KX_GC);
	if (t < 1 || zblocks > 65535) { set_error("stpy_kmv_dx: t=%lld outside [1, 65535 * 16 / groups] (groups = 1 up to d = 16, ceil(d / 8) beyond)", (long long)t); return -10; }
	if (lda < d || ldb < d) { set_error("stpy_kmv_dx: lda=%lld or ldb=%lld below d=%d", (long long)lda, (long long)ldb, d); return -5; }
	if (ldv < q) { set_error("stpy_kmv_dx: ldv=%lld below q=%lld", (long long)ldv, (long long)q); return -13; }
	if (ldo < (int64_t)d + 1) { set_error("stpy_kmv_dx: ldo=%lld below d + 1 = %lld", (long long)ldo, (long long)d + 1); return -22; }
	if (ldo > ((int64_t)1 << 62) / n || ldc < n * ldo) { set_error("stpy_kmv_dx: ldc=%lld below n * ldo = %lld * %lld", (long long)ldc, (long long)n, (long long)ldo); return -23; }
	if (!kd_finite(kappa)) { set_error("stpy_kmv_dx: kappa=%g must be finite", kappa); return -11; }
	if (!a || !inv_ls || !out || (q > 0 && (!b || !Vt))) { set_error("stpy_kmv_dx: null pointer"); return -3; }          // (q == 0 reads neither b nor Vt)
	const int64_t need = kx_workspace_bytes(dtype, n, q, d, t);
	if (!work || work_bytes < need) {
		set_error("stpy_kmv_dx: workspace of %lld bytes, %lld needed (see the *_workspace_bytes query for these arguments)", (long long)(work ? work_bytes : 0), (long long)need);
		return -20;
	}
	if ((uintptr_t)work & 7) { set_error("stpy_kmv_dx: work must be 8-byte aligned"); return -17; }
	hipStream_t st = (hipStream_t)stream;
	if (dtype == STPY_F64)
		return kmv_dx<double>(kind, (const double*)a, n, lda, (const double*)b, q, ldb, d, cols, (const double*)inv_ls, kappa, (const double*)Vt, ldv, t,
		                      (double*)out, ldc, ldo, work, st);
	return kmv_dx<float>(kind, (const float*)a, n, lda, (const float*)b, q, ldb, d, cols, (const float*)inv_ls, kappa, (const float*)Vt, ldv, t,
	                     (float*)out, ldc, ldo, work, st);
}

}  // extern "C"

#endif
