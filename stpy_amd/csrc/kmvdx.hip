// Values and query-point gradients of kernel sums generated on the fly (stpy_kmv_dx): for n query points a_i, q contracted points b_j and t
// coefficient rows Vt (t x q)
//   out[c, i, k] = inv_ls[k] sum_j Vt[c, j] kappa chi(rho_ij) e_ijk (k < d),   out[c, i, d] = sum_j Vt[c, j] kappa phi(rho_ij)   (out[c, i, k] at c ldc + i ldo + k),
// with e_ijk = (a_i - b_j)[cols[k]] * inv_ls[k], rho = sum_k e_k^2 and chi = 2 dphi/drho: out[c, i, k] = d out[c, i, d] / d a_i[cols[k]].  The
// kernel matrix is never formed.  With Vt = alpha^T this is the posterior mean and its input gradient; with the rows of a pathwise
// conditioning solve it is the data term of t posterior draws and their gradients.
//
// The pair walker of kmv_pair.h (the design, the cut, the fp64 rule and the rho == 0 guard are stated there), rectangular (a against b), with
// ONE block of 16 rows c per workgroup.  What this file adds: d + 1 MFMAs per pair against the same A fragment with B = kappa chi e_k and
// B = kappa phi (kp_dx_step; the bits of stpy_kmv for the value column), and a D tile (row = c, col = i) that is STORED per query point.
// Beyond d = 16, rho is gathered 8 coordinates at a time and a workgroup owns the columns of ONE group of 8 coordinates (blockIdx.z walks
// groups as well), so that the register budget does not depend on d.
// Epilogue: the gradient columns are scaled by inv_ls[k] and the tile is stored.  The common case is few queries against a huge q (25 starts
// against 10^6 points: one tile), so the j range is cut into up to 512 pieces; the pieces' tiles land in `work` unscaled and the second launch
// (kp_add_pieces) adds them in piece order, scales and stores.
#include "common.h"
#include "kmv_pair.h"

namespace stpy {

namespace {

template <typename T>
struct KxArgs {
	const T* a; int64_t lda; int n; const T* b; int64_t ldb; int q; int d; const int32_t* cols; const T* inv_ls; T kappa; int kind;
	const T* Vt; int64_t ldv; int t; T* out; int64_t ldc, ldo; T* part; int nsplit, jper, nkc;
};

// DC coordinates at a time; ONE: d <= DC, the coordinates of a_i and the lengthscales are loaded once into registers and the workgroup owns
// every output column; otherwise rho is gathered through LDS and the workgroup owns the columns of coordinate group blockIdx.z % nkc
template <typename T, int DC, bool ONE>
__global__ __launch_bounds__(KP_THREADS)
void kmvx_kernel(KxArgs<T> g)
{
	typedef typename Mfma<T>::v4 v4;
	__shared__ T sv[KP_JC][KP_PB + 1];
	__shared__ T sb[DC][KP_JC];
	__shared__ T sa[ONE ? 1 : DC][KP_TILE];
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
	const int64_t i0 = (int64_t)blockIdx.x * KP_TILE;
	const int64_t i = i0 + 16 * w + li;
	const int kc = ONE ? 0 : (int)blockIdx.z % g.nkc;                  // coordinate group of the outputs
	const int c0 = (ONE ? (int)blockIdx.z : (int)blockIdx.z / g.nkc) * KP_PB;
	const int kb = kc * DC;
	int jb, je;
	kp_range(g.jper, g.q, jb, je);
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
	for (int64_t j0 = jb; j0 < je; j0 += KP_JC) {                         // (64 bits: j0 + 64 may pass 2^31)
		__syncthreads();                                              // (the previous chunk has been read)
		for (int cc = w; cc < KP_PB; cc += 4) {
			const int c = c0 + cc;
			const int64_t j = j0 + lane;
			sv[lane][cc] = (c < g.t && j < je) ? g.Vt[(int64_t)c * g.ldv + j] : (T)0;
		}
		if (ONE) {
			kp_stage_b<T, DC>(sb, g.b, g.ldb, g.d, g.cols, 0, j0, je);
			__syncthreads();
#pragma unroll KX_UNROLL
			for (int s = 0; s < 16; ++s) {
				const int jj = 4 * s + lk;
				kp_dx_step<T, DC>(acc, av, il, sb, sv, g.kind, g.kappa, jj, li, j0, je);
			}
		} else {
			T rho[16];
#pragma unroll
			for (int s = 0; s < 16; ++s) rho[s] = (T)0;
			for (int k0 = 0; k0 < g.d; k0 += DC) {
				if (k0 > 0) __syncthreads();
				for (int e = tid; e < DC * KP_JC; e += KP_THREADS) {
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
			kp_stage_b<T, DC>(sb, g.b, g.ldb, g.d, g.cols, kb, j0, je);
			__syncthreads();
#pragma unroll
			for (int s = 0; s < 16; ++s) {
				const int jj = 4 * s + lk;
				T wphi, wchi;
				kp_weights(g.kind, g.kappa, rho[s], j0 + jj < je, wphi, wchi);
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
__global__ __launch_bounds__(KP_THREADS)
void kmvx_reduce_kernel(KxArgs<T> g)
{
	kp_add_pieces<T, false>(g, (int64_t)g.d + 1);
}

// pieces of the j range for (n, q, d, t); 0 for q == 0
inline int kx_nsplit(int64_t n, int64_t q, int d, int64_t t)
{
	return q < 1 ? 0 : kp_split(kp_tiles(n) * kp_row_blocks(t) * kp_coord_groups(d), q, KP_MAX_SPLIT_QUERY);
}

// one unscaled (t, n, d + 1) tile set per piece when the j range is cut (fewer than KP_FILL workgroups: n t / 1024 < 256), else nothing
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
	const int nkc = (int)kp_coord_groups(d);
	KxArgs<T> g{a, lda, (int)n, b, ldb, (int)q, d, cols, inv_ls, (T)kappa, kind, Vt, ldv, (int)t, out, ldc, ldo, (T*)work, nsplit, (int)kp_piece_length(q, nsplit), nkc};
	if (nsplit >= 1) {
		const dim3 grid((unsigned)kp_tiles(n), (unsigned)nsplit, (unsigned)(kp_row_blocks(t) * nkc));
		if (d <= 4) hipLaunchKernelGGL((kmvx_kernel<T, 4, true>), grid, dim3(KP_THREADS), 0, st, g);
		else if (d <= 8) hipLaunchKernelGGL((kmvx_kernel<T, 8, true>), grid, dim3(KP_THREADS), 0, st, g);
		else if (d <= 16) hipLaunchKernelGGL((kmvx_kernel<T, 16, true>), grid, dim3(KP_THREADS), 0, st, g);
		else hipLaunchKernelGGL((kmvx_kernel<T, KP_GC, false>), grid, dim3(KP_THREADS), 0, st, g);
	}
	kp_launch_add_pieces(kmvx_reduce_kernel<T>, g, nsplit, t * n * ((int64_t)d + 1), st);
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
	const char* name = "stpy_kmv_dx";
	int rc;
	if ((rc = kp_check_stationary(name, kind)) != 0 || (rc = kp_check_sizes(name, dtype, n, q)) != 0) return rc;
	if (n == 0) return 0;          // empty output: nothing to write
	if (d < 1) { set_error("stpy_kmv_dx: d=%d", d); return -6; }
	const int64_t zblocks = (t < 1 ? 0 : kp_row_blocks(t)) * kp_coord_groups(d);
	if (t < 1 || zblocks > 65535) { set_error("stpy_kmv_dx: t=%lld outside [1, 65535 * 16 / groups] (groups = 1 up to d = 16, ceil(d / 8) beyond)", (long long)t); return -10; }
	if ((rc = kp_check_ld_points(name, lda, ldb, d)) != 0 || (rc = kp_check_query_layout(name, n, q, ldv, (int64_t)d + 1, "d + 1", ldo, ldc, kappa)) != 0 ||
	    (rc = kp_check_pointers(name, a, b, q, inv_ls, Vt, out)) != 0 || (rc = kp_check_work(name, work, work_bytes, kx_workspace_bytes(dtype, n, q, d, t), 8)) != 0) return rc;
	hipStream_t st = (hipStream_t)stream;
	if (dtype == STPY_F64)
		return kmv_dx<double>(kind, (const double*)a, n, lda, (const double*)b, q, ldb, d, cols, (const double*)inv_ls, kappa, (const double*)Vt, ldv, t,
		                      (double*)out, ldc, ldo, work, st);
	return kmv_dx<float>(kind, (const float*)a, n, lda, (const float*)b, q, ldb, d, cols, (const float*)inv_ls, kappa, (const float*)Vt, ldv, t,
	                     (float*)out, ldc, ldo, work, st);
}

}  // extern "C"
