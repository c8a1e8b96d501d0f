// Values, query-point gradients AND query-point Hessians of kernel sums generated on the fly (stpy_kmv_dxx): for n query points a_i, q contracted
// points b_j and t coefficient rows Vt (t x q), with e_ijk = (a_i - b_j)[cols[k]] * inv_ls[k], rho = sum_k e_k^2, chi = 2 dphi/drho, psi = 2 dchi/drho,
//   out[c, i, k]                     = inv_ls[k] sum_j Vt[c, j] kappa chi e_ijk                                      k < d   (as stpy_kmv_dx)
//   out[c, i, d]                     =           sum_j Vt[c, j] kappa phi                                                     (as stpy_kmv_dx)
//   out[c, i, d + 1 + k(k+1)/2 + l]  = inv_ls[k] inv_ls[l] sum_j Vt[c, j] kappa (psi e_ijk e_ijl + chi [k == l])     l <= k < d
// (out[c, i, p] at c ldc + i ldo + p): the lower triangle of the Hessian with respect to a_i[cols], row by row.  The kernel matrix is never formed.
// With Vt = alpha^T this is the posterior mean, its input gradient and its input Hessian.
//
// The pair walker of kmv_pair.h (the design, the cut, the fp64 rule and the rho == 0 guard are stated there), rectangular, with ONE block of 16
// rows c and ONE GROUP of output columns per workgroup.  What this file adds: the 1 + d + d(d+1)/2 columns (153 at d = 16) do not fit the
// register file, so the lane re-evaluates the pair (the d scaled differences, rho, phi, chi, psi: kdd_phi_chi_psi) once per group and issues
// at most DC + 1 MFMAs against the same A fragment.  The groups (blockIdx.z walks them as well):
//   group 0              the d gradient columns and the value column: kp_dx_step, the very function stpy_kmv_dx calls;
//   group g = 1 .. ceil(d/2)   Hessian rows k1 = g - 1 and k2 = d - g (one row where they meet): (k1 + 1) + (k2 + 1) = d + 1 columns, so every group
//                        carries the same load.  Row k1 accumulates in acc[l], row k2 in acc[DC - l]: the two ranges are disjoint (DC - k2 >= g > k1).
// Coordinates are indexed by compile-time constants (DC = 4, 8, 16 in registers; l <= k is a uniform branch); the ROW's own difference, whose
// index comes from blockIdx, is formed again from LDS with the same two operations (the same bits as the register copy).  d > 16 is refused.
// Epilogue: columns are scaled (inv_ls[k]; inv_ls[k] inv_ls[l]) and the tile is stored, or, as one of several pieces of a cut j range, lands in
// `work` unscaled for the second launch (kp_add_pieces).
// A pair with rho == 0 contributes exactly 0 to the gradient and kappa chi(0) [k == l] (times the scales) to the Hessian: its e_k are 0.
// SE and MATERN52 only: chi of MATERN12 / MATERN32 has no finite derivative at rho = 0.
#include "common.h"
#include "kmv_pair.h"

namespace stpy {

namespace {

constexpr int KXX_MAX_D = 16;

template <typename T>
struct KxxArgs {
	const T* a; int64_t lda; int n; const T* b; int64_t ldb; int q; int d; const int32_t* cols; const T* inv_ls; T kappa; int kind;
	const T* Vt; int64_t ldv; int t; T* out; int64_t ldc, ldo; T* part; int nsplit, jper, ngroups, ncol;
};

// output columns of a point: d gradients, the value, the lower triangle row by row
inline int64_t kxx_ncol(int d) { return 1 + (int64_t)d + (int64_t)d * (d + 1) / 2; }
inline int kxx_groups(int d) { return 1 + (d + 1) / 2; }

// DC: coordinates held in registers (d <= DC)
template <typename T, int DC>
__global__ __launch_bounds__(KP_THREADS)
void kmvxx_kernel(KxxArgs<T> g)
{
	typedef typename Mfma<T>::v4 v4;
	__shared__ T sv[KP_JC][KP_PB + 1];
	__shared__ T sb[DC][KP_JC];
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
	const int64_t i0 = (int64_t)blockIdx.x * KP_TILE;
	const int64_t i = i0 + 16 * w + li;
	const int grp = (int)blockIdx.z % g.ngroups;                       // column group of the outputs
	const int c0 = ((int)blockIdx.z / g.ngroups) * KP_PB;
	const int k1 = grp > 0 ? grp - 1 : 0, k2 = grp > 0 ? g.d - grp : 0;       // the group's Hessian rows (k1 <= k2 < d <= DC)
	const bool two = grp > 0 && k2 > k1;
	int jb, je;
	kp_range(g.jper, g.q, jb, je);
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
	for (int64_t j0 = jb; j0 < je; j0 += KP_JC) {                        // (64 bits: j0 + 64 may pass 2^31)
		__syncthreads();                                              // (the previous chunk has been read)
		for (int cc = w; cc < KP_PB; cc += 4) {
			const int c = c0 + cc;
			const int64_t j = j0 + lane;
			sv[lane][cc] = (c < g.t && j < je) ? g.Vt[(int64_t)c * g.ldv + j] : (T)0;
		}
		kp_stage_b<T, DC>(sb, g.b, g.ldb, g.d, g.cols, 0, j0, je);
		__syncthreads();
		if (grp == 0) {
#pragma unroll 1
			for (int s = 0; s < 16; ++s) {
				const int jj = 4 * s + lk;
				kp_dx_step<T, DC>(acc, av, il, sb, sv, g.kind, g.kappa, jj, li, j0, je);
			}
		} else {
#pragma unroll 1
			for (int s = 0; s < 16; ++s) {
				const int jj = 4 * s + lk;
				T ek[DC];
				const T rho = kp_pair<T, DC>(av, il, sb, jj, ek);
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
__global__ __launch_bounds__(KP_THREADS)
void kmvxx_reduce_kernel(KxxArgs<T> g)
{
	kp_add_pieces<T, true>(g, g.ncol);
}

// pieces of the j range for (n, q, d, t); 0 for q == 0
inline int kxx_nsplit(int64_t n, int64_t q, int d, int64_t t)
{
	return q < 1 ? 0 : kp_split(kp_tiles(n) * kp_row_blocks(t) * kxx_groups(d), q, KP_MAX_SPLIT_QUERY);
}

// Room for one unscaled (t, n, ncol) tile set per piece of a cut j range, as an envelope that does not decrease in n, q or t (a caller may size one
// buffer for its largest problem): the pieces s are at most S = min(ceil(q / 256), ceil(512 / groups)), and a range is only cut below KP_FILL
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
	int64_t S = q < 1 ? 0 : (q + KP_SPLIT_MIN_J - 1) / KP_SPLIT_MIN_J;
	const int64_t by_groups = (KP_SPLIT_TARGET + groups - 1) / groups;
	if (S > by_groups) S = by_groups;
	if (S > KP_MAX_SPLIT_QUERY) S = KP_MAX_SPLIT_QUERY;
	int64_t elems = 0;
	if (S > 1) {
		const int64_t cap = (int64_t)(KP_SPLIT_TARGET + KP_FILL) * KP_TILE * KP_PB / groups;
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
	KxxArgs<T> g{a, lda, (int)n, b, ldb, (int)q, d, cols, inv_ls, (T)kappa, kind, Vt, ldv, (int)t, out, ldc, ldo, (T*)work, nsplit, (int)kp_piece_length(q, nsplit), ngroups, (int)kxx_ncol(d)};
	if (nsplit >= 1) {
		const dim3 grid((unsigned)kp_tiles(n), (unsigned)nsplit, (unsigned)(kp_row_blocks(t) * ngroups));
		if (d <= 4) hipLaunchKernelGGL((kmvxx_kernel<T, 4>), grid, dim3(KP_THREADS), 0, st, g);
		else if (d <= 8) hipLaunchKernelGGL((kmvxx_kernel<T, 8>), grid, dim3(KP_THREADS), 0, st, g);
		else hipLaunchKernelGGL((kmvxx_kernel<T, 16>), grid, dim3(KP_THREADS), 0, st, g);
	}
	kp_launch_add_pieces(kmvxx_reduce_kernel<T>, g, nsplit, t * n * kxx_ncol(d), st);
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
	const char* name = "stpy_kmv_dxx";
	int rc;
	if (kind != STPY_K_SE && kind != STPY_K_MATERN52) {
		set_error("stpy_kmv_dxx: kernel kind %d has no second derivative here (SE and MATERN52 only: MATERN12 / MATERN32 are singular at r = 0)", kind);
		return -1;
	}
	if ((rc = kp_check_sizes(name, dtype, n, q)) != 0) return rc;
	if (n == 0) return 0;          // empty output: nothing to write
	if (d < 1 || d > KXX_MAX_D) { set_error("stpy_kmv_dxx: d=%d outside [1, %d]", d, KXX_MAX_D); return -6; }
	const int64_t zblocks = (t < 1 ? 0 : kp_row_blocks(t)) * kxx_groups(d);
	if (t < 1 || zblocks > 65535) { set_error("stpy_kmv_dxx: t=%lld outside [1, 65535 * 16 / groups] (groups = 1 + ceil(d / 2))", (long long)t); return -10; }
	if ((rc = kp_check_ld_points(name, lda, ldb, d)) != 0 || (rc = kp_check_query_layout(name, n, q, ldv, kxx_ncol(d), "1 + d + d (d + 1) / 2", ldo, ldc, kappa)) != 0 ||
	    (rc = kp_check_pointers(name, a, b, q, inv_ls, Vt, out)) != 0 || (rc = kp_check_work(name, work, work_bytes, kxx_workspace_bytes(dtype, n, q, d, t), 8)) != 0) return rc;
	hipStream_t st = (hipStream_t)stream;
	if (dtype == STPY_F64)
		return kmv_dxx<double>(kind, (const double*)a, n, lda, (const double*)b, q, ldb, d, cols, (const double*)inv_ls, kappa, (const double*)Vt, ldv, t,
		                       (double*)out, ldc, ldo, work, st);
	return kmv_dxx<float>(kind, (const float*)a, n, lda, (const float*)b, q, ldb, d, cols, (const float*)inv_ls, kappa, (const float*)Vt, ldv, t,
	                      (float*)out, ldc, ldo, work, st);
}

}  // extern "C"
