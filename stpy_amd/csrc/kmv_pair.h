// The pair walker of the matrix-free kernel mat-vec family: what stpy_kmv (kmv.hip), stpy_kmv_dtheta (kmvgrad.hip), stpy_kmv_dx (kmvdx.hip)
// and stpy_kmv_dxx (kmvdxx.hip) share, and the scalar kernel evaluator they share with the pivoted Cholesky (pchol.hip).  No kernels and no
// entry points live here: the evaluator and the device helpers of the chunk walk (all forced inline), the geometry, the host side of the
// launch plan and the argument checks of the C ABI.
//
// The design.  A workgroup of four waves owns KP_TILE = 64 points i, 16 per wave, and one block of rows of Vt (64 for stpy_kmv, KP_PB = 16 for
// the derivative kernels, whose further accumulators hold derivative columns), and walks the contracted points j in chunks of KP_JC = 64 in a
// fixed order.  The product runs on the 16x16x4 MFMA with A = a fragment of Vt (row = row of Vt, k = j) and B = a 4 x 16 fragment of the
// kernel matrix (or of a derivative of it), whose operand map wants ONE element per lane, B[k = lane >> 4][lane & 15]: lane l evaluates the
// pair (i0 + 16 w + (l & 15), j0 + 4 s + (l >> 4)) itself, df_k = (a_ik - b_jk) * inv_ls[k] and rho = fma(df_k, df_k, rho) in the order of k,
// with the ONE scalar evaluator below, and feeds it straight in: kernel values pass through neither LDS nor a shuffle, and every kernel of
// the family has the bits of every other in the columns they share.  D has col = lane & 15 = i.  The chunk of b coordinates and the Vt block
// (row stride: rows + 1) go through LDS; the coordinates of point i stay in registers up to d = 16 (instantiations for 4, 8 and 16) and
// beyond, where a kernel serves it, rho is gathered through LDS DC coordinates at a time.
// The chunk walk.  Shared where a kernel keeps, with the shared form, every register, spill, LDS and occupancy figure of every instantiation AND
// its measured time: kp_dx_step, the whole pair of stpy_kmv_dx, which group 0 of stpy_kmv_dxx calls too; under it kp_pair (the scaled
// differences and rho; also the Hessian groups of dxx) and kp_weights (the j-range mask and the rho == 0 guard of the first-order columns;
// also the d > 16 forms of dx and dtheta); kp_stage_b (a chunk's coordinates to LDS; dx and dxx).  Forced-inline helpers do not compile to
// the text they replace (a call's arguments are known to be defined, loads from the kernel's argument struct are not, and the selects that
// guard the ragged edges fold differently), so each use was held to those two gates, and these keep their text:
//   kmv_kernel, all of it       with kp_stage_b alone the d = 16 forms ran 1.2 - 1.6 % slower (fp32 n = 262144, fp64 t = 64; spread of two
//                               builds of the old text: 0.5 %); through kp_pair fp32 kmv_kernel<8> went 118 -> 67 VGPRs;
//   kmvd_kernel<registers>      with kp_pair + kp_weights fp64 d = 16 ran 5 % slower (n = 65536 and 262144), d = 4 1 - 2 % faster;
//   the Vt block to LDS         fp64 kmvx_kernel<4> 75 -> 77 VGPRs, fp64 kmvd_kernel<4> 79 -> 81, fp32 kmv_kernel<16, general> 180 -> 178;
//   a point's register loads    SGPR spills: fp64 kmv_kernel<4> 16 -> 17, fp64 kmvx_kernel<8> 23 -> 25, fp32 kmvxx_kernel<8> 60 -> 57;
//   the d > 16 rho gather       fp32 kmvx_kernel<8, general> 224 -> 226 VGPRs, fp64 kmvd_kernel<8, general> 200 -> 202 AGPRs.
// The cut.  When the output tiles are too few to fill the chip the j range is cut into blockIdx.y pieces (kp_split, kp_piece_length, kp_range)
// whose partial sums land in `work` and are added in piece order by a second launch: no atomics, no spin-waits, no cooperative grid, no
// scratch, and the same bits on every call and for every leading dimension.
// The fp64 rule.  Every accumulator is a C = D chain on its own, fully live tuple: never two constant-C fp64 MFMAs on overlapping tuples
// (potrf.hip has the measurement).
// The rho == 0 guard.  A pair of coincident points has e_k = 0 for every k and contributes exactly 0 to every first-derivative column; chi of
// Matern 1/2 is -exp(-r) / r there, so kp_weights gives the chi weight of such a pair as 0 instead of multiplying 0 by 0 / 0.
#ifndef STPY_KMV_PAIR_H
#define STPY_KMV_PAIR_H
#include "common.h"

#include <math.h>

namespace stpy {

namespace {

// ------------------------------------------------------------------------------------------------------------ the scalar evaluator
// kappa-free kernel value from the scaled squared distance
__device__ __forceinline__ double pc_phi(int kind, double r2)
{
	switch (kind) {
	case STPY_K_SE: return exp(-0.5 * r2);
	case STPY_K_MATERN12: return exp(-sqrt(r2));
	case STPY_K_MATERN32: { const double r = sqrt(r2) * 1.7320508075688772935; return (1.0 + r) * exp(-r); }
	default: { const double r = sqrt(r2) * 2.2360679774997896964; return (1.0 + r + r * r / 3.0) * exp(-r); }
	}
}

__device__ __forceinline__ float pc_phi(int kind, float r2)
{
	switch (kind) {
	case STPY_K_SE: return expf(-0.5f * r2);
	case STPY_K_MATERN12: return expf(-sqrtf(r2));
	case STPY_K_MATERN32: { const float r = sqrtf(r2) * 1.7320508075688772935f; return (1.0f + r) * expf(-r); }
	default: { const float r = sqrtf(r2) * 2.2360679774997896964f; return (1.0f + r + r * r / 3.0f) * expf(-r); }
	}
}

__device__ __forceinline__ double pc_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float pc_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double pc_sqrt(double a) { return sqrt(a); }
__device__ __forceinline__ float pc_sqrt(float a) { return sqrtf(a); }
__device__ __forceinline__ double kd_exp(double a) { return exp(a); }
__device__ __forceinline__ float kd_exp(float a) { return expf(a); }

// four kernel values at once, the kind decided once for the four: pc_phi entry by entry (the same bits)
template <typename T>
__device__ __forceinline__ void km_phi4(int kind, const T* r2, T* out)
{
	switch (kind) {
	case STPY_K_SE:
#pragma unroll
		for (int u = 0; u < 4; ++u) out[u] = pc_phi(STPY_K_SE, r2[u]);
		break;
	case STPY_K_MATERN12:
#pragma unroll
		for (int u = 0; u < 4; ++u) out[u] = pc_phi(STPY_K_MATERN12, r2[u]);
		break;
	case STPY_K_MATERN32:
#pragma unroll
		for (int u = 0; u < 4; ++u) out[u] = pc_phi(STPY_K_MATERN32, r2[u]);
		break;
	default:
#pragma unroll
		for (int u = 0; u < 4; ++u) out[u] = pc_phi(STPY_K_MATERN52, r2[u]);
		break;
	}
}

// phi (pc_phi) and chi = 2 dphi/drho of a scaled squared distance
template <typename T>
__device__ __forceinline__ void kd_phi_chi(int kind, T rho, T& phi, T& chi)
{
	switch (kind) {
	case STPY_K_SE:
		phi = pc_phi(STPY_K_SE, rho);
		chi = -phi;
		break;
	case STPY_K_MATERN12:
		phi = pc_phi(STPY_K_MATERN12, rho);
		chi = -phi / pc_sqrt(rho);                                     // (rho == 0: masked by kp_weights)
		break;
	case STPY_K_MATERN32: {
		const T r = pc_sqrt(rho) * (T)1.7320508075688772935;
		phi = pc_phi(STPY_K_MATERN32, rho);
		chi = (T)-3 * kd_exp(-r);
		break;
	}
	default: {
		const T r = pc_sqrt(rho) * (T)2.2360679774997896964;
		phi = pc_phi(STPY_K_MATERN52, rho);
		chi = (T)(-5.0 / 3.0) * ((T)1 + r) * kd_exp(-r);
		break;
	}
	}
}

// phi, chi (kd_phi_chi) and psi = 2 dchi/drho, for SE and MATERN52
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

// ------------------------------------------------------------------------------------------------------------ geometry and the cut
constexpr int KP_THREADS = 256;
constexpr int KP_TILE = 64;            // points i of a workgroup (16 per wave)
constexpr int KP_JC = 64;              // contracted points per LDS chunk
constexpr int KP_PB = 16;              // rows of Vt of a workgroup of the derivative kernels: one MFMA row block (stpy_kmv: 64, four of them)
constexpr int KP_FILL = 256;           // below this many workgroups the j range is cut ...
constexpr int KP_SPLIT_TARGET = 512;   // ... into pieces, up to this many workgroups
constexpr int KP_SPLIT_MIN_J = 4 * KP_JC;          // a piece is at least this long
constexpr int KP_MAX_SPLIT = 64;       // pieces of the square products (stpy_kmv, stpy_kmv_dtheta)
constexpr int KP_MAX_SPLIT_QUERY = 512;          // of stpy_kmv_dx / _dxx: ONE tile of queries against 10^6 points is their common case, and 64 workgroups leave 3/4 of the chip idle
constexpr int KP_GC = 8;               // coordinates of an output group beyond d = 16 (the general form of stpy_kmv_dtheta and stpy_kmv_dx)
constexpr int KP_RED_BLOCKS = 1 << 20; // the piece-adding launch walks its elements with a grid stride from at most this many workgroups

inline int64_t kp_tiles(int64_t n) { return (n + KP_TILE - 1) / KP_TILE; }
inline int64_t kp_row_blocks(int64_t t) { return (t + KP_PB - 1) / KP_PB; }
inline int64_t kp_coord_groups(int d) { return d <= 16 ? 1 : ((int64_t)d + KP_GC - 1) / KP_GC; }

// pieces of a j range of q >= 1 points for `tiles` workgroups: 1 unless they leave most of the chip idle
inline int kp_split(int64_t tiles, int64_t q, int max_split)
{
	if (tiles >= KP_FILL) return 1;
	int64_t s = (KP_SPLIT_TARGET + tiles - 1) / tiles;
	const int64_t by_q = (q + KP_SPLIT_MIN_J - 1) / KP_SPLIT_MIN_J;
	if (s > by_q) s = by_q;
	if (s > max_split) s = max_split;
	return s < 1 ? 1 : (int)s;
}

// points of a piece: whole chunks
inline int64_t kp_piece_length(int64_t q, int nsplit)
{
	if (nsplit <= 1) return q;
	const int64_t jper = (q + nsplit - 1) / nsplit;
	return (jper + KP_JC - 1) / KP_JC * KP_JC;
}

// [jb, je) of piece blockIdx.y, clamped to q
__device__ __forceinline__ void kp_range(int jper, int q, int& jb, int& je)
{
	const int64_t jb64 = (int64_t)blockIdx.y * jper;
	jb = jb64 < q ? (int)jb64 : q;
	je = jb64 + jper < q ? (int)(jb64 + jper) : q;
}

// ------------------------------------------------------------------------------------------------------------ the chunk walk
// coordinates [kb, kb + DC) of the chunk's points to LDS, zero beyond d and je
template <typename T, int DC>
__device__ __forceinline__ void kp_stage_b(T (*sb)[KP_JC], const T* b, int64_t ldb, int d, const int32_t* cols, int kb, int64_t j0, int je)
{
	for (int e = threadIdx.x; e < DC * KP_JC; e += KP_THREADS) {
		const int k = e >> 6, jj = e & 63, kk = kb + k;
		const int64_t j = j0 + jj;
		sb[k][jj] = (kk < d && j < je) ? b[j * ldb + (cols ? cols[kk] : kk)] : (T)0;
	}
}

// the scaled differences ek of the pair (registers of i, chunk point jj) and their squared length
template <typename T, int DC>
__device__ __forceinline__ T kp_pair(const T* av, const T* il, const T (*sb)[KP_JC], int jj, T* ek)
{
	T rho = (T)0;
#pragma unroll
	for (int k = 0; k < DC; ++k) {
		const T df = (av[k] - sb[k][jj]) * il[k];
		ek[k] = df;
		rho = pc_fma(df, df, rho);
	}
	return rho;
}

// the weights of one pair's value and first-derivative columns: kappa phi and kappa chi inside the j range (`in`), 0 beyond; the rho == 0 guard
template <typename T>
__device__ __forceinline__ void kp_weights(int kind, T kappa, T rho, bool in, T& wphi, T& wchi)
{
	T phi, chi;
	kd_phi_chi(kind, rho, phi, chi);
	wchi = (in && rho != (T)0) ? kappa * chi : (T)0;
	wphi = in ? kappa * phi : (T)0;
}

// one pair of stpy_kmv_dx with the coordinates in registers, and of group 0 of stpy_kmv_dxx: acc[k] += a kappa chi e_k, acc[DC] += a kappa phi
template <typename T, int DC>
__device__ __forceinline__ void kp_dx_step(typename Mfma<T>::v4* acc, const T* av, const T* il, const T (*sb)[KP_JC], const T (*sv)[KP_PB + 1],
                                           int kind, T kappa, int jj, int li, int64_t j0, int je)
{
	T ek[DC], wphi, wchi;
	const T rho = kp_pair<T, DC>(av, il, sb, jj, ek);
	kp_weights(kind, kappa, rho, j0 + jj < je, wphi, wchi);
	const T a = sv[jj][li];
#pragma unroll
	for (int k = 0; k < DC; ++k) acc[k] = Mfma<T>::mma(a, wchi * ek[k], acc[k]);
	acc[DC] = Mfma<T>::mma(a, wphi, acc[DC]);
}

// ------------------------------------------------------------------------------------------------------------ sums and the second launch
// sum over a workgroup of KP_THREADS in a fixed order, the same value in every thread; red: 4 words
__device__ __forceinline__ double kp_block_sum(double v, double* red)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
	__syncthreads();                                                  // (red may still be read from the previous sum)
	if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
	__syncthreads();
	return ((red[0] + red[1]) + red[2]) + red[3];
}

// out[c, i, p] = the pieces' (t, n, ncol) tiles added in piece order and scaled as the direct store scales them: inv_ls[p] for the gradient
// columns p < d, nothing for the value p == d, inv_ls[k] inv_ls[l] for the Hessian column p = d + 1 + k (k + 1) / 2 + l; with nsplit == 0 the zero fill
// (g: the argument struct of stpy_kmv_dx or stpy_kmv_dxx; HESSIAN false: nc = d + 1, and the kernel carries no code for the columns beyond)
template <typename T, bool HESSIAN, typename Args>
__device__ __forceinline__ void kp_add_pieces(const Args& g, int64_t nc)
{
	const int64_t total = (int64_t)g.t * g.n * nc;
	for (int64_t e = (int64_t)blockIdx.x * KP_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * KP_THREADS) {
		const int p = (int)(e % nc);
		const int64_t ci = e / nc, c = ci / g.n, i = ci % g.n;
		T v = (T)0;
		for (int s = 0; s < g.nsplit; ++s) v += g.part[(int64_t)s * total + e];
		if (g.nsplit > 0) {
			if (p < g.d) {
				v = g.inv_ls[p] * v;
			} else if (HESSIAN && p > g.d) {
				int k = 0, h = p - g.d - 1;                               // h = k (k + 1) / 2 + l, l <= k
				while ((k + 1) * (k + 2) / 2 <= h) ++k;
				const int l = h - k * (k + 1) / 2;
				v = (g.inv_ls[k] * g.inv_ls[l]) * v;
			}
		}
		g.out[c * g.ldc + i * g.ldo + p] = v;
	}
}

// the launch of a kernel over kp_add_pieces, wanted unless exactly one piece wrote straight to out
template <typename K, typename A>
inline void kp_launch_add_pieces(K kernel, const A& g, int nsplit, int64_t elems, hipStream_t st)
{
	if (nsplit == 1) return;
	const int64_t blocks = (elems + KP_THREADS - 1) / KP_THREADS;
	hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks < KP_RED_BLOCKS ? blocks : KP_RED_BLOCKS)), dim3(KP_THREADS), 0, st, g);
}

// ------------------------------------------------------------------------------------------------------------ the C ABI's shared refusals
// Each returns 0 to go on or the refusal's code, with the message set; every one comes before the first HIP call.
inline int kp_check_stationary(const char* name, int kind)
{
	if (kind < STPY_K_SE || kind > STPY_K_MATERN52) { set_error("%s: kernel kind %d is not stationary (SE, MATERN12/32/52)", name, kind); return -1; }
	return 0;
}

// dtype and the point counts of a rectangular product
inline int kp_check_sizes(const char* name, int dtype, int64_t n, int64_t q)
{
	if (dtype != STPY_F64 && dtype != STPY_F32) { set_error("%s: unknown dtype %d (0 = float64, 1 = float32)", name, dtype); return -2; }
	if (n < 0 || n >= ((int64_t)1 << 31) || q < 0 || q >= ((int64_t)1 << 31)) { set_error("%s: n=%lld or q=%lld outside [0, 2^31)", name, (long long)n, (long long)q); return -4; }
	return 0;
}

inline int kp_check_ld_points(const char* name, int64_t lda, int64_t ldb, int d)
{
	if (lda < d || ldb < d) { set_error("%s: lda=%lld or ldb=%lld below d=%d", name, (long long)lda, (long long)ldb, d); return -5; }
	return 0;
}

// the output layout of stpy_kmv_dx / _dxx (ncol columns per point, described by ncol_text) and their kappa
inline int kp_check_query_layout(const char* name, int64_t n, int64_t q, int64_t ldv, int64_t ncol, const char* ncol_text, int64_t ldo, int64_t ldc, double kappa)
{
	if (ldv < q) { set_error("%s: ldv=%lld below q=%lld", name, (long long)ldv, (long long)q); return -13; }
	if (ldo < ncol) { set_error("%s: ldo=%lld below %s = %lld", name, (long long)ldo, ncol_text, (long long)ncol); return -22; }
	if (ldo > ((int64_t)1 << 62) / n || ldc < n * ldo) { set_error("%s: ldc=%lld below n * ldo = %lld * %lld", name, (long long)ldc, (long long)n, (long long)ldo); return -23; }
	if (!is_finite(kappa)) { set_error("%s: kappa=%g must be finite", name, kappa); return -11; }
	return 0;
}

// the pointers of a rectangular product (q == 0 reads neither b nor Vt)
inline int kp_check_pointers(const char* name, const void* a, const void* b, int64_t q, const void* inv_ls, const void* Vt, const void* out)
{
	if (!a || !inv_ls || !out || (q > 0 && (!b || !Vt))) { set_error("%s: null pointer", name); return -3; }
	return 0;
}

inline int kp_check_work(const char* name, const void* work, int64_t work_bytes, int64_t need, int align)
{
	if (!work || work_bytes < need) {
		set_error("%s: workspace of %lld bytes, %lld needed (see the *_workspace_bytes query for these arguments)", name, (long long)(work ? work_bytes : 0), (long long)need);
		return -20;
	}
	if ((uintptr_t)work & (uintptr_t)(align - 1)) { set_error("%s: work must be %d-byte aligned", name, align); return -17; }
	return 0;
}

}  // namespace

}  // namespace stpy

#endif
