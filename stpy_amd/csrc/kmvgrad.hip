// Bilinear forms of the hyper-parameter derivative of a kernel matrix generated on the fly (stpy_kmv_dtheta): for t pairs of rows (u_c, v_c)
//   out[c, k] = sum_ij u_ci v_cj kappa chi(rho_ij) e_ijk^2 (k < d),   out[c, d] = u_c^T K v_c,   out[c, d + 1] = <u_c, v_c>,
// with e_ijk = (x_i - x_j)[cols[k]] * inv_ls[k], rho = sum_k e_k^2 and chi = 2 dphi/drho: d(u^T K v)/d inv_ls[k] = out[c, k] / inv_ls[k].  K is never formed.
//
// The pair walker of kmv_pair.h (the design, the cut, the fp64 rule and the rho == 0 guard are stated there), square (x against x).  What this
// file adds: the lane forms the d scaled differences of its pair once and issues d + 1 MFMAs against the same A fragment with B = kappa chi e_k^2
// and B = kappa phi (the bits of stpy_kmv for the value column), so the per-pair cost is d + 1 matrix instructions for 16 pairs of rows, not
// 16 (d + 1) fused multiply-adds.  d + 1 accumulator tuples serve ONE block of 16 pairs (68 fp64 values per lane at d = 16), so further blocks of
// 16 pairs go over blockIdx.z.  Beyond d = 16, rho is gathered 8 coordinates at a time and a workgroup owns the outputs of ONE group of 8
// coordinates (blockIdx.z walks groups as well), so that the register budget does not depend on d.
// Epilogue: the D tile is multiplied by Ut[c, i], summed over the 16 lanes of a row by a butterfly and over the four waves in wave order, and
// ONE partial row per workgroup and pair goes to `work`.  A second launch adds the partial rows in a fixed order (double accumulation) and
// computes <u_c, v_c>.
#include "common.h"
#include "kmv_pair.h"

namespace stpy {

namespace {

template <typename T>
struct KdArgs {
	const T* x; int64_t ldx; int n, d; const int32_t* cols; const T* inv_ls; T kappa; int kind;
	const T* Ut; int64_t ldu; const T* Vt; int64_t ldv; int t; T* out; int64_t ldo; T* part; int nsplit, jper, ntiles, nkc;
};

// DC coordinates at a time; ONE: d <= DC, the coordinates of i and the lengthscales are loaded once into registers and the workgroup owns
// every output column; otherwise rho is gathered through LDS and the workgroup owns the columns of coordinate group blockIdx.z % nkc
template <typename T, int DC, bool ONE>
__global__ __launch_bounds__(KP_THREADS)
void kmvd_kernel(KdArgs<T> g)
{
	typedef typename Mfma<T>::v4 v4;
	__shared__ T sv[KP_JC][KP_PB + 1];
	__shared__ T sb[DC][KP_JC];
	__shared__ T sa[ONE ? 1 : DC][KP_TILE];
	__shared__ T red[4][DC + 1][KP_PB];
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
	const int64_t i0 = (int64_t)blockIdx.x * KP_TILE;
	const int64_t i = i0 + 16 * w + li;
	const int kc = ONE ? 0 : (int)blockIdx.z % g.nkc;                  // coordinate group of the outputs
	const int c0 = (ONE ? (int)blockIdx.z : (int)blockIdx.z / g.nkc) * KP_PB;
	const int kb = kc * DC;
	int jb, je;
	kp_range(g.jper, g.n, jb, je);
	v4 acc[DC + 1];
#pragma unroll
	for (int k = 0; k <= DC; ++k) acc[k] = v4{(T)0, (T)0, (T)0, (T)0};
	T av[DC], il[DC];
#pragma unroll
	for (int k = 0; k < DC; ++k) {
		const bool in = kb + k < g.d;
		const int c = in ? (g.cols ? g.cols[kb + k] : kb + k) : 0;
		il[k] = in ? g.inv_ls[kb + k] : (T)0;
		av[k] = (in && i < g.n) ? g.x[i * g.ldx + c] : (T)0;
	}
	constexpr int KD_UNROLL = DC <= 8 ? 2 : 1;
	for (int64_t j0 = jb; j0 < je; j0 += KP_JC) {                         // (64 bits: j0 + 64 may pass 2^31)
		__syncthreads();                                              // (the previous chunk has been read)
		for (int cc = w; cc < KP_PB; cc += 4) {
			const int c = c0 + cc;
			const int64_t j = j0 + lane;
			sv[lane][cc] = (c < g.t && j < je) ? g.Vt[(int64_t)c * g.ldv + j] : (T)0;
		}
		if (ONE) {
			for (int e = tid; e < DC * KP_JC; e += KP_THREADS) {
				const int k = e >> 6, jj = e & 63;
				const int64_t j = j0 + jj;
				sb[k][jj] = (k < g.d && j < je) ? g.x[j * g.ldx + (g.cols ? g.cols[k] : k)] : (T)0;
			}
			__syncthreads();
#pragma unroll KD_UNROLL
			for (int s = 0; s < 16; ++s) {
				const int jj = 4 * s + lk;
				T e2[DC], rho = (T)0;
#pragma unroll
				for (int k = 0; k < DC; ++k) {
					const T df = (av[k] - sb[k][jj]) * il[k];
					e2[k] = df * df;
					rho = pc_fma(df, df, rho);
				}
				T phi, chi;
				kd_phi_chi(g.kind, rho, phi, chi);
				const bool in = j0 + jj < je;
				const T wchi = (in && rho != (T)0) ? g.kappa * chi : (T)0;          // (the rho == 0 guard of kmv_pair.h)
				const T wphi = in ? g.kappa * phi : (T)0;
				const T a = sv[jj][li];
#pragma unroll
				for (int k = 0; k < DC; ++k) acc[k] = Mfma<T>::mma(a, wchi * e2[k], acc[k]);
				acc[DC] = Mfma<T>::mma(a, wphi, acc[DC]);
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
					sb[k][jj] = (kk < g.d && j < je) ? g.x[j * g.ldx + c] : (T)0;
					sa[k][jj] = (kk < g.d && i0 + jj < g.n) ? g.x[(i0 + jj) * g.ldx + c] : (T)0;
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
			for (int e = tid; e < DC * KP_JC; e += KP_THREADS) {
				const int k = e >> 6, jj = e & 63, kk = kb + k;
				const int64_t j = j0 + jj;
				sb[k][jj] = (kk < g.d && j < je) ? g.x[j * g.ldx + (g.cols ? g.cols[kk] : kk)] : (T)0;
			}
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
					acc[k] = Mfma<T>::mma(a, wchi * (df * df), acc[k]);
				}
				acc[DC] = Mfma<T>::mma(a, wphi, acc[DC]);
			}
		}
	}
	// D[row = pair][col = i] times Ut[pair, i], summed over the 16 lanes of a row, then over the waves in wave order
	T ut[4];
#pragma unroll
	for (int r = 0; r < 4; ++r) {
		const int c = c0 + Mfma<T>::crow(lane, r);
		ut[r] = (c < g.t && i < g.n) ? g.Ut[(int64_t)c * g.ldu + i] : (T)0;
	}
#pragma unroll
	for (int k = 0; k <= DC; ++k) {
#pragma unroll
		for (int r = 0; r < 4; ++r) {
			T v = acc[k][r] * ut[r];
#pragma unroll
			for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o);
			if (li == 0) red[w][k][Mfma<T>::crow(lane, r)] = v;
		}
	}
	__syncthreads();
	const int64_t p = (int64_t)blockIdx.y * g.ntiles + blockIdx.x;
	for (int e = tid; e < (DC + 1) * KP_PB; e += KP_THREADS) {
		const int k = e >> 4, row = e & 15, c = c0 + row;
		const int kk = k == DC ? g.d : kb + k;                         // output column: a coordinate of this group, or the value (group 0 writes it)
		if (c >= g.t || (k == DC ? kc != 0 : kk >= g.d)) continue;
		g.part[(p * g.t + c) * (g.d + 1) + kk] = ((red[0][k][row] + red[1][k][row]) + red[2][k][row]) + red[3][k][row];
	}
}

// out[c, 0 .. d] = the partial rows added in a fixed order, out[c, d + 1] = <u_c, v_c>; one workgroup per pair.  No partial rows (n == 0): zeros.
template <typename T>
__global__ __launch_bounds__(KP_THREADS)
void kmvd_reduce_kernel(KdArgs<T> g)
{
	__shared__ double red[4];
	const int c = blockIdx.x;
	const int64_t np = (int64_t)g.nsplit * g.ntiles;
	for (int kk = 0; kk <= g.d; ++kk) {
		double v = 0.0;
		for (int64_t p = threadIdx.x; p < np; p += KP_THREADS) v += (double)g.part[(p * g.t + c) * (g.d + 1) + kk];
		v = kp_block_sum(v, red);
		if (threadIdx.x == 0) g.out[(int64_t)c * g.ldo + kk] = (T)v;
	}
	double v = 0.0;
	for (int i = threadIdx.x; i < g.n; i += KP_THREADS) v += (double)g.Ut[(int64_t)c * g.ldu + i] * (double)g.Vt[(int64_t)c * g.ldv + i];
	v = kp_block_sum(v, red);
	if (threadIdx.x == 0) g.out[(int64_t)c * g.ldo + g.d + 1] = (T)v;
}

// pieces of the j range for (n, d, t); 0 for n == 0
inline int kd_nsplit(int64_t n, int d, int64_t t)
{
	return n < 1 ? 0 : kp_split(kp_tiles(n) * kp_row_blocks(t) * kp_coord_groups(d), n, KP_MAX_SPLIT);
}

// one partial row of d + 1 sums per workgroup (tile of i, piece of j) and pair
inline int64_t kd_workspace_bytes(int dtype, int64_t n, int d, int64_t t)
{
	const int64_t esz = dtype == STPY_F32 ? 4 : 8;
	if (n < 1) n = 1;
	if (t < 1) t = 1;
	if (d < 1) d = 1;
	const int64_t rows = kp_tiles(n) * kd_nsplit(n, d, t);
	return (rows * t * ((int64_t)d + 1) * esz + 255) / 256 * 256;
}

template <typename T>
int kmv_dtheta(int kind, const T* x, int64_t n, int64_t ldx, int d, const int32_t* cols, const T* inv_ls, double kappa,
               const T* Ut, int64_t ldu, const T* Vt, int64_t ldv, int64_t t, T* out, int64_t ldo, void* work, hipStream_t st)
{
	const int nsplit = kd_nsplit(n, d, t);
	const int ntiles = (int)kp_tiles(n);
	const int nkc = (int)kp_coord_groups(d);
	KdArgs<T> g{x, ldx, (int)n, d, cols, inv_ls, (T)kappa, kind, Ut, ldu, Vt, ldv, (int)t, out, ldo, (T*)work, nsplit, (int)kp_piece_length(n, nsplit), ntiles, nkc};
	if (nsplit >= 1) {
		const dim3 grid((unsigned)ntiles, (unsigned)nsplit, (unsigned)(kp_row_blocks(t) * nkc));
		if (d <= 4) hipLaunchKernelGGL((kmvd_kernel<T, 4, true>), grid, dim3(KP_THREADS), 0, st, g);
		else if (d <= 8) hipLaunchKernelGGL((kmvd_kernel<T, 8, true>), grid, dim3(KP_THREADS), 0, st, g);
		else if (d <= 16) hipLaunchKernelGGL((kmvd_kernel<T, 16, true>), grid, dim3(KP_THREADS), 0, st, g);
		else hipLaunchKernelGGL((kmvd_kernel<T, KP_GC, false>), grid, dim3(KP_THREADS), 0, st, g);
	}
	hipLaunchKernelGGL(kmvd_reduce_kernel<T>, dim3((unsigned)t), dim3(KP_THREADS), 0, st, g);
	return check_launch("stpy_kmv_dtheta");
}

}  // namespace

}  // namespace stpy

// ---- C ABI (include/stpy_hip.h); every refusal below comes before the first HIP call
using namespace stpy;

extern "C" {

int64_t stpy_kmv_dtheta_workspace_bytes(int dtype, int64_t n, int d, int64_t t)
{
	return kd_workspace_bytes(dtype, n, d, t);
}

int stpy_kmv_dtheta(int kind, int dtype, const void* x, int64_t n, int64_t ldx, int d, const int32_t* cols, const void* inv_ls, double kappa,
                    const void* Ut, int64_t ldu, const void* Vt, int64_t ldv, int64_t t,
                    void* out, int64_t ldo, void* work, int64_t work_bytes, void* stream)
{
	int rc;
	if ((rc = kp_check_stationary("stpy_kmv_dtheta", kind)) != 0) return rc;
	if (dtype != STPY_F64 && dtype != STPY_F32) { set_error("stpy_kmv_dtheta: unknown dtype %d (0 = float64, 1 = float32)", dtype); return -2; }
	if (n < 0 || n >= ((int64_t)1 << 31)) { set_error("stpy_kmv_dtheta: n=%lld outside [0, 2^31)", (long long)n); return -4; }
	if (d < 1) { set_error("stpy_kmv_dtheta: d=%d", d); return -6; }
	const int64_t zblocks = (t < 1 ? 0 : kp_row_blocks(t)) * kp_coord_groups(d);
	if (t < 1 || zblocks > 65535) { set_error("stpy_kmv_dtheta: t=%lld outside [1, 65535 * 16 / groups] (groups = 1 up to d = 16, ceil(d / 8) beyond)", (long long)t); return -10; }
	if (ldx < d) { set_error("stpy_kmv_dtheta: ldx=%lld below d=%d", (long long)ldx, d); return -5; }
	if (ldu < n || ldv < n || ldo < (int64_t)d + 2) {
		set_error("stpy_kmv_dtheta: ldu=%lld or ldv=%lld below n=%lld, or ldo=%lld below d + 2 = %lld", (long long)ldu, (long long)ldv, (long long)n, (long long)ldo, (long long)d + 2);
		return -13;
	}
	if (!is_finite(kappa)) { set_error("stpy_kmv_dtheta: kappa=%g must be finite", kappa); return -11; }
	if (!out || (n > 0 && (!x || !inv_ls || !Ut || !Vt))) { set_error("stpy_kmv_dtheta: null pointer"); return -3; }          // (n == 0 reads nothing)
	if (n > 0 && (rc = kp_check_work("stpy_kmv_dtheta", work, work_bytes, kd_workspace_bytes(dtype, n, d, t), 8)) != 0) return rc;
	hipStream_t st = (hipStream_t)stream;
	if (dtype == STPY_F64)
		return kmv_dtheta<double>(kind, (const double*)x, n, ldx, d, cols, (const double*)inv_ls, kappa, (const double*)Ut, ldu, (const double*)Vt, ldv, t,
		                          (double*)out, ldo, work, st);
	return kmv_dtheta<float>(kind, (const float*)x, n, ldx, d, cols, (const float*)inv_ls, kappa, (const float*)Ut, ldu, (const float*)Vt, ldv, t,
	                         (float*)out, ldo, work, st);
}

}  // extern "C"
