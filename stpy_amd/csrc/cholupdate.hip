// cholupdate.hip -- rank-k update / downdate of a resident Cholesky factor in place (stpy_chol_update, the incremental step
// behind KernelizedFeatures.add_data_point(iterative=True)):  L' L'^T = L L^T + sign W W^T.
//
// W^T is eliminated against L^T column by column with plane rotations (hyperbolic ones for sign = -1).  For column j and
// column r of W, with a = l_jj, w = w_jr and b = sqrt(a^2 + sign w^2):
//     c = b / a,  s = w / a,  1/c = a / b;      l_ij <- (l_ij + sign s w_ir) / c,   w_ir <- c w_ir - s l_ij(new)      for i > j
// and l_jj <- b, w_jr <- 0.  All kc rotations of a column depend on row j only (l_jj and w_j after the columns before j), so the
// column's pivots come from prefix sums d_r = l_jj^2 + sign sum_{q<r} w_jq^2 (a = sqrt(d_r), b = sqrt(d_{r+1})): kc lanes
// compute them side by side and the square roots / reciprocals are off the row recurrence.
//
// Block columns of 128, two launches per block column: cholupdate_diag_kernel (one workgroup: L_cc and the 128 x kc block of W in
// LDS / registers, writes L'_cc, the rotation table (c, s, 1/c) of the block column and the status word), then
// cholupdate_rows_kernel (64 rows per workgroup, one row per lane: its 128 entries of L pass through LDS so that every global
// access is a run of consecutive addresses, its kc entries of W stay in registers; the table of the 64 columns in flight sits
// in LDS and is read with wave-uniform addresses).  At most CU_KC columns of W ride along in one pass over L; a wider W is cut into chunks, each a complete
// update of its own.  One last launch rebuilds every inverse diagonal tile.  Every sum has a fixed order: bit-reproducible.
#include <atomic>

#include "common.h"

namespace stpy {

constexpr int CU_KC = 32;           // columns of W per pass over L (registers of the row kernel: CU_KC elements per lane)
constexpr int CU_ROWS = 64;         // rows per workgroup of the row kernel (one wave)
constexpr int CU_CT = 64;           // columns of L staged at a time by the row kernel
constexpr int CU_LD = IB + 1;       // LDS row stride of the diagonal block: odd, so a column walk is conflict-free

static inline size_t cu_diag_lds(size_t esz) { return ((size_t)IB * CU_LD + IB + 4 * CU_KC) * esz; }

// ------------------------------------------------------------------------------------------
// Block column c0 / 128: rotations of its nb <= 128 columns against the kc columns of W (W points at the chunk's first column).
// Thread i owns row i of the block: its entries of L in LDS, its kc entries of W in registers.
//   tab[(j * kc + r) * 3 + {0, 1, 2}] = c, s, 1/c of column j, rotation r
//   *info: first column (1-based, global) whose pivot is not positive and finite; its rotations are replaced by the identity
// ------------------------------------------------------------------------------------------
template <typename T, int KC>
__global__ __launch_bounds__(IB)
void cholupdate_diag_kernel(T* __restrict__ L, int64_t ldl, const T* __restrict__ W, int64_t ldw, int64_t n, int64_t c0, int kc, T sgn,
                            T* __restrict__ tab, int32_t* info)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
	T* S = (T*)smem_raw;                  // [IB][CU_LD] lower triangle of L_cc
	T* newd = S + IB * CU_LD;             // [IB] the new diagonal
	T* wrow = newd + IB;                  // [CU_KC] row j of W
	T* tabs = wrow + CU_KC;               // [CU_KC][3] the rotations of column j
	const int tid = threadIdx.x;
	const int nb = (int)(n - c0 < IB ? n - c0 : IB);
	for (int idx = tid; idx < IB * IB; idx += IB) {
		const int i = idx >> 7, j = idx & 127;
		S[i * CU_LD + j] = (i < nb && j <= i) ? L[(c0 + i) * ldl + c0 + j] : T(0);
	}
	T w[KC];
#pragma unroll
	for (int r = 0; r < KC; ++r) w[r] = (tid < nb && r < kc) ? W[(c0 + tid) * ldw + r] : T(0);
	__syncthreads();
	for (int j = 0; j < nb; ++j) {
		if (tid == j) {
#pragma unroll
			for (int r = 0; r < KC; ++r) wrow[r] = w[r];
		}
		__syncthreads();
		if (tid < kc) {
			const int r = tid;
			const T ljj = S[j * CU_LD + j];
			T d = ljj * ljj;
			for (int q = 0; q < r; ++q) d += sgn * (wrow[q] * wrow[q]);
			const T wr = wrow[r];
			const T d1 = d + sgn * (wr * wr);
			const bool good = d1 > T(0) && d1 < (T)__builtin_huge_val();
			const bool ok = good && d > T(0);          // (a pivot that failed earlier in this column was reported by its own lane)
			T cs = T(1), sn = T(0), ic = T(1), b = ljj;
			if (ok) {
				const T a = sqrt(d);
				b = sqrt(d1);
				const T ia = T(1) / a, ib = T(1) / b;
				cs = b * ia; sn = wr * ia; ic = a * ib;
			}
			if (!good) atomicCAS(info, 0, (int32_t)(c0 + j + 1));
			tabs[r * 3 + 0] = cs; tabs[r * 3 + 1] = sn; tabs[r * 3 + 2] = ic;
			T* tg = tab + ((int64_t)j * kc + r) * 3;
			tg[0] = cs; tg[1] = sn; tg[2] = ic;
			if (r == kc - 1) newd[j] = b;
		}
		__syncthreads();
		if (tid > j && tid < nb) {
			T l = S[tid * CU_LD + j];
#pragma unroll
			for (int r = 0; r < KC; ++r) {
				if (r < kc) {
					const T cs = tabs[r * 3 + 0], sn = tabs[r * 3 + 1], ic = tabs[r * 3 + 2];
					l = (l + sgn * sn * w[r]) * ic;
					w[r] = cs * w[r] - sn * l;
				}
			}
			S[tid * CU_LD + j] = l;
		}
	}
	__syncthreads();
	for (int idx = tid; idx < IB * IB; idx += IB) {
		const int i = idx >> 7, j = idx & 127;
		if (i < nb && j <= i) L[(c0 + i) * ldl + c0 + j] = (i == j) ? newd[i] : S[i * CU_LD + j];
	}
}

// ------------------------------------------------------------------------------------------
// The rows below block column c0 / 128 (which is whole: there are rows below it): workgroup b takes rows
// [c0 + 128 + 64 b, + 64), lane = row.  L passes through LDS 64 columns at a time (loads and stores are runs of 64 consecutive
// elements of one row), W (kc <= KC columns) through the same buffer into registers and back.
// ------------------------------------------------------------------------------------------
template <typename T, int KC>
__global__ __launch_bounds__(CU_ROWS)
void cholupdate_rows_kernel(T* __restrict__ L, int64_t ldl, T* __restrict__ W, int64_t ldw, int64_t n, int64_t c0, int kc, T sgn,
                            const T* __restrict__ tab)
{
	__shared__ T tile[CU_ROWS][CU_CT + 1];
	__shared__ T tabs[CU_CT * KC * 3];          // the rotations of the 64 columns in flight
	const int tid = threadIdx.x;
	const int64_t r0 = c0 + IB + (int64_t)blockIdx.x * CU_ROWS;
	if (r0 >= n) return;
	const int rows = (int)(n - r0 < CU_ROWS ? n - r0 : CU_ROWS);
	if (KC == 1) kc = 1;
	for (int idx = tid; idx < rows * kc; idx += CU_ROWS) {
		const int rr = idx / kc, cc = idx - rr * kc;
		tile[rr][cc] = W[(r0 + rr) * ldw + cc];
	}
	__syncthreads();
	T w[KC];
#pragma unroll
	for (int r = 0; r < KC; ++r) w[r] = (tid < rows && r < kc) ? tile[tid][r] : T(0);
	__syncthreads();
	for (int h = 0; h < IB / CU_CT; ++h) {
		T* Lh = L + r0 * ldl + c0 + h * CU_CT + tid;
		// rows at or beyond n repeat the last row (loads in flight sixteen at a time; those copies are never stored)
#pragma unroll
		for (int r8 = 0; r8 < CU_ROWS; r8 += 16) {
			T v[16];
#pragma unroll
			for (int q = 0; q < 16; ++q) v[q] = Lh[(int64_t)(r8 + q < rows ? r8 + q : rows - 1) * ldl];
#pragma unroll
			for (int q = 0; q < 16; ++q) tile[r8 + q][tid] = v[q];
		}
		const T* th = tab + (int64_t)h * CU_CT * kc * 3;
#pragma unroll 8
		for (int idx = tid; idx < CU_CT * kc * 3; idx += CU_ROWS) tabs[idx] = th[idx];
		__syncthreads();
		if (tid < rows) {
			const T* tj = tabs;
			for (int jj = 0; jj < CU_CT; ++jj) {
				T l = tile[tid][jj];
#pragma unroll
				for (int r = 0; r < KC; ++r) {
					if (KC == 1 || r < kc) {
						const T cs = tj[r * 3 + 0], sn = tj[r * 3 + 1], ic = tj[r * 3 + 2];
						l = (l + sgn * sn * w[r]) * ic;
						w[r] = cs * w[r] - sn * l;
					}
				}
				tile[tid][jj] = l;
				tj += kc * 3;
			}
		}
		__syncthreads();
#pragma unroll 16
		for (int rr = 0; rr < CU_ROWS; ++rr)
			if (rr < rows) Lh[(int64_t)rr * ldl] = tile[rr][tid];
		__syncthreads();
	}
	if (tid < rows) {
#pragma unroll
		for (int r = 0; r < KC; ++r)
			if (r < kc) tile[tid][r] = w[r];
	}
	__syncthreads();
	for (int idx = tid; idx < rows * kc; idx += CU_ROWS) {
		const int rr = idx / kc, cc = idx - rr * kc;
		W[(r0 + rr) * ldw + cc] = tile[rr][cc];
	}
}

// ------------------------------------------------------------------------------------------
// inverse(L_cc) of every 128 x 128 diagonal tile (one workgroup per tile; row-major, zero above the diagonal, identity on the rows /
// columns of a ragged last tile at or beyond n: the layout stpy_potrf leaves).  The forward substitution of append_trtri_kernel:
// thread j owns column j of the inverse (in LDS), every thread walks the same row of L (staged in LDS row by row) in a fixed order.
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(IB)
void cholupdate_trtri_kernel(const T* __restrict__ L, int64_t ldl, int64_t n, T* __restrict__ winv)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
	T* xs = (T*)smem_raw;                        // xs[l * IB + j] = X[l][j]
	T* lrow = xs + IB * IB;                      // [2][IB] row i of L_cc (two buffers: one barrier per row)
	const int j = threadIdx.x;
	const int64_t c = (int64_t)blockIdx.x * IB;
	const int nb = (int)(n - c < IB ? n - c : IB);
	const T* Lc = L + c * ldl + c;
	T nxt = j == 0 ? Lc[0] : T(0);
	for (int i = 0; i < IB; ++i) {
		T* li = lrow + (i & 1) * IB;
		li[j] = nxt;
		__syncthreads();
		nxt = (i + 1 < nb && j <= i + 1) ? Lc[(int64_t)(i + 1) * ldl + j] : T(0);          // (the next row is on its way during this one)
		T x = (i == j) ? T(1) : T(0);
		if (i < nb && i > j) {
			T s = T(0);
			for (int l = j; l < i; ++l) s -= li[l] * xs[l * IB + j];
			x = s / li[i];
		} else if (i < nb && i == j) {
			x = T(1) / li[i];
		}
		xs[i * IB + j] = x;
	}
	T* Wc = winv + (int64_t)blockIdx.x * IB * IB;
	for (int i = 0; i < IB; ++i) Wc[i * IB + j] = xs[i * IB + j];
}

int64_t chol_update_workspace_bytes(size_t esz) { return (int64_t)IB * CU_KC * 3 * (int64_t)esz; }

template <typename T, int KC>
static int chol_update_pass(int64_t n, int kc, T sgn, T* L, int64_t ldl, T* Wc, int64_t ldw, T* tab, int32_t* info, hipStream_t st)
{
	int rc;
	const int lds = (int)cu_diag_lds(sizeof(T));
	for (int64_t c0 = 0; c0 < n; c0 += IB) {
		hipLaunchKernelGGL((cholupdate_diag_kernel<T, KC>), dim3(1), dim3(IB), lds, st, L, ldl, (const T*)Wc, ldw, n, c0, kc, sgn, tab, info);
		if ((rc = check_launch("chol_update (diagonal block)"))) return rc;
		const int64_t below = n - c0 - IB;
		if (below > 0) {
			hipLaunchKernelGGL((cholupdate_rows_kernel<T, KC>), dim3((unsigned)((below + CU_ROWS - 1) / CU_ROWS)), dim3(CU_ROWS), 0, st, L, ldl, Wc, ldw, n, c0, kc, sgn,
			                   (const T*)tab);
			if ((rc = check_launch("chol_update (rows)"))) return rc;
		}
	}
	return 0;
}

template <typename T>
int chol_update(int64_t n, int64_t k, int sign, T* L, int64_t ldl, T* winv, T* W, int64_t ldw, void* work, int32_t* info, hipStream_t st)
{
	static std::atomic<bool> attr_set[2];
	const int which = sizeof(T) == 8 ? 0 : 1;
	const int lds_diag = (int)cu_diag_lds(sizeof(T)), lds_tri = (int)((IB * IB + 2 * IB) * sizeof(T));
	if (!attr_set[which].load(std::memory_order_acquire)) {
		hipError_t e = hipFuncSetAttribute((const void*)cholupdate_diag_kernel<T, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_diag);
		if (e == hipSuccess) e = hipFuncSetAttribute((const void*)cholupdate_diag_kernel<T, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_diag);
		if (e == hipSuccess) e = hipFuncSetAttribute((const void*)cholupdate_diag_kernel<T, CU_KC>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_diag);
		if (e == hipSuccess) e = hipFuncSetAttribute((const void*)cholupdate_trtri_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_tri);
		if (e != hipSuccess) { set_error("chol_update: hipFuncSetAttribute failed: %s", hipGetErrorString(e)); return -1000 - (int)e; }
		attr_set[which].store(true, std::memory_order_release);
	}
	if (hipMemsetAsync(info, 0, sizeof(int32_t), st) != hipSuccess) { set_error("chol_update: hipMemsetAsync failed"); return -1004; }
	T* tab = (T*)work;
	const T sgn = sign > 0 ? T(1) : T(-1);
	int rc;
	// chunks of at most CU_KC columns of W, each a complete update of the factor the chunk before left
	for (int64_t k0 = 0; k0 < k; k0 += CU_KC) {
		const int kc = (int)(k - k0 < CU_KC ? k - k0 : CU_KC);
		if (kc == 1) rc = chol_update_pass<T, 1>(n, kc, sgn, L, ldl, W + k0, ldw, tab, info, st);
		else if (kc <= 8) rc = chol_update_pass<T, 8>(n, kc, sgn, L, ldl, W + k0, ldw, tab, info, st);
		else rc = chol_update_pass<T, CU_KC>(n, kc, sgn, L, ldl, W + k0, ldw, tab, info, st);
		if (rc) return rc;
	}
	hipLaunchKernelGGL((cholupdate_trtri_kernel<T>), dim3((unsigned)((n + IB - 1) / IB)), dim3(IB), lds_tri, st, (const T*)L, ldl, n, winv);
	return check_launch("chol_update (inverse diagonal tiles)");
}

}  // namespace stpy

using namespace stpy;

extern "C" {

int64_t stpy_chol_update_workspace_bytes(int dtype, int64_t n, int64_t k)
{
	if (n <= 0 || k <= 0) return 0;
	return chol_update_workspace_bytes(dtype == STPY_F32 ? 4 : 8);
}

int stpy_chol_update(int dtype, int64_t n, int64_t k, int sign, void* L, int64_t ldl, void* winv, int64_t winv_elems,
                     void* W, int64_t ldw, void* work, int64_t work_bytes, int32_t* info_dev, void* stream)
{
	if (n == 0 || k == 0) return 0;          // empty problem: nothing is read or written (empty tensors have null data pointers)
	if (dtype != STPY_F64 && dtype != STPY_F32) { set_error("stpy_chol_update: unknown dtype %d (0 = float64, 1 = float32)", dtype); return -1; }
	if (n < 0) { set_error("stpy_chol_update: n=%lld", (long long)n); return -2; }
	if (k < 0) { set_error("stpy_chol_update: k=%lld", (long long)k); return -3; }
	if (sign != 1 && sign != -1) { set_error("stpy_chol_update: sign=%d (+1: update, -1: downdate)", sign); return -4; }
	if (!L) { set_error("stpy_chol_update: null pointer L"); return -5; }
	if (ldl < n) { set_error("stpy_chol_update: ldl=%lld below n=%lld", (long long)ldl, (long long)n); return -6; }
	if (!winv) { set_error("stpy_chol_update: null pointer winv"); return -7; }
	const int64_t winv_need = ((n + IB - 1) / IB) * (int64_t)IB * IB;
	if (winv_elems < winv_need) {
		set_error("stpy_chol_update: winv holds %lld elements, %lld needed (stpy_potrf_winv_elems(n))", (long long)winv_elems, (long long)winv_need);
		return -21;
	}
	if (!W) { set_error("stpy_chol_update: null pointer W"); return -9; }
	if (ldw < k) { set_error("stpy_chol_update: ldw=%lld below k=%lld", (long long)ldw, (long long)k); return -10; }
	if (!work) { set_error("stpy_chol_update: null pointer work"); return -11; }
	const int64_t work_need = stpy_chol_update_workspace_bytes(dtype, n, k);
	if (work_bytes < work_need) {
		set_error("stpy_chol_update: workspace of %lld bytes, %lld needed (stpy_chol_update_workspace_bytes)", (long long)work_bytes, (long long)work_need);
		return -20;
	}
	if (!info_dev) { set_error("stpy_chol_update: null pointer info_dev"); return -13; }
	hipStream_t st = (hipStream_t)stream;
	if (dtype == STPY_F64)
		return chol_update<double>(n, k, sign, (double*)L, ldl, (double*)winv, (double*)W, ldw, work, info_dev, st);
	return chol_update<float>(n, k, sign, (float*)L, ldl, (float*)winv, (float*)W, ldw, work, info_dev, st);
}

}  // extern "C"
