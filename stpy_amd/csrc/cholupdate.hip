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
//
// Row deletion (stpy_potrf_delete, GaussianProcess.remove_data_point(iterative=True)) is the same update in disguise.  With S the deleted
// and R the kept indices (both increasing), K[R,R] + s^2 I = L[R,:] L[R,:]^T = L[R,R] L[R,R]^T + U U^T, U = L[R,S]: L[R,R] is lower
// triangular because R is sorted, so the new factor is a rank-k POSITIVE update of the compacted triangle -- no downdate, no pivot that can
// fail on finite data.  A few small launches gather out of place (the indices, the index map R, the compacted triangle in the tile-padded layout
// stpy_potrf leaves, U), then the passes above run on (B, U) from the block column of the first deleted index: rows of U above it are
// zero, so the block columns to its left are copied and never rotated.
#include <atomic>
#include <limits.h>

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
static int chol_update_pass(int64_t n, int kc, T sgn, T* L, int64_t ldl, T* Wc, int64_t ldw, T* tab, int32_t* info, hipStream_t st, int64_t c_first)
{
	int rc;
	const int lds = (int)cu_diag_lds(sizeof(T));
	for (int64_t c0 = c_first; c0 < n; c0 += IB) {
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

// c_first: the first block column the passes visit (a multiple of 128; the rows of W above it are zero, so the block columns to its left
// would see identity rotations).  k == 0: no pass, only the status word and the inverse diagonal tiles.
template <typename T>
int chol_update(int64_t n, int64_t k, int sign, T* L, int64_t ldl, T* winv, T* W, int64_t ldw, void* work, int32_t* info, hipStream_t st,
                int64_t c_first = 0)
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
		if (kc == 1) rc = chol_update_pass<T, 1>(n, kc, sgn, L, ldl, W + k0, ldw, tab, info, st, c_first);
		else if (kc <= 8) rc = chol_update_pass<T, 8>(n, kc, sgn, L, ldl, W + k0, ldw, tab, info, st, c_first);
		else rc = chol_update_pass<T, CU_KC>(n, kc, sgn, L, ldl, W + k0, ldw, tab, info, st, c_first);
		if (rc) return rc;
	}
	hipLaunchKernelGGL((cholupdate_trtri_kernel<T>), dim3((unsigned)((n + IB - 1) / IB)), dim3(IB), lds_tri, st, (const T*)L, ldl, n, winv);
	return check_launch("chol_update (inverse diagonal tiles)");
}

// ------------------------------------------------------------------------------------------
// Row deletion, step 0: the (host-validated) indices into the head of the workspace, PD_STAGE of them per launch, passed by value.
// ------------------------------------------------------------------------------------------
constexpr int PD_STAGE = 256;
struct PdStage { int32_t v[PD_STAGE]; };

__global__ __launch_bounds__(PD_STAGE)
void potrf_delete_stage_kernel(PdStage stage, int cnt, int32_t* __restrict__ del)
{
	if ((int)threadIdx.x < cnt) del[threadIdx.x] = stage.v[threadIdx.x];
}

// ------------------------------------------------------------------------------------------
// Row deletion, step 1: the index map.  rmap[i'] = R[i'] = i' + #{r : del[r] - r <= i'} for i' < n1 (del[r] - r does not decrease: a binary
// search), 0 on the padding [n1, n1p).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void potrf_delete_map_kernel(const int32_t* __restrict__ del, int k, int32_t* __restrict__ rmap, int64_t n1, int64_t n1p)
{
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n1p) return;
	int lo = 0, hi = k;
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if ((int64_t)del[mid] - mid <= i) lo = mid + 1;
		else hi = mid;
	}
	rmap[i] = i < n1 ? (int32_t)(i + lo) : 0;
}

// ------------------------------------------------------------------------------------------
// Step 2: B[i', j'] = A[R[i'], R[j']] on the lower tiles, in the layout stpy_potrf leaves at order n1p: diagonal tiles whole with zeros
// above the diagonal, rows / columns [n1, n1p) of the identity; tiles strictly above the diagonal are not written.  HBM-bound, the
// layout rules of gram.hip: lanes run along j', each owns 16 bytes of a row (2 / 4 adjacent columns: one store, 1 KiB per wave and row),
// a workgroup takes PD_ROWS rows of one strip of 64 such lanes, its four waves alternating rows.  The source column R[j'] = j' + shift(j')
// has a shift that does not decrease and is at most k, so a wave's reads are runs of consecutive addresses broken at most k times; a
// lane's column indices are loaded once, the row index is wave-uniform.  vec: B and ldb are 16-byte aligned (else element stores).
// ------------------------------------------------------------------------------------------
constexpr int PD_ROWS = 32;

template <typename T>
__global__ __launch_bounds__(256)
void potrf_delete_gather_kernel(const T* __restrict__ A, int64_t lda, T* __restrict__ B, int64_t ldb, const int32_t* __restrict__ rmap,
                                int64_t n1, int64_t n1p, int vec)
{
	constexpr int V = 16 / (int)sizeof(T);
	typedef T vT __attribute__((ext_vector_type(V)));
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int64_t i0 = (int64_t)blockIdx.y * PD_ROWS;
	const int64_t j0 = ((int64_t)blockIdx.x * 64 + lane) * V;          // (a multiple of V: the V columns share one 128-tile)
	if (j0 >= n1p) return;
	const int64_t tj = j0 / IB;
	if (tj > (i0 + PD_ROWS - 1) / IB) return;
	int32_t src[V];
#pragma unroll
	for (int q = 0; q < V; ++q) src[q] = j0 + q < n1 ? rmap[j0 + q] : 0;
#pragma unroll
	for (int t = 0; t < PD_ROWS / 4; ++t) {
		const int64_t i = i0 + wave + 4 * t;
		if (i >= n1p || tj > i / IB) continue;
		T v[V];
		if (i < n1) {
			const T* Ar = A + (int64_t)rmap[i] * lda;
#pragma unroll
			for (int q = 0; q < V; ++q) v[q] = j0 + q <= i ? Ar[src[q]] : T(0);
		} else {
#pragma unroll
			for (int q = 0; q < V; ++q) v[q] = j0 + q == i ? T(1) : T(0);
		}
		T* Bi = B + i * ldb + j0;
		if (vec) {
			vT o;
#pragma unroll
			for (int q = 0; q < V; ++q) o[q] = v[q];
			*(vT*)Bi = o;
		} else {
#pragma unroll
			for (int q = 0; q < V; ++q) Bi[q] = v[q];
		}
	}
}

// ------------------------------------------------------------------------------------------
// Step 3: U[i', r] = A[R[i'], del[r]] where del[r] < R[i'] (the part of the deleted columns left of the diagonal), else 0; n1p rows of k
// contiguous elements, rows [n1, n1p) zero.  Lanes run along r, then i': the STORES are consecutive; the reads are not -- a lane's
// source is one element of row R[i'], k scattered elements per row and a stride of lda between rows (for k = 1 a column walk), n1 k
// elements in all, a 1 / n1 share of what the gather moves and nothing beside a rotation pass.
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256)
void potrf_delete_u_kernel(const T* __restrict__ A, int64_t lda, const int32_t* __restrict__ del, const int32_t* __restrict__ rmap,
                           T* __restrict__ U, int64_t n1, int64_t total, int k)
{
	for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
		const int64_t i = idx / k;
		const int r = (int)(idx - i * k);
		T v = T(0);
		if (i < n1) {
			const int32_t ri = rmap[i], s = del[r];
			if (s < ri) v = A[(int64_t)ri * lda + s];
		}
		U[idx] = v;
	}
}

static inline int64_t pd_pad(int64_t n) { return (n + IB - 1) / IB * IB; }
static inline int64_t pd_round16(int64_t b) { return (b + 15) / 16 * 16; }
// workspace of stpy_potrf_delete: [del: k int32][rmap: pad(n0) int32][rotation table][U: pad(n0) x k], each part 16-byte aligned.  Sized by
// pad(n0), not pad(n0 - k), so that the query does not shrink when k grows.
static inline int64_t pd_off_map(int64_t k) { return pd_round16(4 * k); }
static inline int64_t pd_off_tab(int64_t n0, int64_t k) { return pd_off_map(k) + 4 * pd_pad(n0); }
static inline int64_t pd_off_u(size_t esz, int64_t n0, int64_t k) { return pd_off_tab(n0, k) + pd_round16(chol_update_workspace_bytes(esz)); }
int64_t potrf_delete_workspace_bytes(size_t esz, int64_t n0, int64_t k) { return pd_off_u(esz, n0, k) + pd_round16(pd_pad(n0) * k * (int64_t)esz); }

template <typename T>
int potrf_delete(int64_t n0, int64_t k, const int32_t* del_host, const T* A, int64_t lda, T* B, int64_t ldb, T* winv, void* work, int32_t* info,
                 hipStream_t st)
{
	const int64_t n1 = n0 - k, n1p = pd_pad(n1);
	char* w = (char*)work;
	int32_t* del = (int32_t*)w;
	int32_t* rmap = (int32_t*)(w + pd_off_map(k));
	void* tab = w + pd_off_tab(n0, k);
	T* U = (T*)(w + pd_off_u(sizeof(T), n0, k));
	int rc;
	// the indices travel as kernel ARGUMENTS, PD_STAGE at a time: a launch copies its arguments, so del_host has been read when this
	// returns and nothing waits for the stream (a copy from pageable host memory would make the runtime drain the stream first)
	for (int64_t r0 = 0; r0 < k; r0 += PD_STAGE) {
		PdStage stage;
		const int cnt = (int)(k - r0 < PD_STAGE ? k - r0 : PD_STAGE);
		for (int q = 0; q < PD_STAGE; ++q) stage.v[q] = q < cnt ? del_host[r0 + q] : 0;
		hipLaunchKernelGGL(potrf_delete_stage_kernel, dim3(1), dim3(PD_STAGE), 0, st, stage, cnt, del + r0);
		if ((rc = check_launch("potrf_delete (indices)"))) return rc;
	}
	hipLaunchKernelGGL(potrf_delete_map_kernel, dim3((unsigned)((n1p + 255) / 256)), dim3(256), 0, st, (const int32_t*)del, (int)k, rmap, n1, n1p);
	if ((rc = check_launch("potrf_delete (index map)"))) return rc;
	constexpr int V = 16 / (int)sizeof(T);
	const int vec = ((uintptr_t)B % 16 == 0 && ldb % V == 0) ? 1 : 0;
	hipLaunchKernelGGL((potrf_delete_gather_kernel<T>), dim3((unsigned)((n1p + 64 * V - 1) / (64 * V)), (unsigned)((n1p + PD_ROWS - 1) / PD_ROWS)), dim3(256), 0, st,
	                   A, lda, B, ldb, (const int32_t*)rmap, n1, n1p, vec);
	if ((rc = check_launch("potrf_delete (gather)"))) return rc;
	// U is zero above the first deleted row: all of it when the deleted rows are the last ones -- then the compacted triangle IS the factor
	const bool rotate = del_host[0] < n1;
	if (rotate) {
		const int64_t total = n1p * k;
		const int64_t blocks = (total + 255) / 256;
		hipLaunchKernelGGL((potrf_delete_u_kernel<T>), dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, A, lda, (const int32_t*)del,
		                   (const int32_t*)rmap, U, n1, total, (int)k);
		if ((rc = check_launch("potrf_delete (deleted columns)"))) return rc;
	}
	return chol_update<T>(n1, rotate ? k : 0, 1, B, ldb, winv, U, k, tab, info, st, rotate ? (del_host[0] / IB) * IB : 0);
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

int64_t stpy_potrf_delete_workspace_bytes(int dtype, int64_t n0, int64_t k)
{
	if (n0 <= 0 || k <= 0) return 0;
	return potrf_delete_workspace_bytes(dtype == STPY_F32 ? 4 : 8, n0, k);
}

int stpy_potrf_delete(int dtype, int64_t n0, int64_t k, const int32_t* del_host, const void* A, int64_t lda, void* B, int64_t ldb,
                      void* winv, int64_t winv_elems, void* work, int64_t work_bytes, int32_t* info_dev, void* stream)
{
	if (k == 0) return 0;          // nothing to delete: nothing is read or written
	if (dtype != STPY_F64 && dtype != STPY_F32) { set_error("stpy_potrf_delete: unknown dtype %d (0 = float64, 1 = float32)", dtype); return -1; }
	if (n0 < 1 || n0 > INT32_MAX) { set_error("stpy_potrf_delete: n0=%lld (1 .. 2^31 - 1)", (long long)n0); return -2; }
	if (k < 0 || k >= n0) { set_error("stpy_potrf_delete: k=%lld rows of n0=%lld (0 <= k < n0)", (long long)k, (long long)n0); return -3; }
	if (!del_host) { set_error("stpy_potrf_delete: null pointer del_host"); return -4; }
	if (!A) { set_error("stpy_potrf_delete: null pointer A"); return -5; }
	if (!B) { set_error("stpy_potrf_delete: null pointer B"); return -7; }
	if (!winv) { set_error("stpy_potrf_delete: null pointer winv"); return -9; }
	if (!work) { set_error("stpy_potrf_delete: null pointer work"); return -11; }
	if (!info_dev) { set_error("stpy_potrf_delete: null pointer info_dev"); return -13; }
	for (int64_t r = 0; r < k; ++r) {
		if (del_host[r] < 0 || del_host[r] >= n0) {
			set_error("stpy_potrf_delete: del_host[%lld]=%d outside [0, n0=%lld)", (long long)r, (int)del_host[r], (long long)n0);
			return -15;
		}
		if (r > 0 && del_host[r] <= del_host[r - 1]) {
			set_error("stpy_potrf_delete: del_host[%lld]=%d after %d: the indices must increase strictly", (long long)r, (int)del_host[r], (int)del_host[r - 1]);
			return -15;
		}
	}
	const int64_t n0p = pd_pad(n0), n1p = pd_pad(n0 - k);
	if (lda < n0p) { set_error("stpy_potrf_delete: lda=%lld below the padded old order %lld", (long long)lda, (long long)n0p); return -6; }
	if (ldb < n1p) { set_error("stpy_potrf_delete: ldb=%lld below the padded new order %lld", (long long)ldb, (long long)n1p); return -8; }
	const int64_t esz = dtype == STPY_F32 ? 4 : 8;
	const uintptr_t a0 = (uintptr_t)A, a1 = a0 + (uintptr_t)(((n0p - 1) * lda + n0p) * esz);
	const uintptr_t b0 = (uintptr_t)B, b1 = b0 + (uintptr_t)(((n1p - 1) * ldb + n1p) * esz);
	if (a0 < b1 && b0 < a1) { set_error("stpy_potrf_delete: A and B overlap (the compaction is out of place)"); return -16; }
	const int64_t winv_need = (n1p / IB) * (int64_t)IB * IB;
	if (winv_elems < winv_need) {
		set_error("stpy_potrf_delete: winv holds %lld elements, %lld needed (stpy_potrf_winv_elems of the new order)", (long long)winv_elems, (long long)winv_need);
		return -21;
	}
	const int64_t work_need = stpy_potrf_delete_workspace_bytes(dtype, n0, k);
	if (work_bytes < work_need) {
		set_error("stpy_potrf_delete: workspace of %lld bytes, %lld needed (stpy_potrf_delete_workspace_bytes)", (long long)work_bytes, (long long)work_need);
		return -20;
	}
	hipStream_t st = (hipStream_t)stream;
	if (dtype == STPY_F64)
		return potrf_delete<double>(n0, k, del_host, (const double*)A, lda, (double*)B, ldb, (double*)winv, work, info_dev, st);
	return potrf_delete<float>(n0, k, del_host, (const float*)A, lda, (float*)B, ldb, (float*)winv, work, info_dev, st);
}

}  // extern "C"
