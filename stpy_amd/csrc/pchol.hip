// Greedy pivoted partial Cholesky of a kernel matrix whose columns are generated on the fly (stpy_pchol): the landmark choice of the
// Nystrom features.  K (n x n) is never formed; the factor is kept TRANSPOSED, Ft (m x n, row j = column j of F), so that a step reads
// and writes whole rows and the result is the "row x K" operand stpy_syrk / stpy_gemm_nt take.
//
// One launch per step j, plus one before (residual diagonal = kappa, pivots = -1, rank word = m, first partial argmaxes) and one after
// (rows [rank, m) of Ft zeroed, dres set to 0 exactly on the pivots).  Inside a step every workgroup owns a tile of 64 * V points (V = 16 bytes / element: 128 fp64, 256 fp32):
//   1. it reduces the per-tile (value, index) argmaxes the previous launch wrote -- "larger value, then lower index" is a total order, so
//      every workgroup arrives at the same pivot p whatever order it reduces in; p's residual at or below tol * kappa (or not positive)
//      stops the factorisation: workgroup 0 writes the rank word and every later launch returns on reading it;
//   2. chunks of 1024 values Ft[l, p] go to LDS, and the four waves stream the tile's part of rows l = w, w + 4, ... of the chunk with one
//      16-byte load per lane and row (lane owns V neighbouring points), each lane a running sum per point;
//   3. the four wave sums of a point are added in wave order, the new row entry (k(x_i, x_p) - sum) / sqrt(dres[p]) is written, dres
//      updated (the pivot's set to 0 exactly), and the tile's own argmax goes to the OTHER half of the double-buffered partials.
// No workgroup reads what another writes inside a launch: no spin-waits, no cooperative grid, no atomics.  Every sum has a fixed order
// and the argmax does not depend on one, so two calls on the same input give the same bits.
// Kernel values come from direct coordinate differences (kappa (d + 8) eps wherever the data lies, kappa exactly on coincident points).
// Traffic: step j reads j * n elements, a run of rank r reads esz * n * r (r - 1) / 2 bytes; the kernel is a streaming read, bounded by
// HBM once Ft outgrows the Infinity Cache.  The redundant part -- every workgroup gathers Ft[0:j, p] (j scattered lines) and reads all
// the partials -- is j / (64 V) of that.
#include "common.h"
#include "kmv_pair.h"          // pc_phi / pc_fma / pc_sqrt: the one direct-difference evaluator, shared with the matrix-free products

#include <limits.h>
#include <math.h>

namespace stpy {

namespace {

constexpr int PC_THREADS = 256, PC_WAVES = 4;
constexpr int PC_CHUNK = 1024;         // values Ft[l, p] staged in LDS at a time: 8 KiB (fp64); the chunking is why LDS sets no cap on m
constexpr int PC_MAX_M = 8192;         // the cap on m is the launch count of one call (one launch per step), not a memory budget

struct PcholPart { double v; int32_t i; int32_t pad; };          // a tile's largest residual (exact in double for both types) and its lowest index

template <typename T> struct PcVec;
template <> struct PcVec<double> { static constexpr int V = 2; typedef double vec __attribute__((ext_vector_type(2))); };
template <> struct PcVec<float> { static constexpr int V = 4; typedef float vec __attribute__((ext_vector_type(4))); };

template <typename T>
struct PcholArgs {
	const T* x; int64_t ldx; int n, d; const int32_t* cols; const T* inv_ls; T kappa; double thr; int kind;
	T* Ft; int64_t ldf; T* dres; int32_t* piv; int32_t* rank; PcholPart* part; int nblk, m, vec_ok;
};

// the argmax order: larger value first, then the lower index.  A NaN is never better than anything.
__device__ __forceinline__ bool pc_better(double v, int i, double bv, int bi) { return v > bv || (v == bv && i < bi); }

// (value, index) maximum over the workgroup, the same in every thread; rv / ri: PC_WAVES words each
__device__ __forceinline__ void pc_block_argmax(double& bv, int& bi, double* rv, int* ri)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		const double ov = __shfl_xor(bv, o);
		const int oi = __shfl_xor(bi, o);
		if (pc_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
	}
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	if (lane == 0) { rv[w] = bv; ri[w] = bi; }
	__syncthreads();
	bv = rv[0]; bi = ri[0];
#pragma unroll
	for (int k = 1; k < PC_WAVES; ++k)
		if (pc_better(rv[k], ri[k], bv, bi)) { bv = rv[k]; bi = ri[k]; }
}

template <typename T>
__global__ __launch_bounds__(PC_THREADS)
void pchol_init_kernel(PcholArgs<T> a)
{
	constexpr int TILE = 64 * PcVec<T>::V;
	const int64_t g = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x;
	if (g < a.n) a.dres[g] = a.kappa;
	if (g < a.m) a.piv[g] = -1;
	if (g < a.nblk) a.part[g] = PcholPart{(double)a.kappa, (int32_t)(g * TILE), 0};          // all equal: the tile's lowest index
	if (g == 0) *a.rank = a.m;
}

template <typename T>
__global__ __launch_bounds__(PC_THREADS)
void pchol_step_kernel(PcholArgs<T> a, int j)
{
	constexpr int V = PcVec<T>::V, TILE = 64 * V;
	typedef typename PcVec<T>::vec vec;
	__shared__ T fp[PC_CHUNK];
	__shared__ T red[PC_WAVES][TILE];
	__shared__ double rv[PC_WAVES];
	__shared__ int ri[PC_WAVES];
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	if (*a.rank < j) return;                                          // stopped in an earlier launch (the whole grid reads the same word)

	// 1. the pivot: argmax of the partials of the previous launch
	const PcholPart* prev = a.part + (int64_t)(j & 1) * a.nblk;
	double bv = -INFINITY;
	int bi = INT_MAX;
	for (int b = tid; b < a.nblk; b += PC_THREADS) {
		const PcholPart q = prev[b];
		if (pc_better(q.v, q.i, bv, bi)) { bv = q.v; bi = q.i; }
	}
	pc_block_argmax(bv, bi, rv, ri);
	if (!(bv > a.thr) || !(bv > 0.0) || bi < 0 || bi >= a.n) {          // (workgroup-uniform) below the tolerance, or no finite residual left
		if (blockIdx.x == 0 && tid == 0) *a.rank = j;
		return;
	}
	const int p = bi;
	const T dp = (T)bv;
	if (blockIdx.x == 0 && tid == 0) a.piv[j] = p;

	// 2. sum_{l < j} Ft[l, i] Ft[l, p] for the tile's points: wave w takes the rows l = w (mod 4) of every chunk
	const int64_t i0 = (int64_t)blockIdx.x * TILE + lane * V;
	const bool whole = a.vec_ok && i0 + V <= a.n;
	T acc[V];
#pragma unroll
	for (int v = 0; v < V; ++v) acc[v] = (T)0;
	for (int c0 = 0; c0 < j; c0 += PC_CHUNK) {
		const int cl = min(PC_CHUNK, j - c0);
		__syncthreads();                                              // (fp may still be read; rv / ri have been read)
		for (int t = tid; t < cl; t += PC_THREADS) fp[t] = a.Ft[(int64_t)(c0 + t) * a.ldf + p];
		__syncthreads();
		const T* base = a.Ft + (int64_t)c0 * a.ldf + i0;
		if (whole) {
#pragma unroll 8
			for (int l = w; l < cl; l += PC_WAVES) {
				const vec f = *reinterpret_cast<const vec*>(base + (int64_t)l * a.ldf);
				const T s = fp[l];
#pragma unroll
				for (int v = 0; v < V; ++v) acc[v] = pc_fma(f[v], s, acc[v]);
			}
		} else if (i0 < a.n) {
			for (int l = w; l < cl; l += PC_WAVES) {
				const T s = fp[l];
#pragma unroll
				for (int v = 0; v < V; ++v)
					if (i0 + v < a.n) acc[v] = pc_fma(base[(int64_t)l * a.ldf + v], s, acc[v]);
			}
		}
	}
#pragma unroll
	for (int v = 0; v < V; ++v) red[w][lane * V + v] = acc[v];
	__syncthreads();

	// 3. the new row, the residual diagonal, the tile's argmax
	bv = -INFINITY;
	bi = INT_MAX;
	const int64_t i = (int64_t)blockIdx.x * TILE + tid;
	if (tid < TILE && i < a.n) {
		const T s = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
		const T* xi = a.x + i * a.ldx;
		const T* xp = a.x + (int64_t)p * a.ldx;
		T r2 = (T)0;
		for (int k = 0; k < a.d; ++k) {
			const int c = a.cols ? a.cols[k] : k;
			const T u = (xi[c] - xp[c]) * a.inv_ls[k];
			r2 = pc_fma(u, u, r2);
		}
		const T f = (a.kappa * pc_phi(a.kind, r2) - s) / pc_sqrt(dp);
		a.Ft[(int64_t)j * a.ldf + i] = f;
		T dn = a.dres[i] - f * f;
		if (i == p) dn = (T)0;
		a.dres[i] = dn;
		bv = (double)dn;
		bi = (int)i;
	}
	pc_block_argmax(bv, bi, rv, ri);
	if (tid == 0) a.part[(int64_t)((j + 1) & 1) * a.nblk + blockIdx.x] = PcholPart{bv, bi, 0};
}

// rows [rank, m) of Ft <- 0, and dres <- 0 exactly on the pivots (a later step's entry at an earlier pivot is rounding noise, whose square the
// running update has subtracted from that pivot's zero)
template <typename T>
__global__ __launch_bounds__(PC_THREADS)
void pchol_tail_kernel(T* Ft, int64_t ldf, int n, int m, const int32_t* rank, const int32_t* piv, T* dres)
{
	const int r0 = *rank;
	if (blockIdx.x == 0 && blockIdx.y == 0)
		for (int j = threadIdx.x; j < r0; j += PC_THREADS) dres[piv[j]] = (T)0;
	const int64_t i = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x;
	if (i >= n) return;
	for (int r = r0 + (int)blockIdx.y; r < m; r += (int)gridDim.y) Ft[(int64_t)r * ldf + i] = (T)0;
}

template <typename T>
inline int64_t pchol_tiles(int64_t n) { return (n + 64 * PcVec<T>::V - 1) / (64 * PcVec<T>::V); }

template <typename T>
int pchol(int kind, const T* x, int64_t n, int64_t ldx, int d, const int32_t* cols, const T* inv_ls, double kappa, int64_t m, double tol,
          T* Ft, int64_t ldf, T* dres, int32_t* piv, int32_t* rank, void* work, hipStream_t st)
{
	const int64_t nblk = pchol_tiles<T>(n);
	const int vec_ok = ((uintptr_t)Ft % 16 == 0) && (ldf % PcVec<T>::V == 0);
	PcholArgs<T> a{x, ldx, (int)n, d, cols, inv_ls, (T)kappa, tol * kappa, kind, Ft, ldf, dres, piv, rank, (PcholPart*)work, (int)nblk, (int)m, vec_ok};
	hipLaunchKernelGGL(pchol_init_kernel<T>, dim3((unsigned)((n + PC_THREADS - 1) / PC_THREADS)), dim3(PC_THREADS), 0, st, a);
	for (int j = 0; j < (int)m; ++j)
		hipLaunchKernelGGL(pchol_step_kernel<T>, dim3((unsigned)nblk), dim3(PC_THREADS), 0, st, a, j);
	hipLaunchKernelGGL(pchol_tail_kernel<T>, dim3((unsigned)((n + PC_THREADS - 1) / PC_THREADS), (unsigned)(m < 64 ? m : 64)), dim3(PC_THREADS), 0, st,
	                   Ft, ldf, (int)n, (int)m, (const int32_t*)rank, (const int32_t*)piv, dres);
	return check_launch("pchol");
}

inline int64_t pchol_workspace_bytes(int dtype, int64_t n)
{
	const int64_t nblk = n <= 0 ? 1 : (dtype == STPY_F32 ? pchol_tiles<float>(n) : pchol_tiles<double>(n));
	return 2 * nblk * (int64_t)sizeof(PcholPart);          // the double-buffered per-tile argmaxes
}

}  // namespace

}  // namespace stpy

// ---- C ABI (include/stpy_hip.h); every refusal below comes before the first HIP call
using namespace stpy;

extern "C" {

int64_t stpy_pchol_workspace_bytes(int dtype, int64_t n, int d, int64_t m)
{
	(void)d; (void)m;
	return pchol_workspace_bytes(dtype, n);
}

int stpy_pchol(int kind, int dtype, const void* x, int64_t n, int64_t ldx, int d, const int32_t* cols, const void* inv_ls,
               double kappa, int64_t m, double tol, void* Ft, int64_t ldf, void* dres, int32_t* piv, int32_t* rank_dev,
               void* work, int64_t work_bytes, void* stream)
{
	if (kind < STPY_K_SE || kind > STPY_K_MATERN52) { set_error("stpy_pchol: kernel kind %d is not stationary (SE, MATERN12/32/52)", kind); return -1; }
	if (dtype != STPY_F64 && dtype != STPY_F32) { set_error("stpy_pchol: unknown dtype %d (0 = float64, 1 = float32)", dtype); return -2; }
	if (n < 0 || n >= ((int64_t)1 << 31)) { set_error("stpy_pchol: n=%lld outside [0, 2^31)", (long long)n); return -4; }
	if (n == 0) return 0;          // empty problem: nothing to write
	if (d < 1) { set_error("stpy_pchol: d=%d", d); return -6; }
	if (ldx < d) { set_error("stpy_pchol: ldx=%lld below d=%d", (long long)ldx, d); return -5; }
	if (m < 1 || m > n || m > PC_MAX_M) { set_error("stpy_pchol: m=%lld outside [1, min(n=%lld, %d)]", (long long)m, (long long)n, PC_MAX_M); return -10; }
	if (!(tol >= 0.0) || !is_finite(tol)) { set_error("stpy_pchol: tol=%g must be finite and not negative", tol); return -11; }
	if (ldf < n) { set_error("stpy_pchol: ldf=%lld below n=%lld", (long long)ldf, (long long)n); return -13; }
	if (!x || !inv_ls || !Ft || !dres || !piv || !rank_dev || !work) { set_error("stpy_pchol: null pointer"); return -3; }
	const int64_t need = pchol_workspace_bytes(dtype, n);
	if (work_bytes < need) {
		set_error("stpy_pchol: workspace of %lld bytes, %lld needed (see the *_workspace_bytes query for these arguments)", (long long)work_bytes, (long long)need);
		return -20;
	}
	if ((uintptr_t)work & 7) { set_error("stpy_pchol: work must be 8-byte aligned"); return -17; }
	hipStream_t st = (hipStream_t)stream;
	if (dtype == STPY_F64)
		return pchol<double>(kind, (const double*)x, n, ldx, d, cols, (const double*)inv_ls, kappa, m, tol, (double*)Ft, ldf, (double*)dres, piv, rank_dev, work, st);
	return pchol<float>(kind, (const float*)x, n, ldx, d, cols, (const float*)inv_ls, kappa, m, tol, (float*)Ft, ldf, (float*)dres, piv, rank_dev, work, st);
}

}  // extern "C"

