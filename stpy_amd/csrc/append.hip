// append.hip -- the bordered Cholesky factor: extend a resident tile-padded factor of order n0 by k new rows
// (stpy_potrf_append, the incremental update behind GaussianProcess.add_data_point(iterative=True)).
//
//   [K11 K21^T]   [L11  0 ] [L11^T L21^T]        L21 = K21 L11^-T          (forward solve with k right-hand sides)
//   [K21 K22  ] = [L21 L22] [  0   L22^T]   =>   S   = K22 + s^2 I - L21 L21^T,  L22 = chol(S)
//                                                z2  = L22^-1 (y2 - L21 z1)
// The solve streams L11 from HBM once per dataflow launch (8 right-hand sides in fp64, 16 in fp32), or runs the MFMA block solve for
// many), the rest is O(k^2 n0 + k^3).  Rows [0, n0) of the factor and the inverse diagonal blocks below the first touched tile are
// never written: the append leaves exactly the layout stpy_potrf leaves for the bordered matrix, so every consumer runs on it.
#include <atomic>

#include "common.h"

namespace stpy {

int g_append_mfma_above = 32;        // stpy_tune key 34: more right-hand sides than this take the MFMA block solve (0 = always)

// ------------------------------------------------------------------------------------------
// X <- B L11^-T for the k x n0 block X = A[n0:n1, 0:n0] (in place; rows = right-hand sides), KC of them per launch.
// The forward vector solve of solve.hip (trsv_flow_kernel) with KC right-hand sides: workgroup k (its START ticket) owns block
// row i = k of L11, streams L_ij for j < i once (one or two register images ahead), multiplies each with the published 128 x KC
// block X_j^T as soon as it is there, and publishes X_i^T = inverse(L_ii) (B_i^T - sum_j L_ij X_j^T) in place over B_i^T.
// The last block may be ragged (n0 % 128): its rows / columns at or beyond n0 are neither read nor written, and the identity-bordered
// inverse diagonal block of the old tail tile serves it (its columns beyond n0 meet zeros).
// Hand-off exactly as trsv_flow_kernel: sc1 stores of the block, every storing wave drains, barrier, one lane publishes the counter
// with an sc1 store; the consumer polls the counter from one lane (bounded), barrier, sc1 loads.  A wait that gives up sets the
// sticky error word (stpy_async_status) and poisons this block (and so every later one) with NaN.
// ------------------------------------------------------------------------------------------
template <typename T, int KC, bool TWO>
__global__ __launch_bounds__(256, 1)
void append_flow_kernel(const T* __restrict__ L, int64_t ldl, const T* __restrict__ W, T* X, int64_t ldx, int n0, int kc, int nblk, TrsvSync* sy)
{
	__shared__ int s_k, s_ready, s_failed;
	__shared__ T tsh[IB][KC + 1];          // published X_j^T (column c of block j, right-hand side r), then y_i
	const int tid = threadIdx.x;
	if (tid == 0) { s_k = (int)atomicAdd(&sy->ticket, 1u); s_failed = 0; }
	__syncthreads();
	const int k = s_k;
	if (k >= nblk) return;
	const int i = k;
	const int rows_i = min(IB, n0 - i * IB);          // rows (and columns) of block i inside L11
	const int c8 = tid & 15, rr = tid >> 4;
	auto load_block = [&](T (&v)[8][8], const T* base) {
#pragma unroll
		for (int ps = 0; ps < 8; ++ps) {
			const bool live = ps * 16 + rr < rows_i;
			const T* p = base + (int64_t)(live ? ps * 16 + rr : 0) * ldl + c8 * 8;
#pragma unroll
			for (int e = 0; e < 8; ++e) v[ps][e] = live ? p[e] : T(0);
		}
	};
	auto wait_for = [&](int j) {
		if (tid == 0) {
			unsigned c = load_sc1(&sy->count);
			for (int spin = 0; (int)c <= j && spin < 1000000; ++spin) {
				const int dist = k - (int)c;
				if (dist > 8) __builtin_amdgcn_s_sleep(127); else if (dist > 2) __builtin_amdgcn_s_sleep(32); else __builtin_amdgcn_s_sleep(2);
				c = load_sc1(&sy->count);
			}
			if ((int)c <= j) { atomicExch(&sy->error, 1u); s_failed = 1; c = (unsigned)nblk; }
			s_ready = (int)c;
		}
		__syncthreads();
		const int r = s_ready;
		__syncthreads();
		return r;
	};
	T acc[8][KC];          // acc[ps][r]: partial dot of row ps*16+rr (this thread's 8 columns) with right-hand side r
#pragma unroll
	for (int ps = 0; ps < 8; ++ps)
#pragma unroll
		for (int r = 0; r < KC; ++r) acc[ps][r] = T(0);
	int ready = 0;
	auto consume = [&](const T (&lv)[8][8], int q) {
		if (q >= ready) ready = wait_for(q);
		// X_q^T -> LDS (block q < i is whole: q*128 + 128 <= t0 <= n0)
		for (int idx = tid; idx < IB * KC; idx += 256) {
			const int r = idx / IB, c = idx - r * IB;
			tsh[c][r] = r < kc ? load_sc1(X + (int64_t)r * ldx + (int64_t)q * IB + c) : T(0);
		}
		__syncthreads();
#pragma unroll
		for (int e = 0; e < 8; ++e) {
			T tv[KC];
#pragma unroll
			for (int r = 0; r < KC; ++r) tv[r] = tsh[c8 * 8 + e][r];
#pragma unroll
			for (int ps = 0; ps < 8; ++ps)
#pragma unroll
				for (int r = 0; r < KC; ++r) acc[ps][r] += lv[ps][e] * tv[r];
		}
		__syncthreads();          // (tsh is refilled by the next block)
	};
	auto block_of = [&](int q) { return L + (int64_t)i * IB * ldl + (int64_t)q * IB; };
	const int nprev = k;
	if (TWO) {
		T lv0[8][8], lv1[8][8];
		if (nprev > 0) load_block(lv0, block_of(0));
		for (int q = 0; q < nprev; q += 2) {
			if (q + 1 < nprev) load_block(lv1, block_of(q + 1));
			consume(lv0, q);
			if (q + 1 < nprev) {
				if (q + 2 < nprev) load_block(lv0, block_of(q + 2));
				consume(lv1, q + 1);
			}
		}
	} else {
		T lv0[8][8];
		for (int q = 0; q < nprev; ++q) {
			load_block(lv0, block_of(q));
			consume(lv0, q);
		}
	}
	// ---- y_i = B_i^T - accumulated products (rows / columns at or beyond n0: zero), into tsh[row][r]
	for (int idx = tid; idx < IB * KC; idx += 256) {
		const int r = idx / IB, c = idx - r * IB;
		tsh[c][r] = (r < kc && c < rows_i) ? X[(int64_t)r * ldx + (int64_t)i * IB + c] : T(0);
	}
	__syncthreads();
#pragma unroll
	for (int ps = 0; ps < 8; ++ps)
#pragma unroll
		for (int r = 0; r < KC; ++r) {
			T sum = acc[ps][r];
			sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 2); sum += __shfl_xor(sum, 4); sum += __shfl_xor(sum, 8);
			acc[ps][r] = sum;
		}
	if (c8 == 0) {
#pragma unroll
		for (int ps = 0; ps < 8; ++ps) {
			const int row = ps * 16 + rr;
#pragma unroll
			for (int r = 0; r < KC; ++r) tsh[row][r] = row < rows_i ? tsh[row][r] - acc[ps][r] : T(0);
		}
	}
	__syncthreads();
	if (s_failed) {          // (uniform) a wait timed out -> poison this block
		for (int idx = tid; idx < IB * KC; idx += 256) tsh[idx / KC][idx % KC] = (T)__builtin_nan("");
		__syncthreads();
	}
	// ---- X_i^T = inverse(L_ii) y_i, published write-through
#pragma unroll
	for (int ps = 0; ps < 8; ++ps)
#pragma unroll
		for (int r = 0; r < KC; ++r) acc[ps][r] = T(0);
#pragma unroll
	for (int e = 0; e < 8; ++e) {
		T tv[KC];
#pragma unroll
		for (int r = 0; r < KC; ++r) tv[r] = tsh[c8 * 8 + e][r];
#pragma unroll
		for (int ps = 0; ps < 8; ++ps) {
			const T w = W[(int64_t)i * IB * IB + (ps * 16 + rr) * IB + c8 * 8 + e];
#pragma unroll
			for (int r = 0; r < KC; ++r) acc[ps][r] += w * tv[r];
		}
	}
#pragma unroll
	for (int ps = 0; ps < 8; ++ps) {
		const int row = ps * 16 + rr;
#pragma unroll
		for (int r = 0; r < KC; ++r) {
			T sum = acc[ps][r];
			sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 2); sum += __shfl_xor(sum, 4); sum += __shfl_xor(sum, 8);
			if (c8 == 0 && r < kc && row < rows_i) store_sc1(X + (int64_t)r * ldx + (int64_t)i * IB + row, sum);
		}
	}
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // every storing wave drains its write-through stores ...
	__syncthreads();                                           // ... before ONE lane publishes the counter
	if (tid == 0) store_sc1(&sy->count, (unsigned)(k + 1));
}

// rhs[r] = y[r] - <X_r, z1> (r < k; X: k x n0 with leading dimension ldx): one workgroup per row, fixed-order sums
template <typename T>
__global__ __launch_bounds__(256)
void append_rhs_kernel(const T* __restrict__ X, int64_t ldx, int64_t n0, const T* __restrict__ z1, const T* __restrict__ y, T* __restrict__ rhs)
{
	__shared__ T red[256];
	const int tid = threadIdx.x, r = blockIdx.x;
	T s = T(0);
	for (int64_t c = tid; c < n0; c += 256) s += X[(int64_t)r * ldx + c] * z1[c];
	red[tid] = s;
	__syncthreads();
	for (int w = 128; w > 0; w >>= 1) {
		if (tid < w) red[tid] += red[tid + w];
		__syncthreads();
	}
	if (tid == 0) rhs[r] = y[r] - red[0];
}

// ------------------------------------------------------------------------------------------
// S = L22 L22^T in place for k <= 128 (one workgroup, S in LDS: right-looking, column by column), then z2 = L22^-1 rhs.
// S: A[n0:n1, n0:n1] (lower triangle read).  Writes the lower triangle back and zeros columns (r, n1p) of every new row r.
// The first non-positive pivot j sets *info = n0 + j + 1 (global, 1-based) and ends the factorisation.
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256)
void append_potf2_kernel(T* __restrict__ S, int64_t lds, int k, const T* __restrict__ rhs, T* __restrict__ z2, int64_t n0, int32_t* info)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
	T* s = (T*)smem_raw;                         // k x k, leading dimension IB + 1
	constexpr int LD = IB + 1;
	__shared__ T zs[IB];
	__shared__ int s_bad;
	const int tid = threadIdx.x;
	for (int idx = tid; idx < k * k; idx += 256) {
		const int i = idx / k, j = idx - i * k;
		s[i * LD + j] = j <= i ? S[(int64_t)i * lds + j] : T(0);
	}
	if (tid < IB) zs[tid] = (rhs && tid < k) ? rhs[tid] : T(0);
	if (tid == 0) s_bad = 0;
	__syncthreads();
	for (int j = 0; j < k; ++j) {
		const T d = s[j * LD + j];
		if (!(d > T(0))) {          // (uniform: every thread reads the same LDS word)
			if (tid == 0) { s_bad = j + 1; atomicCAS(info, 0, (int32_t)(n0 + j + 1)); }
			break;
		}
		const T piv = sqrt(d);
		__syncthreads();          // everybody has read the diagonal
		if (tid == 0) s[j * LD + j] = piv;
		for (int i = j + 1 + tid; i < k; i += 256) s[i * LD + j] /= piv;
		__syncthreads();
		// trailing update s[i][l] -= s[i][j] s[l][j], j < l <= i < k
		const int m = k - j - 1;
		for (int idx = tid; idx < m * m; idx += 256) {
			const int ii = idx / m, ll = idx - ii * m;
			if (ll <= ii) s[(j + 1 + ii) * LD + j + 1 + ll] -= s[(j + 1 + ii) * LD + j] * s[(j + 1 + ll) * LD + j];
		}
		__syncthreads();
	}
	__syncthreads();
	// z2 = L22^-1 rhs (forward substitution in LDS; skipped after a failed pivot)
	if (rhs && s_bad == 0) {
		for (int j = 0; j < k; ++j) {
			if (tid == 0) zs[j] /= s[j * LD + j];
			__syncthreads();
			for (int i = j + 1 + tid; i < k; i += 256) zs[i] -= s[i * LD + j] * zs[j];
			__syncthreads();
		}
	}
	for (int idx = tid; idx < k * k; idx += 256) {
		const int i = idx / k, j = idx - i * k;
		if (j <= i) S[(int64_t)i * lds + j] = s[i * LD + j];
	}
	if (z2 && tid < k) z2[tid] = zs[tid];
}

// padded scratch copy of S (k > 128): P[i][j] = S[i][j] on and below the diagonal (i, j < k), zero above, identity border up to kp
template <typename T>
__global__ void append_pad_kernel(const T* __restrict__ S, int64_t lds, int64_t k, T* __restrict__ P, int64_t kp)
{
	const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= kp * kp) return;
	const int64_t i = idx / kp, j = idx - i * kp;
	P[idx] = (i < k && j < k) ? (j <= i ? S[i * lds + j] : T(0)) : (i == j ? T(1) : T(0));
}

// ... and back: the lower triangle of the factored scratch copy into S
template <typename T>
__global__ void append_unpad_kernel(const T* __restrict__ P, int64_t kp, int64_t k, T* __restrict__ S, int64_t lds)
{
	const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= k * k) return;
	const int64_t i = idx / k, j = idx - i * k;
	if (j <= i) S[i * lds + j] = P[i * kp + j];
}

// the scratch factorisation's status (pivot index inside S) as a global one; the first failure wins
__global__ void append_info_kernel(const int32_t* __restrict__ info_s, int64_t n0, int32_t* info)
{
	if (threadIdx.x == 0 && *info_s != 0) atomicCAS(info, 0, (int32_t)(n0 + *info_s));
}

// The layout stpy_potrf leaves around the new rows: zeros in columns (r, n1p) of every new row r in [n0, n1), identity rows
// [n1, n1p) (zero left of the diagonal).  One workgroup row per matrix row (blockIdx.y).
template <typename T>
__global__ void append_border_kernel(T* __restrict__ A, int64_t lda, int64_t n0, int64_t n1, int64_t n1p)
{
	const int64_t r = n0 + blockIdx.y;
	const int64_t c0 = r < n1 ? r + 1 : 0;
	for (int64_t c = c0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n1p; c += (int64_t)gridDim.x * blockDim.x)
		A[r * lda + c] = (c == r) ? T(1) : T(0);
}

// z[n0:n1) = z2 (or nothing), z[n1:n1p) = 0
template <typename T>
__global__ void append_z_kernel(T* __restrict__ z, const T* __restrict__ z2, int64_t n0, int64_t k, int64_t n1p)
{
	const int64_t i = n0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n1p) z[i] = (i - n0 < k) ? z2[i - n0] : T(0);
}

// ------------------------------------------------------------------------------------------
// inverse(L_cc) of the 128 x 128 diagonal tiles c >= t0 / 128 (one workgroup per tile; row-major, zero above the diagonal): the
// forward substitution L X = I row by row, thread j owns column j of X (in LDS), every thread walks the same row of L (uniform loads)
// in a fixed order.
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(IB)
void append_trtri_kernel(const T* __restrict__ A, int64_t lda, int64_t t0, T* __restrict__ winv)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
	T* xs = (T*)smem_raw;                        // xs[l * IB + j] = X[l][j]
	const int j = threadIdx.x;
	const int64_t c = t0 + (int64_t)blockIdx.x * IB;
	const T* Lc = A + c * lda + c;
	for (int i = 0; i < IB; ++i) {
		const T* li = Lc + (int64_t)i * lda;
		T s = (i == j) ? T(1) : T(0);
		for (int l = 0; l < i; ++l) s -= li[l] * xs[l * IB + j];
		xs[i * IB + j] = (i >= j) ? s / li[i] : T(0);
	}
	T* Wc = winv + (c / IB) * IB * IB;
	for (int i = 0; i < IB; ++i) Wc[i * IB + j] = xs[i * IB + j];
}

static inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

// workspace: the MFMA route's zero-padded copy of the right-hand sides (k x n0p), the right-hand side / solution of z2 (k), and for
// k > 128 the padded Schur block, its inverse diagonal blocks, its factorisation's workspace, two solve vectors and a status word
int64_t potrf_append_workspace_bytes(size_t esz, int64_t n0, int64_t k)
{
	const int64_t n0p = (n0 + IB - 1) / IB * IB, kp = (k + IB - 1) / IB * IB;
	int64_t b = align256(k * n0p * (int64_t)esz) + 2 * align256(kp * (int64_t)esz);
	if (k > IB)
		b += align256(kp * kp * (int64_t)esz) + align256(kp * IB * (int64_t)esz) + align256(potrf_workspace_bytes(kp, potrf_auto_nb(kp), (int)esz)) +
		     2 * align256(kp * (int64_t)esz) + 256;
	return b;
}

template <typename T>
int potrf_append(int64_t n0, int64_t k, T* A, int64_t lda, T* winv, T* z, const T* y, void* work, int32_t* info, hipStream_t st)
{
	const int64_t n1 = n0 + k, n0p = (n0 + IB - 1) / IB * IB, n1p = (n1 + IB - 1) / IB * IB, t0 = n0 / IB * IB, kp = (k + IB - 1) / IB * IB;
	char* wp = (char*)work;
	T* Bc = (T*)wp;                   wp += align256(k * n0p * (int64_t)sizeof(T));
	T* rhs = (T*)wp;                  wp += align256(kp * (int64_t)sizeof(T));
	T* z2 = (T*)wp;                   wp += align256(kp * (int64_t)sizeof(T));
	T* X = A + n0 * lda;              // the new rows: K21 on entry, L21 on exit
	T* S = X + n0;                    // their diagonal block: K22 + s^2 I on entry, L22 on exit
	if (hipMemsetAsync(info, 0, sizeof(int32_t), st) != hipSuccess) { set_error("potrf_append: hipMemsetAsync failed"); return -1004; }
	int rc;

	// ---- 1. L21 = K21 L11^-T
	LookAhead* la = nullptr;
	if ((rc = lookahead_acquire(st, &la))) return rc;
	const bool aligned = lda % (16 / (int64_t)sizeof(T)) == 0 && (((uintptr_t)A | (uintptr_t)winv) & 15) == 0;
	const bool flow = g_trsv_flow && la->trsv_sync && n0 <= INT32_MAX && !(aligned && k > g_append_mfma_above);
	if (flow) {
		const int nblk = (int)(n0p / IB);
		constexpr int PAD_LDS = 84 * 1024;          // one workgroup per CU, as the vector solve (solve.hip: trsv)
		// right-hand sides per launch: 4 / 8 keep two register images of L ahead; fp32 also takes 16 (one image ahead) -- fp64 at 16
		// would not fit its 8 x 16 accumulators and an image of L into 256 VGPRs without scratch
		constexpr int WIDE = sizeof(T) == 8 ? 8 : 16;
		static std::atomic<bool> attr_set[2];
		const int which = sizeof(T) == 8 ? 0 : 1;
		if (!attr_set[which].load(std::memory_order_acquire)) {
			hipError_t e = hipFuncSetAttribute((const void*)append_flow_kernel<T, 4, true>, hipFuncAttributeMaxDynamicSharedMemorySize, PAD_LDS);
			if (e == hipSuccess) e = hipFuncSetAttribute((const void*)append_flow_kernel<T, 8, true>, hipFuncAttributeMaxDynamicSharedMemorySize, PAD_LDS);
			if (e == hipSuccess && WIDE > 8) e = hipFuncSetAttribute((const void*)append_flow_kernel<T, WIDE, false>, hipFuncAttributeMaxDynamicSharedMemorySize, PAD_LDS);
			if (e != hipSuccess) { set_error("potrf_append: hipFuncSetAttribute failed: %s", hipGetErrorString(e)); return -1000 - (int)e; }
			attr_set[which].store(true, std::memory_order_release);
		}
		for (int64_t c0 = 0; c0 < k; ) {
			const int kc = (int)(k - c0 < WIDE ? k - c0 : WIDE);
			if (hipMemsetAsync(la->trsv_sync, 0, 2 * sizeof(unsigned), st) != hipSuccess) { set_error("potrf_append: hipMemsetAsync failed"); return -1004; }
			T* Xc = X + c0 * lda;
			TrsvSync* sy = (TrsvSync*)la->trsv_sync;
			if (kc <= 4) hipLaunchKernelGGL((append_flow_kernel<T, 4, true>), dim3((unsigned)nblk), dim3(256), PAD_LDS, st, A, lda, winv, Xc, lda, (int)n0, kc, nblk, sy);
			else if (kc <= 8) hipLaunchKernelGGL((append_flow_kernel<T, 8, true>), dim3((unsigned)nblk), dim3(256), PAD_LDS, st, A, lda, winv, Xc, lda, (int)n0, kc, nblk, sy);
			else hipLaunchKernelGGL((append_flow_kernel<T, WIDE, false>), dim3((unsigned)nblk), dim3(256), PAD_LDS, st, A, lda, winv, Xc, lda, (int)n0, kc, nblk, sy);
			if ((rc = check_launch("potrf_append (flow solve)"))) return rc;
			c0 += kc;
		}
	} else {
		// the MFMA block solve on a zero-padded copy of order n0p: rows [n0, n0p) of L11's tail tile now hold the new rows, which only
		// reach output columns >= n0 (column j of B L^-T depends on rows <= j of L), and those are dropped when the copy comes back
		if (hipMemset2DAsync(Bc, n0p * sizeof(T), 0, n0p * sizeof(T), k, st) != hipSuccess ||
		    hipMemcpy2DAsync(Bc, n0p * sizeof(T), X, lda * sizeof(T), n0 * sizeof(T), k, hipMemcpyDeviceToDevice, st) != hipSuccess) {
			set_error("potrf_append: copy of the right-hand sides failed"); return -1004;
		}
		if ((rc = trsm_right_lt<T>(k, n0p, A, lda, winv, Bc, n0p, 0, st))) return rc;
		if (hipMemcpy2DAsync(X, lda * sizeof(T), Bc, n0p * sizeof(T), n0 * sizeof(T), k, hipMemcpyDeviceToDevice, st) != hipSuccess) {
			set_error("potrf_append: copy of the solution failed"); return -1004;
		}
	}

	// ---- 2. rhs = y2 - L21 z1
	if (z) {
		hipLaunchKernelGGL((append_rhs_kernel<T>), dim3((unsigned)k), dim3(256), 0, st, (const T*)X, lda, n0, (const T*)z, y, rhs);
		if ((rc = check_launch("potrf_append (rhs)"))) return rc;
	}

	// ---- 3. S = K22 + s^2 I - L21 L21^T (lower tiles), L22 = chol(S), z2 = L22^-1 rhs
	if ((rc = gemm_nt<T>(k, k, n0, X, lda, X, lda, S, lda, (T*)nullptr, 0, 1, 1, st))) return rc;
	if (k <= IB) {
		const int lds_bytes = (int)(k * (IB + 1) * sizeof(T));
		static std::atomic<bool> attr_p[2];
		const int which = sizeof(T) == 8 ? 0 : 1;
		if (!attr_p[which].load(std::memory_order_acquire)) {
			hipError_t e = hipFuncSetAttribute((const void*)append_potf2_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(IB * (IB + 1) * sizeof(T)));
			if (e != hipSuccess) { set_error("potrf_append: hipFuncSetAttribute failed: %s", hipGetErrorString(e)); return -1000 - (int)e; }
			attr_p[which].store(true, std::memory_order_release);
		}
		hipLaunchKernelGGL((append_potf2_kernel<T>), dim3(1), dim3(256), lds_bytes, st, S, lda, (int)k, z ? (const T*)rhs : (const T*)nullptr, z ? z2 : (T*)nullptr, n0, info);
		if ((rc = check_launch("potrf_append (potf2)"))) return rc;
	} else {
		T* P = (T*)wp;                    wp += align256(kp * kp * (int64_t)sizeof(T));
		T* winv_s = (T*)wp;               wp += align256(kp * IB * (int64_t)sizeof(T));
		T* pwork = (T*)wp;                wp += align256(potrf_workspace_bytes(kp, potrf_auto_nb(kp), (int)sizeof(T)));
		T* rpad = (T*)wp;                 wp += align256(kp * (int64_t)sizeof(T));
		T* zpad = (T*)wp;                 wp += align256(kp * (int64_t)sizeof(T));
		int32_t* info_s = (int32_t*)wp;
		hipLaunchKernelGGL((append_pad_kernel<T>), dim3((unsigned)((kp * kp + 255) / 256)), dim3(256), 0, st, (const T*)S, lda, k, P, kp);
		if ((rc = check_launch("potrf_append (pad)"))) return rc;
		if ((rc = potrf<T>(kp, P, kp, winv_s, pwork, 0, info_s, st))) return rc;
		hipLaunchKernelGGL(append_info_kernel, dim3(1), dim3(64), 0, st, (const int32_t*)info_s, n0, info);
		hipLaunchKernelGGL((append_unpad_kernel<T>), dim3((unsigned)((k * k + 255) / 256)), dim3(256), 0, st, (const T*)P, kp, k, S, lda);
		if ((rc = check_launch("potrf_append (unpad)"))) return rc;
		if (z) {
			if (hipMemsetAsync(rpad, 0, kp * sizeof(T), st) != hipSuccess ||
			    hipMemcpyAsync(rpad, rhs, k * sizeof(T), hipMemcpyDeviceToDevice, st) != hipSuccess) { set_error("potrf_append: copy failed"); return -1004; }
			if ((rc = trsv<T>(kp, P, kp, winv_s, rpad, zpad, 0, st))) return rc;
			if (hipMemcpyAsync(z2, zpad, k * sizeof(T), hipMemcpyDeviceToDevice, st) != hipSuccess) { set_error("potrf_append: copy failed"); return -1004; }
		}
	}

	// ---- 4. the layout around the new rows, the refreshed inverse diagonal tiles, z
	{
		const unsigned gx = (unsigned)((n1p + 255) / 256 < 64 ? (n1p + 255) / 256 : 64);
		hipLaunchKernelGGL((append_border_kernel<T>), dim3(gx, (unsigned)(n1p - n0)), dim3(256), 0, st, A, lda, n0, n1, n1p);
		if ((rc = check_launch("potrf_append (border)"))) return rc;
	}
	{
		static std::atomic<bool> attr_t[2];
		const int which = sizeof(T) == 8 ? 0 : 1;
		const int lds_bytes = (int)(IB * IB * sizeof(T));
		if (!attr_t[which].load(std::memory_order_acquire)) {
			hipError_t e = hipFuncSetAttribute((const void*)append_trtri_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
			if (e != hipSuccess) { set_error("potrf_append: hipFuncSetAttribute failed: %s", hipGetErrorString(e)); return -1000 - (int)e; }
			attr_t[which].store(true, std::memory_order_release);
		}
		hipLaunchKernelGGL((append_trtri_kernel<T>), dim3((unsigned)((n1p - t0) / IB)), dim3(IB), lds_bytes, st, (const T*)A, lda, t0, winv);
		if ((rc = check_launch("potrf_append (trtri)"))) return rc;
	}
	if (z) {
		hipLaunchKernelGGL((append_z_kernel<T>), dim3((unsigned)((n1p - n0 + 255) / 256)), dim3(256), 0, st, z, (const T*)z2, n0, k, n1p);
		if ((rc = check_launch("potrf_append (z)"))) return rc;
	}
	return 0;
}

template int potrf_append<double>(int64_t, int64_t, double*, int64_t, double*, double*, const double*, void*, int32_t*, hipStream_t);
template int potrf_append<float>(int64_t, int64_t, float*, int64_t, float*, float*, const float*, void*, int32_t*, hipStream_t);

}  // namespace stpy
