// rffgrad.hip -- input gradients of a Fourier-feature expansion (stpy_rff_grad): for n points x_t and m features
//   phi_tj = a_j cos(<W_j, x_t> + b_j)      (no bias: cos for j < m/2, sin for j >= m/2; a_j = scale * feat_scale[j])
// the value, gradient and (order 2) Hessian in x_t of sum_j C_tj phi_tj, with per-point coefficients C (n x m) or one shared row:
//   val[t] = sum_j C_tj phi_tj,   G[t][k] = sum_j C_tj phi'_tj W_jk,   H[t][k][l] = -sum_j C_tj phi_tj W_jk W_jl.
// In matrix words G = (C o Phi') W: two contractions with a pointwise step between them, and neither Phi, Phi' nor the (d, m, n)
// Jacobian of the embedding reaches memory.
//
// Tiling (value and gradient).  A WAVE owns 16 points and walks a chunk of the feature range in tiles of 16 features.  Per tile
//   1. Q^T (16 features x 16 points) = W_tile x_tile^T on the 16x16x4 MFMA (K = d; the wave's x fragments stay in registers
//      for d <= 64, further coordinates are re-read through L1);
//   2. the MFMA result layout hands lane (r, g) four features of point r: trig, amplitude and coefficient are applied in place
//      (fp64: libm sincos as rff_trig_f64_kernel; fp32: the hardware sin / cos on the phase in revolutions, as the embed's GEMM
//      epilogue), the value is summed on the VALU;
//   3. those four registers ARE the A fragments (16 points x 4 features each) of the second contraction G_tile += P' W_tile
//      (K = the tile, N = d in blocks of 16 coordinates): the same feature permutation is applied to the W rows of the B operand,
//      which a contraction does not notice.  The result never passes through LDS between the two contractions.
// The accumulators are ND x 4 registers (ND = blocks of 16 coordinates, at most 4).  Two kernels share this scheme:
//   rff_grad_lds_kernel (d <= 64, the shapes that matter): the four waves of a workgroup take neighbouring point tiles of ONE
//      chunk and share its W rows through LDS (see there);
//   rff_grad_kernel (d > 64): every wave on its own, W fragments straight from L1 / L2, and a grid dimension over blocks of 64
//      output coordinates, each of which recomputes the phases (as gram_grad_kernel does for its output blocks).
// Few points against many features: the feature range is cut into chunks so that the chip is filled; every (chunk, point)
// partial sum lands in the workspace and a second kernel adds them in chunk order (no atomics: bit-identical from run to run)
// and applies SET / ADD.  The Hessian (order 2) is a per-point weighted Gram matrix, not a contraction shared between points;
// it is summed by a plain VALU kernel over the same chunks (small problems by contract: one d x d block per point).
#include "common.h"

namespace stpy {

constexpr int RG_WAVES = 4;                     // waves per workgroup: four neighbouring point tiles of one chunk
constexpr int RG_SF = 32;                       // features per LDS slab (d <= 64)
constexpr int RG_CB = 64;                       // output coordinates per pass (4 MFMA column blocks)
constexpr int RG_XREG = 16;                     // K steps of the phase contraction whose x fragments stay in registers (d <= 64)
constexpr int64_t RG_TARGET_WGS = 2048;         // workgroups wanted: eight per CU
constexpr int RG_MIN_CHUNK = 64;                // features per chunk at least (amortises the x fragments and the partial-sum traffic)

template <typename T>
struct RffGradArgs {
	const T* x; const T* W; const T* bias; const T* fscale; const T* C;
	T* part;                          // [nsplit][n][Q] partial sums: value, d gradient entries, (d * d Hessian entries)
	int64_t ldx, ldw, ldc;
	int64_t n, m, chunk, ntiles;
	int d, Q, nsplit, half, cvec;     // cvec: rows of C may be read as aligned 4-element vectors
	T scale;
};

static void rffgrad_plan(int64_t n, int64_t m, int d, int64_t* ntiles, int* ncb, int64_t* chunk, int* nsplit)
{
	*ntiles = (n + 15) / 16;
	*ncb = (d + RG_CB - 1) / RG_CB;
	const int64_t base = (*ntiles + RG_WAVES - 1) / RG_WAVES * *ncb;
	int64_t want = (RG_TARGET_WGS + base - 1) / base;
	const int64_t maxs = (m + RG_MIN_CHUNK - 1) / RG_MIN_CHUNK;
	if (want > maxs) want = maxs;
	if (want < 1) want = 1;
	int64_t c = (m + want - 1) / want;
	c = (c + RG_SF - 1) / RG_SF * RG_SF;
	*chunk = c;
	*nsplit = (int)((m + c - 1) / c);
}

// sin and cos of the phase: fp64 libm; fp32 the embed epilogue's reduction to revolutions and the hardware functions
__device__ __forceinline__ void rg_sincos(double q, double& s, double& c) { sincos(q, &s, &c); }
__device__ __forceinline__ void rg_sincos(float q, float& s, float& c)
{
	float t = q * 0.15915494309189535f;
	t -= rintf(t);
	s = __builtin_amdgcn_sinf(t);
	c = __builtin_amdgcn_cosf(t);
}

// d <= 64 (DP = 16 ND padded coordinates): a workgroup owns four point tiles (one per wave) and one chunk.  The chunk's W rows
// pass through LDS in slabs of RG_SF features -- read from memory once per workgroup, coalesced, the next slab's loads in flight
// while the current one is computed -- as rows of DP + 4 elements: DP zero-padded coordinates (no guards in the MFMA loops), then
// the feature's amplitude (0 past the chunk: such features drop out) and its bias.  The row stride keeps both fragment reads
// at the minimum number of LDS passes (fp64: 16 rows x 4 k and 4 rows x 16 coordinates both map onto all 32 double slots twice).
// Feature order inside a 16-tile: the phase MFMA reads W row perm(r) for its operand row r, so that lane (r16, kq) receives
// features 4 kq .. 4 kq + 3 -- contiguous in C (one aligned 4-element load per lane when the layout allows) and exactly the
// features of K step i = 0 .. 3, lane group kq, of the second contraction.
template <typename T, int ND>
__global__ __launch_bounds__(64 * RG_WAVES)
void rff_grad_lds_kernel(RffGradArgs<T> p)
{
	typedef Mfma<T> MM;
	typedef typename MM::v4 v4;
	constexpr int DP = 16 * ND, LDW = DP + 4, PER = RG_SF * DP / (64 * RG_WAVES);
	__shared__ __attribute__((aligned(16))) T ws[RG_SF * LDW];
	const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, kq = lane >> 4;
	const int64_t ntg = (p.ntiles + RG_WAVES - 1) / RG_WAVES;
	const int split = (int)(blockIdx.x / ntg);
	const int64_t t0 = ((blockIdx.x - (int64_t)split * ntg) * RG_WAVES + (tid >> 6)) * 16;      // (tiles past the last recompute the last point)
	const int d = p.d;
	const int64_t jbeg = (int64_t)split * p.chunk, jend = min(p.m, jbeg + p.chunk);
	const int64_t pt = min(t0 + r16, p.n - 1);
	const T* xrow = p.x + pt * p.ldx;
	const T* crow_ptr = p.C + pt * p.ldc;
	const int arow = sizeof(T) == 8 ? 4 * (r16 & 3) + (r16 >> 2) : r16;      // perm(crow(lane, i)) = 4 kq + i for both result layouts

	T xf[4 * ND];
#pragma unroll
	for (int s = 0; s < 4 * ND; ++s) { const int k = 4 * s + kq; xf[s] = k < d ? xrow[k] : T(0); }
	v4 acc[ND];
#pragma unroll
	for (int c = 0; c < ND; ++c) acc[c] = v4{T(0), T(0), T(0), T(0)};
	T vacc = T(0);

	T pre[PER], pa = T(0), pb = T(0);
	auto load_slab = [&](int64_t j0) {
#pragma unroll
		for (int it = 0; it < PER; ++it) {
			const int idx = tid + it * 64 * RG_WAVES, r = idx / DP, c = idx % DP;
			const int64_t j = j0 + r;
			pre[it] = (j < jend && c < d) ? p.W[j * p.ldw + c] : T(0);
		}
		if (tid < RG_SF) {
			const int64_t j = j0 + tid;
			pa = j < jend ? p.scale * (p.fscale ? p.fscale[j] : T(1)) : T(0);
			pb = (p.bias && j < jend) ? p.bias[j] : T(0);
		}
	};
	load_slab(jbeg);
	for (int64_t j0 = jbeg; j0 < jend; j0 += RG_SF) {
#pragma unroll
		for (int it = 0; it < PER; ++it) {
			const int idx = tid + it * 64 * RG_WAVES;
			ws[(idx / DP) * LDW + idx % DP] = pre[it];
		}
		if (tid < RG_SF) { ws[tid * LDW + DP] = pa; ws[tid * LDW + DP + 1] = pb; }
		__syncthreads();
		if (j0 + RG_SF < jend) load_slab(j0 + RG_SF);
#pragma unroll 1
		for (int ft = 0; ft < RG_SF / 16; ++ft) {
			if (j0 + 16 * ft >= jend) break;
			const T* const base = ws + ft * 16 * LDW;
			// ---- phases of 16 features x 16 points
			v4 q = v4{T(0), T(0), T(0), T(0)};
#pragma unroll
			for (int s = 0; s < 4 * ND; ++s) q = MM::mma(base[arow * LDW + 4 * s + kq], xf[s], q);
			// ---- coefficients of features jb .. jb + 3 of point r16
			const int64_t jb = j0 + 16 * ft + 4 * kq;
			T cv[4];
			if (p.cvec && jb + 3 < p.m) {
				const v4 c4 = *(const v4*)(crow_ptr + jb);
#pragma unroll
				for (int i = 0; i < 4; ++i) cv[i] = c4[i];
			} else {
#pragma unroll
				for (int i = 0; i < 4; ++i) cv[i] = crow_ptr[min(jb + i, p.m - 1)];
			}
			T pd[4];
#pragma unroll
			for (int i = 0; i < 4; ++i) {
				const T* const wr = base + (4 * kq + i) * LDW;
				const T ca = cv[i] * wr[DP];
				T sn, cs;
				rg_sincos(q[i] + wr[DP + 1], sn, cs);
				const bool use_cos = p.bias != nullptr || jb + i < p.half;
				vacc += ca * (use_cos ? cs : sn);
				pd[i] = ca * (use_cos ? -sn : cs);
			}
			// ---- G_tile += P' W_slab: register i = K step i of the 16-feature tile
#pragma unroll
			for (int c = 0; c < ND; ++c)
#pragma unroll
				for (int i = 0; i < 4; ++i) acc[c] = MM::mma(pd[i], base[(4 * kq + i) * LDW + 16 * c + r16], acc[c]);
		}
		__syncthreads();
	}

	T* const part = p.part + (int64_t)split * p.n * p.Q;
#pragma unroll
	for (int c = 0; c < ND; ++c) {
		const int k = 16 * c + r16;
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			const int64_t t = t0 + MM::crow(lane, i);
			if (k < d && t < p.n) part[t * p.Q + 1 + k] = acc[c][i];
		}
	}
	vacc += __shfl_xor(vacc, 16);
	vacc += __shfl_xor(vacc, 32);
	if (kq == 0 && t0 + r16 < p.n) part[(t0 + r16) * p.Q] = vacc;
}

// d > 64: every wave on its own, W fragments straight from L1 / L2, one pass per block of 64 output coordinates (blockIdx.y).
template <typename T, int ND>
__global__ __launch_bounds__(64 * RG_WAVES)
void rff_grad_kernel(RffGradArgs<T> p)
{
	typedef Mfma<T> MM;
	typedef typename MM::v4 v4;
	const int lane = threadIdx.x & 63, r16 = lane & 15, kq = lane >> 4;
	const int64_t unit = (int64_t)blockIdx.x * RG_WAVES + (threadIdx.x >> 6);         // waves of a workgroup: neighbouring point tiles of one chunk
	if (unit >= p.ntiles * p.nsplit) return;
	const int split = (int)(unit / p.ntiles);
	const int64_t t0 = (unit - (int64_t)split * p.ntiles) * 16;
	const int c0 = (int)blockIdx.y * RG_CB;                                           // first output coordinate of this pass
	const int d = p.d;
	const int64_t jbeg = (int64_t)split * p.chunk, jend = min(p.m, jbeg + p.chunk);
	const int64_t pt = min(t0 + r16, p.n - 1);                                        // points past n recompute the last one and are never stored
	const T* xrow = p.x + pt * p.ldx;
	const T* crow_ptr = p.C + pt * p.ldc;                                             // ldc == 0: the shared row

	T xf[RG_XREG];
#pragma unroll
	for (int s = 0; s < RG_XREG; ++s) { const int k = 4 * s + kq; xf[s] = k < d ? xrow[k] : T(0); }

	v4 acc[ND];
#pragma unroll
	for (int c = 0; c < ND; ++c) acc[c] = v4{T(0), T(0), T(0), T(0)};
	T vacc = T(0);

	for (int64_t j0 = jbeg; j0 < jend; j0 += 16) {
		// ---- phases of 16 features x 16 points
		const T* wa = p.W + min(j0 + r16, p.m - 1) * p.ldw;
		v4 q = v4{T(0), T(0), T(0), T(0)};
#pragma unroll
		for (int s = 0; s < RG_XREG; ++s) {
			if (4 * s < d) { const int k = 4 * s + kq; q = MM::mma(k < d ? wa[k] : T(0), xf[s], q); }
		}
		for (int s = RG_XREG; 4 * s < d; ++s) {
			const int k = 4 * s + kq;
			q = MM::mma(k < d ? wa[k] : T(0), k < d ? xrow[k] : T(0), q);
		}
		// ---- trig, amplitude, coefficient: lane (r16, kq) holds features j0 + crow(lane, i) of point r16
		T pd[4];
		const T* wb[4];
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			const int64_t j = j0 + MM::crow(lane, i);
			const bool valid = j < jend;
			const int64_t jc = min(j, p.m - 1);
			wb[i] = p.W + jc * p.ldw;
			const T a = p.scale * (p.fscale ? p.fscale[jc] : T(1));
			const T cv = valid ? crow_ptr[jc] * a : T(0);
			T sn, cs;
			rg_sincos(p.bias ? q[i] + p.bias[jc] : q[i], sn, cs);
			const bool use_cos = p.bias != nullptr || jc < p.half;
			vacc += cv * (use_cos ? cs : sn);
			pd[i] = cv * (use_cos ? -sn : cs);
		}
		// ---- G_tile += P' W_slab: register i = K step i of the 16-feature slab
#pragma unroll
		for (int c = 0; c < ND; ++c) {
			const int k = c0 + 16 * c + r16;
#pragma unroll
			for (int i = 0; i < 4; ++i) acc[c] = MM::mma(pd[i], k < d ? wb[i][k] : T(0), acc[c]);
		}
	}

	// ---- partial sums: acc[c][i] = G[point crow(lane, i)][coordinate c0 + 16 c + r16]; the value is summed over the four lane groups
	T* const part = p.part + (int64_t)split * p.n * p.Q;
#pragma unroll
	for (int c = 0; c < ND; ++c) {
		const int k = c0 + 16 * c + r16;
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			const int64_t t = t0 + MM::crow(lane, i);
			if (k < d && t < p.n) part[t * p.Q + 1 + k] = acc[c][i];
		}
	}
	vacc += __shfl_xor(vacc, 16);
	vacc += __shfl_xor(vacc, 32);
	if (blockIdx.y == 0 && kq == 0 && t0 + r16 < p.n) part[(t0 + r16) * p.Q] = vacc;
}

// Hessian partial sums of one point, one chunk and 256 (k, l) pairs: -sum_j C_tj phi_tj W_jk W_jl.  Slabs of 256 features: every
// thread forms one feature's weight u_j into LDS, then every thread sums its pair over the slab in feature order.
template <typename T>
__global__ __launch_bounds__(256)
void rff_hess_kernel(RffGradArgs<T> p, int npb)
{
	__shared__ T su[256];
	int64_t bid = blockIdx.x;
	const int pb = (int)(bid % npb); bid /= npb;
	const int split = (int)(bid % p.nsplit);
	const int64_t t = bid / p.nsplit;
	const int tid = threadIdx.x, d = p.d;
	const int64_t jbeg = (int64_t)split * p.chunk, jend = min(p.m, jbeg + p.chunk);
	const T* xrow = p.x + t * p.ldx;
	const T* crow_ptr = p.C + t * p.ldc;
	const int pair = pb * 256 + tid;
	const bool live = pair < d * d;
	const int k = live ? pair / d : 0, l = live ? pair - k * d : 0;
	T acc = T(0);
	for (int64_t j0 = jbeg; j0 < jend; j0 += 256) {
		const int64_t j = j0 + tid;
		T u = T(0);
		if (j < jend) {
			const T* w = p.W + j * p.ldw;
			T q = T(0);
			for (int kk = 0; kk < d; ++kk) q += w[kk] * xrow[kk];
			T sn, cs;
			rg_sincos(p.bias ? q + p.bias[j] : q, sn, cs);
			const bool use_cos = p.bias != nullptr || j < p.half;
			u = -crow_ptr[j] * p.scale * (p.fscale ? p.fscale[j] : T(1)) * (use_cos ? cs : sn);
		}
		__syncthreads();
		su[tid] = u;
		__syncthreads();
		if (live) {
			const int cnt = (int)min((int64_t)256, jend - j0);
			for (int jj = 0; jj < cnt; ++jj) {
				const T* w = p.W + (j0 + jj) * p.ldw;
				acc += su[jj] * w[k] * w[l];
			}
		}
	}
	if (live) p.part[((int64_t)split * p.n + t) * p.Q + 1 + d + pair] = acc;
}

// chunk partial sums in chunk order, SET / ADD into val, G and H
template <typename T>
__global__ __launch_bounds__(256)
void rff_grad_finish_kernel(const T* __restrict__ part, int nsplit, int64_t n, int Q, int d, int combine, T* val, T* G, int64_t ldg, T* H)
{
	const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (idx >= n * Q) return;
	const int64_t t = idx / Q;
	const int q = (int)(idx - t * Q);
	T* o;
	if (q == 0) {
		if (!val) return;
		o = val + t;
	} else if (q <= d) {
		o = G + t * ldg + (q - 1);
	} else {
		const int k = (q - 1 - d) / d, l = (q - 1 - d) - k * d;
		o = H + (t * ldg + k) * ldg + l;
	}
	T s = T(0);
	for (int sp = 0; sp < nsplit; ++sp) s += part[((int64_t)sp * n + t) * Q + q];
	*o = combine == STPY_OUT_ADD ? *o + s : s;
}

int64_t rff_grad_workspace_bytes(int64_t n, int d, int64_t m, int order, size_t esz)
{
	if (n <= 0 || m <= 0 || d <= 0) return 0;
	int64_t ntiles, chunk;
	int ncb, nsplit;
	rffgrad_plan(n, m, d, &ntiles, &ncb, &chunk, &nsplit);
	const int64_t Q = 1 + d + (order == 2 ? (int64_t)d * d : 0);
	return (int64_t)nsplit * n * Q * (int64_t)esz;
}

template <typename T>
int rff_grad(const T* x, int64_t n, int64_t ldx, int d, const T* W, int64_t ldw, int64_t m, const T* bias, const T* fscale, double scale,
             const T* C, int64_t ldc, int order, int combine, T* val, T* G, int64_t ldg, T* H, void* work, hipStream_t st)
{
	int64_t ntiles, chunk;
	int ncb, nsplit;
	rffgrad_plan(n, m, d, &ntiles, &ncb, &chunk, &nsplit);
	const int64_t Q64 = 1 + d + (order == 2 ? (int64_t)d * d : 0);
	if (Q64 > INT32_MAX) { set_error("stpy_rff_grad: d=%d too large for order %d", d, order); return -5; }
	RffGradArgs<T> p;
	p.x = x; p.W = W; p.bias = bias; p.fscale = fscale; p.C = C;
	p.part = (T*)work;
	p.ldx = ldx; p.ldw = ldw; p.ldc = ldc;
	p.n = n; p.m = m; p.chunk = chunk; p.ntiles = ntiles;
	p.d = d; p.Q = (int)Q64; p.nsplit = nsplit; p.half = (int)(m / 2);
	p.scale = (T)scale;
	p.cvec = (ldc % 4 == 0 && ((uintptr_t)C % (4 * sizeof(T))) == 0) ? 1 : 0;
	const int64_t wgs = d <= RG_CB ? (ntiles + RG_WAVES - 1) / RG_WAVES * nsplit : (ntiles * nsplit + RG_WAVES - 1) / RG_WAVES;
	if (wgs > INT32_MAX || ncb > 65535) { set_error("stpy_rff_grad: %lld x %d workgroups exceed one launch", (long long)wgs, ncb); return -3; }
	const dim3 grid((unsigned)wgs, (unsigned)ncb), block(64 * RG_WAVES);
	if (d <= 16) hipLaunchKernelGGL((rff_grad_lds_kernel<T, 1>), grid, block, 0, st, p);
	else if (d <= 32) hipLaunchKernelGGL((rff_grad_lds_kernel<T, 2>), grid, block, 0, st, p);
	else if (d <= 48) hipLaunchKernelGGL((rff_grad_lds_kernel<T, 3>), grid, block, 0, st, p);
	else if (d <= RG_CB) hipLaunchKernelGGL((rff_grad_lds_kernel<T, 4>), grid, block, 0, st, p);
	else hipLaunchKernelGGL((rff_grad_kernel<T, 4>), grid, block, 0, st, p);
	int rc = check_launch("stpy_rff_grad");
	if (rc) return rc;
	if (order == 2) {
		const int npb = (d * d + 255) / 256;
		const int64_t hw = n * nsplit * npb;
		if (hw > INT32_MAX) { set_error("stpy_rff_grad: %lld Hessian workgroups exceed one launch", (long long)hw); return -14; }
		hipLaunchKernelGGL((rff_hess_kernel<T>), dim3((unsigned)hw), dim3(256), 0, st, p, npb);
		rc = check_launch("stpy_rff_grad hessian");
		if (rc) return rc;
	}
	const int64_t total = n * Q64;
	if ((total + 255) / 256 > INT32_MAX) { set_error("stpy_rff_grad: output too large for one launch"); return -3; }
	hipLaunchKernelGGL((rff_grad_finish_kernel<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
	                   (const T*)work, nsplit, n, (int)Q64, d, combine, val, G, ldg, H);
	return check_launch("stpy_rff_grad finish");
}

}  // namespace stpy

using namespace stpy;

extern "C" {

int64_t stpy_rff_grad_workspace_bytes(int dtype, int64_t n, int d, int64_t m, int order)
{
	return rff_grad_workspace_bytes(n, d, m, order, dtype == STPY_F32 ? 4 : 8);
}

int stpy_rff_grad(int dtype, const void* x, int64_t n, int64_t ldx, int d,
                  const void* W, int64_t ldw, int64_t m, const void* bias, const void* feat_scale, double scale,
                  const void* C, int64_t ldc, int order, int combine, void* val, void* G, int64_t ldg, void* H,
                  void* work, int64_t work_bytes, void* stream)
{
	if (n <= 0 || m <= 0) return 0;          // empty problem: nothing is written (empty tensors have null data pointers)
	if (dtype != STPY_F64 && dtype != STPY_F32) { set_error("stpy_rff_grad: unknown dtype %d (0 = float64, 1 = float32)", dtype); return -1; }
	if (!x) { set_error("stpy_rff_grad: null pointer x"); return -2; }
	if (d <= 0) { set_error("stpy_rff_grad: d=%d must be positive", d); return -5; }
	if (ldx < d) { set_error("stpy_rff_grad: ldx=%lld below d=%d", (long long)ldx, d); return -4; }
	if (!W) { set_error("stpy_rff_grad: null pointer W"); return -6; }
	if (ldw < d) { set_error("stpy_rff_grad: ldw=%lld below d=%d", (long long)ldw, d); return -7; }
	if (m % 2 != 0 && !bias) { set_error("stpy_rff_grad: m=%lld must be even without a bias (cos | sin halves)", (long long)m); return -8; }
	if (m > INT32_MAX) { set_error("stpy_rff_grad: m exceeds int32"); return -8; }
	if (!C) { set_error("stpy_rff_grad: null pointer C (coefficients)"); return -12; }
	if (ldc != 0 && ldc < m) { set_error("stpy_rff_grad: ldc=%lld (0 = one shared row, else >= m=%lld)", (long long)ldc, (long long)m); return -13; }
	if (order != 1 && order != 2) { set_error("stpy_rff_grad: order %d (1 = value and gradient, 2 = also the Hessian)", order); return -14; }
	if (combine != STPY_OUT_SET && combine != STPY_OUT_ADD) { set_error("stpy_rff_grad: combine %d (SET or ADD)", combine); return -15; }
	if (!G) { set_error("stpy_rff_grad: null pointer G"); return -17; }
	if (ldg < d) { set_error("stpy_rff_grad: ldg=%lld below d=%d", (long long)ldg, d); return -18; }
	if (order == 2 && !H) { set_error("stpy_rff_grad: order 2 needs H"); return -19; }
	if (!work) { set_error("stpy_rff_grad: null workspace"); return -20; }
	const int64_t need = stpy_rff_grad_workspace_bytes(dtype, n, d, m, order);
	if (work_bytes < need) {
		set_error("stpy_rff_grad: workspace of %lld bytes, %lld needed (stpy_rff_grad_workspace_bytes)", (long long)work_bytes, (long long)need); return -21;
	}
	hipStream_t st = (hipStream_t)stream;
	if (dtype == STPY_F64)
		return rff_grad<double>((const double*)x, n, ldx, d, (const double*)W, ldw, m, (const double*)bias, (const double*)feat_scale, scale,
		                        (const double*)C, ldc, order, combine, (double*)val, (double*)G, ldg, (double*)H, work, st);
	return rff_grad<float>((const float*)x, n, ldx, d, (const float*)W, ldw, m, (const float*)bias, (const float*)feat_scale, scale,
	                       (const float*)C, ldc, order, combine, (float*)val, (float*)G, ldg, (float*)H, work, st);
}

}  // extern "C"
