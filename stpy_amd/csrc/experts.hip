// Local GP experts (stpy_experts_fit / _predict / _combine / _predict_grad / _combine_grad, and the routed prediction stpy_experts_centroids /
// _route / _predict_routed / _predict_routed_grad; LocalExpertsGaussianProcess): E exact GPs on E different blocks of the data under ONE
// hyper-parameter candidate, the mirror image of the batched evidence (reduce.hip: B candidates on the same data), from the same one-workgroup
// building blocks (lb_block.h).
//
// Layout.  The points are gathered by expert: xs (N x ldx), ys (N), offsets[E + 1]; expert e owns the rows offsets[e] .. offsets[e + 1], n_e of
// them, NP_e = n_e rounded up to 32.  With NPM = nmax rounded up to 32:
//   factor  E slices of NPM^2 doubles: V_e = L_e^-T, upper triangular, row-major with row stride NP_e, bordered by an identity, the blocks just
//           below its block diagonal stored as zero (what lies further below is never written and never read).  Kept by the caller from the
//           fit to the predictions.
//   work    fit: E slices of NPM^2 + 32 NPM doubles (A_e, then the inverse diagonal blocks); dead after the call.
//           predict: one slice of 32 NPM doubles per (expert, test tile): the k* tile, TRANSPOSED (32 test points x NP_e).
// The fit is lb_fit<GRAD, true> of lb_block.h, the body lml_batch_kernel calls too: here with the expert's rows in place of the candidate's
// hyper-parameters, V in the factor buffer instead of the workspace, alpha stored, and the K^-1 / H passes left out without a gradient.
//
// Prediction, per (expert, tile of 32 test points): k* from direct differences with the evaluator of the fit (lb_r2 + lb_phi: the same bits on a
// training point), mu = k*^T alpha by one wave per test point, v = L^-1 k* = V^T k* on the fp64 MFMA 64 rows at a time -- lb_panel's loop with
// the A tile fetched TRANSPOSED from V (V[k][i] is (L^-1)[i][k]; lanes run along i, so the global reads stay coalesced) -- and the column sums of
// v o v straight from the accumulators: v is never stored.  The tile is 32 because that is the width of the panel product (two 16-column MFMA
// halves share one A fragment); 64 columns would run the product twice over the same V for half as many k* slices, and the slice, 128 KB at
// n_e = 512, is what bounds how many test points one launch can take.
// With input gradients (stpy_experts_predict_grad / _combine_grad): the same grid and the same body for steps 1 - 3, v written out beside the sums,
// w = K^-1 k* = V v by lb_panel<0> as it stands (A = V upper triangular from its row 0), then d mu / dx and d var / dx from direct differences,
// one wave per test point; workspace two slices of 32 NPM doubles per (expert, tile).  The combination differentiates what it computes: the clamp
// (zero where active) and rBCM's variance-dependent weights.
// Routed prediction (further down): the same bodies on a work list of (expert, 32 pairs) tiles in place of the grid of (expert, tile) -- a tile is
// known to the bodies only through ExpertsTileDense / ExpertsTileRouted: which test point a column reads and where its results go.
// Every sum has a fixed order and no workgroup reads what another wrote: an expert's outputs are bit-identical wherever it sits in whatever batch.
// Compiled inside api.hip (which includes this file, as it includes pchol.hip and the kmv family; it also compiles on its own, as the resource
// test does) and NOT beside lml_batch_kernel in reduce.hip: more kernels in that translation unit change its LDS layout and with it its instructions.
// Barriers: every __syncthreads() is reached by the whole workgroup; the early exits, here and in lb_fit, test workgroup-uniform words.
#include "common.h"
#include "lb_block.h"

namespace stpy {

constexpr int EX_TILE = 32;          // test points per workgroup of the prediction

struct ExpertsFitArgs {
	const double* xs; int64_t N, ldx; int d; const int32_t* cols; const double* ys; const int32_t* offsets; int nmax;
	const double* inv_ls; const double* noise; double kappa, weight; const int32_t* pidx; int np;
	double* factor; int64_t fslice; double* alpha; double* value; double* grad; int64_t ldg; int32_t* info;
	double* work; int64_t wslice;          // doubles per expert
	int kind;
};

struct ExpertsPredictArgs {
	const double* xs; int64_t N, ldx; int d; const int32_t* cols; const int32_t* offsets; int nmax;
	const double* inv_ls; double kappa; const double* factor; int64_t fslice; const double* alpha; const int32_t* info;
	const double* xt; int64_t M, ldt; double* mu_e; double* var_e; int64_t ldm;
	double* work; int64_t wslice; int ntiles;
	int kind;
};

struct ExpertsPredictGradArgs {
	ExpertsPredictArgs p;          // wslice: TWO halves of 32 NPM doubles
	double* gmu_e; double* gvar_e; int64_t ldg, lde;          // (E, M, d): row stride ldg, expert stride lde
};

inline int64_t experts_npm(int64_t nmax) { return (nmax + 31) / 32 * 32; }
inline int64_t experts_factor_slice(int64_t nmax) { return experts_npm(nmax) * experts_npm(nmax); }
inline int64_t experts_fit_slice(int64_t nmax) { return experts_npm(nmax) * experts_npm(nmax) + 32 * experts_npm(nmax); }
inline int64_t experts_predict_slice(int64_t nmax) { return EX_TILE * experts_npm(nmax); }

// The shell of lb_fit<GRAD, true> (lb_block.h) for expert blockIdx.x: the offsets check, then the expert's rows, its slice of the workspace (A_e, then
// the inverse diagonal blocks) and of the factor buffer (V_e), its part of alpha.  Without a gradient the K^-1 / H passes are not compiled in.
// (__launch_bounds__(256) and not (256, 2): the kernel needs about 200 VGPRs either way, two workgroups per CU, but under the tighter bound the
// allocator parks one of the VGPRs that hold spilled SGPRs in scratch)
template <bool GRAD>
__global__ __launch_bounds__(256)
void experts_fit_kernel(ExpertsFitArgs p)
{
	const int b = blockIdx.x, tid = threadIdx.x;
	const int lo = p.offsets[b], hi = p.offsets[b + 1];
	if (lo < 0 || hi < lo || hi > p.N || hi - lo > p.nmax) {          // (the same words for every thread) nothing of this expert is sized for: report it
		const bool inside = lo >= 0 && hi >= lo && hi <= p.N;
		if (inside)
			for (int i = lo + tid; i < hi; i += 256) p.alpha[i] = 0.0;
		if (tid == 0) {
			if (GRAD)
				for (int k = 0; k <= p.np; ++k) p.grad[(int64_t)b * p.ldg + k] = 0.0;
			p.value[b] = __builtin_huge_val();
			p.info[b] = inside ? -1 : -2;
		}
		return;
	}
	const int n = hi - lo, NP = (n + 31) & ~31;
	double* A = p.work + (int64_t)b * p.wslice;
	lb_fit<GRAD, true>(LbFit{p.xs + (int64_t)lo * p.ldx, p.ldx, n, p.d, p.cols, p.ys + lo, p.inv_ls, p.noise[0], p.kappa, p.weight, p.pidx, p.np, p.kind,
	                   A, p.factor + (int64_t)b * p.fslice, A + (int64_t)NP * NP, p.alpha + lo, p.value + b,
	                   GRAD ? p.grad + (int64_t)b * p.ldg : nullptr, p.info + b});
}

// total[0] = sum_e value[e], total[1 + q] = sum_e grad[e*ldg + q] (q <= np; only with a gradient): one workgroup, thread q owns output q and adds
// in expert order
__global__ __launch_bounds__(64)
void experts_total_kernel(const double* value, const double* grad, int64_t ldg, int np, int64_t E, double* total)
{
	const int nout = grad ? np + 2 : 1;
	for (int q = threadIdx.x; q < nout; q += 64) {
		double s = 0.0;
		if (q == 0)
			for (int64_t e = 0; e < E; ++e) s += value[e];
		else
			for (int64_t e = 0; e < E; ++e) s += grad[e * ldg + q - 1];
		total[q] = s;
	}
}

// What column t of a tile stands for: the test point it reads (row(t), -1: an empty column) and where its results go (out(t) into mu / var,
// gout(t) into the gradient arrays).  The body below knows a tile only through one of these two.
//   ExpertsTileDense    the tile of the all-experts kernels: 32 consecutive test points from t0, mt of them in range; mu, var, gmu, gvar are the
//                       caller's pointers at (e, t0)
//   ExpertsTileRouted   a tile of the work list of the routed kernels: trow / oidx / gidx are 32-entry tables in LDS (experts_routed_tile fills
//                       them from wpair); mu, var, gmu, gvar are the caller's array bases
struct ExpertsTileDense {
	int64_t t0; int mt; int64_t ldg;
	__device__ __forceinline__ bool has(int t) const { return t < mt; }
	__device__ __forceinline__ int64_t row(int t) const { return t0 + t; }
	__device__ __forceinline__ int64_t out(int t) const { return t; }
	__device__ __forceinline__ int64_t gout(int t) const { return (int64_t)t * ldg; }
};

struct ExpertsTileRouted {
	const int64_t* trow; const int64_t* oidx; const int64_t* gidx;
	__device__ __forceinline__ bool has(int t) const { return trow[t] >= 0; }
	__device__ __forceinline__ int64_t row(int t) const { return trow[t]; }
	__device__ __forceinline__ int64_t out(int t) const { return oidx[t]; }
	__device__ __forceinline__ int64_t gout(int t) const { return gidx[t]; }
};

// Steps 1 - 3 of a prediction for one (expert, tile): the ONE body of experts_predict_kernel, experts_predict_grad_kernel and their routed twins,
// so that the four write the same bits to mu and var (every sum below runs over k for one fixed column: a column's results do not depend on
// which tile, or which column of it, it sits in).  x, al, V: the expert's rows, its alpha and its factor slice; n of them, NP = n rounded up to 32; KT: 32 x NP doubles
// of workspace.  With STORE_V the accumulators of step 3 are also written out, VT[t][k] = (L^-1 k*_t)_k for all 32 t and k < NP (zero for t >= mt and
// k >= n): what the variance gradient's second triangular product reads.  As, Bs, ssq: the caller's LDS.  Entered and left by the whole workgroup.
template <bool STORE_V, class Tile>
__device__ __forceinline__ void experts_predict_body(const ExpertsPredictArgs& p, const double* x, const double* al, const double* V, int n, int NP,
                                                     const Tile& tl, double* KT, double* VT, double* mu, double* var,
                                                     double* As, double* Bs, double (*ssq)[EX_TILE])
{
	typedef Mfma<double>::v4 v4;
	typedef Mfma<double>::v2 v2;
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	const int ld = NP;
	const double* il = p.inv_ls;

	// ---- 1. the k* tile
	for (int k = tid; k < NP; k += 256) {
		const double* xk = x + (int64_t)k * p.ldx;
		for (int t = 0; t < EX_TILE; ++t) {
			double v = 0.0;
			if (k < n && tl.has(t)) v = p.kappa * lb_phi(p.kind, lb_r2(xk, p.xt + tl.row(t) * p.ldt, p.cols, il, p.d));
			KT[(int64_t)t * ld + k] = v;
		}
	}
	__syncthreads();

	// ---- 2. mu_t = sum_k k*_kt alpha_k: one wave per test point, lanes strided over k, shuffle tree
	for (int t = w; t < EX_TILE; t += 4) {
		if (!tl.has(t)) continue;          // (wave-uniform)
		const double* kr = KT + (int64_t)t * ld;
		double s = 0.0;
		for (int k = lane; k < n; k += 64) s = fma(kr[k], al[k], s);
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
		if (lane == 0) mu[tl.out(t)] = s;
	}

	// ---- 3. v = L^-1 k* = V^T k*, 64 rows per round, and the column sums of v o v from the accumulators.  Row i of L^-1 ends at column i: the round
	// that starts at row r0 runs over k < r0 + 64 (the block of V below the diagonal block of the round's first 32 rows is stored as zero).
	const int ar = tid & 63, ak = (tid >> 6) * 8;         // A tile (64 rows x 32 k), fetched transposed: this thread's row and the first of its 8 k
	const int br = tid >> 3, bk = (tid & 7) * 4;          // B tile (32 test points x 32 k): row, first of 4 k
	const int fr = lane & 15, fk = lane >> 4;             // MFMA operand fragment
	double q0 = 0.0, q1 = 0.0;
	for (int r0 = 0; r0 < NP; r0 += 64) {
		const int kend = min(r0 + 64, NP);
		const bool arow = r0 + ar < NP;
		const double* ap = V + (int64_t)ak * ld + r0 + ar;
		const double* bp = KT + (int64_t)br * ld + bk;
		double ra[8];
		v2 rb[2];
		auto fetch = [&](int kc) {
#pragma unroll
			for (int c = 0; c < 8; ++c) ra[c] = arow ? ap[(int64_t)(kc + c) * ld] : 0.0;
#pragma unroll
			for (int c = 0; c < 2; ++c) rb[c] = *reinterpret_cast<const v2*>(bp + kc + 2 * c);
		};
		v4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
		fetch(0);
		for (int kc = 0; kc < kend; kc += 32) {
#pragma unroll
			for (int c = 0; c < 4; ++c) *reinterpret_cast<v2*>(As + ar * LB_LDS + ak + 2 * c) = v2{ra[2 * c], ra[2 * c + 1]};
#pragma unroll
			for (int c = 0; c < 2; ++c) *reinterpret_cast<v2*>(Bs + br * LB_LDS + bk + 2 * c) = rb[c];
			__syncthreads();
			if (kc + 32 < kend) fetch(kc + 32);
#pragma unroll
			for (int kk = 0; kk < 8; ++kk) {
				const double a = As[(16 * w + fr) * LB_LDS + 4 * kk + fk];
				const double b0 = Bs[fr * LB_LDS + 4 * kk + fk], b1 = Bs[(16 + fr) * LB_LDS + 4 * kk + fk];
				acc0 = Mfma<double>::mma(a, b0, acc0);
				acc1 = Mfma<double>::mma(a, b1, acc1);
			}
			__syncthreads();
		}
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			q0 = fma(acc0[i], acc0[i], q0);
			q1 = fma(acc1[i], acc1[i], q1);
			if (STORE_V) {
				const int row = r0 + 16 * w + Mfma<double>::crow(lane, i);
				if (row < NP) {
					VT[(int64_t)fr * ld + row] = acc0[i];
					VT[(int64_t)(16 + fr) * ld + row] = acc1[i];
				}
			}
		}
	}
	// (lanes fr, fr + 16, fr + 32, fr + 48 hold the four row groups of column fr: a symmetric tree, then the four waves in index order)
	q0 += __shfl_xor(q0, 16); q0 += __shfl_xor(q0, 32);
	q1 += __shfl_xor(q1, 16); q1 += __shfl_xor(q1, 32);
	if (lane < 16) {
		ssq[w][fr] = q0;
		ssq[w][16 + fr] = q1;
	}
	__syncthreads();
	if (tid < EX_TILE && tl.has(tid)) var[tl.out(tid)] = p.kappa - (((ssq[0][tid] + ssq[1][tid]) + ssq[2][tid]) + ssq[3][tid]);
}

// whether expert e has a factor the launch is sized for (workgroup-uniform)
__device__ __forceinline__ bool experts_has_factor(const ExpertsPredictArgs& p, int e, int64_t lo, int64_t hi)
{
	return p.info[e] == 0 && lo >= 0 && hi >= lo && hi <= p.N && hi - lo <= p.nmax;
}

__global__ __launch_bounds__(256, 2)
void experts_predict_kernel(ExpertsPredictArgs p)
{
	__shared__ __attribute__((aligned(16))) double As[64 * LB_LDS];
	__shared__ __attribute__((aligned(16))) double Bs[32 * LB_LDS];
	__shared__ double ssq[4][EX_TILE];
	const int tid = threadIdx.x;
	const int e = blockIdx.x / p.ntiles, tile = blockIdx.x - e * p.ntiles;
	const int64_t t0 = (int64_t)tile * EX_TILE;
	const int mt = (int)min((int64_t)EX_TILE, p.M - t0);
	const int64_t lo = p.offsets[e], hi = p.offsets[e + 1];
	double* mu = p.mu_e + (int64_t)e * p.ldm + t0;
	double* var = p.var_e + (int64_t)e * p.ldm + t0;
	if (!experts_has_factor(p, e, lo, hi)) {          // (workgroup-uniform) an expert without a factor: the prior
		if (tid < mt) {
			mu[tid] = 0.0;
			var[tid] = p.kappa;
		}
		return;
	}
	const int n = (int)(hi - lo), NP = (n + 31) & ~31;
	double* KT = p.work + (int64_t)blockIdx.x * p.wslice;          // KT[t][k] = k(xt_{t0 + t}, x_k), zero for t >= mt and k >= n
	experts_predict_body<false>(p, p.xs + lo * p.ldx, p.alpha + lo, p.factor + (int64_t)e * p.fslice, n, NP, ExpertsTileDense{t0, mt, 0}, KT, nullptr, mu, var,
	                            As, Bs, ssq);
}

// Steps 4 - 5 of a prediction with input gradients for one (expert, tile), after experts_predict_body<true> on the same tile: the ONE body of
// experts_predict_grad_kernel and its routed twin (the numbering is that of the comment on experts_predict_grad_kernel).  gmu, gvar: where
// tl.gout(t) counts from.  Entered by the whole workgroup.
template <class Tile>
__device__ __forceinline__ void experts_grad_body(const ExpertsPredictArgs& p, const double* x, const double* al, const double* V, int n, int NP,
                                                  const Tile& tl, double* KT, double* VT, double* gmu, double* gvar, double* As, double* Bs)
{
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;

	// ---- 4. W = V VT^T (lb_panel opens with a barrier: the stores of VT, and the last reads of the k* tile, are behind it)
	lb_panel<0>(KT, EX_TILE, V, NP, VT, NP, NP, NP, 0, As, Bs);
	__syncthreads();

	// ---- 5. the gradients
	const double* il = p.inv_ls;
	for (int t = w; t < EX_TILE; t += 4) {
		if (!tl.has(t)) continue;          // (wave-uniform; no barrier below)
		const double* xt = p.xt + tl.row(t) * p.ldt;
		double* Ft = VT + (int64_t)t * NP;
		double* gm = gmu + tl.gout(t);
		double* gv = gvar + tl.gout(t);
		for (int m0 = 0; m0 < p.d; m0 += 4) {
			double sm[4] = {0.0, 0.0, 0.0, 0.0}, sv[4] = {0.0, 0.0, 0.0, 0.0};
			for (int k = lane; k < n; k += 64) {
				const double* xk = x + (int64_t)k * p.ldx;
				double F;
				if (m0 == 0) {
					F = lb_dfactor(p.kind, lb_r2(xk, xt, p.cols, il, p.d));
					Ft[k] = F;
				} else
					F = Ft[k];
				const double a = al[k] * F, b = KT[(int64_t)k * EX_TILE + t] * F;
#pragma unroll
				for (int c = 0; c < 4; ++c)
					if (m0 + c < p.d) {
						const int col = p.cols ? p.cols[m0 + c] : m0 + c;
						const double u = xt[col] - xk[col];
						sm[c] = fma(a, u, sm[c]);
						sv[c] = fma(b, u, sv[c]);
					}
			}
#pragma unroll
			for (int c = 0; c < 4; ++c) {
#pragma unroll
				for (int o = 32; o > 0; o >>= 1) {
					sm[c] += __shfl_xor(sm[c], o);
					sv[c] += __shfl_xor(sv[c], o);
				}
			}
			if (lane == 0) {
#pragma unroll
				for (int c = 0; c < 4; ++c)
					if (m0 + c < p.d) {
						const double s2 = p.kappa * (il[m0 + c] * il[m0 + c]);
						gm[m0 + c] = -(s2 * sm[c]);
						gv[m0 + c] = 2.0 * (s2 * sv[c]);
					}
			}
		}
	}
}

// The prediction with its input gradients, per (expert, tile of 32 test points); the workspace slice is two halves of 32 NPM doubles.
//   1 - 3. experts_predict_body<true>: mu, var as experts_predict_kernel writes them, and v = L^-1 k* kept: VT[t][k] (second half of the slice);
//   4. w = K^-1 k* = L^-T v = V v, W[i][t] = sum_{k >= i} V[i][k] VT[t][k]: lb_panel<0> with A = V upper triangular from its row 0 (the round that
//      starts at row r0 reads V from column r0 on; the block just below the block diagonal is stored as zero, what lies further below is not
//      read), B = VT, C = W (NP x 32, row stride 32) over the k* tile, which is dead by then;
//   5. with F = lb_dfactor(r^2), r^2 recomputed from the points (direct differences), per selected column m:
//        gmu[t][m]  = -kappa il_m^2 sum_k alpha_k F_tk (xt_m - x_km),     gvar[t][m] = 2 kappa il_m^2 sum_k w_tk F_tk (xt_m - x_km)
//      (d k(x, x) / dx = 0 for a stationary term; Matern 1/2 on a coincident pair: F = 0): one wave per test point, lanes strided over k, a fixed
//      shuffle tree, four columns per pass over k; the first pass leaves F in VT[t][k] (dead after step 4; each lane re-reads what it stored).
__global__ __launch_bounds__(256, 2)
void experts_predict_grad_kernel(ExpertsPredictGradArgs g)
{
	__shared__ __attribute__((aligned(16))) double As[64 * LB_LDS];
	__shared__ __attribute__((aligned(16))) double Bs[32 * LB_LDS];
	__shared__ double ssq[4][EX_TILE];
	const ExpertsPredictArgs& p = g.p;
	const int tid = threadIdx.x;
	const int e = blockIdx.x / p.ntiles, tile = blockIdx.x - e * p.ntiles;
	const int64_t t0 = (int64_t)tile * EX_TILE;
	const int mt = (int)min((int64_t)EX_TILE, p.M - t0);
	const int64_t lo = p.offsets[e], hi = p.offsets[e + 1];
	double* mu = p.mu_e + (int64_t)e * p.ldm + t0;
	double* var = p.var_e + (int64_t)e * p.ldm + t0;
	double* gmu = g.gmu_e + (int64_t)e * g.lde + t0 * g.ldg;
	double* gvar = g.gvar_e + (int64_t)e * g.lde + t0 * g.ldg;
	if (!experts_has_factor(p, e, lo, hi)) {          // (workgroup-uniform) an expert without a factor: the prior, which is flat
		if (tid < mt) {
			mu[tid] = 0.0;
			var[tid] = p.kappa;
		}
		for (int i = tid; i < mt * p.d; i += 256) {
			const int t = i / p.d, m = i - t * p.d;
			gmu[(int64_t)t * g.ldg + m] = 0.0;
			gvar[(int64_t)t * g.ldg + m] = 0.0;
		}
		return;
	}
	const int n = (int)(hi - lo), NP = (n + 31) & ~31;
	const double* x = p.xs + lo * p.ldx;
	const double* al = p.alpha + lo;
	const double* V = p.factor + (int64_t)e * p.fslice;
	double* KT = p.work + (int64_t)blockIdx.x * p.wslice;          // the k* tile, then W[k][t] = (K^-1 k*_t)_k
	double* VT = KT + (p.wslice >> 1);                             // VT[t][k] = (L^-1 k*_t)_k, then F_tk
	const ExpertsTileDense tl{t0, mt, g.ldg};
	experts_predict_body<true>(p, x, al, V, n, NP, tl, KT, VT, mu, var, As, Bs, ssq);
	experts_grad_body(p, x, al, V, n, NP, tl, KT, VT, gmu, gvar, As, Bs);
}

// ---- Routed prediction: each test point asks its k nearest experts only (stpy_experts_centroids / _route / _predict_routed / _predict_routed_grad).
// The work list (built by the caller, on the device): tile w belongs to expert wexp[w] and its column c to pair wpair[32 w + c] = t k + j -- test
// point t, slot j of its selection -- or to nobody (-1).  The tile runs the bodies above; its results go to slot j of point t: mu_s[j ldm + t],
// gmu_s[j lde + t ldg + m], the layout the combination kernels read with E := k.  Whatever the list holds, nothing is written out of bounds: a tile
// whose expert is outside [0, E) returns at once, a pair outside [0, M k) is an empty column.
constexpr int EX_ROUTE_K = 16;          // stpy_experts_route_max_k(): a lane of the routing kernel keeps this many candidates in registers

struct ExpertsRouteList { const int32_t* wexp; const int32_t* wpair; int k; int64_t E; };

// the tables of ExpertsTileRouted for tile blockIdx.x; ends with a barrier (entered by the whole workgroup)
__device__ __forceinline__ void experts_routed_tile(const ExpertsRouteList& r, int64_t M, int64_t ldm, int64_t ldg, int64_t lde,
                                                    int64_t* trow, int64_t* oidx, int64_t* gidx)
{
	const int tid = threadIdx.x;
	if (tid < EX_TILE) {
		const int64_t pr = r.wpair[(int64_t)blockIdx.x * EX_TILE + tid];
		const bool ok = pr >= 0 && pr < M * r.k;
		const int64_t t = ok ? pr / r.k : 0, j = ok ? pr - t * r.k : 0;
		trow[tid] = ok ? t : -1;
		oidx[tid] = j * ldm + t;
		gidx[tid] = j * lde + t * ldg;
	}
	__syncthreads();
}

__global__ __launch_bounds__(256, 2)
void experts_predict_routed_kernel(ExpertsPredictArgs p, ExpertsRouteList r)
{
	__shared__ __attribute__((aligned(16))) double As[64 * LB_LDS];
	__shared__ __attribute__((aligned(16))) double Bs[32 * LB_LDS];
	__shared__ double ssq[4][EX_TILE];
	__shared__ int64_t trow[EX_TILE], oidx[EX_TILE], gidx[EX_TILE];
	const int tid = threadIdx.x;
	const int e = r.wexp[blockIdx.x];
	if (e < 0 || e >= r.E) return;          // (workgroup-uniform, before any barrier) a tile the list does not use
	experts_routed_tile(r, p.M, p.ldm, 0, 0, trow, oidx, gidx);
	const ExpertsTileRouted tl{trow, oidx, gidx};
	const int64_t lo = p.offsets[e], hi = p.offsets[e + 1];
	if (!experts_has_factor(p, e, lo, hi)) {          // (workgroup-uniform) an expert without a factor: the prior
		if (tid < EX_TILE && tl.has(tid)) {
			p.mu_e[tl.out(tid)] = 0.0;
			p.var_e[tl.out(tid)] = p.kappa;
		}
		return;
	}
	const int n = (int)(hi - lo), NP = (n + 31) & ~31;
	double* KT = p.work + (int64_t)blockIdx.x * p.wslice;
	experts_predict_body<false>(p, p.xs + lo * p.ldx, p.alpha + lo, p.factor + (int64_t)e * p.fslice, n, NP, tl, KT, nullptr, p.mu_e, p.var_e, As, Bs, ssq);
}

__global__ __launch_bounds__(256, 2)
void experts_predict_routed_grad_kernel(ExpertsPredictGradArgs g, ExpertsRouteList r)
{
	__shared__ __attribute__((aligned(16))) double As[64 * LB_LDS];
	__shared__ __attribute__((aligned(16))) double Bs[32 * LB_LDS];
	__shared__ double ssq[4][EX_TILE];
	__shared__ int64_t trow[EX_TILE], oidx[EX_TILE], gidx[EX_TILE];
	const ExpertsPredictArgs& p = g.p;
	const int tid = threadIdx.x;
	const int e = r.wexp[blockIdx.x];
	if (e < 0 || e >= r.E) return;          // (workgroup-uniform, before any barrier) a tile the list does not use
	experts_routed_tile(r, p.M, p.ldm, g.ldg, g.lde, trow, oidx, gidx);
	const ExpertsTileRouted tl{trow, oidx, gidx};
	const int64_t lo = p.offsets[e], hi = p.offsets[e + 1];
	if (!experts_has_factor(p, e, lo, hi)) {          // (workgroup-uniform) an expert without a factor: the prior, which is flat
		if (tid < EX_TILE && tl.has(tid)) {
			p.mu_e[tl.out(tid)] = 0.0;
			p.var_e[tl.out(tid)] = p.kappa;
		}
		for (int i = tid; i < EX_TILE * p.d; i += 256) {
			const int t = i / p.d, m = i - t * p.d;
			if (tl.has(t)) {
				g.gmu_e[tl.gout(t) + m] = 0.0;
				g.gvar_e[tl.gout(t) + m] = 0.0;
			}
		}
		return;
	}
	const int n = (int)(hi - lo), NP = (n + 31) & ~31;
	const double* x = p.xs + lo * p.ldx;
	const double* al = p.alpha + lo;
	const double* V = p.factor + (int64_t)e * p.fslice;
	double* KT = p.work + (int64_t)blockIdx.x * p.wslice;
	double* VT = KT + (p.wslice >> 1);
	experts_predict_body<true>(p, x, al, V, n, NP, tl, KT, VT, p.mu_e, p.var_e, As, Bs, ssq);
	experts_grad_body(p, x, al, V, n, NP, tl, KT, VT, g.gmu_e, g.gvar_e, As, Bs);
}

// cent[e*ldc + m] = (sum over the expert's rows, in row order, of x_i[cols[m]] * inv_ls[m]) / n_e: one wave per expert, lane m owns coordinate m
// and walks the rows one after the other.  An expert without rows (or whose offsets leave [0, N]) gets +inf in every coordinate.
__global__ __launch_bounds__(64)
void experts_centroids_kernel(const double* xs, int64_t N, int64_t ldx, int d, const int32_t* cols, const int32_t* offsets, const double* inv_ls,
                              double* cent, int64_t ldc)
{
	const int64_t e = blockIdx.x;
	const int64_t lo = offsets[e], hi = offsets[e + 1];
	const bool ok = lo >= 0 && hi > lo && hi <= N;
	for (int m = threadIdx.x; m < d; m += 64) {
		double s = __builtin_huge_val();
		if (ok) {
			const int col = cols ? cols[m] : m;
			const double il = inv_ls[m];
			s = 0.0;
			for (int64_t i = lo; i < hi; ++i) s += xs[i * ldx + col] * il;
			s /= (double)(hi - lo);
		}
		cent[e * ldc + m] = s;
	}
}

// (D, e) before (D', e'): the smaller distance, then the lower expert id
__device__ __forceinline__ bool experts_nearer(double D, int e, double D2, int e2) { return D < D2 || (D == D2 && e < e2); }

// The k nearest centroids of every test point: one wave per test point, lane l looks at the experts l, l + 64, ... in ascending order and keeps
// its EX_ROUTE_K nearest as a sorted list in registers (every index below is a compile-time constant: no scratch); then k rounds in which the
// wave agrees on the nearest list head (a butterfly minimum under a strict total order: the same answer in every lane) and its owner drops it;
// lane r remembers the winner of round r, counts how many winners have a lower id, and stores its own at that rank: sel[t*k ..] ascending in
// expert id.  D_e = sum_m (xt[cols[m]] inv_ls[m] - cent[e, m])^2, m ascending, capped at DBL_MAX (a NaN too), so that an expert without rows
// (cent[e, 0] = +inf: D_e = +inf) comes after every other.  No barrier, no LDS, no atomics.
__global__ __launch_bounds__(256)
void experts_route_kernel(const double* cent, int64_t ldc, int64_t E, int d, const int32_t* cols, const double* inv_ls, const double* xt, int64_t M,
                          int64_t ldt, int k, int32_t* sel)
{
	const int lane = threadIdx.x & 63;
	const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (t >= M) return;          // (wave-uniform)
	const double inf = __builtin_huge_val();
	const double* x = xt + t * ldt;
	double bd[EX_ROUTE_K];
	int be[EX_ROUTE_K];
#pragma unroll
	for (int i = 0; i < EX_ROUTE_K; ++i) {
		bd[i] = inf;
		be[i] = INT32_MAX;
	}
	for (int64_t e64 = lane; e64 < E; e64 += 64) {
		const int e = (int)e64;
		const double* c = cent + e64 * ldc;
		double D = 0.0;
		for (int m = 0; m < d; ++m) {
			const double u = x[cols ? cols[m] : m] * inv_ls[m] - c[m];
			D = fma(u, u, D);
		}
		D = c[0] == inf ? inf : fmin(D, 1.7976931348623157e308);
		if (experts_nearer(D, e, bd[EX_ROUTE_K - 1], be[EX_ROUTE_K - 1])) {
#pragma unroll
			for (int i = EX_ROUTE_K - 1; i >= 1; --i) {
				const bool up = experts_nearer(D, e, bd[i - 1], be[i - 1]), here = experts_nearer(D, e, bd[i], be[i]);
				bd[i] = up ? bd[i - 1] : (here ? D : bd[i]);
				be[i] = up ? be[i - 1] : (here ? e : be[i]);
			}
			if (experts_nearer(D, e, bd[0], be[0])) {
				bd[0] = D;
				be[0] = e;
			}
		}
	}
	int mine = INT32_MAX;
#pragma unroll
	for (int r = 0; r < EX_ROUTE_K; ++r) {
		if (r < k) {          // (uniform)
			double hd = bd[0];
			int he = be[0];
#pragma unroll
			for (int o = 32; o > 0; o >>= 1) {
				const double od = __shfl_xor(hd, o);
				const int oe = __shfl_xor(he, o);
				if (experts_nearer(od, oe, hd, he)) {
					hd = od;
					he = oe;
				}
			}
			if (be[0] == he) {
#pragma unroll
				for (int i = 0; i < EX_ROUTE_K - 1; ++i) {
					bd[i] = bd[i + 1];
					be[i] = be[i + 1];
				}
				bd[EX_ROUTE_K - 1] = inf;
				be[EX_ROUTE_K - 1] = INT32_MAX;
			}
			if (lane == r) mine = he;
		}
	}
	int rank = 0;
#pragma unroll
	for (int r = 0; r < EX_ROUTE_K; ++r)
		if (r < k) rank += __shfl(mine, r) < mine ? 1 : 0;
	if (lane < k && mine >= 0 && mine < E) sel[t * k + rank] = mine;
}

// One expert's term of the combination, the step both experts_combine_kernel and experts_combine_grad_kernel take (the same bits in mu and var):
// v = clamp(var_e), c = 1 / v, beta by the mode, and the three running sums in expert order.
struct ExpertsCombineSums { double prec, wm, bsum; };

__device__ __forceinline__ void experts_combine_step(int mode, double ve, double me, double vmin, double kappa, double logk, double inv_e,
                                                     double& v, double& c, double& beta, ExpertsCombineSums& s)
{
	v = fmin(fmax(ve, vmin), kappa);
	c = 1.0 / v;
	beta = mode == 1 ? inv_e : (mode == 3 ? 0.5 * (logk - log(v)) : 1.0);
	s.prec = fma(beta, c, s.prec);
	s.wm = fma(beta * c, me, s.wm);
	s.bsum += beta;
}

// 1 / var from the sums
__device__ __forceinline__ double experts_combine_prec(int mode, int64_t E, double kappa, const ExpertsCombineSums& s)
{
	double prec = s.prec;
	if (mode == 2) prec += (1.0 - (double)E) / kappa;
	if (mode == 3) prec += (1.0 - s.bsum) / kappa;
	return prec;
}

// one thread per test point, experts in expert order (the table of stpy_experts_combine in the header)
__global__ __launch_bounds__(256)
void experts_combine_kernel(int mode, int64_t E, int64_t M, const double* mu_e, const double* var_e, int64_t ldm, double kappa, double* mu, double* var)
{
	const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (t >= M) return;
	const double vmin = kappa * 2.220446049250313e-16, logk = log(kappa), inv_e = 1.0 / (double)E;
	ExpertsCombineSums s{0.0, 0.0, 0.0};
	for (int64_t e = 0; e < E; ++e) {
		double v, c, beta;
		experts_combine_step(mode, var_e[e * ldm + t], mu_e[e * ldm + t], vmin, kappa, logk, inv_e, v, c, beta, s);
	}
	const double vout = 1.0 / experts_combine_prec(mode, E, kappa, s);
	var[t] = vout;
	mu[t] = vout * s.wm;
}

struct ExpertsCombineGradArgs {
	int mode, d; int64_t E, M; const double* mu_e; const double* var_e; int64_t ldm; const double* gmu_e; const double* gvar_e; int64_t ldg, lde;
	double kappa; double* mu; double* var; double* dmu; double* dstd; int64_t ldo;
};

// The combination and its chain rule (the table of stpy_experts_combine_grad in the header): one thread per test point, experts in expert order,
// EXC_COLS coordinates per pass over the experts; the first pass is also the forward pass (a thread walks E experts one after the other, and
// what a pass costs is the latency of that walk, so the passes are what there is to save: one for d <= 8).  v = clamp(var_e): dv = gvar_e where
// kappa eps <= var_e <= kappa (the clamp is inactive, ties included), else 0 -- the derivative of the function as implemented.
constexpr int EXC_COLS = 8;

__global__ __launch_bounds__(256)
void experts_combine_grad_kernel(ExpertsCombineGradArgs p)
{
	const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (t >= p.M) return;
	const int mode = p.mode;
	const double kappa = p.kappa;
	const double vmin = kappa * 2.220446049250313e-16, logk = log(kappa), inv_e = 1.0 / (double)p.E;
	double vout = 0.0, wm = 0.0, half_isd = 0.0;
	for (int m0 = 0; m0 < p.d; m0 += EXC_COLS) {
		ExpertsCombineSums s{0.0, 0.0, 0.0};
		double dprec[EXC_COLS], dwm[EXC_COLS], dbs[EXC_COLS];
#pragma unroll
		for (int q = 0; q < EXC_COLS; ++q) dprec[q] = dwm[q] = dbs[q] = 0.0;
		for (int64_t e = 0; e < p.E; ++e) {
			const double ve = p.var_e[e * p.ldm + t], me = p.mu_e[e * p.ldm + t];
			double v, c, beta;
			experts_combine_step(mode, ve, me, vmin, kappa, logk, inv_e, v, c, beta, s);
			const bool open = ve >= vmin && ve <= kappa;
			const double bc = beta * c, cc = -(c * c), hv = -0.5 * c;          // (d c = cc dv, d beta = hv dv under rBCM)
			const double* gm = p.gmu_e + e * p.lde + t * p.ldg + m0;
			const double* gv = p.gvar_e + e * p.lde + t * p.ldg + m0;
#pragma unroll
			for (int q = 0; q < EXC_COLS; ++q)
				if (m0 + q < p.d) {
					const double dv = open ? gv[q] : 0.0;
					const double dbeta = mode == 3 ? hv * dv : 0.0;
					const double dbc = fma(dbeta, c, beta * (cc * dv));          // d (beta c)
					dprec[q] += dbc;
					dwm[q] += fma(dbc, me, bc * gm[q]);
					dbs[q] += dbeta;
				}
		}
		if (m0 == 0) {          // (every pass recomputes the same sums; the first one stores them)
			vout = 1.0 / experts_combine_prec(mode, p.E, kappa, s);
			wm = s.wm;
			half_isd = 0.5 / sqrt(vout);
			p.var[t] = vout;
			p.mu[t] = vout * wm;
		}
#pragma unroll
		for (int q = 0; q < EXC_COLS; ++q)
			if (m0 + q < p.d) {
				const double dp = mode == 3 ? dprec[q] - dbs[q] / kappa : dprec[q];
				const double dvar = -(vout * vout) * dp;
				p.dmu[t * p.ldo + m0 + q] = fma(dvar, wm, vout * dwm[q]);
				p.dstd[t * p.ldo + m0 + q] = dvar * half_isd;
			}
	}
}

}  // namespace stpy

// ---- C ABI (include/stpy_hip.h); every refusal below comes before the first HIP call
using namespace stpy;

static bool experts_common_refused(const char* who, int kind, int dtype, int64_t N, int64_t ldx, int d, int64_t E, int64_t nmax, int* rc)
{
	*rc = 0;
	if (dtype != STPY_F64) { set_error("%s: dtype %d: the local experts are float64 only (0)", who, dtype); *rc = -2; }
	else if (kind < STPY_K_SE || kind > STPY_K_MATERN52) { set_error("%s: kernel kind %d is not one stationary term (SE, MATERN12/32/52)", who, kind); *rc = -1; }
	else if (nmax < 0 || nmax > LB_MAX_N) { set_error("%s: nmax=%lld outside [0, %d] (stpy_experts_max_n)", who, (long long)nmax, LB_MAX_N); *rc = -4; }
	else if (N < 0 || N > INT32_MAX || E < 0 || E > INT32_MAX) { set_error("%s: N=%lld E=%lld out of range", who, (long long)N, (long long)E); *rc = -9; }
	else if (d < 1) { set_error("%s: bad dimension d=%d", who, d); *rc = -6; }
	else if (ldx < d) { set_error("%s: leading dimension ldx=%lld (d=%d)", who, (long long)ldx, d); *rc = -5; }
	return *rc != 0;
}

extern "C" {

int64_t stpy_experts_max_n(void) { return LB_MAX_N; }

int64_t stpy_experts_factor_bytes(int dtype, int64_t nmax, int64_t E)
{
	return dtype != STPY_F64 || nmax <= 0 || nmax > LB_MAX_N || E <= 0 ? 0 : E * experts_factor_slice(nmax) * (int64_t)sizeof(double);
}

int64_t stpy_experts_fit_workspace_bytes(int dtype, int64_t nmax, int d, int64_t E)
{
	(void)d;
	return dtype != STPY_F64 || nmax <= 0 || nmax > LB_MAX_N || E <= 0 ? 0 : E * experts_fit_slice(nmax) * (int64_t)sizeof(double);
}

int stpy_experts_fit(int kind, int dtype, const void* xs, int64_t N, int64_t ldx, int d, const int32_t* cols, const void* ys,
                     const int32_t* offsets, int64_t E, int64_t nmax, const void* inv_ls, const void* noise, double kappa, double weight,
                     const int32_t* pidx, int np, void* factor, int64_t factor_bytes, void* alpha, void* value, void* grad, int64_t ldg,
                     void* total, int32_t* info, void* work, int64_t work_bytes, void* stream)
{
	if (E == 0 || N == 0) return 0;          // empty problem: nothing to write
	int rc;
	if (experts_common_refused("stpy_experts_fit", kind, dtype, N, ldx, d, E, nmax, &rc)) return rc;
	if (grad && (np < 1 || ldg < (int64_t)np + 1)) {
		set_error("stpy_experts_fit: with a gradient np=%d must be positive and ldg=%lld at least np + 1", np, (long long)ldg);
		return np < 1 ? -16 : -19;
	}
	if (!xs || !ys || !offsets || !inv_ls || !noise || !factor || !alpha || !value || !total || !info || !work || (grad && !pidx)) {
		set_error("stpy_experts_fit: null pointer");
		return -3;
	}
	if (!(kappa > 0.0) || !is_finite(kappa) || !is_finite(weight)) { set_error("stpy_experts_fit: kappa=%g must be positive and finite, weight=%g finite", kappa, weight); return -11; }
	const int64_t need = stpy_experts_fit_workspace_bytes(dtype, nmax, d, E), fneed = stpy_experts_factor_bytes(dtype, nmax, E);
	if (work_bytes < need) {
		set_error("stpy_experts_fit: workspace of %lld bytes, %lld needed (see the *_workspace_bytes query for these arguments)", (long long)work_bytes, (long long)need);
		return -20;
	}
	if (factor_bytes < fneed) {
		set_error("stpy_experts_fit: factor buffer of %lld bytes, %lld needed (stpy_experts_factor_bytes)", (long long)factor_bytes, (long long)fneed);
		return -22;
	}
	if ((((uintptr_t)xs | (uintptr_t)ys | (uintptr_t)alpha) & 7) || (((uintptr_t)work | (uintptr_t)factor) & 15)) {
		set_error("stpy_experts_fit: work and factor must be 16-byte aligned, xs / ys / alpha 8-byte");
		return -21;
	}
	ExpertsFitArgs p{(const double*)xs, N, ldx, d, cols, (const double*)ys, offsets, (int)nmax, (const double*)inv_ls, (const double*)noise, kappa, weight,
	                 pidx, grad ? np : 0, (double*)factor, experts_factor_slice(nmax), (double*)alpha, (double*)value, (double*)grad, ldg, info,
	                 (double*)work, experts_fit_slice(nmax), kind};
	hipStream_t st = (hipStream_t)stream;
	if (grad) hipLaunchKernelGGL(experts_fit_kernel<true>, dim3((unsigned)E), dim3(256), 0, st, p);
	else hipLaunchKernelGGL(experts_fit_kernel<false>, dim3((unsigned)E), dim3(256), 0, st, p);
	hipLaunchKernelGGL(experts_total_kernel, dim3(1), dim3(64), 0, st, (const double*)value, (const double*)grad, ldg, grad ? np : 0, E, (double*)total);
	return check_launch("experts_fit");
}

int64_t stpy_experts_predict_workspace_bytes(int dtype, int64_t nmax, int d, int64_t E, int64_t M)
{
	(void)d;
	if (dtype != STPY_F64 || nmax <= 0 || nmax > LB_MAX_N || E <= 0 || M <= 0) return 0;
	return E * ((M + EX_TILE - 1) / EX_TILE) * experts_predict_slice(nmax) * (int64_t)sizeof(double);
}

int stpy_experts_predict(int kind, int dtype, const void* xs, int64_t N, int64_t ldx, int d, const int32_t* cols, const int32_t* offsets,
                         int64_t E, int64_t nmax, const void* inv_ls, double kappa, const void* factor, int64_t factor_bytes,
                         const void* alpha, const int32_t* info, const void* xt, int64_t M, int64_t ldt,
                         void* mu_e, void* var_e, int64_t ldm, void* work, int64_t work_bytes, void* stream)
{
	if (E == 0 || N == 0 || M == 0) return 0;
	int rc;
	if (experts_common_refused("stpy_experts_predict", kind, dtype, N, ldx, d, E, nmax, &rc)) return rc;
	const int64_t ntiles = M < 0 ? 0 : (M + EX_TILE - 1) / EX_TILE;
	if (M < 0 || E * ntiles > INT32_MAX) { set_error("stpy_experts_predict: M=%lld out of range (E x tiles of 32 test points must stay below 2^31)", (long long)M); return -9; }
	if (ldt < d || ldm < M) { set_error("stpy_experts_predict: leading dimensions ldt=%lld (d=%d) ldm=%lld (M=%lld)", (long long)ldt, d, (long long)ldm, (long long)M); return ldt < d ? -5 : -13; }
	if (!xs || !offsets || !inv_ls || !factor || !alpha || !info || !xt || !mu_e || !var_e || !work) { set_error("stpy_experts_predict: null pointer"); return -3; }
	if (!(kappa > 0.0) || !is_finite(kappa)) { set_error("stpy_experts_predict: kappa=%g must be positive and finite", kappa); return -11; }
	const int64_t need = stpy_experts_predict_workspace_bytes(dtype, nmax, d, E, M), fneed = stpy_experts_factor_bytes(dtype, nmax, E);
	if (work_bytes < need) {
		set_error("stpy_experts_predict: workspace of %lld bytes, %lld needed (see the *_workspace_bytes query for these arguments)", (long long)work_bytes, (long long)need);
		return -20;
	}
	if (factor_bytes < fneed) {
		set_error("stpy_experts_predict: factor buffer of %lld bytes, %lld needed (stpy_experts_factor_bytes)", (long long)factor_bytes, (long long)fneed);
		return -22;
	}
	if ((((uintptr_t)xs | (uintptr_t)xt | (uintptr_t)alpha | (uintptr_t)mu_e | (uintptr_t)var_e) & 7) || (((uintptr_t)work | (uintptr_t)factor) & 15)) {
		set_error("stpy_experts_predict: work and factor must be 16-byte aligned, the other arrays 8-byte");
		return -21;
	}
	ExpertsPredictArgs p{(const double*)xs, N, ldx, d, cols, offsets, (int)nmax, (const double*)inv_ls, kappa, (const double*)factor, experts_factor_slice(nmax),
	                     (const double*)alpha, info, (const double*)xt, M, ldt, (double*)mu_e, (double*)var_e, ldm, (double*)work, experts_predict_slice(nmax),
	                     (int)ntiles, kind};
	hipLaunchKernelGGL(experts_predict_kernel, dim3((unsigned)(E * ntiles)), dim3(256), 0, (hipStream_t)stream, p);
	return check_launch("experts_predict");
}

int stpy_experts_combine(int mode, int64_t E, int64_t M, const void* mu_e, const void* var_e, int64_t ldm, double kappa, void* mu, void* var, void* stream)
{
	if (E == 0 || M == 0) return 0;
	if (mode < 0 || mode > 3) { set_error("stpy_experts_combine: mode %d (0 PoE, 1 gPoE, 2 BCM, 3 rBCM)", mode); return -10; }
	if (E < 0 || M < 0 || M > (int64_t)INT32_MAX * 256) { set_error("stpy_experts_combine: E=%lld M=%lld out of range", (long long)E, (long long)M); return -9; }
	if (ldm < M) { set_error("stpy_experts_combine: leading dimension ldm=%lld (M=%lld)", (long long)ldm, (long long)M); return -13; }
	if (!mu_e || !var_e || !mu || !var) { set_error("stpy_experts_combine: null pointer"); return -3; }
	if (!(kappa > 0.0) || !is_finite(kappa)) { set_error("stpy_experts_combine: kappa=%g must be positive and finite", kappa); return -11; }
	if (((uintptr_t)mu_e | (uintptr_t)var_e | (uintptr_t)mu | (uintptr_t)var) & 7) { set_error("stpy_experts_combine: arrays must be 8-byte aligned"); return -21; }
	hipLaunchKernelGGL(experts_combine_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mode, E, M, (const double*)mu_e,
	                   (const double*)var_e, ldm, kappa, (double*)mu, (double*)var);
	return check_launch("experts_combine");
}

int64_t stpy_experts_predict_grad_workspace_bytes(int dtype, int64_t nmax, int d, int64_t E, int64_t M)
{
	return 2 * stpy_experts_predict_workspace_bytes(dtype, nmax, d, E, M);
}

int stpy_experts_predict_grad(int kind, int dtype, const void* xs, int64_t N, int64_t ldx, int d, const int32_t* cols, const int32_t* offsets,
                              int64_t E, int64_t nmax, const void* inv_ls, double kappa, const void* factor, int64_t factor_bytes,
                              const void* alpha, const int32_t* info, const void* xt, int64_t M, int64_t ldt,
                              void* mu_e, void* var_e, int64_t ldm, void* gmu_e, void* gvar_e, int64_t ldg, int64_t lde,
                              void* work, int64_t work_bytes, void* stream)
{
	const char* who = "stpy_experts_predict_grad";
	if (E == 0 || N == 0 || M == 0) return 0;
	int rc;
	if (experts_common_refused(who, kind, dtype, N, ldx, d, E, nmax, &rc)) return rc;
	const int64_t ntiles = M < 0 ? 0 : (M + EX_TILE - 1) / EX_TILE;
	if (M < 0 || E * ntiles > INT32_MAX) { set_error("%s: M=%lld out of range (E x tiles of 32 test points must stay below 2^31)", who, (long long)M); return -9; }
	if (ldt < d || ldm < M) { set_error("%s: leading dimensions ldt=%lld (d=%d) ldm=%lld (M=%lld)", who, (long long)ldt, d, (long long)ldm, (long long)M); return ldt < d ? -5 : -13; }
	if (ldg < d || lde / ldg < M) {          // (lde < M ldg without forming the product)
		set_error("%s: gradient strides ldg=%lld (d=%d) lde=%lld (at least M ldg, M=%lld)", who, (long long)ldg, d, (long long)lde, (long long)M);
		return -19;
	}
	if (!xs || !offsets || !inv_ls || !factor || !alpha || !info || !xt || !mu_e || !var_e || !gmu_e || !gvar_e || !work) { set_error("%s: null pointer", who); return -3; }
	if (!(kappa > 0.0) || !is_finite(kappa)) { set_error("%s: kappa=%g must be positive and finite", who, kappa); return -11; }
	const int64_t need = stpy_experts_predict_grad_workspace_bytes(dtype, nmax, d, E, M), fneed = stpy_experts_factor_bytes(dtype, nmax, E);
	if (work_bytes < need) {
		set_error("%s: workspace of %lld bytes, %lld needed (see the *_workspace_bytes query for these arguments)", who, (long long)work_bytes, (long long)need);
		return -20;
	}
	if (factor_bytes < fneed) {
		set_error("%s: factor buffer of %lld bytes, %lld needed (stpy_experts_factor_bytes)", who, (long long)factor_bytes, (long long)fneed);
		return -22;
	}
	if ((((uintptr_t)xs | (uintptr_t)xt | (uintptr_t)alpha | (uintptr_t)mu_e | (uintptr_t)var_e | (uintptr_t)gmu_e | (uintptr_t)gvar_e) & 7)
	    || (((uintptr_t)work | (uintptr_t)factor) & 15)) {
		set_error("%s: work and factor must be 16-byte aligned, the other arrays 8-byte", who);
		return -21;
	}
	ExpertsPredictGradArgs g{{(const double*)xs, N, ldx, d, cols, offsets, (int)nmax, (const double*)inv_ls, kappa, (const double*)factor, experts_factor_slice(nmax),
	                          (const double*)alpha, info, (const double*)xt, M, ldt, (double*)mu_e, (double*)var_e, ldm, (double*)work, 2 * experts_predict_slice(nmax),
	                          (int)ntiles, kind},
	                         (double*)gmu_e, (double*)gvar_e, ldg, lde};
	hipLaunchKernelGGL(experts_predict_grad_kernel, dim3((unsigned)(E * ntiles)), dim3(256), 0, (hipStream_t)stream, g);
	return check_launch("experts_predict_grad");
}

int stpy_experts_combine_grad(int mode, int64_t E, int64_t M, int d, const void* mu_e, const void* var_e, int64_t ldm,
                              const void* gmu_e, const void* gvar_e, int64_t ldg, int64_t lde, double kappa,
                              void* mu, void* var, void* dmu, void* dstd, int64_t ldo, void* stream)
{
	const char* who = "stpy_experts_combine_grad";
	if (E == 0 || M == 0) return 0;
	if (mode < 0 || mode > 3) { set_error("%s: mode %d (0 PoE, 1 gPoE, 2 BCM, 3 rBCM)", who, mode); return -10; }
	if (E < 0 || M < 0 || M > (int64_t)INT32_MAX * 256) { set_error("%s: E=%lld M=%lld out of range", who, (long long)E, (long long)M); return -9; }
	if (d < 1) { set_error("%s: bad dimension d=%d", who, d); return -6; }
	if (ldm < M) { set_error("%s: leading dimension ldm=%lld (M=%lld)", who, (long long)ldm, (long long)M); return -13; }
	if (ldg < d || lde / ldg < M || ldo < d) {
		set_error("%s: gradient strides ldg=%lld ldo=%lld (d=%d) lde=%lld (at least M ldg, M=%lld)", who, (long long)ldg, (long long)ldo, d, (long long)lde, (long long)M);
		return -19;
	}
	if (!mu_e || !var_e || !gmu_e || !gvar_e || !mu || !var || !dmu || !dstd) { set_error("%s: null pointer", who); return -3; }
	if (!(kappa > 0.0) || !is_finite(kappa)) { set_error("%s: kappa=%g must be positive and finite", who, kappa); return -11; }
	if (((uintptr_t)mu_e | (uintptr_t)var_e | (uintptr_t)gmu_e | (uintptr_t)gvar_e | (uintptr_t)mu | (uintptr_t)var | (uintptr_t)dmu | (uintptr_t)dstd) & 7) {
		set_error("%s: arrays must be 8-byte aligned", who);
		return -21;
	}
	ExpertsCombineGradArgs p{mode, d, E, M, (const double*)mu_e, (const double*)var_e, ldm, (const double*)gmu_e, (const double*)gvar_e, ldg, lde, kappa,
	                         (double*)mu, (double*)var, (double*)dmu, (double*)dstd, ldo};
	hipLaunchKernelGGL(experts_combine_grad_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
	return check_launch("experts_combine_grad");
}

// ---- routing
int64_t stpy_experts_route_max_k(void) { return EX_ROUTE_K; }

int stpy_experts_centroids(int dtype, const void* xs, int64_t N, int64_t ldx, int d, const int32_t* cols, const int32_t* offsets, int64_t E,
                           const void* inv_ls, void* cent, int64_t ldc, void* stream)
{
	const char* who = "stpy_experts_centroids";
	if (E == 0) return 0;
	int rc;
	if (experts_common_refused(who, STPY_K_SE, dtype, N, ldx, d, E, 0, &rc)) return rc;
	if (ldc < d) { set_error("%s: leading dimension ldc=%lld (d=%d)", who, (long long)ldc, d); return -5; }
	if ((N > 0 && !xs) || !offsets || !inv_ls || !cent) { set_error("%s: null pointer", who); return -3; }
	if (((uintptr_t)xs | (uintptr_t)inv_ls | (uintptr_t)cent) & 7) { set_error("%s: arrays must be 8-byte aligned", who); return -21; }
	hipLaunchKernelGGL(experts_centroids_kernel, dim3((unsigned)E), dim3(64), 0, (hipStream_t)stream, (const double*)xs, N, ldx, d, cols, offsets,
	                   (const double*)inv_ls, (double*)cent, ldc);
	return check_launch("experts_centroids");
}

// k outside [1, min(E, cap)] (-23), shared by the three entry points that take it
static bool experts_k_refused(const char* who, int k, int64_t E, int64_t M, int* rc)
{
	*rc = 0;
	if (k < 1 || k > EX_ROUTE_K || k > E) {
		set_error("%s: k=%d outside [1, min(E=%lld, %d)] (stpy_experts_route_max_k)", who, k, (long long)E, EX_ROUTE_K);
		*rc = -23;
	} else if (M < 0 || M > INT32_MAX / k) { set_error("%s: M=%lld out of range (M k pair ids must stay below 2^31)", who, (long long)M); *rc = -9; }
	return *rc != 0;
}

int stpy_experts_route(int dtype, const void* cent, int64_t ldc, int64_t E, int d, const int32_t* cols, const void* inv_ls,
                       const void* xt, int64_t M, int64_t ldt, int k, int32_t* sel, void* stream)
{
	const char* who = "stpy_experts_route";
	if (E == 0 || M == 0) return 0;
	int rc;
	if (experts_common_refused(who, STPY_K_SE, dtype, 0, d, d, E, 0, &rc)) return rc;
	if (experts_k_refused(who, k, E, M, &rc)) return rc;
	if (ldc < d || ldt < d) { set_error("%s: leading dimensions ldc=%lld ldt=%lld (d=%d)", who, (long long)ldc, (long long)ldt, d); return -5; }
	if (!cent || !inv_ls || !xt || !sel) { set_error("%s: null pointer", who); return -3; }
	if ((((uintptr_t)cent | (uintptr_t)inv_ls | (uintptr_t)xt) & 7) || ((uintptr_t)sel & 3)) { set_error("%s: cent / inv_ls / xt must be 8-byte aligned, sel 4-byte", who); return -21; }
	hipLaunchKernelGGL(experts_route_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const double*)cent, ldc, E, d, cols,
	                   (const double*)inv_ls, (const double*)xt, M, ldt, k, sel);
	return check_launch("experts_route");
}

int64_t stpy_experts_predict_routed_workspace_bytes(int dtype, int64_t nmax, int d, int64_t T)
{
	(void)d;
	if (dtype != STPY_F64 || nmax <= 0 || nmax > LB_MAX_N || T <= 0) return 0;
	return T * experts_predict_slice(nmax) * (int64_t)sizeof(double);
}

int64_t stpy_experts_predict_routed_grad_workspace_bytes(int dtype, int64_t nmax, int d, int64_t T)
{
	return 2 * stpy_experts_predict_routed_workspace_bytes(dtype, nmax, d, T);
}

// the checks the two routed predictions share (gmu_s == NULL: without gradients)
static int experts_routed_refused(const char* who, bool grad, int kind, int dtype, const void* xs, int64_t N, int64_t ldx, int d, const int32_t* offsets,
                                  int64_t E, int64_t nmax, const void* inv_ls, double kappa, const void* factor, int64_t factor_bytes, const void* alpha,
                                  const int32_t* info, const void* xt, int64_t M, int64_t ldt, int k, const int32_t* wexp, const int32_t* wpair, int64_t T,
                                  const void* mu_s, const void* var_s, int64_t ldm, const void* gmu_s, const void* gvar_s, int64_t ldg, int64_t lde,
                                  const void* work, int64_t work_bytes)
{
	int rc;
	if (experts_common_refused(who, kind, dtype, N, ldx, d, E, nmax, &rc)) return rc;
	if (experts_k_refused(who, k, E, M, &rc)) return rc;
	if (T < 0 || T > INT32_MAX) { set_error("%s: T=%lld tiles out of range", who, (long long)T); return -9; }
	if (ldt < d || ldm < M) { set_error("%s: leading dimensions ldt=%lld (d=%d) ldm=%lld (M=%lld)", who, (long long)ldt, d, (long long)ldm, (long long)M); return ldt < d ? -5 : -13; }
	if (grad && (ldg < d || lde / ldg < M)) {
		set_error("%s: gradient strides ldg=%lld (d=%d) lde=%lld (at least M ldg, M=%lld)", who, (long long)ldg, d, (long long)lde, (long long)M);
		return -19;
	}
	if (!xs || !offsets || !inv_ls || !factor || !alpha || !info || !xt || !wexp || !wpair || !mu_s || !var_s || !work || (grad && (!gmu_s || !gvar_s))) {
		set_error("%s: null pointer", who);
		return -3;
	}
	if (!(kappa > 0.0) || !is_finite(kappa)) { set_error("%s: kappa=%g must be positive and finite", who, kappa); return -11; }
	const int64_t need = (grad ? 2 : 1) * stpy_experts_predict_routed_workspace_bytes(dtype, nmax, d, T), fneed = stpy_experts_factor_bytes(dtype, nmax, E);
	if (work_bytes < need) {
		set_error("%s: workspace of %lld bytes, %lld needed (see the *_workspace_bytes query for these arguments)", who, (long long)work_bytes, (long long)need);
		return -20;
	}
	if (factor_bytes < fneed) {
		set_error("%s: factor buffer of %lld bytes, %lld needed (stpy_experts_factor_bytes)", who, (long long)factor_bytes, (long long)fneed);
		return -22;
	}
	if ((((uintptr_t)xs | (uintptr_t)xt | (uintptr_t)alpha | (uintptr_t)mu_s | (uintptr_t)var_s | (uintptr_t)gmu_s | (uintptr_t)gvar_s) & 7)
	    || (((uintptr_t)work | (uintptr_t)factor) & 15) || (((uintptr_t)wexp | (uintptr_t)wpair) & 3)) {
		set_error("%s: work and factor must be 16-byte aligned, the other arrays 8-byte, wexp / wpair 4-byte", who);
		return -21;
	}
	return 0;
}

int stpy_experts_predict_routed(int kind, int dtype, const void* xs, int64_t N, int64_t ldx, int d, const int32_t* cols, const int32_t* offsets,
                                int64_t E, int64_t nmax, const void* inv_ls, double kappa, const void* factor, int64_t factor_bytes,
                                const void* alpha, const int32_t* info, const void* xt, int64_t M, int64_t ldt,
                                int k, const int32_t* wexp, const int32_t* wpair, int64_t T,
                                void* mu_s, void* var_s, int64_t ldm, void* work, int64_t work_bytes, void* stream)
{
	if (E == 0 || N == 0 || M == 0 || T == 0) return 0;
	const int rc = experts_routed_refused("stpy_experts_predict_routed", false, kind, dtype, xs, N, ldx, d, offsets, E, nmax, inv_ls, kappa, factor, factor_bytes,
	                                      alpha, info, xt, M, ldt, k, wexp, wpair, T, mu_s, var_s, ldm, nullptr, nullptr, 0, 0, work, work_bytes);
	if (rc) return rc;
	ExpertsPredictArgs p{(const double*)xs, N, ldx, d, cols, offsets, (int)nmax, (const double*)inv_ls, kappa, (const double*)factor, experts_factor_slice(nmax),
	                     (const double*)alpha, info, (const double*)xt, M, ldt, (double*)mu_s, (double*)var_s, ldm, (double*)work, experts_predict_slice(nmax),
	                     0, kind};
	hipLaunchKernelGGL(experts_predict_routed_kernel, dim3((unsigned)T), dim3(256), 0, (hipStream_t)stream, p, ExpertsRouteList{wexp, wpair, k, E});
	return check_launch("experts_predict_routed");
}

int stpy_experts_predict_routed_grad(int kind, int dtype, const void* xs, int64_t N, int64_t ldx, int d, const int32_t* cols, const int32_t* offsets,
                                     int64_t E, int64_t nmax, const void* inv_ls, double kappa, const void* factor, int64_t factor_bytes,
                                     const void* alpha, const int32_t* info, const void* xt, int64_t M, int64_t ldt,
                                     int k, const int32_t* wexp, const int32_t* wpair, int64_t T,
                                     void* mu_s, void* var_s, int64_t ldm, void* gmu_s, void* gvar_s, int64_t ldg, int64_t lde,
                                     void* work, int64_t work_bytes, void* stream)
{
	if (E == 0 || N == 0 || M == 0 || T == 0) return 0;
	const int rc = experts_routed_refused("stpy_experts_predict_routed_grad", true, kind, dtype, xs, N, ldx, d, offsets, E, nmax, inv_ls, kappa, factor,
	                                      factor_bytes, alpha, info, xt, M, ldt, k, wexp, wpair, T, mu_s, var_s, ldm, gmu_s, gvar_s, ldg, lde, work, work_bytes);
	if (rc) return rc;
	ExpertsPredictGradArgs g{{(const double*)xs, N, ldx, d, cols, offsets, (int)nmax, (const double*)inv_ls, kappa, (const double*)factor, experts_factor_slice(nmax),
	                          (const double*)alpha, info, (const double*)xt, M, ldt, (double*)mu_s, (double*)var_s, ldm, (double*)work, 2 * experts_predict_slice(nmax),
	                          0, kind},
	                         (double*)gmu_s, (double*)gvar_s, ldg, lde};
	hipLaunchKernelGGL(experts_predict_routed_grad_kernel, dim3((unsigned)T), dim3(256), 0, (hipStream_t)stream, g, ExpertsRouteList{wexp, wpair, k, E});
	return check_launch("experts_predict_routed_grad");
}

}  // extern "C"
