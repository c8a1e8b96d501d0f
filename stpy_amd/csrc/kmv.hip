// Matrix-free products and solves with a kernel matrix generated on the fly: stpy_kmv, Yt = Vt (K + diag_add I) for a block of right-hand
// sides stored one per row, and stpy_pcg, block preconditioned conjugate gradients on that operator.  K is never formed.
//
// stpy_kmv is the plain pair walker of kmv_pair.h (the design, the cut and the fp64 rule are stated there) with the widest row block: up to 64
// right-hand sides (four accumulator tuples, ragged blocks zero-filled) share one kernel evaluation, and blockIdx.z walks further 64s.  The
// values are those of the pivoted Cholesky (pc_phi: the operator is the one the preconditioner's factor was built from, bitwise symmetric
// when a == b, exactly kappa on coincident points).  The register forms evaluate a chunk in four rounds of four values per lane, which keeps
// the fp64 kernels at 93 / 111 / 159 VGPRs (four, four and three waves per SIMD): with one wave per SIMD the load -> LDS -> barrier of every
// chunk was exposed and the kernel ran 3.8 times slower.  Beyond d = 16 the coordinates go through LDS, 16 at a time.  D has col = i, so rows
// of Yt are written in runs of 16 neighbouring elements; the second launch of a cut range adds diag_add Vt as the direct store does.
//
// stpy_pcg.  Ordinary preconditioned CG per column with M^-1 = I - G G^T (two NT products on the library's MFMA contraction per iteration).
// One workgroup per column does that column's dot products (double accumulation, fixed order) and updates with scalars that never leave
// the device; a frozen column is skipped by every kernel that writes X, R, P or its counter.
#include "common.h"
#include "kmv_pair.h"

namespace stpy {

namespace {

constexpr int KM_TC = 64;              // right-hand sides per pass (4 accumulator tuples)

template <typename T>
struct KmvArgs {
	const T* a; int64_t lda; int n; const T* b; int64_t ldb; int q; int d; const int32_t* cols; const T* inv_ls; T kappa, diag_add; int kind;
	const T* Vt; int64_t ldv; int t; T* Yt; int64_t ldy; T* part; int nsplit, jper;
};

// DC coordinates at a time; ONE: d <= DC, the a coordinates and the lengthscales are loaded once into registers
template <typename T, int DC, bool ONE>
__global__ __launch_bounds__(KP_THREADS, ONE ? 3 : 1)          // (second figure: waves per SIMD the register budget must allow)
void kmv_kernel(KmvArgs<T> g)
{
	typedef typename Mfma<T>::v4 v4;
	__shared__ T sv[KP_JC][KM_TC + 1];
	__shared__ T sb[DC][KP_JC];
	__shared__ T sa[ONE ? 1 : DC][KP_TILE];
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
	const int64_t i0 = (int64_t)blockIdx.x * KP_TILE;
	const int64_t i = i0 + 16 * w + li;
	const int c0 = (int)blockIdx.z * KM_TC;
	const int nb = min(4, (g.t - c0 + 15) >> 4);
	int jb, je;
	kp_range(g.jper, g.q, jb, je);
	v4 acc[4];
#pragma unroll
	for (int b = 0; b < 4; ++b) acc[b] = v4{(T)0, (T)0, (T)0, (T)0};
	T av[DC], il[DC];
	if (ONE) {
#pragma unroll
		for (int k = 0; k < DC; ++k) {
			const bool in = k < g.d;
			const int c = in ? (g.cols ? g.cols[k] : k) : 0;
			il[k] = in ? g.inv_ls[k] : (T)0;
			av[k] = (in && i < g.n) ? g.a[i * g.lda + c] : (T)0;
		}
	}
	for (int64_t j0 = jb; j0 < je; j0 += KP_JC) {          // (64 bits: j0 + 64 may pass 2^31)
		__syncthreads();                                              // (the previous chunk has been read)
		for (int cc = w; cc < 16 * nb; cc += 4) {
			const int c = c0 + cc;
			const int64_t j = j0 + lane;
			sv[lane][cc] = (c < g.t && j < je) ? g.Vt[(int64_t)c * g.ldv + j] : (T)0;
		}
		if (ONE) {
			for (int e = tid; e < DC * KP_JC; e += KP_THREADS) {
				const int k = e >> 6, jj = e & 63;
				const int64_t j = j0 + jj;
				sb[k][jj] = (k < g.d && j < je) ? g.b[j * g.ldb + (g.cols ? g.cols[k] : k)] : (T)0;
			}
			__syncthreads();
			// four rounds of four values per lane: a round's four exponentials overlap, and only four squared distances are live at a time
#pragma unroll 1
			for (int sg = 0; sg < 4; ++sg) {
				T r2[4], kv[4];
#pragma unroll
				for (int u = 0; u < 4; ++u) {
					const int jj = 16 * sg + 4 * u + lk;
					r2[u] = (T)0;
#pragma unroll
					for (int k = 0; k < DC; ++k) {
						const T df = (av[k] - sb[k][jj]) * il[k];
						r2[u] = pc_fma(df, df, r2[u]);
					}
				}
				km_phi4(g.kind, r2, kv);
#pragma unroll
				for (int u = 0; u < 4; ++u) {
					const int jj = 16 * sg + 4 * u + lk;
					const T v = j0 + jj < je ? g.kappa * kv[u] : (T)0;
#pragma unroll
					for (int b = 0; b < 4; ++b)
						if (b < nb) acc[b] = Mfma<T>::mma(sv[jj][16 * b + li], v, acc[b]);
				}
			}
		} else {
			T r2[16];
#pragma unroll
			for (int s = 0; s < 16; ++s) r2[s] = (T)0;
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
					av[k] = sa[k][16 * w + li];
					il[k] = k0 + k < g.d ? g.inv_ls[k0 + k] : (T)0;
				}
#pragma unroll
				for (int s = 0; s < 16; ++s) {
#pragma unroll
					for (int k = 0; k < DC; ++k) {
						const T df = (av[k] - sb[k][4 * s + lk]) * il[k];
						r2[s] = pc_fma(df, df, r2[s]);
					}
				}
			}
#pragma unroll
			for (int sg = 0; sg < 4; ++sg) {
				T kv[4];
				km_phi4(g.kind, r2 + 4 * sg, kv);
#pragma unroll
				for (int u = 0; u < 4; ++u) {
					const int jj = 16 * sg + 4 * u + lk;
					const T v = j0 + jj < je ? g.kappa * kv[u] : (T)0;
#pragma unroll
					for (int b = 0; b < 4; ++b)
						if (b < nb) acc[b] = Mfma<T>::mma(sv[jj][16 * b + li], v, acc[b]);
				}
			}
		}
	}
	if (i >= g.n) return;
#pragma unroll
	for (int b = 0; b < 4; ++b) {
#pragma unroll
		for (int r = 0; r < 4; ++r) {
			const int c = c0 + 16 * b + Mfma<T>::crow(lane, r);
			if (b >= nb || c >= g.t) continue;
			if (g.nsplit > 1) {
				g.part[((int64_t)blockIdx.y * g.t + c) * g.n + i] = acc[b][r];
			} else {
				T y = acc[b][r];
				if (g.diag_add != (T)0) y += g.diag_add * g.Vt[(int64_t)c * g.ldv + i];
				g.Yt[(int64_t)c * g.ldy + i] = y;
			}
		}
	}
}

// Yt = the pieces added in piece order (+ diag_add Vt); with nsplit == 0 (q == 0) the zero fill
template <typename T>
__global__ __launch_bounds__(KP_THREADS)
void kmv_reduce_kernel(KmvArgs<T> g)
{
	const int64_t i = (int64_t)blockIdx.x * KP_THREADS + threadIdx.x;
	if (i >= g.n) return;
	for (int c = (int)blockIdx.y; c < g.t; c += (int)gridDim.y) {
		T y = (T)0;
		for (int s = 0; s < g.nsplit; ++s) y += g.part[((int64_t)s * g.t + c) * g.n + i];
		if (g.diag_add != (T)0) y += g.diag_add * g.Vt[(int64_t)c * g.ldv + i];
		g.Yt[(int64_t)c * g.ldy + i] = y;
	}
}

// An upper bound of nsplit * t * n elements that does not decrease in n, q or t: the split happens below KP_FILL tiles only, where
// nsplit <= KP_SPLIT_TARGET / tiles + 1 and n <= 64 tiles / passes, so nsplit n t <= (KP_SPLIT_TARGET + KP_FILL) 64 min(t, 64).
inline int64_t kmv_workspace_bytes(int dtype, int64_t t)
{
	const int64_t esz = dtype == STPY_F32 ? 4 : 8;
	const int64_t tc = t < 1 ? 1 : (t < KM_TC ? t : KM_TC);
	return (int64_t)(KP_SPLIT_TARGET + KP_FILL) * KP_TILE * tc * esz;
}

template <typename T>
int kmv(int kind, const T* a, int64_t n, int64_t lda, const T* b, int64_t q, int64_t ldb, int d, const int32_t* cols, const T* inv_ls,
        double kappa, double diag_add, const T* Vt, int64_t t, int64_t ldv, T* Yt, int64_t ldy, void* work, hipStream_t st)
{
	const int64_t passes = (t + KM_TC - 1) / KM_TC;
	const int nsplit = q == 0 ? 0 : kp_split(kp_tiles(n) * passes, q, KP_MAX_SPLIT);
	if (nsplit > 1 && (int64_t)nsplit * t * n * (int64_t)sizeof(T) > kmv_workspace_bytes(sizeof(T) == 4 ? STPY_F32 : STPY_F64, t)) {          // (cannot happen: see the bound)
		set_error("stpy_kmv: internal: %d pieces of %lld x %lld exceed the workspace bound", nsplit, (long long)t, (long long)n);
		return -21;
	}
	KmvArgs<T> g{a, lda, (int)n, b, ldb, (int)q, d, cols, inv_ls, (T)kappa, (T)diag_add, kind, Vt, ldv, (int)t, Yt, ldy, (T*)work, nsplit, (int)kp_piece_length(q, nsplit)};
	if (nsplit >= 1) {
		const dim3 grid((unsigned)kp_tiles(n), (unsigned)nsplit, (unsigned)passes);
		if (d <= 4) hipLaunchKernelGGL((kmv_kernel<T, 4, true>), grid, dim3(KP_THREADS), 0, st, g);
		else if (d <= 8) hipLaunchKernelGGL((kmv_kernel<T, 8, true>), grid, dim3(KP_THREADS), 0, st, g);
		else if (d <= 16) hipLaunchKernelGGL((kmv_kernel<T, 16, true>), grid, dim3(KP_THREADS), 0, st, g);
		else hipLaunchKernelGGL((kmv_kernel<T, 16, false>), grid, dim3(KP_THREADS), 0, st, g);
	}
	if (nsplit != 1)
		hipLaunchKernelGGL(kmv_reduce_kernel<T>, dim3((unsigned)((n + KP_THREADS - 1) / KP_THREADS), (unsigned)(t < 64 ? t : 64)), dim3(KP_THREADS), 0, st, g);
	return check_launch("stpy_kmv");
}

// ---------------------------------------------------------------------------------------------------------------- block PCG
struct PcgCol { double bb, rr, rz, pad; };          // <B, B>, <R, R>, <R, Z> of a column

template <typename T>
struct PcgState {
	PcgCol* col; int32_t* its; int32_t* frozen; T* R; T* P; T* Z; T* Q; T* W; void* kwork;
};

// What stpy_pcg_lanczos records on top of the solve (all NULL for stpy_pcg): per column and iteration the step length and the direction ratio
// as applied, coef[(c * cap + it - 1) * 2 + {0, 1}], and rz0[c] = <B_c, M^-1 B_c>.  They are the Lanczos coefficients of the preconditioned operator.
struct PcgRec { double* coef; int64_t cap; double* rz0; };

inline int64_t pcg_align(int64_t b) { return (b + 255) / 256 * 256; }

inline int64_t pcg_workspace_bytes(int dtype, int64_t n, int64_t t, int64_t r)
{
	const int64_t esz = dtype == STPY_F32 ? 4 : 8;
	if (n < 1) n = 1;
	if (t < 1) t = 1;
	if (r < 1) r = 1;
	return pcg_align(t * (int64_t)sizeof(PcgCol)) + 2 * pcg_align(t * 4) + 4 * pcg_align(t * n * esz) + pcg_align(t * r * esz) + kmv_workspace_bytes(dtype, t);
}

template <typename T>
inline PcgState<T> pcg_carve(void* work, int64_t n, int64_t t, int64_t r)
{
	char* p = (char*)work;
	PcgState<T> s;
	s.col = (PcgCol*)p; p += pcg_align(t * (int64_t)sizeof(PcgCol));
	s.its = (int32_t*)p; p += pcg_align(t * 4);
	s.frozen = (int32_t*)p; p += pcg_align(t * 4);
	const int64_t vb = pcg_align(t * n * (int64_t)sizeof(T));
	s.R = (T*)p; p += vb;
	s.P = (T*)p; p += vb;
	s.Z = (T*)p; p += vb;
	s.Q = (T*)p; p += vb;
	s.W = (T*)p; p += pcg_align(t * (r < 1 ? 1 : r) * (int64_t)sizeof(T));
	s.kwork = p;
	return s;
}

// X = 0, R = Z = B, the column norms; a zero column (or tol >= 1) starts frozen
template <typename T>
__global__ __launch_bounds__(KP_THREADS)
void pcg_init_kernel(PcgState<T> s, int n, const T* Bt, int64_t ldb, T* Xt, int64_t ldxt, double tol2)
{
	__shared__ double red[4];
	const int c = blockIdx.x;
	const T* B = Bt + (int64_t)c * ldb;
	T* X = Xt + (int64_t)c * ldxt;
	T* R = s.R + (int64_t)c * n;
	T* Z = s.Z + (int64_t)c * n;
	T* P = s.P + (int64_t)c * n;
	double bb = 0.0;
	for (int i = threadIdx.x; i < n; i += KP_THREADS) {
		const T v = B[i];
		X[i] = (T)0; R[i] = v; Z[i] = v; P[i] = (T)0;
		bb += (double)v * (double)v;
	}
	bb = kp_block_sum(bb, red);
	if (threadIdx.x == 0) {
		s.col[c] = PcgCol{bb, bb, 0.0, 0.0};
		s.its[c] = 0;
		s.frozen[c] = (bb <= tol2 * bb) ? 1 : 0;          // (bb == 0, or tol >= 1)
	}
}

// pq = <P, Q>; X += alpha P, R -= alpha Q, Z = R, rr = <R, R>; the column freezes on convergence or on a curvature that is not positive and finite
template <typename T>
__global__ __launch_bounds__(KP_THREADS)
void pcg_step_kernel(PcgState<T> s, int n, T* Xt, int64_t ldxt, double tol2, PcgRec rec)
{
	__shared__ double red[4];
	const int c = blockIdx.x;
	T* R = s.R + (int64_t)c * n;
	T* Z = s.Z + (int64_t)c * n;
	if (s.frozen[c]) {                                                // (workgroup-uniform) Z is the preconditioner's scratch: keep it finite
		for (int i = threadIdx.x; i < n; i += KP_THREADS) Z[i] = R[i];
		return;
	}
	const T* P = s.P + (int64_t)c * n;
	const T* Q = s.Q + (int64_t)c * n;
	T* X = Xt + (int64_t)c * ldxt;
	double pq = 0.0;
	for (int i = threadIdx.x; i < n; i += KP_THREADS) pq += (double)P[i] * (double)Q[i];
	pq = kp_block_sum(pq, red);
	const PcgCol col = s.col[c];
	const int it = s.its[c] + 1;
	if (!(pq > 0.0) || !(pq <= F64_MAX)) {
		for (int i = threadIdx.x; i < n; i += KP_THREADS) Z[i] = R[i];
		if (threadIdx.x == 0) { s.its[c] = -it; s.frozen[c] = 1; }
		return;
	}
	const T alpha = (T)(col.rz / pq);
	if (rec.coef && threadIdx.x == 0 && it <= rec.cap) rec.coef[((int64_t)c * rec.cap + it - 1) * 2] = (double)alpha;
	double rr = 0.0;
	for (int i = threadIdx.x; i < n; i += KP_THREADS) {
		X[i] = pc_fma(alpha, P[i], X[i]);
		const T rv = pc_fma(-alpha, Q[i], R[i]);
		R[i] = rv; Z[i] = rv;
		rr += (double)rv * (double)rv;
	}
	rr = kp_block_sum(rr, red);
	if (threadIdx.x == 0) {
		s.col[c].rr = rr;
		s.its[c] = it;
		if (rr <= tol2 * col.bb) s.frozen[c] = 1;
	}
}

// rz' = <R, Z>; P = Z + (rz' / rz) P (first: P = Z).  A preconditioned residual product that is not positive and finite is flagged like a curvature.
template <typename T>
__global__ __launch_bounds__(KP_THREADS)
void pcg_dir_kernel(PcgState<T> s, int n, int first, PcgRec rec)
{
	__shared__ double red[4];
	const int c = blockIdx.x;
	if (s.frozen[c]) return;
	const T* R = s.R + (int64_t)c * n;
	const T* Z = s.Z + (int64_t)c * n;
	T* P = s.P + (int64_t)c * n;
	double rz = 0.0;
	for (int i = threadIdx.x; i < n; i += KP_THREADS) rz += (double)R[i] * (double)Z[i];
	rz = kp_block_sum(rz, red);
	if (!(rz > 0.0) || !(rz <= F64_MAX)) {
		if (threadIdx.x == 0) { s.its[c] = -(s.its[c] + 1); s.frozen[c] = 1; }
		return;
	}
	const T beta = first ? (T)0 : (T)(rz / s.col[c].rz);
	if (rec.coef && threadIdx.x == 0) {
		const int it = s.its[c];
		if (first) rec.rz0[c] = rz;
		else if (it <= rec.cap) rec.coef[((int64_t)c * rec.cap + it - 1) * 2 + 1] = (double)beta;
	}
	for (int i = threadIdx.x; i < n; i += KP_THREADS) P[i] = pc_fma(beta, P[i], Z[i]);
	__syncthreads();                                                  // (every thread has read the old rz)
	if (threadIdx.x == 0) s.col[c].rz = rz;
}

template <typename T>
__global__ __launch_bounds__(KP_THREADS)
void pcg_finish_kernel(PcgState<T> s, int n, const T* Bt, int64_t ldb, const T* Xt, int64_t ldxt, T* relres, T* bx, int32_t* its)
{
	__shared__ double red[4];
	const int c = blockIdx.x;
	const T* B = Bt + (int64_t)c * ldb;
	const T* X = Xt + (int64_t)c * ldxt;
	double v = 0.0;
	for (int i = threadIdx.x; i < n; i += KP_THREADS) v += (double)B[i] * (double)X[i];
	v = kp_block_sum(v, red);
	if (threadIdx.x == 0) {
		const PcgCol col = s.col[c];
		bx[c] = (T)v;
		relres[c] = col.bb > 0.0 ? (T)sqrt(col.rr / col.bb) : (T)0;
		its[c] = s.its[c];
	}
}

// Z (= R on entry) -= (R Gt^T) Gn^T: the two NT products of M^-1 = I - G G^T
template <typename T>
int pcg_precond(const PcgState<T>& s, int64_t n, int64_t t, int64_t r, const T* Gt, int64_t ldgt, const T* Gn, int64_t ldgn, hipStream_t st)
{
	if (r < 1) return 0;
	int rc = gemm_nt<T>(t, r, n, s.R, n, Gt, ldgt, s.W, r, (T*)nullptr, 0, 0, 0, st);
	if (rc != 0) return rc;
	return gemm_nt<T>(t, n, r, s.W, r, Gn, ldgn, s.Z, n, (T*)nullptr, 0, 1, 0, st);
}

template <typename T>
int pcg(int kind, const T* x, int64_t n, int64_t ldx, int d, const int32_t* cols, const T* inv_ls, double kappa, double diag_add,
        const T* Gt, int64_t ldgt, const T* Gn, int64_t ldgn, int64_t r, const T* Bt, int64_t ldb, T* Xt, int64_t ldxt, int64_t t,
        double tol, int iters, int init, T* relres, T* bx, int32_t* its, void* work, hipStream_t st, PcgRec rec, const char* name)
{
	const PcgState<T> s = pcg_carve<T>(work, n, t, r);
	const dim3 grid((unsigned)t), block(KP_THREADS);
	const double tol2 = tol * tol;
	int rc;
	if (init) {
		hipLaunchKernelGGL(pcg_init_kernel<T>, grid, block, 0, st, s, (int)n, Bt, ldb, Xt, ldxt, tol2);
		if ((rc = pcg_precond<T>(s, n, t, r, Gt, ldgt, Gn, ldgn, st)) != 0) return rc;
		hipLaunchKernelGGL(pcg_dir_kernel<T>, grid, block, 0, st, s, (int)n, 1, rec);
	}
	for (int k = 0; k < iters; ++k) {
		if ((rc = kmv<T>(kind, x, n, ldx, x, n, ldx, d, cols, inv_ls, kappa, diag_add, s.P, t, n, s.Q, n, s.kwork, st)) != 0) return rc;
		hipLaunchKernelGGL(pcg_step_kernel<T>, grid, block, 0, st, s, (int)n, Xt, ldxt, tol2, rec);
		if ((rc = pcg_precond<T>(s, n, t, r, Gt, ldgt, Gn, ldgn, st)) != 0) return rc;
		hipLaunchKernelGGL(pcg_dir_kernel<T>, grid, block, 0, st, s, (int)n, 0, rec);
	}
	hipLaunchKernelGGL(pcg_finish_kernel<T>, grid, block, 0, st, s, (int)n, Bt, ldb, (const T*)Xt, ldxt, relres, bx, its);
	return check_launch(name);
}

}  // namespace

}  // namespace stpy

// ---- C ABI (include/stpy_hip.h); every refusal below comes before the first HIP call
using namespace stpy;

static int pcg_checked(const char* name, int kind, int dtype, const void* x, int64_t n, int64_t ldx, int d, const int32_t* cols, const void* inv_ls,
                       double kappa, double diag_add,
                       const void* Gt, int64_t ldgt, const void* Gn, int64_t ldgn, int64_t r,
                       const void* Bt, int64_t ldb, void* Xt, int64_t ldxt, int64_t t,
                       double tol, int iters, int init,
                       void* relres, void* bx, int32_t* its,
                       void* work, int64_t work_bytes, void* stream, PcgRec rec)
{
	int rc;
	if ((rc = kp_check_stationary(name, kind)) != 0) return rc;
	if (dtype != STPY_F64 && dtype != STPY_F32) { set_error("%s: unknown dtype %d (0 = float64, 1 = float32)", name, dtype); return -2; }
	if (n < 0 || n >= ((int64_t)1 << 31)) { set_error("%s: n=%lld outside [0, 2^31)", name, (long long)n); return -4; }
	if (n == 0) return 0;          // empty problem: nothing to write
	if (d < 1) { set_error("%s: d=%d", name, d); return -6; }
	if (t < 1 || t > 65535) { set_error("%s: t=%lld outside [1, 65535]", name, (long long)t); return -10; }
	if (ldx < d) { set_error("%s: ldx=%lld below d=%d", name, (long long)ldx, d); return -5; }
	if (ldb < n || ldxt < n) { set_error("%s: ldb=%lld or ldxt=%lld below n=%lld", name, (long long)ldb, (long long)ldxt, (long long)n); return -13; }
	if (!is_finite(kappa) || !is_finite(diag_add)) { set_error("%s: kappa=%g and diag_add=%g must be finite", name, kappa, diag_add); return -11; }
	if (!(tol >= 0.0) || !is_finite(tol)) { set_error("%s: tol=%g must be finite and not negative", name, tol); return -14; }
	if (iters < 0) { set_error("%s: iters=%d", name, iters); return -15; }
	if (r < 0 || r >= ((int64_t)1 << 31)) { set_error("%s: r=%lld outside [0, 2^31)", name, (long long)r); return -16; }
	if (r > 0 && (!Gt || !Gn)) { set_error("%s: r=%lld with a null Gt or Gn", name, (long long)r); return -3; }
	if (r > 0 && (ldgt < n || ldgn < r)) { set_error("%s: ldgt=%lld below n=%lld or ldgn=%lld below r=%lld", name, (long long)ldgt, (long long)n, (long long)ldgn, (long long)r); return -18; }
	if (!x || !inv_ls || !Bt || !Xt || !relres || !bx || !its) { set_error("%s: null pointer", name); return -3; }
	if ((rc = kp_check_work(name, work, work_bytes, pcg_workspace_bytes(dtype, n, t, r), 16)) != 0) return rc;
	hipStream_t st = (hipStream_t)stream;
	if (dtype == STPY_F64)
		return pcg<double>(kind, (const double*)x, n, ldx, d, cols, (const double*)inv_ls, kappa, diag_add, (const double*)Gt, ldgt, (const double*)Gn, ldgn, r,
		                   (const double*)Bt, ldb, (double*)Xt, ldxt, t, tol, iters, init, (double*)relres, (double*)bx, its, work, st, rec, name);
	return pcg<float>(kind, (const float*)x, n, ldx, d, cols, (const float*)inv_ls, kappa, diag_add, (const float*)Gt, ldgt, (const float*)Gn, ldgn, r,
	                  (const float*)Bt, ldb, (float*)Xt, ldxt, t, tol, iters, init, (float*)relres, (float*)bx, its, work, st, rec, name);
}

extern "C" {

int64_t stpy_kmv_workspace_bytes(int dtype, int64_t n, int64_t q, int d, int64_t t)
{
	(void)n; (void)q; (void)d;
	return kmv_workspace_bytes(dtype, t);
}

int stpy_kmv(int kind, int dtype, const void* a, int64_t n, int64_t lda, const void* b, int64_t q, int64_t ldb,
             int d, const int32_t* cols, const void* inv_ls, double kappa, double diag_add,
             const void* Vt, int64_t t, int64_t ldv, void* Yt, int64_t ldy, void* work, int64_t work_bytes, void* stream)
{
	const char* name = "stpy_kmv";
	int rc;
	if ((rc = kp_check_stationary(name, kind)) != 0 || (rc = kp_check_sizes(name, dtype, n, q)) != 0) return rc;
	if (n == 0) return 0;          // empty output: nothing to write
	if (d < 1) { set_error("stpy_kmv: d=%d", d); return -6; }
	if (t < 1 || t > (int64_t)65535 * KM_TC) { set_error("stpy_kmv: t=%lld outside [1, %lld]", (long long)t, (long long)65535 * KM_TC); return -10; }
	if ((rc = kp_check_ld_points(name, lda, ldb, d)) != 0) return rc;
	if (ldv < q || ldy < n) { set_error("stpy_kmv: ldv=%lld below q=%lld or ldy=%lld below n=%lld", (long long)ldv, (long long)q, (long long)ldy, (long long)n); return -13; }
	if (!is_finite(kappa) || !is_finite(diag_add)) { set_error("stpy_kmv: kappa=%g and diag_add=%g must be finite", kappa, diag_add); return -11; }
	if (diag_add != 0.0 && q != n) { set_error("stpy_kmv: diag_add=%g needs the same points on both sides, q=%lld != n=%lld", diag_add, (long long)q, (long long)n); return -12; }
	if ((rc = kp_check_pointers(name, a, b, q, inv_ls, Vt, Yt)) != 0 || (rc = kp_check_work(name, work, work_bytes, kmv_workspace_bytes(dtype, t), 8)) != 0) return rc;
	hipStream_t st = (hipStream_t)stream;
	if (dtype == STPY_F64)
		return kmv<double>(kind, (const double*)a, n, lda, (const double*)b, q, ldb, d, cols, (const double*)inv_ls, kappa, diag_add,
		                   (const double*)Vt, t, ldv, (double*)Yt, ldy, work, st);
	return kmv<float>(kind, (const float*)a, n, lda, (const float*)b, q, ldb, d, cols, (const float*)inv_ls, kappa, diag_add,
	                  (const float*)Vt, t, ldv, (float*)Yt, ldy, work, st);
}

int64_t stpy_pcg_workspace_bytes(int dtype, int64_t n, int d, int64_t t, int64_t r)
{
	(void)d;
	return pcg_workspace_bytes(dtype, n, t, r);
}

int stpy_pcg(int kind, int dtype, const void* x, int64_t n, int64_t ldx, int d, const int32_t* cols, const void* inv_ls,
             double kappa, double diag_add,
             const void* Gt, int64_t ldgt, const void* Gn, int64_t ldgn, int64_t r,
             const void* Bt, int64_t ldb, void* Xt, int64_t ldxt, int64_t t,
             double tol, int iters, int init,
             void* relres, void* bx, int32_t* its,
             void* work, int64_t work_bytes, void* stream)
{
	return pcg_checked("stpy_pcg", kind, dtype, x, n, ldx, d, cols, inv_ls, kappa, diag_add, Gt, ldgt, Gn, ldgn, r, Bt, ldb, Xt, ldxt, t, tol, iters, init,
	                   relres, bx, its, work, work_bytes, stream, PcgRec{nullptr, 0, nullptr});
}

int stpy_pcg_lanczos(int kind, int dtype, const void* x, int64_t n, int64_t ldx, int d, const int32_t* cols, const void* inv_ls,
                     double kappa, double diag_add,
                     const void* Gt, int64_t ldgt, const void* Gn, int64_t ldgn, int64_t r,
                     const void* Bt, int64_t ldb, void* Xt, int64_t ldxt, int64_t t,
                     double tol, int iters, int init,
                     void* relres, void* bx, int32_t* its,
                     double* coef, int64_t cap, double* rz0,
                     void* work, int64_t work_bytes, void* stream)
{
	if (cap < 1) { set_error("stpy_pcg_lanczos: cap=%lld", (long long)cap); return -19; }
	if (!coef || !rz0) { set_error("stpy_pcg_lanczos: null coef or rz0"); return -3; }
	return pcg_checked("stpy_pcg_lanczos", kind, dtype, x, n, ldx, d, cols, inv_ls, kappa, diag_add, Gt, ldgt, Gn, ldgn, r, Bt, ldb, Xt, ldxt, t, tol, iters, init,
	                   relres, bx, its, work, work_bytes, stream, PcgRec{coef, cap, rz0});
}

}  // extern "C"
