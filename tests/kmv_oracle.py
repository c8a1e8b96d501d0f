"""
NumPy oracle of the matrix-free route (stpy_kmv, stpy_pcg, IterativeGaussianProcess): the dense product with its per-entry error bound, the
pivoted-Cholesky preconditioner M^-1 = I - G G^T, a restatement of the block preconditioned CG in float64 or float32, and the dense
posterior with the error bounds a CG solve of relative residual tol leaves on it.  Kernel values are those of tests/nystrom_oracle.py
(direct coordinate differences in the working dtype); nothing here touches the GPU or the library.
"""
import numpy as np
import scipy.linalg as sla

from tests import nystrom_oracle as NO

KIND_CODE = {"se": 0, "matern12": 1, "matern32": 2, "matern52": 3}
WIDE_COLS = [6, 1, 3, 0, 5]
# (kind, n, d, gamma, preconditioner rank, coordinates read from a wider x or None)
PCG_CASES = [
	("se", 777, 2, 0.35, 33, None),
	("matern52", 2500, 3, 0.25, 130, None),
	("matern12", 1000, 5, 0.8, 40, WIDE_COLS),
	("se", 300, 1, 0.05, 24, None),
	("se", 129, 2, 0.5, 16, None),
	("matern32", 1500, 4, 0.6, 64, None),
]
PCG_IDS = ["%s-n%d" % (c[0], c[1]) for c in PCG_CASES]
# dtype name -> (noise s, CG tolerance)
SETTINGS = {"float64": (0.1, 1e-8), "float32": (0.3, 1e-4)}
N_KSTAR = 5


def eps_of(dtype):
	return float(np.finfo(dtype).eps)


def kmv_bound(kind, a, b, gamma, V, cols=None, kappa=1.0):
	"""(K V in float64 as (|a|, t), the per-entry bound 2 eps-free factor (|K| |V|)): the caller multiplies by 2 eps (q + d + 8)."""
	K = NO.kernel(kind, a, b, gamma, kappa, cols)
	return K @ V, np.abs(K) @ np.abs(V)


def case_data(idx, dtype=np.float64, m_test=N_KSTAR):
	"""Points, targets and test points of a PCG case: uniform(-1, 1) from a fixed seed; float32 runs get the float32-rounded values (returned
	as float64 arrays holding them, so that the float64 checks see the same problem)."""
	kind, n, d, gamma, r, cols = PCG_CASES[idx]
	rng = np.random.RandomState(7300 + idx)
	width = 8 if cols else d
	x = rng.uniform(-1, 1, size=(n, width))
	xt = rng.uniform(-1, 1, size=(m_test, width))
	w = rng.uniform(-1, 1, size=(width,))
	y = np.sin(3.0 * x @ w) + 0.1 * rng.standard_normal(n)
	if np.dtype(dtype) == np.float32:
		x, xt, y = (v.astype(np.float32).astype(np.float64) for v in (x, xt, y))
	return x, y.reshape(-1, 1), xt


def rhs(idx, dtype=np.float64):
	"""(n, 1 + N_KSTAR) right-hand sides of a case in float64: y and five columns k(x, xt_j)."""
	kind, n, d, gamma, r, cols = PCG_CASES[idx]
	x, y, xt = case_data(idx, dtype)
	return np.concatenate([y, NO.kernel(kind, x, xt, gamma, cols=cols)], axis=1)


def preconditioner(kind, x, gamma, s, r, cols=None, dtype=np.float64, kappa=1.0):
	"""G (n, rank) with (s^2 I + F F^T)^-1 = (I - G G^T) / s^2, F the greedy pivoted-Cholesky factor of rank <= r: G = F L^-T, L L^T = s^2 I + F^T F."""
	if r < 1:
		return None
	_, Ft, _, rank = NO.pivoted_cholesky(kind, np.asarray(x, dtype=dtype), gamma, r, kappa=kappa, cols=cols, dtype=dtype)
	Ft = Ft[:rank]
	C = (Ft @ Ft.T + dtype(s * s) * np.eye(rank, dtype=dtype)).astype(dtype)
	L = np.linalg.cholesky(C).astype(dtype)
	return sla.solve_triangular(L, Ft, lower=True).T.astype(dtype)          # (L^-1 F^T)^T = F L^-T


def pcg(A, B, tol, maxiter, G=None, dtype=np.float64):
	"""Block preconditioned CG as stpy_pcg states it, all arithmetic in ``dtype``: per column, X = 0, R = B, Z = R - G (G^T R), P = Z; then
	alpha = <R, Z> / <P, A P>, X += alpha P, R -= alpha A P, frozen once |R| <= tol |B| (recurrence residual) or on a curvature that is not
	positive and finite (its = -(iteration)).  Returns (X, its, relres)."""
	A = np.asarray(A, dtype=dtype)
	B = np.asarray(B, dtype=dtype)
	n, t = B.shape

	def minv(R):
		return R if G is None else (R - G @ (G.T @ R)).astype(dtype)
	X = np.zeros((n, t), dtype=dtype)
	R = B.copy()
	bb = np.sum(B * B, axis=0)
	rr = bb.copy()
	its = np.zeros(t, dtype=np.int64)
	frozen = rr <= dtype(tol) ** 2 * bb
	Z = minv(R)
	P = Z.copy()
	rz = np.sum(R * Z, axis=0)
	for it in range(1, maxiter + 1):
		if frozen.all():
			break
		Q = (A @ P).astype(dtype)
		pq = np.sum(P * Q, axis=0)
		bad = ~frozen & ~((pq > 0) & np.isfinite(pq))
		its[bad] = -it
		frozen = frozen | bad
		act = ~frozen
		alpha = np.zeros(t, dtype=dtype)
		alpha[act] = rz[act] / pq[act]
		X = (X + alpha * P).astype(dtype)
		R = (R - alpha * Q).astype(dtype)
		its[act] = it
		rr = np.where(act, np.sum(R * R, axis=0), rr)
		frozen = frozen | (act & (rr <= dtype(tol) ** 2 * bb))
		Z = minv(R)
		rz_new = np.sum(R * Z, axis=0)
		go = ~frozen
		beta = np.zeros(t, dtype=dtype)
		beta[go] = rz_new[go] / rz[go]
		P = np.where(go, Z + beta * P, P).astype(dtype)
		rz = np.where(go, rz_new, rz)
	relres = np.where(bb > 0, np.sqrt(rr / np.where(bb > 0, bb, 1)), 0)
	return X, its, relres


def true_relres(A64, B64, X):
	"""|B - A X| / |B| per column in float64 (0 for a zero column)."""
	res = np.linalg.norm(B64 - A64 @ np.asarray(X, dtype=np.float64), axis=0)
	nb = np.linalg.norm(B64, axis=0)
	return np.where(nb > 0, res / np.where(nb > 0, nb, 1), 0)


_ORACLE = {}


def oracle_run(idx, dtype_name):
	"""The oracle's own solve of a case, preconditioned and plain, computed once: dict(A64, B64, G, X, its, its_plain, true, true_plain, cond)."""
	key = (idx, dtype_name)
	if key not in _ORACLE:
		dtype = np.float64 if dtype_name == "float64" else np.float32
		kind, n, d, gamma, r, cols = PCG_CASES[idx]
		s, tol = SETTINGS[dtype_name]
		x, y, xt = case_data(idx, dtype)
		A64 = NO.kernel(kind, x, x, gamma, cols=cols) + s * s * np.eye(n)
		B64 = rhs(idx, dtype)
		A = (NO.kernel(kind, x, x, gamma, cols=cols, dtype=dtype) + dtype(s * s) * np.eye(n, dtype=dtype)).astype(dtype)
		G = preconditioner(kind, x, gamma, s, r, cols=cols, dtype=dtype)
		X, its, _ = pcg(A, B64, tol, 5000, G=G, dtype=dtype)
		Xp, itsp, _ = pcg(A, B64, tol, 5000, G=None, dtype=dtype)
		_ORACLE[key] = dict(A64=A64, B64=B64, G=G, X=X, its=its, its_plain=itsp, true=true_relres(A64, B64, X), true_plain=true_relres(A64, B64, Xp),
							x=x, y=y, xt=xt, s=s, tol=tol)
	return _ORACLE[key]


def posterior(kind, x, y, xt, gamma, s, cols=None, kappa=1.0):
	"""Dense float64 posterior: (mu (M, 1), var (M, 1), W = A^-1 K* (n, M), Ks (n, M), A)."""
	n = x.shape[0]
	A = NO.kernel(kind, x, x, gamma, kappa, cols) + s * s * np.eye(n)
	Ks = NO.kernel(kind, x, xt, gamma, kappa, cols)
	c = sla.cho_factor(A, lower=True)
	alpha = sla.cho_solve(c, y)
	W = sla.cho_solve(c, Ks)
	mu = Ks.T @ alpha
	var = kappa - np.sum(Ks * W, axis=0).reshape(-1, 1)
	return mu, var, W, Ks, A


def posterior_bounds(kind, x, y, xt, gamma, s, tol, eps, cols=None, kappa=1.0):
	"""Per-test-point bounds on |mu - mu*| and |var - var*| of a CG route whose solves have TRUE relative residual <= 2 tol, in arithmetic of
	unit roundoff eps.  With alpha~ = alpha + A^-1 e, |e| <= 2 tol |y|:  |k*_i^T (alpha~ - alpha)| = |(A^-1 k*_i)^T e| <= |A^-1 k*_i| 2 tol |y|,
	plus the product's own bound 2 eps (n + d + 8) sum_j |k*_ij| |alpha_j|.  The variance term <k*_i, w~_i>: the same with |k*_i| for |y|, plus
	the dot-product bound 2 eps n sum |k*_i| |w_i|."""
	mu, var, W, Ks, A = posterior(kind, x, y, xt, gamma, s, cols, kappa)
	n = x.shape[0]
	d = len(cols) if cols else x.shape[1]
	alpha = np.linalg.solve(A, y)
	wn = np.linalg.norm(W, axis=0)
	b_mu = wn * 2 * tol * np.linalg.norm(y) + 2 * eps * (n + d + 8) * (np.abs(Ks).T @ np.abs(alpha))[:, 0]
	b_var = wn * 2 * tol * np.linalg.norm(Ks, axis=0) + 2 * eps * (n + d + 8) * np.sum(np.abs(Ks) * np.abs(W), axis=0) + 2 * eps * n * np.sum(np.abs(Ks) * np.abs(W), axis=0)
	return mu, var, b_mu.reshape(-1, 1), b_var.reshape(-1, 1)
