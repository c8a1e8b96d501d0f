"""
NumPy oracle of the stochastic evidence of IterativeGaussianProcess (stpy_pcg_lanczos, stpy_kmv_dtheta, log_marginal_estimate): the probes,
the block PCG of tests/kmv_oracle.py restated with its coefficients recorded, the Lanczos matrix T_c and the quadrature q_c, the dense
counterparts of q_c and of u^T (dA/dtheta) v, and the dense bilinear forms of stpy_kmv_dtheta in longdouble with their error bound.  Nothing
here touches the GPU or the library.

Notation: A = K + s^2 I, F the rank-r pivoted-Cholesky factor, G = F L^-T with L L^T = s^2 I + F^T F, M^-1 = I - G G^T = s^2 (s^2 I + F F^T)^-1.
Probes z_c = w1_c + F w2_c / s have covariance M.  With m = its[c], a_j / b_j the step lengths / direction ratios of the solve of z_c and
rz0_c = <z_c, M^-1 z_c>:  T_c tridiagonal, T[0,0] = 1/a_1, T[j,j] = 1/a_(j+1) + b_j/a_j, T[j,j+1] = sqrt(b_(j+1))/a_(j+1), eigenpairs (theta, v);
    q_c = rz0_c sum_l v_l[0]^2 (log theta_l - log s^2),      logdet A ~= mean_c q_c + (n - r) log s^2 + 2 sum log L_ll.
Gradient: tr(A^-1 dA) = E[u^T dA v], u = A^-1 z, v = M^-1 z, with the control variate b = v^T dA v / s^2 whose expectation is known exactly:
E[b] = tr(P^-1 dA) = (tr(dA) - sum_l g_l^T dA g_l) / s^2 with P = s^2 I + F F^T = s^2 M (g_l the columns of G; tr(dK/dgamma) = 0).  Where the
preconditioner is exact a_c = b_c and the random part vanishes, as it does in the value; where it is weak the fitted coefficient goes to 0
and the plain estimator is left.  Without it the gradient keeps a standard error of order 1 where the value's is 1e-11, and an optimiser that
is handed both stalls (case 3 at gamma = 0.84, t = 16: trace term -23.1 +- 3.6 plain, -18.6181 +- 1e-12 with it, exact -18.6181; with a fixed
coefficient 1 instead of the fitted one the standard error at the case's own gamma = 0.05 grows from 12 to 450).
"""
import numpy as np
import scipy.linalg as sla

from tests import kmv_oracle as KO
from tests import nystrom_oracle as NO

SQRT3, SQRT5 = NO.SQRT3, NO.SQRT5

# Deviation, relative to the float64 figure, of this oracle's float32 restatement of the estimate on case 4 (se, n = 129, d = 2, s = 0.3,
# tol = 1e-4, t = 16 probes from RandomState(104), float32-rounded data) from its float64 one solved to 1e-8: (value, gradient w.r.t. gamma,
# gradient w.r.t. s).  It holds the float32 rounding AND what stopping at 1e-4 leaves.  Measured 4.28e-7, 7.44e-6 and 2.16e-7 by
# tests/test_slq_cpu.py::test_float32_restatement_constant, which re-checks the figures to a factor 5 either way (the float32 sums depend on the
# BLAS at hand); the GPU test allows the device 10x these.
F32_RESTATEMENT_DEVIATION = (4.3e-7, 7.4e-6, 2.2e-7)


# ------------------------------------------------------------------------------------------------------------ probes and the solve
def probes(n, r, t, seed):
	"""(t, n + r) standard normal draws: columns [0, n) are w1, the next r are w2."""
	return np.random.RandomState(seed).standard_normal((t, n + r))


def factor(kind, x, gamma, s, r, cols=None, dtype=np.float64, kappa=1.0):
	"""(F (n, rank), G (n, rank), sum log L_ll) of the rank <= r preconditioner in ``dtype``; r == 0: (n x 0 matrices, 0)."""
	n = x.shape[0]
	if r < 1:
		return np.zeros((n, 0), dtype=dtype), None, 0.0
	_, Ft, _, rank = NO.pivoted_cholesky(kind, np.asarray(x, dtype=dtype), gamma, r, kappa=kappa, cols=cols, dtype=dtype)
	Ft = Ft[:rank]
	C = (Ft @ Ft.T + dtype(s * s) * np.eye(rank, dtype=dtype)).astype(dtype)
	L = np.linalg.cholesky(C).astype(dtype)
	G = sla.solve_triangular(L, Ft, lower=True).T.astype(dtype)
	return Ft.T.copy(), G, float(np.sum(np.log(np.diag(L).astype(np.float64))))


def probe_vectors(W, F, s):
	"""z (n, t): z_c = w1_c + F w2_c / s."""
	n, r = F.shape
	W = np.asarray(W, dtype=F.dtype)
	return (W[:, :n].T + (F @ W[:, n:n + r].T) / F.dtype.type(s)).astype(F.dtype)


def minv(G, R):
	return R if G is None else R - G @ (G.T @ R)


def pcg_coef(A, B, tol, maxiter, G=None, dtype=np.float64):
	"""kmv_oracle.pcg with what stpy_pcg_lanczos records: returns (X, its, relres, coef (t, maxiter, 2), rz0 (t,)).  coef[c, it-1, 0] is the
	step length of iteration it, coef[c, it-1, 1] the ratio applied to the direction after it (not written once the column is frozen);
	untouched slots hold NaN."""
	A = np.asarray(A, dtype=dtype)
	B = np.asarray(B, dtype=dtype)
	n, t = B.shape
	X = np.zeros((n, t), dtype=dtype)
	R = B.copy()
	bb = np.sum(B * B, axis=0)
	rr = bb.copy()
	its = np.zeros(t, dtype=np.int64)
	coef = np.full((t, maxiter, 2), np.nan)
	frozen = rr <= dtype(tol) ** 2 * bb
	Z = minv(G, R).astype(dtype)
	P = Z.copy()
	rz = np.sum(R * Z, axis=0)
	rz0 = rz.astype(np.float64).copy()
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
		coef[act, it - 1, 0] = alpha[act]
		X = (X + alpha * P).astype(dtype)
		R = (R - alpha * Q).astype(dtype)
		its[act] = it
		rr = np.where(act, np.sum(R * R, axis=0), rr)
		frozen = frozen | (act & (rr <= dtype(tol) ** 2 * bb))
		Z = minv(G, R).astype(dtype)
		rz_new = np.sum(R * Z, axis=0)
		go = ~frozen
		beta = np.zeros(t, dtype=dtype)
		beta[go] = rz_new[go] / rz[go]
		coef[go, it - 1, 1] = beta[go]
		P = np.where(go, Z + beta * P, P).astype(dtype)
		rz = np.where(go, rz_new, rz)
	relres = np.where(bb > 0, np.sqrt(rr / np.where(bb > 0, bb, 1)), 0)
	return X, its, relres, coef, rz0


# ------------------------------------------------------------------------------------------------------------ quadrature
def lanczos_matrix(coef_c, m):
	"""(diagonal (m,), off-diagonal (m - 1,)) of T_c from the first m slots of a column's coefficients."""
	a = np.asarray(coef_c[:m, 0], dtype=np.float64)
	b = np.asarray(coef_c[:m - 1, 1], dtype=np.float64)
	dg = 1.0 / a
	dg[1:] += b / a[:-1]
	return dg, np.sqrt(b) / a[:-1]


def q_from_coef(coef, its, rz0, s):
	"""q_c for every column from recorded coefficients (its > 0 everywhere)."""
	q = np.zeros(len(its))
	for c, m in enumerate(its):
		dg, off = lanczos_matrix(coef[c], int(m))
		theta, V = sla.eigh_tridiagonal(dg, off, lapack_driver="stev") if m > 1 else (dg, np.ones((1, 1)))
		q[c] = rz0[c] * np.sum(V[0] ** 2 * (np.log(theta) - np.log(s * s)))
	return q


def q_dense(A, G, Z, s):
	"""The dense counterpart of q_c for the columns of Z: w^T [log(M^-1/2 A M^-1/2) - log s^2 I] w with w = M^-1/2 z, in float64."""
	n = A.shape[0]
	Mi = np.eye(n) if G is None else np.eye(n) - G @ G.T
	ev, V = np.linalg.eigh((Mi + Mi.T) / 2)
	Mh = (V * np.sqrt(ev)) @ V.T
	Bm = Mh @ A @ Mh
	th, U = np.linalg.eigh((Bm + Bm.T) / 2)
	Wc = U.T @ (Mh @ Z)
	return np.sum(Wc * Wc * (np.log(th) - np.log(s * s))[:, None], axis=0)


def logdet_constant(n, rank, s, sumlogL):
	"""log det(s^2 I + F F^T) = (n - r) log s^2 + 2 sum log L_ll."""
	return (n - rank) * np.log(s * s) + 2.0 * sumlogL


# ------------------------------------------------------------------------------------------------------------ dense derivative forms
def _chi(kind, rho):
	"""chi = 2 dphi/drho in rho's dtype; the value at rho == 0 is not used (the caller masks it)."""
	dt = rho.dtype.type
	with np.errstate(divide="ignore", invalid="ignore"):
		if kind == "se":
			return -np.exp(dt(-0.5) * rho)
		r = np.sqrt(rho)
		if kind == "matern12":
			return -np.exp(-r) / r
		if kind == "matern32":
			return dt(-3) * np.exp(-r * dt(SQRT3))
		if kind == "matern52":
			r5 = r * dt(SQRT5)
			return dt(-5.0) / dt(3.0) * (dt(1) + r5) * np.exp(-r5)
	raise ValueError(kind)


def kmv_dtheta_dense(kind, x, inv_ls, U, V, cols=None, kappa=1.0, dtype=np.longdouble, block=256):
	"""stpy_kmv_dtheta stated densely in ``dtype`` (subtract first, then scale): (out (t, d + 2), S0 (t, d), S1 (t, d), SK (t,), SD (t,)).
	U, V: (t, n).  S0[c, k] = sum_ij |U_ci| |V_cj| kappa |chi_ij| e_ijk^2, S1 the same sum weighted by (1 + rho_ij), SK = sum |U| |K| |V|,
	SD = sum_i |U_ci V_ci|: what the error bounds are made of (float64; only the values themselves need ``dtype``)."""
	x = np.asarray(x, dtype=dtype)
	if cols is not None:
		x = x[:, list(cols)]
	il = np.asarray(inv_ls, dtype=dtype)
	U = np.asarray(U, dtype=dtype)
	V = np.asarray(V, dtype=dtype)
	t, n = U.shape
	d = x.shape[1]
	kap = dtype(kappa)
	out = np.zeros((t, d + 2), dtype=dtype)
	S0 = np.zeros((t, d))
	S1 = np.zeros((t, d))
	SK = np.zeros((t,))
	aU, aV = np.abs(U).astype(np.float64), np.abs(V).astype(np.float64)
	for i0 in range(0, n, block):
		e = (x[i0:i0 + block, None, :] - x[None, :, :]) * il                      # (b, n, d)
		rho = np.zeros(e.shape[:2], dtype=dtype)
		for k in range(d):
			rho = e[:, :, k] * e[:, :, k] + rho
		Kb = kap * NO._phi(kind, rho)
		wc = np.where(rho == 0, dtype(0), kap * _chi(kind, rho))
		Ub, aUb = U[:, i0:i0 + block], aU[:, i0:i0 + block]
		form = lambda L, Mx, R: np.sum((L @ Mx) * R, axis=1)                      # sum_ij L_ci M_ij R_cj
		out[:, d] += form(Ub, Kb, V)
		SK += form(aUb, np.abs(Kb).astype(np.float64), aV)
		rho1 = 1 + rho.astype(np.float64)
		for k in range(d):
			Bk = wc * (e[:, :, k] * e[:, :, k])
			out[:, k] += form(Ub, Bk, V)
			aB = np.abs(Bk).astype(np.float64)
			S0[:, k] += form(aUb, aB, aV)
			S1[:, k] += form(aUb, aB * rho1, aV)
	out[:, d + 1] = np.sum(U * V, axis=1)
	return out, S0, S1, SK, np.sum(aU * aV, axis=1)


def kmv_dtheta_bound(n, d, eps, S0, S1, SK, SD):
	"""(t, d + 2) bound on |device - truth|.  Derivative columns: eps [(d + 12) S1 + 2 (n + 8) S0] -- each e_k carries 2 eps, rho (d + 4) eps,
	chi the relative error of rho times |dlog chi / dlog rho| <= (1 + rho) for all four kinds plus a few eps of exp / sqrt / division, the
	product kappa chi e_k^2 and the multiplication by U a few more: (d + 12) (1 + rho) eps per term; the sums over j (MFMA chain), over i and
	over the partial rows add 2 (n + 8) eps.  Value column: the stpy_kmv bound 2 eps (n + d + 8) SK.  Last column: a dot product, 2 eps n SD."""
	t = S0.shape[0]
	b = np.zeros((t, d + 2))
	b[:, :d] = eps * ((d + 12) * S1 + 2 * (n + 8) * S0)
	b[:, d] = 2 * eps * (n + d + 8) * SK
	b[:, d + 1] = 2 * eps * n * SD
	return b


def kmv_dtheta_emulated(kind, x, inv_ls, U, V, dtype, cols=None, kappa=1.0):
	"""The subtract-first evaluation with every operation rounded to the working ``dtype`` (what the device does, up to summation order)."""
	return kmv_dtheta_dense(kind, np.asarray(x, dtype=dtype), np.asarray(inv_ls, dtype=dtype), np.asarray(U, dtype=dtype), np.asarray(V, dtype=dtype),
							cols=cols, kappa=kappa, dtype=dtype)[0]


def dK_dloggamma(kind, x, gamma, cols=None, kappa=1.0):
	"""Dense dK/dlog gamma_k for each coordinate read, (d, n, n) in float64: -kappa chi e_k^2."""
	xs = np.asarray(x, dtype=np.float64)
	if cols is not None:
		xs = xs[:, list(cols)]
	d = xs.shape[1]
	il = np.ones(d) / np.asarray(gamma, dtype=np.float64)
	e = (xs[:, None, :] - xs[None, :, :]) * il
	rho = np.sum(e * e, axis=2)
	wc = np.where(rho == 0, 0.0, kappa * _chi(kind, rho))
	return np.stack([-wc * e[:, :, k] ** 2 for k in range(d)])


# ------------------------------------------------------------------------------------------------------------ the whole estimate
def exact(kind, x, y, gamma, s, cols=None, kappa=1.0, weight=1.0):
	"""Exact float64 value 1/2 y^T A^-1 y + 1/2 weight logdet A, logdet, and the gradient w.r.t. log gamma_k (d,) and s."""
	n = x.shape[0]
	A = NO.kernel(kind, x, x, gamma, kappa, cols) + s * s * np.eye(n)
	c = sla.cho_factor(A, lower=True)
	alpha = sla.cho_solve(c, y.reshape(-1, 1))[:, 0]
	logdet = 2.0 * np.sum(np.log(np.diag(c[0])))
	Ai = sla.cho_solve(c, np.eye(n))
	dK = dK_dloggamma(kind, x, gamma, cols, kappa)
	g = np.array([-0.5 * alpha @ D @ alpha + 0.5 * weight * np.sum(Ai * D) for D in dK])
	gs = -0.5 * 2 * s * (alpha @ alpha) + 0.5 * weight * 2 * s * np.trace(Ai)
	return dict(value=0.5 * float(y.reshape(-1) @ alpha) + 0.5 * weight * logdet, logdet=logdet, grad_loggamma=g, grad_s=gs, A=A, alpha=alpha,
				trace_terms=np.array([np.sum(Ai * D) for D in dK]))


def estimate(kind, x, y, gamma, s, r, W, tol, cols=None, kappa=1.0, weight=1.0, dtype=np.float64, maxiter=5000):
	"""The estimate as the class computes it, in ``dtype`` (tridiagonal eigenproblems and final scalars in float64), on the probes W
	(t, n + r'): r' >= the rank found; the first ``rank`` columns after n are used.  gamma: scalar or per-coordinate vector.
	Returns a dict: value, stderr, logdet, logdet_stderr, q (t,), grad_loggamma (d,), grad_loggamma_stderr, grad_s, grad_s_stderr, its,
	and the pieces A, G, Z (float64 views of what was solved) for the dense checks."""
	n = x.shape[0]
	dsel = len(cols) if cols is not None else x.shape[1]
	gam = np.ones(dsel) * np.asarray(gamma, dtype=np.float64)
	F, G, sumlogL = factor(kind, x, gam, s, r, cols=cols, dtype=dtype, kappa=kappa)
	rank = F.shape[1]
	Z = probe_vectors(np.asarray(W)[:, :n + rank], F, s)
	A = (NO.kernel(kind, x, x, gam, kappa, cols, dtype=dtype) + dtype(s * s) * np.eye(n, dtype=dtype)).astype(dtype)
	B = np.concatenate([np.asarray(y, dtype=dtype).reshape(-1, 1), Z], axis=1)
	X, its, relres, coef, rz0 = pcg_coef(A, B, tol, maxiter, G=G, dtype=dtype)
	assert np.all(its > 0) and np.all(relres <= tol)
	t = Z.shape[1]
	q = q_from_coef(coef[1:], its[1:], rz0[1:], s)
	logdet = q.mean() + logdet_constant(n, rank, s, sumlogL)
	alpha = X[:, 0].astype(np.float64)
	Vc = minv(G, Z).astype(np.float64)
	Uc = X[:, 1:].astype(np.float64)
	G64 = np.zeros((n, 0)) if G is None else G.astype(np.float64)
	dK = dK_dloggamma(kind, x, gam, cols, kappa)
	if np.ndim(gamma) == 0:
		dK = dK.sum(axis=0, keepdims=True)                                                 # ONE lengthscale: one parameter
	ga = [control_variate(np.array([Uc[:, c] @ D @ Vc[:, c] for c in range(t)]), np.array([Vc[:, c] @ D @ Vc[:, c] for c in range(t)]) / (s * s),
						  -np.sum(G64 * (D @ G64)) / (s * s)) for D in dK]
	aa = np.array([alpha @ D @ alpha for D in dK])
	gs = control_variate(2 * s * np.sum(Uc * Vc, axis=0), 2 * s * np.sum(Vc * Vc, axis=0) / (s * s), 2 * s * (n - np.sum(G64 * G64)) / (s * s))
	se = lambda v: float(np.std(v, ddof=1) / np.sqrt(len(v)))
	return dict(value=0.5 * float(np.asarray(y, dtype=np.float64).reshape(-1) @ alpha) + 0.5 * weight * logdet, stderr=0.5 * weight * se(q),
				logdet=logdet, logdet_stderr=se(q), q=q, its=its, rank=rank,
				grad_loggamma=-0.5 * aa + 0.5 * weight * np.array([g[0] for g in ga]), grad_loggamma_stderr=0.5 * weight * np.array([g[1] for g in ga]),
				trace_terms=np.array([g[0] for g in ga]), trace_stderr=np.array([g[1] for g in ga]), beta=np.array([g[2] for g in ga]),
				grad_s=-0.5 * 2 * s * (alpha @ alpha) + 0.5 * weight * gs[0], grad_s_stderr=0.5 * weight * gs[1],
				A=A.astype(np.float64), G=None if G is None else G.astype(np.float64), Z=Z.astype(np.float64), U=Uc, V=Vc, alpha=alpha,
				coef=coef, rz0=rz0, sumlogL=sumlogL, dK=dK)


def control_variate(a, b, Eb):
	"""(estimate, standard error, beta) of E[a] from paired samples a_c, b_c with E[b] = Eb known: the regression estimator
	mean(a) + beta (Eb - mean(b)), beta = cov(a, b) / var(b) from the samples (0 with fewer than 4 samples or a constant b); standard error =
	the residual standard deviation (two fitted constants) / sqrt(t).  Here a_c = u_c^T dA v_c and b_c = v_c^T dA v_c / s^2."""
	t = len(a)
	vb = np.var(b, ddof=1) if t >= 4 else 0.0
	beta = float(np.cov(a, b)[0, 1] / vb) if vb > 0 else 0.0
	res = a - beta * b
	return float(a.mean() + beta * (Eb - b.mean())), float(np.std(res, ddof=2 if beta != 0.0 else 1) / np.sqrt(t)), beta


def case_estimate(idx, t=16, dtype_name="float64", seed=None, weight=1.0):
	"""``estimate`` on PCG case idx of tests/kmv_oracle.py with the settings of its dtype and probes from RandomState(100 + idx)."""
	kind, n, d, gamma, r, cols = KO.PCG_CASES[idx]
	dtype = np.float64 if dtype_name == "float64" else np.float32
	s, tol = KO.SETTINGS[dtype_name]
	x, y, _ = KO.case_data(idx, dtype)
	W = probes(n, r, t, 100 + idx if seed is None else seed)
	return estimate(kind, x, y, gamma, s, r, W, tol, cols=cols, weight=weight, dtype=dtype), (kind, x, y, gamma, s, r, cols, W, tol)
