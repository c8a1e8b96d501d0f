"""
NumPy oracle of the matrix-free input gradients and pathwise samples (stpy_kmv_dx, IterativeGaussianProcess.mean_value_grad / sample_paths /
sample_and_optimize): the dense statement of stpy_kmv_dx in longdouble with its per-entry error bound and a working-precision emulation,
the dense pathwise (Matheron) draw from given standard normal draws with its analytic gradient, the exact mean and the
exact-for-the-drawn-basis variance of that draw, and a bound on the distance between a device path and the oracle's.  Kernel values are those
of tests/nystrom_oracle.py (direct coordinate differences); nothing here touches the GPU or the library.
"""
import numpy as np
import scipy.linalg as sla

from tests import nystrom_oracle as NO
from tests import slq_oracle as SO

TWO_NU = {"se": None, "matern12": 1, "matern32": 3, "matern52": 5}


# ------------------------------------------------------------------------------------------------------------ stpy_kmv_dx
def kmv_dx_dense(kind, a, b, inv_ls, V, cols=None, kappa=1.0, dtype=np.longdouble, block=128):
	"""stpy_kmv_dx stated densely in ``dtype`` (subtract first, then scale): (out (t, n, d + 1), S0 (t, n, d), S1 (t, n, d), SK (t, n)).
	a: (n, .) query points, b: (q, .) contracted points, V: (t, q).  out[c, i, k] = inv_ls[k] sum_j V_cj kappa chi_ij e_ijk (pairs with
	rho == 0 left out), out[c, i, d] = sum_j V_cj kappa phi_ij.  S0[c, i, k] = inv_ls[k] sum_j |V_cj| kappa |chi_ij| |e_ijk|, S1 the same sum
	weighted by (1 + rho_ij), SK[c, i] = sum_j |K_ij| |V_cj|: what the error bounds are made of (float64)."""
	a = np.asarray(a, dtype=dtype)
	b = np.asarray(b, dtype=dtype)
	if cols is not None:
		a, b = a[:, list(cols)], b[:, list(cols)]
	il = np.asarray(inv_ls, dtype=dtype)
	V = np.asarray(V, dtype=dtype)
	t, q = V.shape
	n, d = a.shape
	kap = dtype(kappa)
	out = np.zeros((t, n, d + 1), dtype=dtype)
	S0, S1, SK = np.zeros((t, n, d)), np.zeros((t, n, d)), np.zeros((t, n))
	aV = np.abs(V).astype(np.float64)
	il64 = il.astype(np.float64)
	for i0 in range(0, n, block):
		e = (a[i0:i0 + block, None, :] - b[None, :, :]) * il                          # (bl, q, d)
		rho = np.zeros(e.shape[:2], dtype=dtype)
		for k in range(d):
			rho = e[:, :, k] * e[:, :, k] + rho
		Kb = kap * NO._phi(kind, rho)
		wc = np.where(rho == 0, dtype(0), kap * SO._chi(kind, rho)) if q else np.zeros(rho.shape, dtype=dtype)
		sl = slice(i0, i0 + block)
		out[:, sl, d] = V @ Kb.T
		SK[:, sl] = aV @ np.abs(Kb).astype(np.float64).T
		rho1 = 1 + rho.astype(np.float64)
		for k in range(d):
			Bk = wc * e[:, :, k]
			out[:, sl, k] = il[k] * (V @ Bk.T)
			aB = np.abs(Bk).astype(np.float64)
			S0[:, sl, k] = il64[k] * (aV @ aB.T)
			S1[:, sl, k] = il64[k] * (aV @ (aB * rho1).T)
	return out, S0, S1, SK


def kmv_dx_bound(q, d, eps, S0, S1, SK):
	"""(t, n, d + 1) bound on |device - truth|.  Gradient columns: eps [(d + 12) S1 + 2 (q + 8) S0], the derivation of
	slq_oracle.kmv_dtheta_bound with one e_k instead of its square: e_k carries 2 eps, rho (d + 4) eps, chi the relative error of rho times
	|dlog chi / dlog rho| <= (1 + rho) for all four kinds plus a few eps of exp / sqrt / division, the products kappa chi e_k and inv_ls[k]
	times the sum a few more: (d + 12) (1 + rho) eps per term; the sum over j (MFMA chain, then the pieces of a cut range) adds 2 (q + 8) eps.
	Value column: the stpy_kmv bound 2 eps (q + d + 8) SK."""
	t, n = SK.shape
	bnd = np.zeros((t, n, d + 1))
	bnd[:, :, :d] = eps * ((d + 12) * S1 + 2 * (q + 8) * S0)
	bnd[:, :, d] = 2 * eps * (q + d + 8) * SK
	return bnd


def kmv_dx_emulated(kind, a, b, inv_ls, V, dtype, cols=None, kappa=1.0):
	"""The subtract-first evaluation with every operation rounded to the working ``dtype`` (what the device does, up to summation order)."""
	return kmv_dx_dense(kind, np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype), np.asarray(inv_ls, dtype=dtype), np.asarray(V, dtype=dtype),
						cols=cols, kappa=kappa, dtype=dtype)[0]


# ------------------------------------------------------------------------------------------------------------ the pathwise draw
def make_draws(kind, size, m, n, dsel, seed):
	"""Standard normal draws of a pathwise sample from RandomState(seed): z (m / 2, dsel), u (m / 2,) chi-square with 2 nu degrees of freedom
	(Matern only, else absent), theta (size, m), eps (size, n)."""
	rng = np.random.RandomState(seed)
	dr = {"z": rng.standard_normal((m // 2, dsel))}
	if TWO_NU[kind] is not None:
		dr["u"] = np.sum(rng.standard_normal((m // 2, TWO_NU[kind])) ** 2, axis=1)
	dr["theta"] = rng.standard_normal((size, m))
	dr["eps"] = rng.standard_normal((size, n))
	return dr


def frequencies(kind, gamma, width, draws, cols=None):
	"""W (m / 2, width): W_j = (z_j tau_j) / gamma on the coordinates read, zero elsewhere; tau = 1 (SE) or sqrt(2 nu / u_j) (Matern: a
	Gaussian scale mixture = the multivariate-t spectral density with 2 nu degrees of freedom)."""
	z = np.asarray(draws["z"], dtype=np.float64)
	sel = list(cols) if cols is not None else list(range(width))
	il = np.ones(len(sel)) / np.asarray(gamma, dtype=np.float64)
	tau = np.ones(z.shape[0]) if TWO_NU[kind] is None else np.sqrt(TWO_NU[kind] / np.asarray(draws["u"], dtype=np.float64))
	W = np.zeros((z.shape[0], width))
	W[:, sel] = z * tau[:, None] * il[None, :]
	return W


def features(x, W, kappa):
	"""Phi (n, m) = sqrt(2 / m) sqrt(kappa) [cos(x W^T) | sin(x W^T)]: the layout of stpy_rff_embed for W stacked twice."""
	q = np.asarray(x, dtype=np.float64) @ W.T
	return np.sqrt(2.0 / (2 * W.shape[0])) * np.sqrt(kappa) * np.concatenate([np.cos(q), np.sin(q)], axis=1)


def features_dx(x, W, kappa):
	"""d Phi / dx as (n, m, width)."""
	q = np.asarray(x, dtype=np.float64) @ W.T
	sc = np.sqrt(2.0 / (2 * W.shape[0])) * np.sqrt(kappa)
	return sc * np.concatenate([-np.sin(q)[:, :, None] * W[None, :, :], np.cos(q)[:, :, None] * W[None, :, :]], axis=1)


def kernel_dx(kind, xt, x, gamma, kappa=1.0, cols=None):
	"""d k(xt_i, x_j) / d xt_i as (M, n, width) in float64 (zero on the columns the kernel does not read, and where rho == 0)."""
	xt, x = np.asarray(xt, dtype=np.float64), np.asarray(x, dtype=np.float64)
	width = xt.shape[1]
	sel = list(cols) if cols is not None else list(range(width))
	il = np.ones(len(sel)) / np.asarray(gamma, dtype=np.float64)
	e = (xt[:, None, sel] - x[None, :, sel]) * il
	rho = np.sum(e * e, axis=2)
	wc = np.where(rho == 0, 0.0, kappa * SO._chi(kind, rho))
	out = np.zeros((xt.shape[0], x.shape[0], width))
	out[:, :, sel] = wc[:, :, None] * e * il
	return out


def draw(kind, x, y, xt, gamma, s, kappa, draws, cols=None, with_eps=True):
	"""The dense pathwise draw in float64: f_s(x*) = phi(x*)^T theta_s + k(x*, X) v_s, v_s = A^-1 (y - Phi(X) theta_s - s eps_s).  Returns a dict:
	f (M, size), g (M, size, width) its analytic input gradient, V (size, n) the rows v_s, R (size, n) the residual rows, W, and the pieces the
	bounds need.  with_eps=False leaves the noise draw out (what the reference's sample_matheron does: the variance is then too small)."""
	x, xt = np.asarray(x, dtype=np.float64), np.asarray(xt, dtype=np.float64)
	n = x.shape[0]
	W = frequencies(kind, gamma, x.shape[1], draws, cols)
	theta, eps = np.asarray(draws["theta"], dtype=np.float64), np.asarray(draws["eps"], dtype=np.float64)
	Phi, Phit = features(x, W, kappa), features(xt, W, kappa)
	A = NO.kernel(kind, x, x, gamma, kappa, cols) + s * s * np.eye(n)
	Ks = NO.kernel(kind, xt, x, gamma, kappa, cols)                                  # (M, n)
	R = np.asarray(y, dtype=np.float64).reshape(1, -1) - theta @ Phi.T - (s * eps if with_eps else 0.0)
	c = sla.cho_factor(A, lower=True)
	V = sla.cho_solve(c, R.T).T
	f = Phit @ theta.T + Ks @ V.T
	dK = kernel_dx(kind, xt, x, gamma, kappa, cols)                                  # (M, n, width)
	g = np.einsum("imk,sm->isk", features_dx(xt, W, kappa), theta) + np.einsum("ink,sn->isk", dK, V)
	return dict(f=f, g=g, V=V, R=R, W=W, Phi=Phi, Phit=Phit, A=A, Ks=Ks, dK=dK, chol=c, theta=theta)


def moments(kind, x, y, xt, gamma, s, kappa, W, cols=None):
	"""(mu (M,), var_W (M,)) of the draw over theta and eps for the GIVEN basis W: the mean is the posterior mean k*^T A^-1 y whatever the basis;
	with B = A^-1 K* and T = Phi* - B^T Phi (one row per test point), f_s - mu = T_i theta_s - s B_i^T eps_s, so var_W = |T_i|^2 + s^2 |B_i|^2.
	(Without eps the second term is missing.)"""
	x, xt = np.asarray(x, dtype=np.float64), np.asarray(xt, dtype=np.float64)
	n = x.shape[0]
	A = NO.kernel(kind, x, x, gamma, kappa, cols) + s * s * np.eye(n)
	Ks = NO.kernel(kind, x, xt, gamma, kappa, cols)                                  # (n, M)
	c = sla.cho_factor(A, lower=True)
	B = sla.cho_solve(c, Ks)
	mu = (B.T @ np.asarray(y, dtype=np.float64).reshape(-1, 1))[:, 0]
	T = features(xt, W, kappa) - B.T @ features(x, W, kappa)
	return mu, np.sum(T * T, axis=1) + s * s * np.sum(B * B, axis=0)


def statistics(f, mu, var_w):
	"""The two statistics of a set of draws f (M, size) in units of their tolerances' scale: |mean - mu| / sqrt(var_W / size) and
	|var / var_W - 1| / sqrt(2 / (size - 1)), per test point."""
	size = f.shape[1]
	return (np.abs(f.mean(axis=1) - mu) / np.sqrt(var_w / size), np.abs(f.var(axis=1, ddof=1) / var_w - 1.0) / np.sqrt(2.0 / (size - 1)))


def _feature_sum_bounds(pts, W, kappa, theta, eps, hw_trig):
	"""Per point and path, a bound on the error of sum_j theta_sj phi_j(x) (M, size) and of its input gradient (M, size, width) evaluated in
	arithmetic of unit roundoff eps.  Phase q_j = <W_j, x>: a d-term dot product, |dq_j| <= (d + 2) eps sum_k |W_jk x_k|; with the hardware
	sin / cos (fp32) the phase is also multiplied by 1 / 2 pi and reduced, an argument error eps |q_j|; the function value itself 4 eps.  A unit
	Lipschitz constant turns the phase error into a feature error, the features are scaled by a = sqrt(2 / m) sqrt(kappa); the m-term sum
	adds 2 (m + 8) eps sum_j |theta_sj| |phi_j| (the gradient: |theta_sj| a |W_jk|)."""
	pts = np.asarray(pts, dtype=np.float64)
	m2, d = W.shape[0], max(1, int(np.count_nonzero(np.abs(W).sum(axis=0))))
	m = 2 * m2
	a = np.sqrt(2.0 / m) * np.sqrt(kappa)
	q = pts @ W.T
	dq = (d + 2) * eps * (np.abs(pts) @ np.abs(W).T) + (eps * np.abs(q) if hw_trig else 0.0) + 4 * eps      # (M, m2): per-feature error / a
	at = np.abs(theta)
	at2 = at[:, :m2] + at[:, m2:]                                                          # cos and sin share the phase
	bv = a * (dq @ at2.T) + 2 * (m + 8) * eps * a * np.sum(at, axis=1)[None, :]
	aW = np.abs(W)
	bg = a * np.einsum("ij,sj,jk->isk", dq, at2, aW) + 2 * (m + 8) * eps * a * (at2 @ aW)[None, :, :]
	return bv, bg


def path_bounds(kind, x, y, xt, gamma, s, kappa, draws, tol, eps, cols=None, hw_trig=False):
	"""(f, g, bound on |device f - f| (M, size), bound on |device g - g| (M, size, width)) for a device route whose solves have TRUE relative
	residual <= 2 tol, in arithmetic of unit roundoff eps (hw_trig: the fp32 hardware sin / cos), in the style of kmv_oracle.posterior_bounds.
	The device path is phi*^T theta + k*^T v~ with v~ = A^-1 (r~ + e): r~ = r + dr the residual row as the device built it, |e| <= 2 tol |r~|.
	  solve:      |k*_i^T A^-1 e| <= |A^-1 k*_i| 2 tol |r_s|         (|r~| = |r| to first order)
	  residual:   |k*_i^T A^-1 dr| <= |A^-1 k*_i| |dr_s|,   |dr_sj| <= the feature-sum bound at x_j (_feature_sum_bounds) + 3 eps (|y_j| + s |eps_sj|)
	  data term:  the product bound of stpy_kmv_dx on (x*, X, v_s): kmv_dx_bound
	  prior term: the feature-sum bound at x*_i
	and the same four terms for the gradient with d k*_i / dx in place of k*_i."""
	o = draw(kind, x, y, xt, gamma, s, kappa, draws, cols)
	x, xt = np.asarray(x, dtype=np.float64), np.asarray(xt, dtype=np.float64)
	n, width = x.shape
	sel = list(cols) if cols is not None else list(range(width))
	d = len(sel)
	il = np.ones(d) / np.asarray(gamma, dtype=np.float64)
	B = sla.cho_solve(o["chol"], o["Ks"].T)                                                  # (n, M)
	dB = sla.cho_solve(o["chol"], o["dK"].transpose(1, 0, 2).reshape(n, -1)).reshape(n, xt.shape[0], width)          # A^-1 d k*_i / dx_k
	rn = np.linalg.norm(o["R"], axis=1)                                                      # (size,)
	bx, _ = _feature_sum_bounds(x, o["W"], kappa, o["theta"], eps, hw_trig)                    # (n, size)
	dr = np.linalg.norm(bx + 3 * eps * (np.abs(np.asarray(y, dtype=np.float64).reshape(-1, 1)) + s * np.abs(np.asarray(draws["eps"], dtype=np.float64)).T), axis=0)
	back = 2 * tol * rn + dr                                                                 # (size,)
	_, S0, S1, SK = kmv_dx_dense(kind, xt, x, il, o["V"], cols=cols, kappa=kappa, dtype=np.float64)
	kb = kmv_dx_bound(n, d, eps, S0, S1, SK)                                                 # (size, M, d + 1)
	pv, pg = _feature_sum_bounds(xt, o["W"], kappa, o["theta"], eps, hw_trig)
	bf = np.linalg.norm(B, axis=0)[:, None] * back[None, :] + kb[:, :, d].T + pv
	bg = np.linalg.norm(dB, axis=0)[:, None, :] * back[None, :, None] + pg
	bg[:, :, sel] += kb[:, :, :d].transpose(1, 0, 2)
	return o["f"], o["g"], bf, bg


# ------------------------------------------------------------------------------------------------------------ the statistical cases
STAT_SIZE, STAT_M, STAT_S, STAT_KAPPA, STAT_MTEST = 512, 2048, 0.1, 1.3, 16
# (kind, n, d, gamma, seed of the data and of the draws)
STAT_CASES = [
	("se", 200, 2, 0.35, 4100),
	("matern52", 300, 3, 0.5, 4101),
	("matern12", 150, 1, 0.8, 4102),
	("matern32", 250, 4, 0.9, 4103),
]
STAT_IDS = ["%s-n%d-d%d" % c[:3] for c in STAT_CASES]
STAT_MEAN_Z, STAT_VAR_Z = 4.5, 4.5


def stat_problem(ci, dtype=np.float64):
	"""(x, y (n, 1), xt, draws) of a statistical case: training points uniform(-1, 1)^d, y = sin(3 <x, w>) + 0.1 noise, 16 test points
	uniform(-1.5, 1.5)^d, draws from make_draws with the case's seed; float32 runs get the float32-rounded points and targets."""
	kind, n, d, gamma, seed = STAT_CASES[ci]
	rng = np.random.RandomState(seed)
	x = rng.uniform(-1, 1, size=(n, d))
	w = rng.uniform(-1, 1, size=(d,))
	y = np.sin(3.0 * x @ w) + 0.1 * rng.standard_normal(n)
	xt = rng.uniform(-1.5, 1.5, size=(STAT_MTEST, d))
	if np.dtype(dtype) == np.float32:
		x, y, xt = (v.astype(np.float32).astype(np.float64) for v in (x, y, xt))
	return x, y.reshape(-1, 1), xt, make_draws(kind, STAT_SIZE, STAT_M, n, d, seed + 50000)
