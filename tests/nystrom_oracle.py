"""
NumPy oracle of the Nystrom route (stpy_pchol, NystromFeatures): a greedy pivoted partial Cholesky in float64 or float32 with an optional
forced pivot list, Cholesky-based Nystrom features, and the primal ridge on a feature map.  Kernel values come from direct coordinate
differences scaled by 1 / gamma, evaluated in the working dtype, as the device does; nothing here touches the GPU or the library.
"""
import numpy as np
import scipy.linalg as sla

SQRT3, SQRT5 = 1.7320508075688772935, 2.2360679774997896964
KINDS = ("se", "matern12", "matern32", "matern52")


def _phi(kind, r2):
	dt = r2.dtype.type
	if kind == "se":
		return np.exp(dt(-0.5) * r2)
	r = np.sqrt(r2)
	if kind == "matern12":
		return np.exp(-r)
	if kind == "matern32":
		r = r * dt(SQRT3)
		return (dt(1) + r) * np.exp(-r)
	if kind == "matern52":
		r = r * dt(SQRT5)
		return (dt(1) + r + r * r / dt(3)) * np.exp(-r)
	raise ValueError(kind)


def kernel(kind, a, b, gamma, kappa=1.0, cols=None, dtype=np.float64):
	"""k(a_i, b_j) as an (|a|, |b|) matrix in ``dtype``; gamma: a scalar or one lengthscale per coordinate read."""
	a = np.asarray(a, dtype=dtype)
	b = np.asarray(b, dtype=dtype)
	if cols is not None:
		a, b = a[:, list(cols)], b[:, list(cols)]
	il = (np.ones(a.shape[1]) / np.asarray(gamma, dtype=np.float64)).astype(dtype)
	u = (a[:, None, :] - b[None, :, :]) * il
	r2 = np.zeros(u.shape[:2], dtype=dtype)
	for k in range(u.shape[2]):
		r2 = u[:, :, k] * u[:, :, k] + r2
	return (dtype(kappa) * _phi(kind, r2)).astype(dtype)


def pivoted_cholesky(kind, x, gamma, m, tol=0.0, kappa=1.0, cols=None, dtype=np.float64, pivots=None, trace=None):
	"""Greedy pivoted partial Cholesky of k(x, x): (piv (m,), Ft (m, n), dres (n,), rank) with the conventions of stpy_pchol -- ties to the
	lowest index, stop at dres[p] <= tol * kappa or <= 0, rows of Ft from the rank on zero, piv -1 there, dres exactly 0 on the pivots.
	``pivots``: a forced pivot list (the stop test is then skipped and the rank is its length).  ``trace``: a list that receives
	(dres[p], max dres) of every step, taken before the step."""
	x = np.asarray(x, dtype=dtype)
	n = x.shape[0]
	Ft = np.zeros((m, n), dtype=dtype)
	dres = np.full((n,), kappa, dtype=dtype)
	piv = np.full((m,), -1, dtype=np.int32)
	steps = m if pivots is None else len(pivots)
	rank = steps
	for j in range(steps):
		p = int(np.argmax(dres)) if pivots is None else int(pivots[j])          # (argmax: the first of equal maxima)
		dp = dres[p]
		if trace is not None:
			trace.append((float(dp), float(dres.max())))
		if pivots is None and (float(dp) <= tol * kappa or float(dp) <= 0.0):
			rank = j
			break
		col = kernel(kind, x, x[p:p + 1], gamma, kappa, cols, dtype)[:, 0]
		if j > 0:
			col = col - Ft[:j].T @ Ft[:j, p]
		f = (col / np.sqrt(dp)).astype(dtype)
		Ft[j] = f
		dres = (dres - f * f).astype(dtype)
		dres[p] = 0
		piv[j] = p
	dres[piv[:rank]] = 0          # (a later step's entry at an earlier pivot is rounding noise; its square is not kept)
	return piv, Ft, dres, rank


def nystrom_features(kind, x, landmarks, q, gamma, kappa=1.0, cols=None, jitter=0.0, m=None):
	"""phi(q) = L^-1 k(x_P, q) with L L^T = K_PP + jitter kappa I, one row per point of q, zero-padded to m columns."""
	xp = np.asarray(x, dtype=np.float64)[list(landmarks)]
	Kpp = kernel(kind, xp, xp, gamma, kappa, cols)
	L = np.linalg.cholesky(Kpp + jitter * kappa * np.eye(len(xp)))
	Phi = sla.solve_triangular(L, kernel(kind, xp, q, gamma, kappa, cols), lower=True).T
	if m is not None and m > Phi.shape[1]:
		Phi = np.concatenate([Phi, np.zeros((Phi.shape[0], m - Phi.shape[1]))], axis=1)
	return Phi


def ridge(Phi, y, Phiq, s, lam=1.0):
	"""Primal ridge on a feature map: theta = (Phi^T Phi + s^2 lam I)^-1 Phi^T y, mean = Phiq theta, std = s sqrt(diag(Phiq V^-1 Phiq^T))."""
	V = Phi.T @ Phi + s * s * lam * np.eye(Phi.shape[1])
	c = sla.cho_factor(V, lower=True)
	theta = sla.cho_solve(c, Phi.T @ np.asarray(y, dtype=np.float64).reshape(-1, 1))
	X = sla.solve_triangular(c[0], Phiq.T, lower=True)
	return Phiq @ theta, s * np.sqrt(np.sum(X * X, axis=0)).reshape(-1, 1)
