"""
NumPy oracle of the local experts' input gradients (stpy_experts_predict_grad / stpy_experts_combine_grad, LocalExpertsGaussianProcess.mean_std_grad):
one expert's d mu / d x and d var / d x at the test points from direct coordinate differences, and the chain rule through the four combination
rules with their clamp, in float64 and -- in the style of XO.expert_extended -- in extended precision.  Written from include/stpy_hip.h, not from
the kernels.  Conventions: gradients over the SELECTED coordinates, in cols order; Matern 1/2 on a coincident pair contributes zero (XO.dfactor);
the clamp's derivative is zero where it is active, and it is inactive on the ties var_e == kappa and var_e == kappa 2^-52.
"""
import numpy as np
import scipy.linalg as sla

from tests import experts_oracle as XO


def _cols(inv_ls, cols):
	return list(range(len(inv_ls))) if cols is None else list(cols)


# ------------------------------------------------------------------------------------------------ one expert
def expert_grad(kind, x, fit, inv_ls, kappa, xt, cols=None):
	"""(gmu, gvar), each (M, d): gradients of XO.expert_predict's (mu, var) in the selected coordinates of the test points.
	gmu = -kappa il^2 sum_k alpha_k F (xt - x_k),  gvar = 2 kappa il^2 sum_k w_k F (xt - x_k)  with w = K^-1 k*"""
	il = np.asarray(inv_ls, dtype=np.float64)
	M, d = len(xt), len(il)
	if len(fit["alpha"]) == 0:
		return np.zeros((M, d)), np.zeros((M, d))
	c = _cols(il, cols)
	xa, ta = np.asarray(x, dtype=np.float64)[:, c], np.asarray(xt, dtype=np.float64)[:, c]
	diff = ta[:, None, :] - xa[None, :, :]                             # (M, n, d)
	r2 = ((diff * il[None, None, :]) ** 2).sum(axis=2)
	F = XO.dfactor(kind, r2)                                           # (M, n)
	ks = kappa * XO.phi(kind, r2).T                                    # (n, M)
	v = sla.solve_triangular(fit["L"], ks, lower=True, check_finite=False)
	w = sla.solve_triangular(fit["L"].T, v, lower=False, check_finite=False)          # (n, M)
	gmu = -kappa * il ** 2 * np.einsum("k,tk,tkm->tm", fit["alpha"], F, diff)
	gvar = 2.0 * kappa * il ** 2 * np.einsum("kt,tk,tkm->tm", w, F, diff)
	return gmu, gvar


def experts_grad(kind, xs, orc, inv_ls, kappa, xt, cols=None):
	"""(gmu_e, gvar_e), each (E, M, d), of every expert of XO.experts' result ``orc``"""
	off = orc["offsets"]
	g = [expert_grad(kind, xs[off[e]:off[e + 1]], orc["fits"][e], inv_ls, kappa, xt, cols) for e in range(len(orc["fits"]))]
	return np.array([a for a, _ in g]), np.array([b for _, b in g])


def expert_grad_extended(kind, x, y, inv_ls, s, kappa, xt, cols=None):
	"""dict(mu, var (M,), gmu, gvar (M, d)) of one expert, every entry in the extended type of XO (long double, or 80-bit mpmath numbers): Gram
	matrix from direct differences, column Cholesky, forward substitution of [y | k*], back substitution of [z | v] for alpha and w."""
	c = _cols(inv_ls, cols)
	hp = XO._hp
	x, y, il = hp(np.asarray(x, dtype=np.float64)[:, c]), hp(np.asarray(y, dtype=np.float64).reshape(-1)), hp(inv_ls)
	t = hp(np.asarray(xt, dtype=np.float64)[:, c])
	kap, sd = hp(kappa), hp(s)
	n, M, d = x.shape[0], t.shape[0], len(c)
	if n == 0:
		return dict(mu=hp(np.zeros(M)), var=hp(np.zeros(M)) + kap, gmu=hp(np.zeros((M, d))), gvar=hp(np.zeros((M, d))))
	r2 = (((x[:, None, :] - x[None, :, :]) * il[None, None, :]) ** 2).sum(axis=2)
	K = kap * XO._hp_phi(kind, r2) + sd * sd * hp(np.eye(n))
	L = 0 * K
	for j in range(n):
		L[j, j] = XO._hp_fn("sqrt")(K[j, j] - L[j, :j] @ L[j, :j])
		L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
	diff = t[:, None, :] - x[None, :, :]                               # (M, n, d)
	r2t = ((diff * il[None, None, :]) ** 2).sum(axis=2)                # (M, n)
	ks = kap * XO._hp_phi(kind, r2t).T                                 # (n, M)
	F = XO._hp_phi(kind, r2t, derivative=True)                         # (M, n)
	B = np.concatenate([y[:, None], ks], axis=1)
	for j in range(n):          # forward substitution: [z | v]
		B[j] = (B[j] - L[j, :j] @ B[:j]) / L[j, j]
	v = B[:, 1:].copy()
	for j in range(n - 1, -1, -1):          # back substitution: [alpha | w]
		B[j] = (B[j] - L[j + 1:, j] @ B[j + 1:]) / L[j, j]
	alpha, w = B[:, 0], B[:, 1:]
	gmu = -kap * il ** 2 * (alpha[None, :, None] * F[:, :, None] * diff).sum(axis=1)
	gvar = 2 * kap * il ** 2 * (w.T[:, :, None] * F[:, :, None] * diff).sum(axis=1)
	return dict(mu=ks.T @ alpha, var=kap - (v * v).sum(axis=0), gmu=gmu, gvar=gvar)


# ------------------------------------------------------------------------------------------------ combination
def combine_grad(mode, mu_e, var_e, gmu_e, gvar_e, kappa, extended=False):
	"""(mu, var (M,), dmu, dstd (M, d)) from (E, M) expert predictions and their (E, M, d) gradients: XO.combine and its chain rule, sums over
	experts in expert order.  dv = gvar_e where the clamp is inactive (kappa 2^-52 <= var_e <= kappa), else 0.  extended: in XO's extended type"""
	if extended:
		mu_e, var_e, gmu_e, gvar_e, kap = XO._hp(mu_e), XO._hp(var_e), XO._hp(gmu_e), XO._hp(gvar_e), XO._hp(kappa)
		log, sqrt = XO._hp_fn("log"), XO._hp_fn("sqrt")
	else:
		mu_e, var_e = np.asarray(mu_e, dtype=np.float64), np.asarray(var_e, dtype=np.float64)
		gmu_e, gvar_e, kap = np.asarray(gmu_e, dtype=np.float64), np.asarray(gvar_e, dtype=np.float64), float(kappa)
		log, sqrt = np.log, np.sqrt
	vmin = kap * 2.0 ** -52
	E = var_e.shape[0]
	low, high = (var_e < vmin).astype(bool), (var_e > kap).astype(bool)
	v = np.where(low, vmin, np.where(high, kap, var_e))
	v = np.where((var_e != var_e).astype(bool), vmin, v)               # (fmax / fmin send a NaN to the lower bound)
	inactive = (var_e >= vmin).astype(bool) & (var_e <= kap).astype(bool)
	dv = np.where(inactive[:, :, None], gvar_e, 0 * gvar_e)
	c = 1 / v
	dc = -(c * c)[:, :, None] * dv
	if mode in (XO.POE, XO.BCM):
		beta, dbeta = 0 * v + 1, 0 * dv
	elif mode == XO.GPOE:
		beta, dbeta = 0 * v + 1 / (0 * kap + E), 0 * dv
	else:
		beta, dbeta = (log(0 * v + kap) - log(v)) / 2, -dv / (2 * v[:, :, None])
	dbc = dbeta * c[:, :, None] + beta[:, :, None] * dc
	prec, dprec = (beta * c).sum(axis=0), dbc.sum(axis=0)
	if mode == XO.BCM:
		prec = prec + (1 - E) / kap
	if mode == XO.RBCM:
		prec, dprec = prec + (1 - beta.sum(axis=0)) / kap, dprec - dbeta.sum(axis=0) / kap
	wm = (beta * c * mu_e).sum(axis=0)
	dwm = (dbc * mu_e[:, :, None] + (beta * c)[:, :, None] * gmu_e).sum(axis=0)
	var = 1 / prec
	dvar = -(var * var)[:, None] * dprec
	return var * wm, var, dvar * wm[:, None] + var[:, None] * dwm, dvar / (2 * sqrt(var))[:, None]


# ------------------------------------------------------------------------------------------------ the synthetic case of the combination's GPU test
SYNTH = dict(E=5, M=50, d=3, kappa=1.3)


def synthetic_combine_case(seed=51):
	"""hand-made (mu_e, var_e) (5, 50) with random (5, 50, 3) gradient arrays: variances log-uniform over four decades below kappa; in columns
	0 .. 6 one expert past or on the clamp -- below kappa 2^-52, zero, negative, equal to kappa (the tie: inactive), above kappa, one ulp above
	it, 1e-300 -- and in columns 10 .. 12 every expert at once (zero, negative, above kappa).  No variance EQUAL to kappa 2^-52: there the clamp
	is inactive by the rule, c = 1 / var_e is 3e15 and d c its square, which no float64 sum survives.  The sums over experts cancel more or less
	with the draw; the seed is one on which the float64 oracle is within 1e-13 of the extended one ENTRY BY ENTRY (tests/test_experts_grad_cpu.py),
	so that the GPU test can ask for 1e-12 entry by entry"""
	S = SYNTH
	rng = np.random.RandomState(seed)
	E, M, d, kappa = S["E"], S["M"], S["d"], S["kappa"]
	var_e = kappa * 10.0 ** rng.uniform(-4, 0, size=(E, M))
	for j, bad in enumerate([kappa * 2.0 ** -60, 0.0, -1.0, kappa, 2.0 * kappa, np.nextafter(kappa, 2.0), 1e-300]):
		var_e[j % E, j] = bad
	for j, bad in enumerate([0.0, -1.0, 2.0 * kappa]):
		var_e[:, 10 + j] = bad
	return dict(mu_e=rng.normal(size=(E, M)), var_e=var_e, gmu_e=rng.normal(size=(E, M, d)), gvar_e=rng.normal(size=(E, M, d)), kappa=kappa)
