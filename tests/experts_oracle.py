"""
NumPy oracle of the local GP experts (stpy_experts_fit / _predict / _combine, LocalExpertsGaussianProcess): the partition rule, one expert's GP
from direct coordinate differences -- alpha, the evidence value and its gradient by the formulas of stpy_lml_batch, the posterior mean and latent
variance -- and the four combination rules with their clamp.  Written from include/stpy_hip.h, not from the kernels.
"""
import numpy as np
import scipy.linalg as sla

SE, MATERN12, MATERN32, MATERN52 = 0, 1, 2, 3
KINDS = (SE, MATERN12, MATERN32, MATERN52)
POE, GPOE, BCM, RBCM = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------ partition
def balanced_sizes(n, expert_size):
	"""E = ceil(n / expert_size) sizes that differ by at most one, the larger ones first"""
	E = (n + expert_size - 1) // expert_size
	return [n // E + (1 if e < n % E else 0) for e in range(E)]


def partition(n, expert_size, mode="random", seed=0):
	"""(order, sizes): the indices of the points expert by expert.  mode: "random" (numpy default_rng(seed) permutation), "contiguous", or a list
	of n expert ids (points of an expert in their given order)"""
	if isinstance(mode, str):
		order = np.random.default_rng(seed).permutation(n) if mode == "random" else np.arange(n)
		return order, balanced_sizes(n, expert_size)
	ids = np.asarray(mode).reshape(-1)
	E = int(ids.max()) + 1
	order = np.concatenate([np.nonzero(ids == e)[0] for e in range(E)])
	return order, [int(np.sum(ids == e)) for e in range(E)]


# ------------------------------------------------------------------------------------------------ one expert
def _u2(xa, xb, inv_ls, cols):
	"""(|a|, |b|, d): squared scaled coordinate differences"""
	cols = list(range(len(inv_ls))) if cols is None else list(cols)
	a, b = np.asarray(xa, dtype=np.float64)[:, cols], np.asarray(xb, dtype=np.float64)[:, cols]
	return ((a[:, None, :] - b[None, :, :]) * np.asarray(inv_ls, dtype=np.float64)[None, None, :]) ** 2


def phi(kind, r2):
	r = np.sqrt(r2)
	if kind == SE:
		return np.exp(-0.5 * r2)
	if kind == MATERN12:
		return np.exp(-r)
	if kind == MATERN32:
		return (1.0 + np.sqrt(3.0) * r) * np.exp(-np.sqrt(3.0) * r)
	return (1.0 + np.sqrt(5.0) * r + 5.0 * r2 / 3.0) * np.exp(-np.sqrt(5.0) * r)


def dfactor(kind, r2):
	"""F with d k / d l_m = kappa F u_m^2 / l_m; zero on coincident points for Matern 1/2"""
	r = np.sqrt(r2)
	if kind == SE:
		return np.exp(-0.5 * r2)
	if kind == MATERN12:
		with np.errstate(divide="ignore", invalid="ignore"):
			return np.where(r > 0, np.exp(-r) / np.where(r > 0, r, 1.0), 0.0)
	if kind == MATERN32:
		return 3.0 * np.exp(-np.sqrt(3.0) * r)
	return (5.0 / 3.0) * (1.0 + np.sqrt(5.0) * r) * np.exp(-np.sqrt(5.0) * r)


def kernel_matrix(kind, xa, xb, inv_ls, kappa, cols=None):
	return kappa * phi(kind, _u2(xa, xb, inv_ls, cols).sum(axis=2))


def expert_fit(kind, x, y, inv_ls, s, kappa, weight=1.0, pidx=None, n_params=0, cols=None):
	"""dict(L, V = L^-T, alpha, value, grad (n_params + 1: lengthscale slots, then the noise std; None without pidx)) of one expert"""
	x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64).reshape(-1)
	n = x.shape[0]
	u2 = _u2(x, x, inv_ls, cols)
	r2 = u2.sum(axis=2)
	K = kappa * phi(kind, r2) + s * s * np.eye(n)
	L = sla.cholesky(K, lower=True, check_finite=False)
	W = sla.solve_triangular(L, np.eye(n), lower=True, check_finite=False)
	z = W @ y
	alpha = W.T @ z
	out = dict(L=L, V=W.T.copy(), alpha=alpha, value=0.5 * float(z @ z) + weight * float(np.sum(np.log(np.diag(L)))), grad=None, K=K)
	if pidx is not None:
		Kinv = W.T @ W
		H = (weight * Kinv - np.outer(alpha, alpha)) * kappa * dfactor(kind, r2)
		g = np.zeros(n_params + 1)
		for k, p in enumerate(pidx):
			g[int(p)] += 0.5 * float(np.sum(H * u2[:, :, k])) * float(inv_ls[k])
		g[n_params] = s * (weight * float(np.trace(Kinv)) - float(alpha @ alpha))
		out["grad"] = g
	return out


def expert_predict(kind, x, fit, inv_ls, kappa, xt, cols=None):
	"""(mu, var) of the latent f at xt: var = kappa - |L^-1 k*|^2"""
	ks = kernel_matrix(kind, x, xt, inv_ls, kappa, cols)          # (n, M)
	v = sla.solve_triangular(fit["L"], ks, lower=True, check_finite=False)
	return ks.T @ fit["alpha"], kappa - np.sum(v * v, axis=0)


def experts(kind, xs, ys, sizes, inv_ls, s, kappa, weight=1.0, pidx=None, n_params=0, cols=None, xt=None):
	"""Every expert of the gathered data: dict(fits, alpha (N), value (E), grad (E, n_params + 1) or None, total, mu_e, var_e (E, M) with xt)"""
	off = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
	fits = [expert_fit(kind, xs[off[e]:off[e + 1]], ys[off[e]:off[e + 1]], inv_ls, s, kappa, weight, pidx, n_params, cols) for e in range(len(sizes))]
	out = dict(fits=fits, offsets=off, alpha=np.concatenate([f["alpha"] for f in fits]), value=np.array([f["value"] for f in fits]),
			   grad=np.array([f["grad"] for f in fits]) if pidx is not None else None)
	out["total"] = np.concatenate([[out["value"].sum()], out["grad"].sum(axis=0)]) if pidx is not None else np.array([out["value"].sum()])
	if xt is not None:
		pr = [expert_predict(kind, xs[off[e]:off[e + 1]], fits[e], inv_ls, kappa, xt, cols) for e in range(len(sizes))]
		out["mu_e"], out["var_e"] = np.array([p[0] for p in pr]), np.array([p[1] for p in pr])
	return out


# ------------------------------------------------------------------------------------------------ combination
def clamp(var_e, kappa):
	return np.minimum(np.maximum(var_e, kappa * 2.0 ** -52), kappa)


def n_clamped(var_e, kappa):
	"""how many expert variances the clamp changes"""
	return int(np.sum(clamp(var_e, kappa) != var_e))


def combine(mode, mu_e, var_e, kappa):
	"""(mu, var) (M,) from (E, M) expert predictions; sums over experts in expert order"""
	mu_e, v = np.asarray(mu_e, dtype=np.float64), clamp(np.asarray(var_e, dtype=np.float64), kappa)
	E = v.shape[0]
	c = 1.0 / v
	if mode in (POE, BCM):
		beta = np.ones_like(v)
	elif mode == GPOE:
		beta = np.full_like(v, 1.0 / E)
	else:
		beta = 0.5 * (np.log(kappa) - np.log(v))
	prec = np.sum(beta * c, axis=0)
	if mode == BCM:
		prec = prec + (1.0 - E) / kappa
	if mode == RBCM:
		prec = prec + (1.0 - np.sum(beta, axis=0)) / kappa
	var = 1.0 / prec
	return var * np.sum(beta * c * mu_e, axis=0), var


# ------------------------------------------------------------------------------------------------ the reference case of the GPU tests
REF = dict(N=167, d=3, expert_size=34, s=0.1, kappa=1.3, ls=0.4, M=65, M_train=20)


def reference_case(seed=5):
	"""x (167, 3) in the unit cube shifted off-centre, y, the random partition (E = 5: 34, 34, 33, 33, 33), 65 test points of which the first 20
	are training points (four of every expert)"""
	rng = np.random.RandomState(seed)
	x = rng.uniform(0.0, 1.0, size=(REF["N"], REF["d"])) + np.array([0.5, -0.25, 2.0])
	y = np.sin(4.0 * x[:, 0]) * np.cos(3.0 * x[:, 1]) + 0.5 * x[:, 2] + 0.1 * rng.normal(size=REF["N"])
	order, sizes = partition(REF["N"], REF["expert_size"], "random", 0)
	xs, ys = x[order], y[order]
	off = np.concatenate([[0], np.cumsum(sizes)])
	pick = np.concatenate([off[e] + np.arange(4) * 7 for e in range(len(sizes))])
	xt = np.concatenate([xs[pick], rng.uniform(-0.2, 1.2, size=(REF["M"] - REF["M_train"], REF["d"])) + np.array([0.5, -0.25, 2.0])])
	return dict(x=x, y=y, order=order, sizes=sizes, xs=xs, ys=ys, xt=xt, inv_ls=np.full(REF["d"], 1.0 / REF["ls"]), s=REF["s"], kappa=REF["kappa"])
