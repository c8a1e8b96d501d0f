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
	if n == 0:          # an empty expert: no evidence, no gradient, the prior
		return dict(L=np.zeros((0, 0)), V=np.zeros((0, 0)), alpha=np.zeros(0), value=0.0, grad=None if pidx is None else np.zeros(n_params + 1), K=np.zeros((0, 0)))
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
	if len(fit["alpha"]) == 0:
		return np.zeros(len(xt)), np.full(len(xt), float(kappa))
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


# ------------------------------------------------------------------------------------------------ the mixed-size case of the GPU tests
# one expert per regime of the kernels (blocks of 32 rows, rounds of 64, the cap of 512); all but the last have NP_e < NPM = 512
BORDER = dict(sizes=[1, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 200, 511, 512], d=5, shift=(0.5, -0.25, 2.0, 10.0, -3.0),
			  ls=(0.4, 0.7, 0.3, 0.9, 0.5), s=0.1, kappa=1.3, M=97, far=40.0)


def border_case(seed=17):
	"""xs (1962, 5), gathered by expert, in the unit cube shifted off-centre; ys as in reference_case; 97 test points: two training points of every
	expert (its first and its last row; one for the one-point expert), 69 uniform in the cube widened by 0.2, and one 40 units away along every
	axis, where every expert returns the prior"""
	B = BORDER
	rng = np.random.RandomState(seed)
	sizes, d, shift = list(B["sizes"]), B["d"], np.array(B["shift"])
	N = sum(sizes)
	xs = rng.uniform(0.0, 1.0, size=(N, d)) + shift
	ys = np.sin(4.0 * xs[:, 0]) * np.cos(3.0 * xs[:, 1]) + 0.5 * xs[:, 2] + 0.1 * rng.normal(size=N)
	off = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
	pick = np.concatenate([[off[e]] if sizes[e] == 1 else [off[e], off[e + 1] - 1] for e in range(len(sizes))])
	free = rng.uniform(-0.2, 1.2, size=(B["M"] - len(pick) - 1, d)) + shift
	xt = np.concatenate([xs[pick], free, (shift + B["far"])[None, :]])
	return dict(xs=xs, ys=ys, sizes=sizes, offsets=off, xt=xt, pick=pick, inv_ls=1.0 / np.array(B["ls"]), s=B["s"], kappa=B["kappa"])


# ------------------------------------------------------------------------------------------------ one expert again, in extended precision
# The formulas of expert_fit / expert_predict restated with plain loops in np.longdouble (x87: 64-bit mantissa, eps 1.1e-19), or, where long double
# is no wider than double, in mpmath numbers of 80 bits held in object arrays: the yardstick of the float64 oracle above.
_LD = bool(np.finfo(np.longdouble).eps < 2e-19)


def _hp(a):
	"""float64 data -> the extended type, exactly"""
	a = np.asarray(a, dtype=np.float64)
	if _LD:
		return a.astype(np.longdouble)
	import mpmath
	mpmath.mp.prec = 80
	return np.frompyfunc(mpmath.mpf, 1, 1)(a) if a.ndim else mpmath.mpf(float(a))


def _hp_fn(name):
	if _LD:
		return getattr(np, name)
	import mpmath
	return np.frompyfunc(getattr(mpmath, name), 1, 1)


def _hp_phi(kind, r2, derivative=False):
	sqrt, exp = _hp_fn("sqrt"), _hp_fn("exp")
	r, s3, s5 = sqrt(r2), sqrt(_hp(3.0)), sqrt(_hp(5.0))
	if kind == SE:
		return exp(-r2 / 2)
	if kind == MATERN12:
		if not derivative:
			return exp(-r)
		pos = (r > 0).astype(bool)          # (coincident points: F = 0, as in dfactor)
		return np.where(pos, exp(-r) / np.where(pos, r, 1), 0 * r)
	if kind == MATERN32:
		return 3 * exp(-s3 * r) if derivative else (1 + s3 * r) * exp(-s3 * r)
	return (_hp(5.0) / 3) * (1 + s5 * r) * exp(-s5 * r) if derivative else (1 + s5 * r + 5 * r2 / 3) * exp(-s5 * r)


def expert_extended(kind, x, y, inv_ls, s, kappa, weight=1.0, pidx=None, n_params=0, cols=None, xt=None):
	"""dict(alpha, value, grad (or None), mu, var (with xt)) of one expert, every entry in the extended type: Gram matrix from direct differences,
	column Cholesky, forward substitution of [y | k* | I], back substitution for alpha, K^-1 = W^T W for the gradient.  n = 512: about a second"""
	cols = list(range(len(inv_ls))) if cols is None else list(cols)
	x, y, il = _hp(np.asarray(x, dtype=np.float64)[:, cols]), _hp(np.asarray(y, dtype=np.float64).reshape(-1)), _hp(inv_ls)
	kap, sd, w = _hp(kappa), _hp(s), _hp(weight)
	n, log = x.shape[0], _hp_fn("log")
	u2 = ((x[:, None, :] - x[None, :, :]) * il[None, None, :]) ** 2
	r2 = u2.sum(axis=2)
	K = kap * _hp_phi(kind, r2) + sd * sd * _hp(np.eye(n))
	L = 0 * K
	for j in range(n):
		L[j, j] = _hp_fn("sqrt")(K[j, j] - L[j, :j] @ L[j, :j])
		L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
	rhs = [y[:, None]]
	if xt is not None:
		t = _hp(np.asarray(xt, dtype=np.float64)[:, cols])
		ks = kap * _hp_phi(kind, (((x[:, None, :] - t[None, :, :]) * il[None, None, :]) ** 2).sum(axis=2))
		rhs.append(ks)
	if pidx is not None:
		rhs.append(_hp(np.eye(n)))
	B = np.concatenate(rhs, axis=1)
	for j in range(n):          # forward substitution, all right-hand sides at once
		B[j] = (B[j] - L[j, :j] @ B[:j]) / L[j, j]
	z = B[:, 0]
	alpha = z.copy()
	for j in range(n - 1, -1, -1):          # back substitution
		alpha[j] = (alpha[j] - L[j + 1:, j] @ alpha[j + 1:]) / L[j, j]
	out = dict(alpha=alpha, value=(z @ z) / 2 + w * log(np.diagonal(L)).sum(), grad=None)
	at = 1
	if xt is not None:
		v = B[:, 1:1 + ks.shape[1]]
		out["mu"], out["var"] = ks.T @ alpha, kap - (v * v).sum(axis=0)
		at += ks.shape[1]
	if pidx is not None:
		W = B[:, at:]
		Kinv = W.T @ W
		H = (w * Kinv - alpha[:, None] * alpha[None, :]) * kap * _hp_phi(kind, r2, derivative=True)
		g = [0 * kap for _ in range(n_params + 1)]
		for k, p in enumerate(pidx):
			g[int(p)] = g[int(p)] + (H * u2[:, :, k]).sum() * il[k] / 2
		g[n_params] = sd * (w * np.trace(Kinv) - alpha @ alpha)
		out["grad"] = np.array(g)
	return out
