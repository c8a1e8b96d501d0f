"""
NumPy twin of the local experts' spatial partition and routed prediction (partition="kdtree", stpy_experts_centroids / _route /
_predict_routed(_grad), LocalExpertsGaussianProcess(predict_experts=k)): the k-d partition by its stated rule (a plain recursion), the centroids,
the routing (stable argsort of the distances, then the chosen ids sorted), the work list and the routed combination, which is XO.combine / the
chain rule of tests/experts_grad_oracle.py applied to the gathered (k, M) arrays.  Written from include/stpy_hip.h and the partition rule, not from
the kernels or the class.
"""
import numpy as np

from tests import experts_grad_oracle as GO
from tests import experts_oracle as XO


# ------------------------------------------------------------------------------------------------ partition
def scaled(x, inv_ls, cols=None):
	"""z = x[:, cols] * inv_ls, one multiplication per entry"""
	x = np.asarray(x, dtype=np.float64)
	return (x if cols is None else x[:, list(cols)]) * np.asarray(inv_ls, dtype=np.float64)


def kdtree(z, sizes, splits=None):
	"""order: the point indices leaf by leaf.  A node owns the leaves [a, b) and a set of points (ascending indices); b - a == 1: that leaf.
	Otherwise mid = a + ceil((b - a) / 2), the coordinate with the largest max - min (ties: the lowest position), points sorted by
	(z in that coordinate, index), the first sum(sizes[a:mid]) left.  splits: a list that receives (a, b, coordinate, left indices, right indices)"""
	z, sizes = np.asarray(z, dtype=np.float64), [int(s) for s in sizes]
	out = []

	def node(a, b, pts):
		if b - a == 1:
			out.append(np.sort(pts))
			return
		mid = a + (b - a + 1) // 2
		zz = z[pts]
		spread = zz.max(axis=0) - zz.min(axis=0)
		c = int(np.nonzero(spread == spread.max())[0][0])
		pts = pts[np.lexsort((pts, zz[:, c]))]
		nl = sum(sizes[a:mid])
		if splits is not None:
			splits.append((a, b, c, pts[:nl], pts[nl:]))
		node(a, mid, pts[:nl])
		node(mid, b, pts[nl:])

	if len(sizes):
		node(0, len(sizes), np.arange(z.shape[0]))
	return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def kd_partition(x, expert_size, inv_ls, cols=None, splits=None):
	"""(order, sizes) of partition="kdtree": XO.balanced_sizes, left to right"""
	sizes = XO.balanced_sizes(len(x), expert_size)
	return kdtree(scaled(x, inv_ls, cols), sizes, splits), sizes


# ------------------------------------------------------------------------------------------------ routing
def centroids(xs, sizes, inv_ls, cols=None):
	"""(E, d): the mean of every expert's rows in scaled coordinates, summed in row order; +inf for an expert without rows"""
	z = scaled(xs, inv_ls, cols)
	off = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
	cent = np.full((len(sizes), z.shape[1]), np.inf)
	for e in range(len(sizes)):
		if off[e + 1] > off[e]:
			s = np.zeros(z.shape[1])
			for row in z[off[e]:off[e + 1]]:
				s = s + row
			cent[e] = s / (off[e + 1] - off[e])
	return cent


def distances(cent, xt, inv_ls, cols=None):
	"""(M, E): D_e = sum_m (z_m - cent[e, m])^2, m ascending; +inf for an expert without rows"""
	zt = scaled(xt, inv_ls, cols)
	D = np.zeros((zt.shape[0], cent.shape[0]))
	with np.errstate(invalid="ignore"):
		for m in range(zt.shape[1]):
			D = D + (zt[:, m:m + 1] - cent[None, :, m]) ** 2
	D = np.minimum(np.where(np.isnan(D), np.finfo(np.float64).max, D), np.finfo(np.float64).max)
	D[:, np.isinf(cent[:, 0])] = np.inf
	return D


def route(cent, xt, inv_ls, k, cols=None):
	"""sel (M, k): the k smallest D_e, ties to the lower id (a stable argsort), then ascending in expert id"""
	D = distances(cent, xt, inv_ls, cols)
	return np.sort(np.argsort(D, axis=1, kind="stable")[:, :k], axis=1)


def smallest_gap(cent, xt, inv_ls, k, cols=None):
	"""the smallest relative gap between the k-th and the (k + 1)-th distance over the test points (inf for k = E)"""
	D = np.sort(distances(cent, xt, inv_ls, cols), axis=1)
	if k >= D.shape[1]:
		return np.inf
	with np.errstate(invalid="ignore", divide="ignore"):
		gap = np.where(D[:, k] > 0, (D[:, k] - D[:, k - 1]) / D[:, k], 0.0)          # (both zero: a tie)
	return float(np.min(np.where(np.isfinite(D[:, k]), gap, np.inf)))


# ------------------------------------------------------------------------------------------------ work list
def tile_bound(E, M, k):
	return (M * k) // 32 + min(E, M * k)


def work_list(sel, E):
	"""(wexp (T,), wpair (32 T,)), T = tile_bound: pair ids p = t k + j stably sorted by expert, cut into tiles of 32 per expert, experts
	ascending; -1 for unused tiles and empty columns"""
	M, k = sel.shape
	T = tile_bound(E, M, k)
	wexp, wpair = np.full(T, -1, dtype=np.int64), np.full(32 * T, -1, dtype=np.int64)
	e = sel.reshape(-1)
	w = 0
	for ex in range(E):
		ps = np.nonzero(e == ex)[0]
		for i in range(0, len(ps), 32):
			wexp[w] = ex
			wpair[32 * w:32 * w + len(ps[i:i + 32])] = ps[i:i + 32]
			w += 1
	return wexp, wpair


# ------------------------------------------------------------------------------------------------ routed combination
def gather(sel, a):
	"""(k, M, ...) from (E, M, ...): a[sel[t, j], t]"""
	return np.asarray(a)[sel.T, np.arange(sel.shape[0])[None, :]]


def routed_combine(mode, sel, mu_e, var_e, kappa):
	"""(mu, var) of the routed prediction: XO.combine over the k gathered slots (E := k)"""
	return XO.combine(mode, gather(sel, mu_e), gather(sel, var_e), kappa)


def routed_combine_grad(mode, sel, mu_e, var_e, gmu_e, gvar_e, kappa):
	"""(mu, var, dmu, dstd) with the selection held fixed"""
	return GO.combine_grad(mode, gather(sel, mu_e), gather(sel, var_e), gather(sel, gmu_e), gather(sel, gvar_e), kappa)


# ------------------------------------------------------------------------------------------------ the accuracy table of the class docstring
ACCURACY = [dict(seed=1, N=2048, d=2, size=64, ls=0.15, s=0.1), dict(seed=2, N=2048, d=3, size=64, ls=0.30, s=0.1), dict(seed=3, N=1000, d=2, size=48, ls=0.15, s=0.05)]


def accuracy_case(c, kappa=1.0, m_test=300):
	"""dict(kd_all, kd_k4, random_all, random_k4): RMSE against the noiseless f = sin(6 x_0) cos(5 x_1) + 0.5 x_{d-1} on the unit cube, SE kernel, rBCM"""
	rng = np.random.RandomState(c["seed"])
	f = lambda x: np.sin(6 * x[:, 0]) * np.cos(5 * x[:, 1]) + 0.5 * x[:, -1]
	x = rng.uniform(size=(c["N"], c["d"]))
	y = f(x) + c["s"] * rng.normal(size=c["N"])
	xt = rng.uniform(size=(m_test, c["d"]))
	inv_ls, out = np.full(c["d"], 1.0 / c["ls"]), {}
	for name in ("kd", "random"):
		order, sizes = kd_partition(x, c["size"], inv_ls) if name == "kd" else XO.partition(c["N"], c["size"], "random", 0)
		xs, ys = x[order], y[order]
		o = XO.experts(XO.SE, xs, ys, sizes, inv_ls, c["s"], kappa, xt=xt)
		rmse = lambda mu: float(np.sqrt(np.mean((mu - f(xt)) ** 2)))
		out[name + "_all"] = rmse(XO.combine(XO.RBCM, o["mu_e"], o["var_e"], kappa)[0])
		sel = route(centroids(xs, sizes, inv_ls), xt, inv_ls, 4)
		out[name + "_k4"] = rmse(routed_combine(XO.RBCM, sel, o["mu_e"], o["var_e"], kappa)[0])
	return out
