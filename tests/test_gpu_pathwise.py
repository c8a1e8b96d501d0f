"""
IterativeGaussianProcess.mean_value_grad / sample_paths / sample_and_optimize on the device (stpy_kmv_dx for the data term, stpy_rff_embed /
stpy_rff_grad for the prior term, stpy_pcg for the pathwise-conditioning solve), both dtypes, against the dense float64 oracle of
tests/pathwise_oracle.py.  The bounds are derived per test point and path (pathwise_oracle.path_bounds), not chosen: a solve stopped at
relative residual tol leaves v~ = v + A^-1 e with |e| <= 2 tol |r|, the residual rows carry the rounding of the feature sums, and both
terms of a path carry their products' own bounds.  The statistical checks are those of tests/test_pathwise_cpu.py, with its seeds, on
draws that the DEVICE conditioned.
"""
import numpy as np
import pytest
import scipy.linalg as sla
import torch

from tests import kmv_oracle as KO
from tests import pathwise_oracle as PO

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
TORCH = {"float64": torch.float64, "float32": torch.float32}
NP = {"float64": np.float64, "float32": np.float32}
M_FEATURES = 256          # of the bound tests (the statistical tests use pathwise_oracle.STAT_M)


def kernel_object(kind, gamma, width, cols, kappa=1.0):
	from stpy_amd import KernelFunction
	kw = dict(gamma=gamma, d=width, kappa=kappa, group=list(cols) if cols else None)
	if kind == "se":
		return KernelFunction(kernel_name="squared_exponential", **kw)
	return KernelFunction(kernel_name="matern", nu={"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}[kind], **kw)


# --------------------------------------------------------------------------------------------- mean_value_grad
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("idx", [0, 2], ids=[KO.PCG_IDS[0], KO.PCG_IDS[2]])
def test_mean_value_grad_against_the_dense_oracle(idx, dtype_name):
	from stpy_amd import IterativeGaussianProcess
	kind, n, d, gamma, r, cols = KO.PCG_CASES[idx]
	s, tol = KO.SETTINGS[dtype_name]
	eps = KO.eps_of(NP[dtype_name])
	x, y, xt = KO.case_data(idx, NP[dtype_name], m_test=9)
	gp = IterativeGaussianProcess(kernel=kernel_object(kind, gamma, x.shape[1], cols), s=s, precond_rank=r)
	tx, ty, txt = (torch.from_numpy(v).to(TORCH[dtype_name]) for v in (x, y, xt))
	gp.fit_gp(tx, ty)
	before = gp.cg_info["kmv_launches"]
	mu, grad = gp.mean_value_grad(txt)
	assert gp.cg_info["kmv_launches"] == before + 1
	assert mu.shape == (9, 1) and grad.shape == (9, x.shape[1]) and mu.dtype == TORCH[dtype_name] and not mu.is_cuda
	mu, grad = mu.numpy().astype(np.float64), grad.numpy().astype(np.float64)
	# the value column against the class's own mean (stpy_kmv, the same alpha): the two products' bounds
	alpha_dev = gp.A.numpy().astype(np.float64)
	Ks = KO.NO.kernel(kind, xt, x, gamma, cols=cols)
	prod = 2 * eps * (n + d + 8) * (np.abs(Ks) @ np.abs(alpha_dev))
	assert np.all(np.abs(mu - gp.mean(txt).numpy().astype(np.float64)) <= 2 * prod)
	# the gradient against the dense oracle: |(A^-1 dk*_i/dx_k)^T e| <= |A^-1 dk*_i/dx_k| 2 tol |y|, plus the product bound of stpy_kmv_dx
	A = KO.NO.kernel(kind, x, x, gamma, cols=cols) + s * s * np.eye(n)
	c = sla.cho_factor(A, lower=True)
	alpha = sla.cho_solve(c, y)
	dK = PO.kernel_dx(kind, xt, x, gamma, cols=cols)                                      # (M, n, width)
	want = np.einsum("ink,n->ik", dK, alpha[:, 0])
	dB = sla.cho_solve(c, dK.transpose(1, 0, 2).reshape(n, -1)).reshape(n, 9, x.shape[1])
	sel = list(cols) if cols else list(range(x.shape[1]))
	_, S0, S1, SK = PO.kmv_dx_dense(kind, xt, x, np.ones(d) / gamma, alpha.T, cols=cols, dtype=np.float64)
	kb = PO.kmv_dx_bound(n, d, eps, S0, S1, SK)[0]
	bound = np.linalg.norm(dB, axis=0) * 2 * tol * np.linalg.norm(y)
	bound[:, sel] += kb[:, :d]
	err = np.abs(grad - want)
	print("%s %s: gradient error / bound %.3g" % (KO.PCG_IDS[idx], dtype_name, np.max(err[:, sel] / bound[:, sel])))
	assert np.all(err <= bound)
	if cols:
		rest = [k for k in range(x.shape[1]) if k not in cols]
		assert np.all(grad[:, rest] == 0)
	# an unfitted object returns the prior mean, and the old refusals stand on a fitted one
	with pytest.raises(NotImplementedError, match="square root"):
		gp.sample(txt, size=2)
	for fn in (gp.mean, gp.mean_std, gp.mean_value_grad):
		with pytest.raises(NotImplementedError, match="requires_grad"):
			fn(txt.clone().requires_grad_(True))


# --------------------------------------------------------------------------------------------- sample_paths against the oracle's draw
_GPS = {}


def fitted_stat(ci, dtype_name, rhs_block=64):
	"""One fit per statistical case and dtype (noise and tolerance: kmv_oracle.SETTINGS for the bound tests)."""
	key = (ci, dtype_name)
	if key not in _GPS:
		from stpy_amd import IterativeGaussianProcess
		kind, n, d, gamma, seed = PO.STAT_CASES[ci]
		s = KO.SETTINGS[dtype_name][0]
		x, y, xt, _ = PO.stat_problem(ci, NP[dtype_name])
		gp = IterativeGaussianProcess(kernel=kernel_object(kind, gamma, d, None, kappa=PO.STAT_KAPPA), s=s, precond_rank=32, rhs_block=rhs_block)
		gp.fit_gp(torch.from_numpy(x).to(TORCH[dtype_name]), torch.from_numpy(y).to(TORCH[dtype_name]))
		_GPS[key] = (gp, x, y, xt)
	return _GPS[key]


@pytest.mark.parametrize("size", [5, 70])
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("ci", [0, 1], ids=[PO.STAT_IDS[0], PO.STAT_IDS[1]])
def test_sample_paths_with_the_oracles_draws_lie_inside_the_path_bound(ci, dtype_name, size):
	kind, n, d, gamma, seed = PO.STAT_CASES[ci]
	s, tol = KO.SETTINGS[dtype_name]
	gp, x, y, xt = fitted_stat(ci, dtype_name)
	draws = PO.make_draws(kind, size, M_FEATURES, n, d, 700 + ci)
	paths = gp.sample_paths(size=size, num_features=M_FEATURES, draws=draws)
	info = gp.path_info
	assert info["features"] == M_FEATURES and 0 < info["relres"] <= tol and info["iterations"] > 0
	assert info["kmv_launches"] > 0 and info["kmv_launches"] % 10 == 0          # blocks of check_every iterations, one or two solves
	txt = torch.from_numpy(xt).to(TORCH[dtype_name])
	f, g = paths.value_grad(txt)
	assert f.shape == (PO.STAT_MTEST, size) and g.shape == (PO.STAT_MTEST, size, d) and not f.is_cuda
	assert torch.equal(paths(txt), f)
	fo, go, bf, bg = PO.path_bounds(kind, x, y, xt, gamma, s, PO.STAT_KAPPA, draws, tol, KO.eps_of(NP[dtype_name]), hw_trig=dtype_name == "float32")
	ef, eg = np.abs(f.numpy().astype(np.float64) - fo), np.abs(g.numpy().astype(np.float64) - go)
	print("%s %s size %d: value error / bound %.3g, gradient error / bound %.3g, %s" % (PO.STAT_IDS[ci], dtype_name, size, (ef / bf).max(), (eg / bg).max(), info))
	assert np.all(np.isfinite(f.numpy())) and np.all(np.isfinite(g.numpy()))
	assert np.all(ef <= bf)
	assert np.all(eg <= bg)
	# point i on path which[i]: the matching entries of the full call, bit for bit
	which = torch.tensor([(3 * i + 1) % size for i in range(PO.STAT_MTEST)])
	fw, gw = paths.value_grad(txt, which)
	assert fw.shape == (PO.STAT_MTEST,) and gw.shape == (PO.STAT_MTEST, d)
	rows = torch.arange(PO.STAT_MTEST)
	assert torch.equal(fw, f[rows, which]) and torch.equal(gw, g[rows, which])


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_sample_paths_same_seed_same_bits(dtype_name):
	gp, x, y, xt = fitted_stat(1, dtype_name)
	txt = torch.from_numpy(xt).to(TORCH[dtype_name])
	a = gp.sample_paths(size=3, num_features=64, seed=5).value_grad(txt)
	b = gp.sample_paths(size=3, num_features=64, seed=5).value_grad(txt)
	c = gp.sample_paths(size=3, num_features=64, seed=6).value_grad(txt)
	assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
	assert not torch.equal(a[0], c[0])


# --------------------------------------------------------------------------------------------- statistics of the device's draws
@pytest.mark.parametrize("ci", [0, 2], ids=[PO.STAT_IDS[0], PO.STAT_IDS[2]])
def test_device_draws_have_the_posterior_mean_and_the_variance_of_the_drawn_basis(ci):
	"""The two assertions of tests/test_pathwise_cpu.py, same setup and seeds, on paths conditioned by the device (float64, s = 0.1)."""
	from stpy_amd import IterativeGaussianProcess
	kind, n, d, gamma, seed = PO.STAT_CASES[ci]
	x, y, xt, draws = PO.stat_problem(ci)
	gp = IterativeGaussianProcess(kernel=kernel_object(kind, gamma, d, None, kappa=PO.STAT_KAPPA), s=PO.STAT_S, precond_rank=32)
	gp.fit_gp(torch.from_numpy(x), torch.from_numpy(y))
	paths = gp.sample_paths(size=PO.STAT_SIZE, num_features=PO.STAT_M, draws=draws)
	f = paths(torch.from_numpy(xt)).numpy()
	assert f.shape == (PO.STAT_MTEST, PO.STAT_SIZE)
	mu, var_w = PO.moments(kind, x, y, xt, gamma, PO.STAT_S, PO.STAT_KAPPA, PO.frequencies(kind, gamma, d, draws))
	zm, zv = PO.statistics(f, mu, var_w)
	print("%s: mean statistic %.2f, variance statistic %.2f, %s" % (PO.STAT_IDS[ci], zm.max(), zv.max(), gp.path_info))
	assert np.all(np.abs(f.mean(axis=1) - mu) <= PO.STAT_MEAN_Z * np.sqrt(var_w / PO.STAT_SIZE))
	assert np.all(np.abs(f.var(axis=1, ddof=1) / var_w - 1.0) <= PO.STAT_VAR_Z * np.sqrt(2.0 / (PO.STAT_SIZE - 1)))


# --------------------------------------------------------------------------------------------- sample_and_optimize
def test_sample_and_optimize_returns_the_best_start_of_every_path():
	"""size = 3 paths, 8 starts each, d = 2.  Every returned value is its path at the returned point (the same sums evaluated in a launch of
	another shape: 1e-9 covers the rounding of a few hundred float64 terms of order one); it is not below the path's value at any of its
	starts (the method keeps a start that its climb did not improve); and the points lie in the bounds."""
	gp, x, y, xt = fitted_stat(0, "float64")
	np.random.seed(11)
	sol, vals = gp.sample_and_optimize(size=3, multistart=8, num_features=M_FEATURES, seed=2)
	assert sol.shape == (3, 2) and vals.shape == (3,) and not sol.is_cuda
	info = gp.optimize_info
	paths, starts = info["paths"], info["starts"]
	assert starts.shape == (3, 8, 2) and info["evaluations"] >= 2
	lo, hi = x.min(axis=0), x.max(axis=0)
	assert np.all(sol.numpy() >= lo - 1e-12) and np.all(sol.numpy() <= hi + 1e-12)
	assert np.all(starts >= lo) and np.all(starts <= hi)
	at_sol = paths.value_grad(sol, torch.arange(3))[0].numpy()
	assert np.allclose(vals.numpy(), at_sol, rtol=0, atol=1e-9)
	for s in range(3):
		at_starts = paths.value_grad(torch.from_numpy(starts[s]), torch.full((8,), s, dtype=torch.long))[0].numpy()
		assert vals.numpy()[s] >= at_starts.max() - 1e-9, (s, vals.numpy()[s], at_starts)
	# the same seeds give the same answer
	np.random.seed(11)
	sol2, vals2 = gp.sample_and_optimize(size=3, multistart=8, num_features=M_FEATURES, seed=2)
	assert torch.equal(sol, sol2) and torch.equal(vals, vals2)
