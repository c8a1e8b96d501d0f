"""
IterativeGaussianProcess.mean_std_grad / mean_value_grad_hessian / mean_gradient_hessian / ucb_optimize on the device, both dtypes, on the first
four cases of tests/kmv_oracle.PCG_CASES (the Hessian where the kind allows: cases 0, 1 and 3) with M = 37 test points and rhs_block = 16
(two full blocks and a ragged one), against the dense float64 oracle of tests/kmv_dxx_oracle.py.

The bounds are derived per entry, not chosen (kmv_dxx_oracle.posterior_deriv_bounds, an extension of kmv_oracle.posterior_bounds): a solve of
true relative residual 2 tol leaves |A^-1 h| 2 tol |y| on a mean derivative whose kernel-derivative vector is h and |A^-1 g_k| 2 tol |k*| on
sum_j w_j d_k k_j; each product adds its own rounding bound; the standard deviation's gradient takes both through 1 / (2 std) to first order,
together with the variance bound.  That propagation needs var >= 100 b_var, which is a property of the test POINTS and is checked for every
one of them on the CPU (tests/test_kmv_dxx_cpu.py): nothing is filtered here.
"""
import math

import numpy as np
import pytest
import torch

from tests import kmv_oracle as KO
from tests import kmv_dxx_oracle as XO
from tests.test_gpu_iterative_gp import kernel_object

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
TORCH = {"float64": torch.float64, "float32": torch.float32}
NP = {"float64": np.float64, "float32": np.float32}
CASES = [0, 1, 2, 3]
IDS = [KO.PCG_IDS[i] for i in CASES]
M, RHS_BLOCK = 37, 16
_FITS, _DENSE = {}, {}


def fitted(idx, dtype_name):
	"""One fit, one mean_std_grad and (where the kind allows) one mean_value_grad_hessian per case and dtype, with the oracle's derivatives and
	bounds, shared by the tests."""
	key = (idx, dtype_name)
	if key not in _FITS:
		from stpy_amd import IterativeGaussianProcess
		kind, n, d, gamma, r, cols = KO.PCG_CASES[idx]
		s, tol = KO.SETTINGS[dtype_name]
		x, y, xt = XO.test_points(idx, NP[dtype_name], m_test=M)
		gp = IterativeGaussianProcess(kernel=kernel_object(kind, gamma, x.shape[1], cols), s=s, precond_rank=r, rhs_block=RHS_BLOCK)
		tx, ty, txt = (torch.from_numpy(v).to(TORCH[dtype_name]) for v in (x, y, xt))
		gp.fit_gp(tx, ty)
		solves = gp._solves
		dmu, dstd = gp.mean_std_grad(txt)
		f = dict(gp=gp, dmu=dmu, dstd=dstd, solves=gp._solves - solves, data=(tx, ty, txt), raw=(x, y, xt),
				 ref=XO.posterior_deriv_bounds(kind, x, y, xt, gamma, s, tol, KO.eps_of(NP[dtype_name]), cols))
		if kind in XO.HESSIAN_KINDS:
			before = gp.cg_info["kmv_launches"]
			f["mgh"] = gp.mean_value_grad_hessian(txt)
			f["mgh_launches"] = gp.cg_info["kmv_launches"] - before
		_FITS[key] = f
	return _FITS[key]


def dense(idx):
	"""The factorising class on the float64 data of a case."""
	if idx not in _DENSE:
		from stpy_amd import GaussianProcess
		kind, n, d, gamma, r, cols = KO.PCG_CASES[idx]
		tx, ty, txt = fitted(idx, "float64")["data"]
		gp = GaussianProcess(kernel=kernel_object(kind, gamma, tx.shape[1], cols), s=KO.SETTINGS["float64"][0])
		gp.fit_gp(tx, ty)
		_DENSE[idx] = gp
	return _DENSE[idx]


def _report(what, err, bound):
	with np.errstate(divide="ignore", invalid="ignore"):
		ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
	print("%s: largest error / bound %.3g" % (what, ratio.max()))


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("idx", CASES, ids=IDS)
def test_mean_std_grad_against_the_dense_oracle(idx, dtype_name):
	f = fitted(idx, dtype_name)
	o = f["ref"]
	x, y, xt = f["raw"]
	dmu, dstd = f["dmu"], f["dstd"]
	assert dmu.shape == (M, x.shape[1]) and dstd.shape == (M, x.shape[1]) and dmu.dtype == TORCH[dtype_name] and not dmu.is_cuda and not dstd.is_cuda
	assert f["solves"] == math.ceil(M / RHS_BLOCK)                                    # the block solves of mean_std, no further one
	dmu, dstd = dmu.numpy().astype(np.float64), dstd.numpy().astype(np.float64)
	assert np.all(np.isfinite(dmu)) and np.all(np.isfinite(dstd))
	assert np.all(o["ok"])                                                            # (checked per point on the CPU as well)
	e_mu, e_std = np.abs(dmu - o["dmu"]), np.abs(dstd - o["dstd"])
	_report("%s %s d mu" % (KO.PCG_IDS[idx], dtype_name), e_mu, o["b_dmu"])
	_report("%s %s d std" % (KO.PCG_IDS[idx], dtype_name), e_std, o["b_dstd"])
	assert np.all(e_mu <= o["b_dmu"])
	assert np.all(e_std <= o["b_dstd"])
	cols = KO.PCG_CASES[idx][5]
	if cols:
		rest = [k for k in range(x.shape[1]) if k not in cols]
		assert np.all(dmu[:, rest] == 0) and np.all(dstd[:, rest] == 0)
	# the gradient of the mean is that of mean_value_grad, bit for bit (the same launch)
	assert np.array_equal(f["gp"].mean_value_grad(f["data"][2])[1].numpy(), f["dmu"].numpy())


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("idx", [0, 1, 3], ids=[KO.PCG_IDS[i] for i in (0, 1, 3)])
def test_mean_value_grad_hessian_against_the_dense_oracle(idx, dtype_name):
	f = fitted(idx, dtype_name)
	o = f["ref"]
	x, y, xt = f["raw"]
	gp, (tx, ty, txt) = f["gp"], f["data"]
	width = x.shape[1]
	mu, g, H = f["mgh"]
	assert f["mgh_launches"] == 1
	assert mu.shape == (M, 1) and g.shape == (M, width) and H.shape == (M, width, width) and H.dtype == TORCH[dtype_name] and not H.is_cuda
	assert torch.equal(H, H.transpose(1, 2))                                          # symmetric bit for bit
	mu, g, H = (v.numpy().astype(np.float64) for v in (mu, g, H))
	e_mu, e_g, e_H = np.abs(mu[:, 0] - o["mu"]), np.abs(g - o["dmu"]), np.abs(H - o["H"])
	_report("%s %s mean" % (KO.PCG_IDS[idx], dtype_name), e_mu, o["b_mu"])
	_report("%s %s gradient" % (KO.PCG_IDS[idx], dtype_name), e_g, o["b_dmu"])
	_report("%s %s Hessian" % (KO.PCG_IDS[idx], dtype_name), e_H, o["b_H"])
	assert np.all(e_mu <= o["b_mu"]) and np.all(e_g <= o["b_dmu"]) and np.all(e_H <= o["b_H"])
	# the value column against the class's own mean (stpy_kmv, the same alpha): nothing in the existing code makes mean_value_grad's value the bits
	# of ``mean`` (tests/test_gpu_pathwise.py compares them within the two products' bounds), so the same holds here
	kind, n, d, gamma, r, cols = KO.PCG_CASES[idx]
	alpha_dev = gp.A.numpy().astype(np.float64)
	Ks = KO.NO.kernel(kind, xt, x, gamma, cols=cols)
	prod = 2 * KO.eps_of(NP[dtype_name]) * (n + d + 8) * (np.abs(Ks) @ np.abs(alpha_dev))
	assert np.all(np.abs(mu - gp.mean(txt).numpy().astype(np.float64)) <= 2 * prod)
	# the reference's convention: the first row
	g1 = gp.mean_gradient_hessian(txt)
	g2, H2 = gp.mean_gradient_hessian(txt, hessian=True)
	assert g1.shape == (width,) and H2.shape == (width, width)
	assert np.array_equal(g1.numpy(), gp.mean_value_grad(txt[:1])[1][0].numpy())
	assert np.array_equal(g2.numpy(), f["mgh"][1][0].numpy()) and np.array_equal(H2.numpy(), f["mgh"][2][0].numpy())


@pytest.mark.parametrize("idx", CASES, ids=IDS)
def test_against_the_exact_gaussian_process(idx):
	"""The factorising class on the same data (float64): the same bounds plus the project's 1e-8."""
	f = fitted(idx, "float64")
	o = f["ref"]
	gp = dense(idx)
	txt = f["data"][2]
	dmu, dstd = gp.mean_std_grad(txt)
	assert np.all(np.abs(f["dmu"].numpy() - dmu.numpy()) <= o["b_dmu"] + 1e-8)
	assert np.all(np.abs(f["dstd"].numpy() - dstd.numpy()) <= o["b_dstd"] + 1e-8)
	if "mgh" in f:
		g, H = gp.mean_gradient_hessian(txt, hessian=True)
		g_it, H_it = f["gp"].mean_gradient_hessian(txt, hessian=True)
		assert np.all(np.abs(g_it.numpy() - g.numpy()) <= o["b_dmu"][0] + 1e-8)
		assert np.all(np.abs(H_it.numpy() - H.numpy()) <= o["b_H"][0] + 1e-8)
	else:
		with pytest.raises(NotImplementedError, match="singular at r = 0"):
			f["gp"].mean_value_grad_hessian(txt)
		assert f["gp"].mean_gradient_hessian(txt).shape == (txt.shape[1],)


# --------------------------------------------------------------------------------------------- ucb_optimize
UCB_N, UCB_GAMMA, UCB_BETA, UCB_STARTS, UCB_BLOCK = 256, 0.4, 4.0, 20, 8
UCB_BOUNDS = [(-1.0, 1.0), (-1.2, 1.2)]


def _ucb_problem(dtype_name):
	rng = np.random.RandomState(6100)
	x = rng.uniform(-1, 1, size=(UCB_N, 2))
	y = (np.sin(3.0 * x[:, 0]) * np.cos(2.0 * x[:, 1]) + 0.1 * rng.standard_normal(UCB_N)).reshape(-1, 1)
	if dtype_name == "float32":
		x, y = (v.astype(np.float32).astype(np.float64) for v in (x, y))
	return x, y


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("lcb", [False, True], ids=["ucb", "lcb"])
def test_ucb_optimize(lcb, dtype_name):
	from stpy_amd import GaussianProcess, IterativeGaussianProcess
	s, tol = KO.SETTINGS[dtype_name]
	eps = KO.eps_of(NP[dtype_name])
	x, y = _ucb_problem(dtype_name)
	tx, ty = (torch.from_numpy(v).to(TORCH[dtype_name]) for v in (x, y))
	gp = IterativeGaussianProcess(gamma=UCB_GAMMA, s=s, d=2, precond_rank=32, rhs_block=UCB_BLOCK, bounds=UCB_BOUNDS)
	gp.fit_gp(tx, ty)
	np.random.seed(11)
	sol, val = gp.ucb_optimize(UCB_BETA, multistart=UCB_STARTS, lcb=lcb)
	info = gp.optimize_info
	sign, sb = (-1.0 if lcb else 1.0), math.sqrt(UCB_BETA)
	assert sol.shape == (2,) and val.shape == () and sol.dtype == torch.float64
	sol_np, val = sol.numpy(), float(val)
	assert all(lo <= v <= hi for v, (lo, hi) in zip(sol_np, UCB_BOUNDS))
	per = math.ceil(UCB_STARTS / UCB_BLOCK)
	assert info["evaluations"] >= 2 and info["solves"] == info["evaluations"] * per and info["kmv_launches"] > info["solves"]
	assert info["starts"].shape == (UCB_STARTS, 2)
	# the starts are the reference's draws for this seed
	np.random.seed(11)
	from stpy_amd.continuous_processes.gauss_procc import _draw_starts
	assert np.array_equal(np.asarray(_draw_starts(UCB_STARTS, 2, UCB_BOUNDS)), info["starts"])
	# the value, recomputed by mean_std at the returned point (rounded to the dtype, as the optimiser's last evaluation saw it): both
	# evaluations are within the posterior bounds of the dense truth; |sqrt(v~) - sqrt(v)| = |v~ - v| / (sqrt(v~) + sqrt(v)) <= b_var / sqrt(v), no margin needed
	pt = sol_np.reshape(1, 2).astype(NP[dtype_name]).astype(np.float64)
	mu_o, var_o, b_mu, b_var = (v[0, 0] for v in KO.posterior_bounds("se", x, y, pt, UCB_GAMMA, s, tol, eps))
	b_val = b_mu + sb * b_var / math.sqrt(var_o)
	mu, std = gp.mean_std(torch.from_numpy(pt).to(TORCH[dtype_name]))
	again = float(mu) + sign * sb * float(std)
	truth = mu_o + sign * sb * math.sqrt(var_o)
	print("%s %s: value %.6f, recomputed %.6f, dense truth %.6f, bound %.3g, %s" % ("lcb" if lcb else "ucb", dtype_name, val, again, truth, b_val, {k: v for k, v in info.items() if k != "starts"}))
	assert abs(val - truth) <= b_val and abs(again - truth) <= b_val and abs(val - again) <= 2 * b_val
	# never below the acquisition at a drawn start: exactly, against the values the optimiser's first evaluation saw, and within the posterior
	# bounds against a second evaluation of the starts
	assert info["start_values"].shape == (UCB_STARTS,) and val >= info["start_values"].max()
	mu0, std0 = gp.mean_std(torch.from_numpy(info["starts"]).to(TORCH[dtype_name]))
	acq0 = (mu0 + sign * sb * std0).numpy().astype(np.float64)[:, 0]
	o0 = KO.posterior_bounds("se", x, y, info["starts"].astype(NP[dtype_name]).astype(np.float64), UCB_GAMMA, s, tol, eps)
	slack = (o0[2] + sb * o0[3] / np.sqrt(o0[1]))[:, 0]                                  # two evaluations of the same start differ by at most twice this
	assert np.all(np.abs(acq0 - info["start_values"]) <= 2 * slack)
	assert np.all(val >= acq0 - 2 * slack)
	# the dense class at the returned point (float64 data only: it would see other numbers otherwise)
	if dtype_name == "float64":
		dg = GaussianProcess(gamma=UCB_GAMMA, s=s, d=2)
		dg.fit_gp(tx, ty)
		dmu, dstd = dg.mean_std(torch.from_numpy(pt))
		assert abs(val - (float(dmu) + sign * sb * float(dstd))) <= b_val + 1e-8


def test_ucb_optimize_unfitted_and_without_bounds():
	from stpy_amd import IterativeGaussianProcess
	gp = IterativeGaussianProcess(gamma=0.4, s=0.1, kappa=1.3, d=2)
	with pytest.raises(ValueError, match="bounds"):
		gp.ucb_optimize(4.0)
	gp.bounds = UCB_BOUNDS
	np.random.seed(3)
	sol, val = gp.ucb_optimize(4.0, multistart=5)                                      # the prior: flat, mu = 0, std = sqrt(kappa)
	assert all(lo <= v <= hi for v, (lo, hi) in zip(sol.numpy(), UCB_BOUNDS))
	assert abs(float(val) - 2.0 * math.sqrt(1.3)) <= 1e-14 and gp.optimize_info["solves"] == 0
