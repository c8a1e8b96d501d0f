"""
IterativeGaussianProcess on the device (matrix-free fit and prediction: stpy_pchol preconditioner, stpy_pcg, stpy_kmv), both dtypes, on the
first four cases of tests/kmv_oracle.PCG_CASES with M = 37 test points (rhs_block = 16: two full blocks and a ragged one).

Against the oracle's dense float64 solve the bounds are derived per test point, not chosen (kmv_oracle.posterior_bounds): a solve stopped
at relative residual tol (true residual <= 2 tol, tests/test_gpu_pcg.py) leaves alpha~ = alpha + A^-1 e with |e| <= 2 tol |y|, so
    |mu - mu*|_i  <= |A^-1 k*_i| 2 tol |y|     + 2 eps (n + d + 8) sum_j |k*_ij| |alpha_j|                      (the product's own bound)
    |var - var*|_i <= |A^-1 k*_i| 2 tol |k*_i| + 2 eps (n + d + 8) sum_j |k*_ij| |w_ij| + 2 eps n sum_j |k*_ij| |w_ij|   (product and dot product)
with eps that of the dtype.  Variances are compared, not standard deviations (a square root near zero has no bounded error).
"""
import os

import numpy as np
import pytest
import torch

from tests import kmv_oracle as KO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["float64", "float32"]
TORCH = {"float64": torch.float64, "float32": torch.float32}
NP = {"float64": np.float64, "float32": np.float32}
CASES = [0, 1, 2, 3]
IDS = [KO.PCG_IDS[i] for i in CASES]
M = 37


def kernel_object(kind, gamma, width, cols, kappa=1.0):
	from stpy_amd import KernelFunction
	kw = dict(gamma=gamma, d=width, kappa=kappa, group=list(cols) if cols else None)
	if kind == "se":
		return KernelFunction(kernel_name="squared_exponential", **kw)
	return KernelFunction(kernel_name="matern", nu={"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}[kind], **kw)


_FITS = {}


def fitted(idx, dtype_name):
	"""One fit and one mean_std per case and dtype, with the oracle's posterior and bounds, shared by the tests."""
	key = (idx, dtype_name)
	if key not in _FITS:
		from stpy_amd import IterativeGaussianProcess
		kind, n, d, gamma, r, cols = KO.PCG_CASES[idx]
		s, tol = KO.SETTINGS[dtype_name]
		x, y, xt = KO.case_data(idx, NP[dtype_name], m_test=M)
		gp = IterativeGaussianProcess(kernel=kernel_object(kind, gamma, x.shape[1], cols), s=s, precond_rank=r, rhs_block=16)
		tx, ty, txt = (torch.from_numpy(v).to(TORCH[dtype_name]) for v in (x, y, xt))
		gp.fit_gp(tx, ty)
		info_fit = dict(gp.cg_info)
		mu, std = gp.mean_std(txt)
		ref = KO.posterior_bounds(kind, x, y, xt, gamma, s, tol, KO.eps_of(NP[dtype_name]), cols)
		_FITS[key] = dict(gp=gp, mu=mu.numpy().astype(np.float64), std=std.numpy().astype(np.float64), ref=ref, info_fit=info_fit, data=(tx, ty, txt),
						  raw=(x, y, xt))
	return _FITS[key]


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("idx", CASES, ids=IDS)
def test_posterior_against_the_dense_oracle(idx, dtype_name):
	f = fitted(idx, dtype_name)
	mu_o, var_o, b_mu, b_var = f["ref"]
	e_mu, e_var = np.abs(f["mu"] - mu_o), np.abs(f["std"] ** 2 - var_o)
	print("%s %s: mean error / bound %.3g, variance error / bound %.3g, fit: %s" % (KO.PCG_IDS[idx], dtype_name, (e_mu / b_mu).max(), (e_var / b_var).max(), f["info_fit"]))
	assert f["mu"].shape == (M, 1) and f["std"].shape == (M, 1) and f["mu"].dtype == np.float64
	assert np.all(np.isfinite(f["mu"])) and np.all(np.isfinite(f["std"]))
	assert np.all(e_mu <= b_mu)
	assert np.all(e_var <= b_var)
	# alpha itself: the TRUE relative residual of the fitted weights is within twice the tolerance
	x, y, xt = f["raw"]
	kind, n, d, gamma, r, cols = KO.PCG_CASES[idx]
	s, tol = KO.SETTINGS[dtype_name]
	A = KO.NO.kernel(kind, x, x, gamma, cols=cols) + s * s * np.eye(n)
	alpha = f["gp"].A.numpy().astype(np.float64)
	assert alpha.shape == (n, 1) and KO.true_relres(A, y, alpha)[0] <= 2 * tol


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("idx", CASES, ids=IDS)
def test_mean_alone_and_cg_info(idx, dtype_name):
	f = fitted(idx, dtype_name)
	gp = f["gp"]
	tx, ty, txt = f["data"]
	kind, n, d, gamma, r, cols = KO.PCG_CASES[idx]
	o = KO.oracle_run(idx, dtype_name)
	info = f["info_fit"]
	assert gp.fitted and info["rank"] == r and 0 < info["relres"] <= KO.SETTINGS[dtype_name][1]
	# the fit is the y column of the solver test: about the oracle's count, within the same geometric-mean bound where that one is asserted
	assert info["iterations"] > 0 and info["kmv_launches"] == 10 * ((info["iterations"] + 9) // 10)
	if o["its"][0] / o["its_plain"][0] < 0.5:
		assert info["iterations"] <= np.sqrt(float(o["its"][0]) * float(o["its_plain"][0]))
	before = gp.cg_info["kmv_launches"]
	mu = gp.mean(txt)
	assert gp.cg_info["kmv_launches"] == before + 1
	assert np.array_equal(mu.numpy().astype(np.float64), f["mu"])          # bit for bit the mean of mean_std
	ucb, lcb = gp.ucb(txt[:5]), gp.lcb(txt[:5])
	assert np.allclose((ucb + lcb).numpy() / 2, f["mu"][:5], rtol=0, atol=1e-5) and np.all((ucb - lcb).numpy() >= 0)


@pytest.mark.parametrize("idx", CASES, ids=IDS)
def test_against_the_exact_gaussian_process(idx):
	"""The factorising class on the same data (float64): the same bounds plus the project's 1e-8."""
	from stpy_amd import GaussianProcess
	f = fitted(idx, "float64")
	kind, n, d, gamma, r, cols = KO.PCG_CASES[idx]
	tx, ty, txt = f["data"]
	gp = GaussianProcess(kernel=kernel_object(kind, gamma, tx.shape[1], cols), s=KO.SETTINGS["float64"][0])
	gp.fit_gp(tx, ty)
	mu, std = gp.mean_std(txt)
	_, _, b_mu, b_var = f["ref"]
	assert np.all(np.abs(f["mu"] - mu.numpy()) <= b_mu + 1e-8)
	assert np.all(np.abs(f["std"] ** 2 - std.numpy() ** 2) <= b_var + 1e-8)


def test_reference_golden_G2():
	"""The reference's own posterior on a single-term SE problem (d = 8, kappa = 1.7; read only): mean and std within the derived bound plus
	the project's 1e-8 for the reference's arithmetic."""
	from stpy_amd import IterativeGaussianProcess
	g = np.load(os.path.join(ROOT, "tests", "golden", "G2_se_d8.npz"))
	gamma, s, kappa = float(g["gamma"]), float(g["s"]), float(g["kappa"])
	gp = IterativeGaussianProcess(gamma=gamma, s=s, kappa=kappa, kernel_name="squared_exponential", d=8, precond_rank=64)
	gp.fit_gp(torch.from_numpy(g["x"]), torch.from_numpy(g["y"]))
	mu, std = gp.mean_std(torch.from_numpy(g["xtest"]))
	mu_o, var_o, b_mu, b_var = KO.posterior_bounds("se", g["x"], g["y"], g["xtest"], gamma, s, 1e-8, KO.eps_of(np.float64), None, kappa)
	assert np.abs(mu_o - g["mu"]).max() <= 1e-8 and np.abs(np.sqrt(var_o) - g["std"]).max() <= 1e-8          # the oracle agrees with the reference
	assert np.all(np.abs(mu.numpy() - g["mu"]) <= b_mu + 1e-8)
	assert np.all(np.abs(std.numpy() ** 2 - g["std"] ** 2) <= b_var + 1e-8)
	assert gp.cg_info["rank"] == 64 and gp.A.shape == (256, 1)


def test_unfitted_prior_and_failed_fits():
	from stpy_amd import IterativeGaussianProcess
	x, y, xt = KO.case_data(0, np.float64, m_test=9)
	tx, ty, txt = (torch.from_numpy(v) for v in (x, y, xt))
	gp = IterativeGaussianProcess(gamma=0.35, s=0.1, kappa=1.3, d=2, precond_rank=0, maxiter=20, check_every=7)
	mu, std = gp.mean_std(txt)
	assert np.all(mu.numpy() == 0) and np.allclose(std.numpy(), np.sqrt(1.3), rtol=0, atol=1e-15) and np.all(gp.mean(txt).numpy() == 0)
	# plain CG needs 242 iterations here: 20 are too few -- an error that names the residual reached, and an object that stays unfitted
	with pytest.raises(RuntimeError, match="relative residual"):
		gp.fit_gp(tx, ty)
	assert gp.fitted is False and gp.A is None
	assert np.all(gp.mean_std(txt)[0].numpy() == 0)
	# a fit that succeeded before does not survive a failed refit either
	gp.maxiter = 1000
	gp.fit_gp(tx, ty)
	assert gp.fitted and gp.cg_info["rank"] == 0 and gp.cg_info["iterations"] > 100
	gp.maxiter = 20
	with pytest.raises(RuntimeError):
		gp.fit(tx, ty)
	assert gp.fitted is False and gp.A is None
	# a noise "variance" that makes the operator indefinite: the curvature flag becomes a LinAlgError
	bad = IterativeGaussianProcess(gamma=0.05, s=0.0, kappa=-1.0, d=2, precond_rank=0)
	with pytest.raises(torch.linalg.LinAlgError):
		bad.fit_gp(tx, ty)
	assert bad.fitted is False


def test_mean_std_blocks():
	"""M above rhs_block and not a multiple of it (M = 37 at rhs_block = 16 in ``fitted``); here the same posterior with rhs_block = 5 and 64:
	blocks only group the solves, so the variances agree within the solver's bound."""
	from stpy_amd import IterativeGaussianProcess
	f = fitted(3, "float64")
	tx, ty, txt = f["data"]
	kind, n, d, gamma, r, cols = KO.PCG_CASES[3]
	_, _, _, b_var = f["ref"]
	for rb in (5, 64):
		gp = IterativeGaussianProcess(kernel=kernel_object(kind, gamma, 1, None), s=0.1, precond_rank=r, rhs_block=rb)
		gp.fit_gp(tx, ty)
		mu, std = gp.mean_std(txt)
		assert np.array_equal(mu.numpy(), f["mu"])
		assert np.all(np.abs(std.numpy() ** 2 - f["std"] ** 2) <= 2 * b_var)
