"""
NystromFeatures on the device (stpy_amd/continuous_processes/nystrom_fea.py): the reference's uniform route against golden N1 (the
reference's own NystromFeatures), repeated draws, and the pivoted route plugged into KernelizedFeatures against the NumPy oracle's
Cholesky features on the kernel's own pivots.  Feature Gram matrices and ridge predictions do not see the rotation between the
reference's eigenvector features and the Cholesky features, so those are what is compared, at the project's 1e-8.
"""
import os

import numpy as np
import pytest
import torch

from tests import nystrom_oracle as NO
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

TOL = 1e-8


def T(a):
	return torch.from_numpy(np.ascontiguousarray(a))


def N(t):
	return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def n1():
	return np.load(os.path.join(ROOT, "tests", "golden", "N1_nystrom_uniform.npz"))


def _n1_model(g, **kw):
	from stpy_amd import KernelFunction, NystromFeatures
	kernel = KernelFunction(kernel_name="squared_exponential", gamma=float(g["gamma"]), d=2)
	return NystromFeatures(kernel, m=int(g["m"]), approx="uniform", s=float(g["s"]), **kw)


def test_uniform_matches_reference_golden(n1):
	nys = _n1_model(n1)
	x, y, xq = T(n1["x"]), T(n1["y"]), T(n1["xq"])
	nys.fit_gp(x, y, indices=n1["C"])
	assert nys.fit is True and nys.get_m() == 8 and np.array_equal(np.asarray(nys.C), n1["C"])
	Eq, Ex = N(nys.embed(xq)), N(nys.embed(x))
	assert Eq.shape == (9, 8) and Ex.shape == (200, 8)
	assert np.abs(Eq @ Eq.T - n1["gram_qq"]).max() <= TOL
	assert np.abs(Eq @ Ex.T - n1["gram_qx"]).max() <= TOL
	mu, std = nys.mean_std(xq)
	assert not mu.is_cuda and tuple(mu.shape) == (9, 1)
	assert np.abs(N(mu) - n1["mu"]).max() <= TOL and np.abs(N(std) - n1["std"]).max() <= TOL
	# outer_kernel: Phi Phi^T + s^2 I
	K = N(nys.outer_kernel())
	assert np.abs(K - (Ex @ Ex.T + float(n1["s"]) ** 2 * np.eye(200))).max() <= TOL
	# device inputs give device outputs
	assert nys.embed(xq.cuda()).is_cuda
	# a sampled theta has the feature count, and a draw is reproducible from the torch seed
	torch.manual_seed(3)
	th = nys.sample_theta(size=2)
	torch.manual_seed(3)
	f = nys.sample(xq, size=2)
	assert tuple(th.shape) == (8, 2) and np.abs(N(f) - Eq @ N(th)).max() <= TOL


def test_uniform_draws_where_the_reference_draws(n1):
	nys = _n1_model(n1)
	np.random.seed(int(n1["seed"]))
	nys.fit_gp(T(n1["x"]), T(n1["y"]))
	assert np.array_equal(np.asarray(nys.C), n1["C"])
	mu, std = nys.mean_std(T(n1["xq"]))
	assert np.abs(N(mu) - n1["mu"]).max() <= TOL and np.abs(N(std) - n1["std"]).max() <= TOL


def test_repeated_draw_zero_pads(n1):
	"""A draw with repeats: the distinct landmarks in order of first occurrence, the map keeps m columns and the trailing ones are zero
	(the reference zeroes the features of the zero eigenvalues a repeat produces); predictions are the oracle's on those landmarks."""
	C = np.array([5, 17, 5, 40, 17, 99, 3, 120])
	distinct = [5, 17, 40, 99, 3, 120]
	gam, s = float(n1["gamma"]), float(n1["s"])
	nys = _n1_model(n1)
	nys.fit_gp(T(n1["x"]), T(n1["y"]), indices=C)
	Eq, Ex = N(nys.embed(T(n1["xq"]))), N(nys.embed(T(n1["x"])))
	assert Ex.shape == (200, 8) and np.all(Ex[:, 6:] == 0) and np.all(Eq[:, 6:] == 0)
	Oq = NO.nystrom_features("se", n1["x"], distinct, n1["xq"], gam, m=8)
	Ox = NO.nystrom_features("se", n1["x"], distinct, n1["x"], gam, m=8)
	assert np.abs(Eq - Oq).max() <= TOL and np.abs(Ex - Ox).max() <= TOL          # (same Cholesky features, not only the same Gram matrix)
	mu_o, std_o = NO.ridge(Ox, n1["y"], Oq, s)
	mu, std = nys.mean_std(T(n1["xq"]))
	assert np.abs(N(mu) - mu_o).max() <= TOL and np.abs(N(std) - std_o).max() <= TOL


def test_nothing_route_and_failed_factor(n1):
	from stpy_amd import KernelFunction, NystromFeatures
	gam = float(n1["gamma"])
	kernel = KernelFunction(kernel_name="squared_exponential", gamma=gam, d=2)
	nys = NystromFeatures(kernel, m=6, approx="nothing", s=0.1)
	nys.fit_gp(T(n1["x"]), T(n1["y"]))
	E = N(nys.embed(T(n1["xq"])))
	assert np.abs(E - NO.kernel("se", n1["xq"], n1["x"][:6], gam)).max() <= TOL          # M = I: the kernel columns themselves
	# two coincident landmarks: K_PP is singular, the factorisation fails and says what to do; a jitter repairs it
	x = n1["x"].copy()
	x[11] = x[4]
	nys = NystromFeatures(kernel, m=3, approx="uniform", s=0.1)
	with pytest.raises(torch.linalg.LinAlgError, match="jitter"):
		nys.fit_gp(T(x), T(n1["y"]), indices=[4, 30, 11])
	assert nys.fit is False
	nys = NystromFeatures(kernel, m=3, approx="uniform", s=0.1, jitter=1e-6)
	nys.fit_gp(T(x), T(n1["y"]), indices=[4, 30, 11])
	Eo = NO.nystrom_features("se", x, [4, 30, 11], n1["xq"], gam, jitter=1e-6)
	E = N(nys.embed(T(n1["xq"])))
	assert np.abs(E @ E.T - Eo @ Eo.T).max() <= 1e-6          # (a matrix of condition 1e6: the Gram matrix is good to cond * eps, far below this)


# ------------------------------------------------------------------------------------------------ the pivoted route in KernelizedFeatures
N_P, D_P, M_P, GAMMA_P, S_P = 2500, 3, 130, 0.25, 0.1


@pytest.fixture(scope="module")
def pivoted():
	from stpy_amd import KernelFunction, NystromFeatures
	rng = np.random.RandomState(4101)
	x = rng.uniform(-1, 1, size=(N_P, D_P))
	y = np.sin(3 * x[:, :1]) * np.cos(2 * x[:, 1:2]) + x[:, 2:3] ** 2 + S_P * rng.normal(size=(N_P, 1))
	xq = rng.uniform(-1, 1, size=(50, D_P))
	kernel = KernelFunction(kernel_name="squared_exponential", gamma=GAMMA_P, d=D_P)
	nys = NystromFeatures(kernel, m=M_P, approx="pivoted", s=S_P)
	nys.fit_gp(T(x), T(y))
	piv = np.asarray(nys.C)
	assert len(piv) == M_P and len(set(piv.tolist())) == M_P
	Ox = NO.nystrom_features("se", x, piv, x, GAMMA_P)
	Oq = NO.nystrom_features("se", x, piv, xq, GAMMA_P)
	print("cond(K_PP) of the pivoted landmarks: %.3e" % np.linalg.cond(NO.kernel("se", x[piv], x[piv], GAMMA_P)))
	return dict(x=x, y=y, xq=xq, kernel=kernel, nys=nys, piv=piv, Ox=Ox, Oq=Oq)


def test_pivoted_features_in_kernelized_features(pivoted):
	from stpy_amd.continuous_processes.kernelized_features import KernelizedFeatures
	p = pivoted
	kf = KernelizedFeatures(embedding=p["nys"], m=M_P, s=S_P, lam=1., d=D_P)
	kf.fit_gp(T(p["x"]), T(p["y"]))
	mu, std = kf.mean_std(T(p["xq"]))
	mu_o, std_o = NO.ridge(p["Ox"], p["y"], p["Oq"], S_P)
	e_mu, e_std = np.abs(N(mu) - mu_o).max(), np.abs(N(std) - std_o).max()
	print("pivoted Nystrom ridge against the oracle: |mu| %.3e |std| %.3e" % (e_mu, e_std))
	assert e_mu <= TOL and e_std <= TOL
	# ... and the class's own delegation is that estimator
	mu2, std2 = p["nys"].mean_std(T(p["xq"]))
	assert np.abs(N(mu2) - mu_o).max() <= TOL and np.abs(N(std2) - std_o).max() <= TOL
	# input gradients are out of scope and say so
	xg = T(p["xq"]).clone().requires_grad_(True)
	with pytest.raises(NotImplementedError):
		m_, s_ = kf.mean_std(xg)
		(m_.sum() + s_.sum()).backward()


def test_pivoted_trace_error_beats_uniform(pivoted):
	from stpy_amd import NystromFeatures
	p = pivoted
	n = N_P
	err_piv = float(p["nys"].trace_error)
	want = n - float(np.sum(p["Ox"] * p["Ox"]))                         # trace(K - K_nP K_PP^-1 K_Pn) from the oracle's features
	assert abs(err_piv - want) <= TOL * n
	uni = NystromFeatures(p["kernel"], m=M_P, approx="uniform", s=S_P)
	np.random.seed(11)
	uni.fit_gp(T(p["x"]), T(p["y"]))
	Eu = N(uni.embed(T(p["x"])))
	err_uni = n - float(np.sum(Eu * Eu))
	print("trace error at m = %d: pivoted %.4f, uniform %.4f (trace K = %d)" % (M_P, err_piv, err_uni, n))
	assert 0 < err_piv < err_uni


def test_pivoted_iterative_update_matches_refit(pivoted):
	from stpy_amd.continuous_processes.kernelized_features import KernelizedFeatures
	p = pivoted
	x, y, xq = T(p["x"]), T(p["y"]), T(p["xq"])
	full = KernelizedFeatures(embedding=p["nys"], m=M_P, s=S_P, lam=1., d=D_P)
	full.fit_gp(x, y)
	mu_f, std_f = full.mean_std(xq)
	inc = KernelizedFeatures(embedding=p["nys"], m=M_P, s=S_P, lam=1., d=D_P)
	inc.fit_gp(x[:-5], y[:-5])
	inc.mean_std(xq)
	inc.add_data_point(x[-5:], y[-5:], iterative=True)
	mu_i, std_i = inc.mean_std(xq)
	assert np.abs(N(mu_i) - N(mu_f)).max() <= TOL and np.abs(N(std_i) - N(std_f)).max() <= TOL


def test_pivoted_fit_over_several_slabs(pivoted):
	"""The normal equations accumulated over row slabs of 128 (a slab budget of one byte; the rows after the first 300 arrive as 18 slabs)
	against the fit that embeds all rows at once: the map acts row by row."""
	from stpy_amd.continuous_processes.kernelized_features import KernelizedFeatures
	p = pivoted
	x, y, xq = T(p["x"]), T(p["y"]), T(p["xq"])
	one = KernelizedFeatures(embedding=p["nys"], m=M_P, s=S_P, lam=1., d=D_P)
	one.fit_gp(x, y)
	mu_1, std_1 = one.mean_std(xq)
	calls = []
	emb = p["nys"].embed
	slabbed = KernelizedFeatures(embedding=p["nys"], m=M_P, s=S_P, lam=1., d=D_P)
	slabbed.slab_bytes = 1
	slabbed.fit_gp(x[:300], y[:300])
	slabbed.mean_std(xq)
	p["nys"].embed = lambda q: (calls.append(int(q.shape[0])), emb(q))[1]
	try:
		slabbed.add_data_point(x[300:], y[300:])
		mu_s, std_s = slabbed.mean_std(xq)
	finally:
		del p["nys"].embed
	slabs = [c for c in calls if c <= 128]
	assert len(slabs) >= 18 and sum(slabs) >= N_P - 300, calls
	assert np.abs(N(mu_s) - N(mu_1)).max() <= TOL and np.abs(N(std_s) - N(std_1)).max() <= TOL
