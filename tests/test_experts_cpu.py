"""
Local GP experts, the parts that need no GPU: the NumPy oracle (tests/experts_oracle.py) against oracle/gp_oracle.py and central differences, the
combination identities, the distance of the GPU tests' reference case from the combination's clamp, the float64 oracle against an
extended-precision restatement on the GPU tests' mixed-size case (experts of 1 .. 512 points), the host side of
LocalExpertsGaussianProcess with the device out of reach, the argument checks of the C entry points (every refusal comes before the first HIP
call, so placeholder pointers are safe), and the resource usage of the kernels.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from tests import experts_oracle as XO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stpy_amd", "csrc")


def _spec(kind, ls, kappa):
	if kind == XO.SE:
		return [("squared_exponential", {"gamma": ls, "kappa": kappa}, "-")]
	return [("matern", {"gamma": ls, "nu": {XO.MATERN12: 0.5, XO.MATERN32: 1.5, XO.MATERN52: 2.5}[kind], "kappa": kappa}, "-")]


# --------------------------------------------------------------------------------------------- 1. the oracle against gp_oracle
@pytest.mark.parametrize("kind", XO.KINDS)
def test_oracle_expert_is_the_exact_gp_on_its_slice(kind):
	"""gp_oracle's SE expands the norms, this oracle takes direct differences: the two kernels differ by a few eps |x|^2 / l^2 = 1e-14, amplified
	by at most cond(K) <= kappa n / s^2 = 4.4e3 in the solves: 1e-9 covers it with two orders to spare."""
	r = XO.reference_case()
	ls, off = XO.REF["ls"], np.concatenate([[0], np.cumsum(r["sizes"])])
	for e in (0, 3):
		x, y = r["xs"][off[e]:off[e + 1]], r["ys"][off[e]:off[e + 1]]
		f = XO.expert_fit(kind, x, y, r["inv_ls"], r["s"], r["kappa"], 0.7, [0, 0, 0], 1)
		L, alpha = O.fit(x, y, _spec(kind, ls, r["kappa"]), r["s"])
		assert np.allclose(f["alpha"], alpha.ravel(), rtol=0, atol=1e-9 * np.max(np.abs(alpha)))
		mu, var = XO.expert_predict(kind, x, f, r["inv_ls"], r["kappa"], r["xt"])
		mu0, sd0 = O.mean_std(x, L, alpha, r["xt"], _spec(kind, ls, r["kappa"]))
		assert np.allclose(mu, mu0.ravel(), rtol=0, atol=1e-9 * np.max(np.abs(mu0)))
		assert np.allclose(var, sd0.ravel() ** 2, rtol=0, atol=1e-9 * r["kappa"])
		v0 = float(O.log_marginal(x, y, _spec(kind, ls, r["kappa"]), r["s"], None, 0.7)[0, 0])
		assert abs(f["value"] - v0) <= 1e-9 * abs(v0)
		# the factor: V = L^-T
		assert np.allclose(f["V"] @ f["V"].T @ f["K"], np.eye(len(y)), rtol=0, atol=1e-10)


@pytest.mark.parametrize("kind", XO.KINDS)
def test_oracle_gradient_is_the_central_difference(kind):
	"""central differences of the oracle's own value, h = 1e-5 relative: truncation h^2 f''' / 6 and rounding eps |f| / h are both near 1e-10
	of the gradient, inside the 1e-6 asked for"""
	r = XO.reference_case()
	x, y = r["xs"][:34], r["ys"][:34]
	ls, s, w = np.array([0.4, 0.7, 0.3]), r["s"], 0.7
	g = XO.expert_fit(kind, x, y, 1.0 / ls, s, r["kappa"], w, [0, 1, 2], 3)["grad"]
	val = lambda ls_, s_: XO.expert_fit(kind, x, y, 1.0 / ls_, s_, r["kappa"], w)["value"]
	num = np.zeros(4)
	for m in range(3):
		h = 1e-5 * ls[m]
		e = np.zeros(3)
		e[m] = h
		num[m] = (val(ls + e, s) - val(ls - e, s)) / (2 * h)
	h = 1e-5 * s
	num[3] = (val(ls, s + h) - val(ls, s - h)) / (2 * h)
	print(kind, g, num)
	assert np.all(np.abs(g - num) <= 1e-6 * np.abs(num))
	# an isotropic lengthscale: one slot collects the three coordinates
	g1 = XO.expert_fit(kind, x, y, np.full(3, 2.5), s, r["kappa"], w, [0, 0, 0], 1)["grad"]
	h = 1e-5 * 0.4
	num1 = (val(np.full(3, 0.4 + h), s) - val(np.full(3, 0.4 - h), s)) / (2 * h)
	assert abs(g1[0] - num1) <= 1e-6 * abs(num1)


def test_partition_rule():
	assert XO.balanced_sizes(167, 34) == [34, 34, 33, 33, 33] and XO.balanced_sizes(10, 256) == [10] and XO.balanced_sizes(512, 256) == [256, 256]
	order, sizes = XO.partition(167, 34, "random", 0)
	assert sorted(order.tolist()) == list(range(167)) and np.array_equal(order, np.random.default_rng(0).permutation(167))
	order, sizes = XO.partition(7, 3, "contiguous")
	assert order.tolist() == list(range(7)) and sizes == [3, 2, 2]
	order, sizes = XO.partition(6, 3, [2, 0, 2, 1, 0, 2])
	assert order.tolist() == [1, 4, 3, 0, 2, 5] and sizes == [2, 1, 3]


# --------------------------------------------------------------------------------------------- 2. combination identities
def test_combination_identities():
	rng = np.random.RandomState(0)
	kappa = 1.7
	mu1, v1 = rng.normal(size=(1, 9)), rng.uniform(0.01, 1.0, size=(1, 9)) * kappa
	for mode in (XO.POE, XO.GPOE, XO.BCM):          # one expert: itself
		mu, var = XO.combine(mode, mu1, v1, kappa)
		assert np.allclose(mu, mu1[0], rtol=1e-14, atol=0) and np.allclose(var, v1[0], rtol=1e-14, atol=0), mode
	mu, var = XO.combine(XO.RBCM, mu1, v1, kappa)          # ... except under rBCM, which weighs the expert by its information gain
	assert not np.allclose(var, v1[0], rtol=1e-3, atol=0)
	# far from the data every expert returns the prior: BCM and rBCM return it too (PoE would claim kappa / E)
	mu_e, v_e = np.zeros((6, 4)), np.full((6, 4), kappa)
	for mode in (XO.BCM, XO.RBCM):
		mu, var = XO.combine(mode, mu_e, v_e, kappa)
		assert np.all(mu == 0.0) and np.allclose(var, kappa, rtol=1e-14, atol=0), mode
	assert np.allclose(XO.combine(XO.POE, mu_e, v_e, kappa)[1], kappa / 6, rtol=1e-14, atol=0)
	assert np.allclose(XO.combine(XO.GPOE, mu_e, v_e, kappa)[1], kappa, rtol=1e-14, atol=0)
	# the precision of BCM and rBCM is at least 1 / kappa on anything the clamp lets through, the clamped extremes included
	for trial in range(50):
		E = rng.randint(1, 9)
		v = kappa * 10.0 ** rng.uniform(-18, 1, size=(E, 16))
		v[rng.rand(E, 16) < 0.1] = 0.0
		v[rng.rand(E, 16) < 0.1] = -1.0
		for mode in (XO.BCM, XO.RBCM):
			mu, var = XO.combine(mode, rng.normal(size=(E, 16)), v, kappa)
			assert np.all(np.isfinite(mu)) and np.all(var > 0) and np.all(1.0 / var >= (1.0 / kappa) * (1 - 1e-12)), (mode, trial)
	assert XO.n_clamped(np.array([[0.0, kappa, 2 * kappa, 0.5 * kappa]]), kappa) == 2


# --------------------------------------------------------------------------------------------- 3. the reference case stays away from the clamp
@pytest.mark.parametrize("kind", XO.KINDS)
def test_reference_case_is_far_from_the_clamp(kind):
	r = XO.reference_case()
	assert r["sizes"] == [34, 34, 33, 33, 33] and r["xt"].shape == (65, 3)
	assert all(np.any(np.all(r["xs"] == t, axis=1)) for t in r["xt"][:20]) and not any(np.any(np.all(r["xs"] == t, axis=1)) for t in r["xt"][20:])
	o = XO.experts(kind, r["xs"], r["ys"], r["sizes"], r["inv_ls"], r["s"], r["kappa"], xt=r["xt"])
	assert XO.n_clamped(o["var_e"], r["kappa"]) == 0
	lo = float(o["var_e"].min() / r["kappa"])
	print("kind", kind, "min var_e / kappa", lo, "max", float(o["var_e"].max() / r["kappa"]))
	assert lo > 1e-3
	# the float64 formulas against np.longdouble (one expert, a Cholesky written out): far inside the 1e-8 of the GPU tests
	x, y = r["xs"][:34].astype(np.longdouble), r["ys"][:34].astype(np.longdouble)
	il, xt = r["inv_ls"].astype(np.longdouble), r["xt"].astype(np.longdouble)
	r2 = (((x[:, None, :] - x[None, :, :]) * il) ** 2).sum(axis=2)
	r2t = (((x[:, None, :] - xt[None, :, :]) * il) ** 2).sum(axis=2)

	def phi(q):
		rr = np.sqrt(q)
		s3, s5 = np.sqrt(np.longdouble(3)), np.sqrt(np.longdouble(5))
		return [np.exp(-q / 2), np.exp(-rr), (1 + s3 * rr) * np.exp(-s3 * rr), (1 + s5 * rr + 5 * q / 3) * np.exp(-s5 * rr)][kind]
	kap = np.longdouble(r["kappa"])
	K = kap * phi(r2) + np.longdouble(r["s"]) ** 2 * np.eye(34, dtype=np.longdouble)
	Lc = np.zeros_like(K)
	for j in range(34):
		Lc[j, j] = np.sqrt(K[j, j] - Lc[j, :j] @ Lc[j, :j])
		Lc[j + 1:, j] = (K[j + 1:, j] - Lc[j + 1:, :j] @ Lc[j, :j]) / Lc[j, j]
	B = np.concatenate([y[:, None], kap * phi(r2t)], axis=1)
	for j in range(34):          # forward substitution, all right-hand sides at once
		B[j] = (B[j] - Lc[j, :j] @ B[:j]) / Lc[j, j]
	var_x = kap - (B[:, 1:] ** 2).sum(axis=0)
	assert float(np.max(np.abs(o["var_e"][0] - var_x))) <= 1e-12 * r["kappa"]


@pytest.mark.parametrize("kind", XO.KINDS)
def test_border_case_oracle_against_extended_precision(kind):
	"""The mixed-size case of the GPU tests (sizes 1 .. 512, one per regime of the kernels): the float64 oracle against the restatement in extended
	precision (XO.expert_extended), every expert, with the scaling of the GPU tests' _close.  The bound is their TOL / 100 = 1e-10: rounding of
	the float64 solves is about eps cond(K_e), cond(K_e) <= 1 + kappa n / s^2 = 6.7e4 at the cap (measured: 1e3 .. 2e4), so 1e-11 at the worst.
	Measured (alpha / mu / var / value / gradient row; largest cond(K_e); min var_e / kappa):
	SE         4.5e-13 / 6.9e-14 / 8.0e-15 / 1.4e-14 / 2.1e-13; 1.7e4; 1.7e-3
	Matern 1/2 1.2e-14 / 2.2e-15 / 9.8e-16 / 4.9e-14 / 5.2e-16; 1.2e3; 7.5e-3
	Matern 3/2 4.8e-14 / 1.1e-14 / 1.9e-15 / 7.1e-16 / 3.3e-15; 9.6e3; 6.9e-3
	Matern 5/2 2.3e-13 / 2.5e-14 / 3.0e-15 / 4.4e-15 / 9.7e-14; 1.4e4; 6.0e-3"""
	c = XO.border_case()
	B = XO.BORDER
	assert c["sizes"] == B["sizes"] and sum(c["sizes"]) == 1962 and max(c["sizes"]) == 512 and c["xt"].shape == (97, 5)
	n_train = len(c["pick"])
	assert n_train == 27 and np.array_equal(c["xt"][:n_train], c["xs"][c["pick"]])
	assert not any(np.any(np.all(c["xs"] == t, axis=1)) for t in c["xt"][n_train:])
	pidx = list(range(B["d"]))
	o = XO.experts(kind, c["xs"], c["ys"], c["sizes"], c["inv_ls"], c["s"], c["kappa"], 0.7, pidx, B["d"], xt=c["xt"])
	# nothing near the clamp, as on the reference case
	assert XO.n_clamped(o["var_e"], c["kappa"]) == 0
	lo = float(o["var_e"].min() / c["kappa"])
	assert lo > 1e-3, lo
	# the far point: the prior, from every expert
	assert np.all(np.abs(o["mu_e"][:, -1]) < 1e-30) and np.all(o["var_e"][:, -1] == c["kappa"])
	off = c["offsets"]
	x = [XO.expert_extended(kind, c["xs"][off[e]:off[e + 1]], c["ys"][off[e]:off[e + 1]], c["inv_ls"], c["s"], c["kappa"], 0.7, pidx, B["d"], xt=c["xt"])
		 for e in range(len(c["sizes"]))]
	f64 = lambda a: np.asarray(a, dtype=np.float64)
	alpha_x, mu_x = np.concatenate([f["alpha"] for f in x]), np.array([f["mu"] for f in x])
	err = dict(alpha=np.max(np.abs(f64(o["alpha"] - alpha_x))) / np.max(np.abs(f64(alpha_x))),
			   mu=np.max(np.abs(f64(o["mu_e"] - mu_x))) / np.max(np.abs(f64(mu_x))),
			   var=np.max(np.abs(f64(o["var_e"] - np.array([f["var"] for f in x])))) / c["kappa"],
			   value=max(abs(float(o["value"][e] - f["value"])) / abs(float(f["value"])) for e, f in enumerate(x)),
			   grad=max(np.max(np.abs(f64(o["grad"][e] - f["grad"]))) / np.max(np.abs(f64(f["grad"]))) for e, f in enumerate(x)))
	print("kind", kind, "min var_e / kappa", lo, "cond", max(float(np.linalg.cond(f["K"])) for f in o["fits"]), {k: float(v) for k, v in err.items()})
	assert all(v <= 1e-10 for v in err.values()), err


def test_extended_precision_fallback_agrees():
	"""the mpmath route of XO.expert_extended (taken where long double is no wider than double) against the long-double one, on a small expert"""
	c = XO.border_case()
	a, b = int(c["offsets"][3]), int(c["offsets"][4])
	args = (c["xs"][a:b], c["ys"][a:b], c["inv_ls"], c["s"], c["kappa"], 0.7, [0, 1, 2, 3, 4], 5)
	if not XO._LD:
		pytest.skip("long double is no wider than double here: the mpmath route is the one the test above took")
	for kind in XO.KINDS:
		ld = XO.expert_extended(kind, *args, xt=c["xt"][:9])
		XO._LD = False
		try:
			mp = XO.expert_extended(kind, *args, xt=c["xt"][:9])
		finally:
			XO._LD = True
		for key in ("alpha", "mu", "var", "grad"):
			d = np.max(np.abs(np.asarray(ld[key], dtype=np.float64) - np.asarray(mp[key], dtype=np.float64)))
			assert d <= 1e-13 * np.max(np.abs(np.asarray(ld[key], dtype=np.float64))), (kind, key, d)
		assert abs(float(ld["value"]) - float(mp["value"])) <= 1e-13 * abs(float(ld["value"]))


# --------------------------------------------------------------------------------------------- 4. host behaviour without the device
@pytest.fixture
def no_device(monkeypatch):
	from stpy_amd import _lib

	def boom(*a, **k):
		raise AssertionError("the device was touched")
	for name in ("device", "to_device", "load"):
		monkeypatch.setattr(_lib, name, boom)
	return _lib


def test_host_side_without_the_device(no_device):
	import stpy_amd
	from stpy_amd.continuous_processes import local_experts as LE
	from stpy_amd.kernels import KernelFunction
	gp = stpy_amd.LocalExpertsGaussianProcess(gamma=0.4, s=0.1, kappa=1.3, d=3, expert_size=34)
	assert gp.experts_info == {"E": 0, "sizes": [], "launches": 0, "factor_bytes": 0} and gp.fitted is False
	assert "local experts" in gp.description()
	for kw in (dict(expert_size=0), dict(expert_size=513), dict(combine="mean"), dict(partition="kmeans"), dict(max_size=0)):
		with pytest.raises(ValueError):
			stpy_amd.LocalExpertsGaussianProcess(d=2, **kw)
	for name in ("matern", "ard", "ard_matern"):
		stpy_amd.LocalExpertsGaussianProcess(kernel_name=name, d=2, nu=2.5)
	with pytest.raises(NotImplementedError, match="composite"):
		stpy_amd.LocalExpertsGaussianProcess(kernel=KernelFunction(kernel_name="ard", d=2) + KernelFunction(kernel_name="matern", d=2))
	with pytest.raises(NotImplementedError):
		stpy_amd.LocalExpertsGaussianProcess(kernel_name="linear", d=2)
	x, y = torch.rand(40, 3).double(), torch.rand(40, 1).double()
	with pytest.raises(NotImplementedError, match="Sigma"):
		gp.fit_gp(x, y, Sigma=torch.eye(40).double())
	with pytest.raises(NotImplementedError, match="float32"):
		gp.fit_gp(x.float(), y.float())
	with pytest.raises(NotImplementedError, match="requires_grad"):
		gp.mean_std(x.clone().requires_grad_(True))
	with pytest.raises(NotImplementedError):
		gp.optimize_params(type="rots")
	with pytest.raises(NotImplementedError):
		gp.ucb_optimize(2.0)
	with pytest.raises(AttributeError):
		gp.log_marginal(gp.kernel_object, {}, 1.0)
	with pytest.raises(NotImplementedError):
		gp.log_marginal(gp.kernel_object, {'1': {'gamma': torch.ones(1)}}, 1.0)
	mu, sd = gp.mean_std(x)          # unfitted: the prior
	assert torch.all(mu == 0) and torch.allclose(sd, torch.full((40, 1), 1.3 ** 0.5).double())
	# an explicit assignment above the cap is refused before anything is sent anywhere
	gp2 = stpy_amd.LocalExpertsGaussianProcess(d=3, partition=torch.cat([torch.zeros(513, dtype=torch.int64), torch.ones(7, dtype=torch.int64)]))
	with pytest.raises(ValueError, match="expert 0 has 513"):
		gp2.fit_gp(torch.rand(520, 3).double(), torch.rand(520, 1).double())
	assert gp2.fitted is False
	# the partition: the oracle's rule, deterministic in the seed, balanced within one
	for n, size in ((167, 34), (1000, 256), (5, 512), (512, 512), (513, 512)):
		o1, s1 = LE.partition_points(n, size, "random", 3)
		o2, s2 = LE.partition_points(n, size, "random", 3)
		o3, _ = LE.partition_points(n, size, "random", 4)
		oo, so = XO.partition(n, size, "random", 3)
		assert np.array_equal(o1, o2) and np.array_equal(o1, oo) and s1.tolist() == so and (n < 10 or not np.array_equal(o1, o3))
		assert s1.sum() == n and s1.max() - s1.min() <= 1 and s1.max() <= size and len(s1) == -(-n // size)
		assert LE.partition_points(n, size, "contiguous")[0].tolist() == list(range(n))
	o, s = LE.partition_points(6, 3, torch.tensor([2, 0, 2, 1, 0, 2]))
	assert o.tolist() == [1, 4, 3, 0, 2, 5] and s.tolist() == [2, 1, 3]
	with pytest.raises(ValueError):
		LE.partition_points(6, 3, torch.tensor([0.0, 1.0, 0.0, 1.0, 0.0, 1.0]))
	with pytest.raises(ValueError):
		LE.partition_points(6, 3, torch.tensor([0, 1, 0]))


# --------------------------------------------------------------------------------------------- 5. argument checks of the C ABI
def test_experts_argument_checks():
	from stpy_amd import _lib as L
	lib = L.load()
	P, N = ctypes.c_void_p(0x1000), None          # a non-null, 16-byte aligned pointer no refused call may dereference
	Q = ctypes.c_void_p(0x1004)                    # ... and a misaligned one
	assert lib.stpy_experts_max_n() == lib.stpy_lml_batch_max_n() == 512
	big = 1 << 50

	def fit(kind=0, dtype=0, xs=P, n=100, ldx=4, d=4, cols=N, ys=P, offsets=P, E=3, nmax=64, inv_ls=P, noise=P, kappa=1.0, weight=1.0, pidx=P, np_=1,
			factor=P, fbytes=big, alpha=P, value=P, grad=P, ldg=2, total=P, info=P, work=P, wbytes=big):
		return lib.stpy_experts_fit(kind, dtype, xs, n, ldx, d, cols, ys, offsets, E, nmax, inv_ls, noise, kappa, weight, pidx, np_, factor, fbytes, alpha,
									value, grad, ldg, total, info, work, wbytes, N)

	def predict(kind=0, dtype=0, xs=P, n=100, ldx=4, d=4, cols=N, offsets=P, E=3, nmax=64, inv_ls=P, kappa=1.0, factor=P, fbytes=big, alpha=P, info=P,
				xt=P, M=70, ldt=4, mu_e=P, var_e=P, ldm=70, work=P, wbytes=big):
		return lib.stpy_experts_predict(kind, dtype, xs, n, ldx, d, cols, offsets, E, nmax, inv_ls, kappa, factor, fbytes, alpha, info, xt, M, ldt,
										mu_e, var_e, ldm, work, wbytes, N)

	def combine(mode=3, E=3, M=70, mu_e=P, var_e=P, ldm=70, kappa=1.0, mu=P, var=P):
		return lib.stpy_experts_combine(mode, E, M, mu_e, var_e, ldm, kappa, mu, var, N)

	wfit, wpred, fb = lib.stpy_experts_fit_workspace_bytes(0, 64, 4, 3), lib.stpy_experts_predict_workspace_bytes(0, 64, 4, 3, 70), lib.stpy_experts_factor_bytes(0, 64, 3)
	assert wfit == 3 * (64 * 64 + 32 * 64) * 8 and fb == 3 * 64 * 64 * 8 and wpred == 3 * 3 * 32 * 64 * 8
	assert lib.stpy_experts_fit_workspace_bytes(0, 33, 4, 3) == wfit and lib.stpy_experts_fit_workspace_bytes(1, 64, 4, 3) == 0
	common = {"unknown kind": dict(kind=9), "negative kind": dict(kind=-1), "LINEAR": dict(kind=4), "fp32": dict(dtype=1), "unknown dtype": dict(dtype=7),
			  "nmax above the cap": dict(nmax=513), "ldx < d": dict(ldx=3), "d < 1": dict(d=0), "null xs": dict(xs=N), "null offsets": dict(offsets=N),
			  "null inv_ls": dict(inv_ls=N), "null factor": dict(factor=N), "null alpha": dict(alpha=N), "null info": dict(info=N), "null work": dict(work=N),
			  "kappa 0": dict(kappa=0.0), "kappa nan": dict(kappa=float("nan")), "misaligned work": dict(work=Q), "misaligned factor": dict(factor=Q),
			  "misaligned xs": dict(xs=Q), "small factor": dict(fbytes=fb - 1), "E out of range": dict(E=1 << 31)}
	cases = [("stpy_experts_fit", fit, dict(common, **{"null ys": dict(ys=N), "null noise": dict(noise=N), "null value": dict(value=N), "null total": dict(total=N),
			  "grad without pidx": dict(pidx=N), "np < 1": dict(np_=0), "ldg < np + 1": dict(np_=2, ldg=2), "small workspace": dict(wbytes=wfit - 1)})),
			 ("stpy_experts_predict", predict, dict(common, **{"null xt": dict(xt=N), "null mu_e": dict(mu_e=N), "null var_e": dict(var_e=N), "ldt < d": dict(ldt=3),
			  "ldm < M": dict(ldm=69), "negative M": dict(M=-1), "small workspace": dict(wbytes=wpred - 1), "misaligned mu_e": dict(mu_e=Q)})),
			 ("stpy_experts_combine", combine, {"mode 4": dict(mode=4), "mode -1": dict(mode=-1), "null mu_e": dict(mu_e=N), "null var_e": dict(var_e=N),
			  "null mu": dict(mu=N), "null var": dict(var=N), "ldm < M": dict(ldm=69), "kappa 0": dict(kappa=0.0), "kappa inf": dict(kappa=float("inf")),
			  "negative E": dict(E=-1), "misaligned var": dict(var=Q)})]
	for name, call, refused in cases:
		for what, kw in refused.items():
			lib.stpy_lml_batch(0, 1, N, 1, 1, 1, N, N, 1, N, 1, N, 1.0, 1.0, N, 1, N, N, 2, N, N, 0, N)          # (leaves some OTHER message behind)
			before = lib.stpy_last_error_string()
			rc = call(**kw)
			assert rc < 0, (name, what, rc)
			msg = lib.stpy_last_error_string()
			assert msg and name.encode() in msg and msg != before, (name, what, msg)
	# float32 is -2, as for stpy_lml_batch
	assert fit(dtype=1) == -2 and predict(dtype=1) == -2
	# a fit without a gradient needs neither pidx nor np
	# (nothing refused is left: such a call would launch, so it is not made here)
	# the empty problems: 0 without looking at a pointer
	assert fit(E=0, xs=N, ys=N, offsets=N, work=N, factor=N) == 0 and fit(n=0, xs=N) == 0
	assert predict(E=0, xs=N, work=N) == 0 and predict(M=0, xt=N) == 0 and predict(n=0, xs=N) == 0
	assert combine(E=0, mu_e=N) == 0 and combine(M=0, mu=N) == 0
	# the queries do not decrease in nmax, E, M
	last = 0
	for nmax in (1, 31, 32, 33, 100, 256, 511, 512):
		b = lib.stpy_experts_fit_workspace_bytes(0, nmax, 4, 5) + lib.stpy_experts_predict_workspace_bytes(0, nmax, 4, 5, 33) + lib.stpy_experts_factor_bytes(0, nmax, 5)
		assert b > 0 and b >= last
		last = b
	assert lib.stpy_experts_predict_workspace_bytes(0, 64, 4, 3, 64) < lib.stpy_experts_predict_workspace_bytes(0, 64, 4, 3, 65)


# --------------------------------------------------------------------------------------------- 6. kernel resources
def test_experts_kernel_resources(tmp_path):
	"""Every kernel of csrc/experts.hip: no scratch (in particular no stack: the diagonal-block routine is inlined), at most 40 KiB of LDS -- the
	figure of DESIGN.md "Local experts", which lets two fits (or four predictions) share a CU under the 160 KB limit"""
	out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-comment", "-c", os.path.join(CSRC, "experts.hip"),
						  "-o", str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True).stderr
	blocks = [b for b in re.split(r"remark: Function Name: ", out)[1:] if "experts_" in b.split()[0]]
	names = " ".join(b.split()[0] for b in blocks)
	for kernel in ("experts_fit_kernelILb1", "experts_fit_kernelILb0", "experts_predict_kernel", "experts_combine_kernel", "experts_total_kernel"):
		assert kernel in names, (kernel, names)
	for b in blocks:
		name = b.split()[0]
		assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, name
		assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) <= 40960, name
		assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)) >= 2, name
