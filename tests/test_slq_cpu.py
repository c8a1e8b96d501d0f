"""
The stochastic evidence, the parts that need no GPU: the oracle of tests/slq_oracle.py against dense linear algebra (the quadrature from CG
coefficients, the estimates against the exact evidence and its gradient, an optimisation run on the estimate), the error bound of
stpy_kmv_dtheta against a working-precision emulation, the argument checks of stpy_kmv_dtheta and stpy_pcg_lanczos (every refusal comes
before the first HIP call, so placeholder pointers are safe), the kernels' resource usage, and the host refusals of the new methods.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.optimize
import torch

from tests import kmv_oracle as KO
from tests import slq_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stpy_amd", "csrc")
P, N = ctypes.c_void_p(0x1000), None          # a non-null pointer no refused call may dereference
BIG = 1 << 40
CASES = (0, 3, 4)
T_PROBES = 16


def _estimate(idx):
	return SO.case_estimate(idx, T_PROBES)


# --------------------------------------------------------------------------------------------- 1. the bound of stpy_kmv_dtheta
def _dtheta_inputs(n, d, t, seed, duplicates=False):
	rng = np.random.RandomState(seed)
	x = rng.uniform(-1, 1, size=(n, d))
	if duplicates:
		x[n // 2:n // 2 + n // 4] = x[:n // 4]                          # rho == 0 off the diagonal
	il = rng.uniform(0.5, 3.0, size=(d,)) / np.sqrt(d)
	return x, il, rng.standard_normal((t, n)), rng.standard_normal((t, n))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("kind", list(KO.KIND_CODE))
def test_kmv_dtheta_bound_holds_for_a_working_precision_emulation(kind, dtype):
	"""The subtract-first evaluation in the working dtype stays within the bound of slq_oracle.kmv_dtheta_bound with at least 4x room, on
	plain and on duplicated points (the Matern 1/2 guard: no NaN, exactly the longdouble truth's zero contribution)."""
	eps = KO.eps_of(dtype)
	for (n, d, t, dup) in ((65, 1, 2, False), (129, 3, 3, True), (200, 7, 2, False), (64, 12, 1, True)):
		x, il, U, V = (v.astype(dtype).astype(np.float64) for v in _dtheta_inputs(n, d, t, 11 * n + d, dup))
		truth, S0, S1, SK, SD = SO.kmv_dtheta_dense(kind, x, il, U, V, kappa=1.3)
		bound = SO.kmv_dtheta_bound(n, d, eps, *(np.asarray(v, dtype=np.float64) for v in (S0, S1, SK, SD)))
		got = SO.kmv_dtheta_emulated(kind, x, il, U, V, dtype, kappa=1.3)
		assert np.all(np.isfinite(got.astype(np.float64)))
		err = np.abs(got.astype(np.longdouble) - truth).astype(np.float64)
		ratio = float(np.max(err / bound))
		print("%s %s n=%d d=%d: largest error / bound %.3f" % (kind, np.dtype(dtype).name, n, d, ratio))
		assert 4 * ratio <= 1.0, (kind, n, d, ratio)


def test_kmv_dtheta_dense_is_the_derivative_of_the_kernel():
	"""out[c, k] / inv_ls[k] is d(u^T K v) / d inv_ls[k] (central differences of the dense kernel), for all four kinds."""
	x, il, U, V = _dtheta_inputs(40, 3, 2, 5)
	gam = 1.0 / il
	for kind in KO.KIND_CODE:
		out = SO.kmv_dtheta_dense(kind, x, il, U, V, kappa=0.7)[0].astype(np.float64)
		K = SO.NO.kernel(kind, x, x, gam, 0.7)
		assert np.allclose(out[:, 3], np.einsum("ci,ij,cj->c", U, K, V), rtol=1e-12)
		assert np.allclose(out[:, 4], np.sum(U * V, axis=1), rtol=1e-12)
		for k in range(3):
			h = 1e-6 * il[k]
			ilp, ilm = il.copy(), il.copy()
			ilp[k] += h
			ilm[k] -= h
			fd = np.einsum("ci,ij,cj->c", U, (SO.NO.kernel(kind, x, x, 1.0 / ilp, 0.7) - SO.NO.kernel(kind, x, x, 1.0 / ilm, 0.7)) / (2 * h), V)
			assert np.allclose(out[:, k] / il[k], fd, rtol=1e-6, atol=1e-8), (kind, k)


# --------------------------------------------------------------------------------------------- 2. the quadrature and the estimates
@pytest.mark.parametrize("idx", CASES, ids=[KO.PCG_IDS[i] for i in CASES])
def test_quadrature_from_cg_coefficients_is_the_dense_form(idx):
	e, (kind, x, y, gamma, s, r, cols, W, tol) = _estimate(idx)
	qd = SO.q_dense(e["A"], e["G"], e["Z"], s)
	rel = np.abs(qd - e["q"]).max() / np.abs(qd).max()
	print("%s: q from coefficients against the dense form, relative to max|q|: %.2e" % (KO.PCG_IDS[idx], rel))
	assert rel <= 1e-10


@pytest.mark.parametrize("idx", CASES, ids=[KO.PCG_IDS[i] for i in CASES])
def test_estimates_lie_within_three_standard_errors_of_the_exact_ones(idx):
	e, (kind, x, y, gamma, s, r, cols, W, tol) = _estimate(idx)
	ex = SO.exact(kind, x, y, gamma, s, cols)
	g_exact = ex["grad_loggamma"].sum()                                   # ONE gamma: the sum over the coordinates it scales
	print("%s: value %.4f +- %.4f (exact %.4f), d/dlog gamma %.4f +- %.4f (exact %.4f), d/ds %.3f +- %.3f (exact %.3f), fitted beta %.4f" % (
		KO.PCG_IDS[idx], e["value"], e["stderr"], ex["value"], e["grad_loggamma"][0], e["grad_loggamma_stderr"][0], g_exact, e["grad_s"], e["grad_s_stderr"],
		ex["grad_s"], e["beta"][0]))
	assert abs(e["value"] - ex["value"]) <= 3 * e["stderr"]
	assert abs(e["logdet"] - ex["logdet"]) <= 3 * e["logdet_stderr"]
	assert abs(e["grad_loggamma"][0] - g_exact) <= 3 * e["grad_loggamma_stderr"][0]
	assert abs(e["grad_s"] - ex["grad_s"]) <= 3 * e["grad_s_stderr"]


def test_the_control_variates_matter():
	"""Case 3 where the rank-24 factor is exact to rounding (gamma = 0.5): the value's standard error and the gradient's are both below 1e-6
	with the control variates; the plain trace estimator mean_c u_c^T dA v_c keeps a standard error above 1 there."""
	kind, n, d, gamma, r, cols = KO.PCG_CASES[3]
	s, tol = KO.SETTINGS["float64"]
	x, y, _ = KO.case_data(3)
	e = SO.estimate(kind, x, y, 0.5, s, r, SO.probes(n, r, T_PROBES, 103), tol)
	plain = np.array([e["U"][:, c] @ e["dK"][0] @ e["V"][:, c] for c in range(T_PROBES)])
	print("se 300 at gamma 0.5: stderr value %.2e, gradient %.2e (beta %.6f); plain trace estimator %.2e" % (
		e["stderr"], e["grad_loggamma_stderr"][0], e["beta"][0], plain.std(ddof=1) / 4))
	assert e["stderr"] < 1e-6 and e["grad_loggamma_stderr"][0] < 1e-6 and plain.std(ddof=1) / 4 > 1.0


def f32_deviation():
	"""(value, d/dgamma, d/ds) deviations of the float32 restatement of case 4 from the float64 one solved to 1e-8, relative to the latter."""
	e32, (kind, x, y, gamma, s, r, cols, W, tol) = SO.case_estimate(4, T_PROBES, "float32")
	e64 = SO.estimate(kind, x, y, gamma, s, r, W, 1e-8, cols=cols, dtype=np.float64)
	return tuple(abs(a - b) / abs(b) for a, b in ((e32["value"], e64["value"]), (e32["grad_loggamma"][0], e64["grad_loggamma"][0]), (e32["grad_s"], e64["grad_s"]))), e64


def test_float32_restatement_constant():
	"""slq_oracle.F32_RESTATEMENT_DEVIATION is what this file computes, within a factor 5 either way."""
	got, _ = f32_deviation()
	print("float32 restatement of case 4 against float64: value %.3e, d/dgamma %.3e, d/ds %.3e (relative)" % got)
	for g, const in zip(got, SO.F32_RESTATEMENT_DEVIATION):
		assert const / 5 <= g <= 5 * const, (g, const)


def test_oracle_optimisation_run():
	"""scipy L-BFGS-B on the ORACLE's estimate of case 3 (se, n = 300, d = 1) with t = 16 fixed probes, from gamma = 0.5: the end point's exact
	dense objective is below the start's and not above the minimum of the exact objective over 200 log-spaced gamma in [0.01, 1] by more than
	4 standard errors of the estimate there.  t = 16 suffices (8 evaluations; the end point lies BELOW the grid's minimum by 2e-4)."""
	kind, n, d, gamma0, r, cols = KO.PCG_CASES[3]
	s, tol = KO.SETTINGS["float64"]
	x, y, _ = KO.case_data(3)
	W = SO.probes(n, r, T_PROBES, 103)

	def fun(g):
		e = SO.estimate(kind, x, y, float(g[0]), s, r, W, tol)
		return e["value"], np.array([e["grad_loggamma"][0] / g[0]])
	res = scipy.optimize.minimize(fun, np.array([0.5]), jac=True, method="L-BFGS-B", bounds=[(0.01, 1.0)], options={"maxiter": 100, "gtol": 1e-4, "ftol": 1e-12})
	g_end = float(res.x[0])
	stderr = SO.estimate(kind, x, y, g_end, s, r, W, tol)["stderr"]
	f_end, f_start, f_grid = SO.exact(kind, x, y, g_end, s)["value"], SO.exact(kind, x, y, 0.5, s)["value"], grid_minimum()
	print("oracle run: gamma %.5f after %d evaluations, exact objective %.6f (start %.6f, grid minimum %.6f), stderr there %.2e" % (
		g_end, res.nfev, f_end, f_start, f_grid, stderr))
	assert f_end < f_start
	assert f_end <= f_grid + 4 * stderr


_GRID = {}


def grid_minimum():
	"""Minimum of the exact objective of case 3 over 200 log-spaced gamma in [0.01, 1] (computed once; the GPU test reads it too)."""
	if "min" not in _GRID:
		kind, n, d, gamma0, r, cols = KO.PCG_CASES[3]
		s, _ = KO.SETTINGS["float64"]
		x, y, _ = KO.case_data(3)
		_GRID["min"] = min(SO.exact(kind, x, y, g, s)["value"] for g in np.exp(np.linspace(np.log(0.01), np.log(1.0), 200)))
	return _GRID["min"]


# --------------------------------------------------------------------------------------------- 3. argument checks
def _leave_another_message(lib):
	lib.stpy_lml_batch(0, 1, N, 1, 1, 1, N, N, 1, N, 1, N, 1.0, 1.0, N, 1, N, N, 2, N, N, 0, N)
	return lib.stpy_last_error_string()


def _all_refused(lib, call, refused, name):
	for what, (kw, code) in refused.items():
		before = _leave_another_message(lib)
		rc = call(**kw)
		assert rc == code, (what, rc, code)
		msg = lib.stpy_last_error_string()
		assert msg and name in msg and msg != before, (what, msg)


def test_kmv_dtheta_argument_checks():
	from stpy_amd import _lib as L
	lib = L.load()

	def call(kind=0, dtype=0, x=P, n=64, ldx=4, d=4, cols=N, inv_ls=P, kappa=1.0, Ut=P, ldu=64, Vt=P, ldv=64, t=3, out=P, ldo=6, work=P, work_bytes=BIG):
		return lib.stpy_kmv_dtheta(kind, dtype, x, n, ldx, d, cols, inv_ls, kappa, Ut, ldu, Vt, ldv, t, out, ldo, work, work_bytes, N)

	need = lib.stpy_kmv_dtheta_workspace_bytes(0, 64, 4, 3)
	assert need > 0
	refused = {
		"unknown kind": (dict(kind=9), -1), "negative kind": (dict(kind=-1), -1), "LINEAR": (dict(kind=4), -1),
		"unknown dtype": (dict(dtype=7), -2), "negative dtype": (dict(dtype=-1), -2),
		"null x": (dict(x=N), -3), "null inv_ls": (dict(inv_ls=N), -3), "null Ut": (dict(Ut=N), -3), "null Vt": (dict(Vt=N), -3), "null out": (dict(out=N), -3),
		"negative n": (dict(n=-1), -4), "n >= 2^31": (dict(n=1 << 31, ldu=1 << 31, ldv=1 << 31), -4),
		"ldx < d": (dict(ldx=3), -5), "d < 1": (dict(d=0), -6), "negative d": (dict(d=-2), -6), "t < 1": (dict(t=0), -10), "negative t": (dict(t=-4), -10),
		"nan kappa": (dict(kappa=float("nan")), -11), "inf kappa": (dict(kappa=float("inf")), -11),
		"ldu < n": (dict(ldu=63), -13), "ldv < n": (dict(ldv=63), -13), "ldo < d + 2": (dict(ldo=5), -13),
		"misaligned work": (dict(work=ctypes.c_void_p(0x1004)), -17),
		"null work": (dict(work=N), -20), "undersized work": (dict(work_bytes=need - 1), -20),
		"undersized work fp32": (dict(dtype=1, work_bytes=lib.stpy_kmv_dtheta_workspace_bytes(1, 64, 4, 3) - 1), -20),
	}
	_all_refused(lib, call, refused, b"stpy_kmv_dtheta")
	# the workspace holds one partial row per workgroup and pair: positive, and enough for the cut j range of a small problem
	for dtype in (0, 1):
		for (n, d, t) in ((1, 1, 1), (64, 4, 3), (2500, 3, 5), (777, 20, 33), (65536, 16, 17)):
			assert lib.stpy_kmv_dtheta_workspace_bytes(dtype, n, d, t) >= ((n + 63) // 64) * t * (d + 1) * (4 if dtype else 8)


def test_pcg_lanczos_argument_checks():
	from stpy_amd import _lib as L
	lib = L.load()

	def call(kind=0, dtype=0, x=P, n=64, ldx=4, d=4, cols=N, inv_ls=P, kappa=1.0, diag_add=0.01, Gt=P, ldgt=64, Gn=P, ldgn=8, r=8, Bt=P, ldb=64,
			 Xt=P, ldxt=64, t=3, tol=1e-8, iters=10, init=1, relres=P, bx=P, its=P, coef=P, cap=10, rz0=P, work=P, work_bytes=BIG):
		return lib.stpy_pcg_lanczos(kind, dtype, x, n, ldx, d, cols, inv_ls, kappa, diag_add, Gt, ldgt, Gn, ldgn, r, Bt, ldb, Xt, ldxt, t, tol, iters, init,
									relres, bx, its, coef, cap, rz0, work, work_bytes, N)

	need = lib.stpy_pcg_workspace_bytes(0, 64, 4, 3, 8)
	refused = {
		"null coef": (dict(coef=N), -3), "null rz0": (dict(rz0=N), -3), "cap < 1": (dict(cap=0), -19), "negative cap": (dict(cap=-5), -19),
		"unknown kind": (dict(kind=9), -1), "unknown dtype": (dict(dtype=7), -2), "null x": (dict(x=N), -3), "null Bt": (dict(Bt=N), -3),
		"null its": (dict(its=N), -3), "negative n": (dict(n=-1), -4), "ldx < d": (dict(ldx=3), -5), "d < 1": (dict(d=0), -6), "t < 1": (dict(t=0), -10),
		"nan kappa": (dict(kappa=float("nan")), -11), "ldb < n": (dict(ldb=63), -13), "negative tol": (dict(tol=-1e-3), -14), "iters < 0": (dict(iters=-1), -15),
		"r < 0": (dict(r=-1), -16), "r > 0 with null Gt": (dict(Gt=N), -3), "ldgn < r": (dict(ldgn=7), -18),
		"null work": (dict(work=N), -20), "undersized work": (dict(work_bytes=need - 1), -20),
	}
	_all_refused(lib, call, refused, b"stpy_pcg_lanczos")
	assert call(n=0) == 0                                                 # the empty problem


# --------------------------------------------------------------------------------------------- 4. kernel resources
def test_kmv_dtheta_kernel_resources(tmp_path):
	"""kmvgrad.hip compiles alone; every kernel: no scratch, no spills, at most 64 KiB of LDS."""
	out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-comment", "-c", os.path.join(CSRC, "kmvgrad.hip"),
						  "-o", str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True).stderr
	blocks = [b for b in re.split(r"remark: Function Name: ", out)[1:] if "kmvd" in b.split()[0]]
	assert sum("kmvd_kernel" in b.split()[0] for b in blocks) == 8          # registers up to d = 4, 8 and 16, the general form, in both types
	assert sum("kmvd_reduce_kernel" in b.split()[0] for b in blocks) == 2
	for b in blocks:
		name = b.split()[0]
		assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, name
		assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, name
		assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) <= 65536, name


# --------------------------------------------------------------------------------------------- 5. the class refuses on the host
def test_estimate_methods_refuse_on_the_host(monkeypatch):
	from stpy_amd import IterativeGaussianProcess, KernelFunction, _lib

	def no_device(*a, **k):
		raise AssertionError("the device was touched")
	for name in ("device", "to_device", "load", "pchol", "pcg", "pcg_lanczos", "kmv", "kmv_dtheta", "gemm_nt"):
		monkeypatch.setattr(_lib, name, no_device)
	for bad in (dict(num_probes=1), dict(num_probes=0), dict(num_probes=-3)):
		with pytest.raises(ValueError, match="num_probes"):
			IterativeGaussianProcess(d=2, **bad)
	gp = IterativeGaussianProcess(gamma=0.4, s=0.2, d=2, num_probes=5, probe_seed=11)
	assert (gp.num_probes, gp.probe_seed) == (5, 11) and gp.evidence_info is None
	assert IterativeGaussianProcess(d=2).num_probes == 16 and IterativeGaussianProcess(d=2).probe_seed == 0
	gp.x, gp.y = torch.zeros(20, 2).double(), torch.zeros(20, 1).double()
	unsupported = {
		"another item": {"1": {"gamma": torch.tensor([0.3])}},
		"cov": {"0": {"cov": torch.eye(2).double()}},
		"groups": {"0": {"ard_gamma": torch.ones(2).double(), "groups": [[0], [1]]}},
		"degree": {"0": {"degree": 2}},
		"gradient of kappa": {"0": {"gamma": torch.tensor([0.3]), "kappa": torch.tensor([1.0], requires_grad=True)}},
		"not a dictionary": {"0": 3.0},
	}
	for what, X in unsupported.items():
		with pytest.raises(NotImplementedError, match="log_marginal_estimate"):
			gp.log_marginal_estimate(gp.kernel_object, X, 1.0)
	with pytest.raises(NotImplementedError):
		gp.log_marginal_estimate(KernelFunction(kernel_name="linear", d=2), {}, 1.0)
	with pytest.raises(AttributeError, match="fit_gp"):
		IterativeGaussianProcess(d=2).log_marginal_estimate()
	for kw in (dict(type="rots"), dict(type="covariance"), dict(regularizer=("lasso", 0.1))):
		with pytest.raises(NotImplementedError, match="optimize_params_estimate"):
			gp.optimize_params_estimate(**kw)
	gp.num_probes = 1                                                       # (set after construction: refused at the call as well)
	with pytest.raises(ValueError, match="num_probes"):
		gp.log_marginal_estimate()
	# the exact names go on refusing
	with pytest.raises(NotImplementedError, match="Lanczos"):
		gp.log_marginal(gp.kernel_object, {}, 1.0)
	with pytest.raises(NotImplementedError, match="Lanczos"):
		gp.optimize_params(type="bandwidth", restarts=1)
	assert gp.fitted is False and gp.evidence_info is None
