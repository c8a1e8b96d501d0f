"""
Matrix-free second-order and standard-deviation input derivatives, the parts that need no GPU: the argument checks of stpy_kmv_dxx (every
refusal comes before the first HIP call, so placeholder pointers are safe), its workspace query, the kernels' resource usage, the oracle of
tests/kmv_dxx_oracle.py against central differences and against a working-precision emulation, the condition the derivative tests put on
their test points, and the host behaviour of the new methods of IterativeGaussianProcess.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import kmv_oracle as KO
from tests import kmv_dxx_oracle as XO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stpy_amd", "csrc")
P, N = ctypes.c_void_p(0x1000), None          # a non-null pointer no refused call may dereference
BIG = 1 << 40


# --------------------------------------------------------------------------------------------- 1. argument checks and the workspace query
def _leave_another_message(lib):
	lib.stpy_lml_batch(0, 1, N, 1, 1, 1, N, N, 1, N, 1, N, 1.0, 1.0, N, 1, N, N, 2, N, N, 0, N)
	return lib.stpy_last_error_string()


def test_kmv_dxx_argument_checks():
	from stpy_amd import _lib as L
	lib = L.load()

	def call(kind=0, dtype=0, a=P, n=64, lda=4, b=P, q=64, ldb=4, d=4, cols=N, inv_ls=P, kappa=1.0, Vt=P, ldv=64, t=3, out=P, ldc=64 * 15, ldo=15,
			 work=P, work_bytes=BIG):
		return lib.stpy_kmv_dxx(kind, dtype, a, n, lda, b, q, ldb, d, cols, inv_ls, kappa, Vt, ldv, t, out, ldc, ldo, work, work_bytes, N)

	need = lib.stpy_kmv_dxx_workspace_bytes(0, 64, 64, 4, 3)
	assert need > 0
	wide = dict(d=17, lda=17, ldb=17, ldo=171, ldc=64 * 171)
	refused = {
		"unknown kind": (dict(kind=9), -1), "negative kind": (dict(kind=-1), -1), "LINEAR": (dict(kind=4), -1), "POLY": (dict(kind=5 | (2 << 8)), -1),
		"MATERN12": (dict(kind=1), -1), "MATERN32": (dict(kind=2), -1),
		"unknown dtype": (dict(dtype=7), -2), "negative dtype": (dict(dtype=-1), -2),
		"null a": (dict(a=N), -3), "null b": (dict(b=N), -3), "null inv_ls": (dict(inv_ls=N), -3), "null Vt": (dict(Vt=N), -3), "null out": (dict(out=N), -3),
		"null work": (dict(work=N), -20), "undersized work": (dict(work_bytes=need - 1), -20),
		"undersized work fp32": (dict(dtype=1, work_bytes=lib.stpy_kmv_dxx_workspace_bytes(1, 64, 64, 4, 3) - 1), -20),
		"undersized work, cut range": (dict(n=5, q=2500, ldv=2500, ldc=75, work_bytes=lib.stpy_kmv_dxx_workspace_bytes(0, 5, 2500, 4, 3) - 1), -20),
		"misaligned work": (dict(work=ctypes.c_void_p(0x1004)), -17),
		"negative n": (dict(n=-1), -4), "n >= 2^31": (dict(n=1 << 31, ldc=15 << 31), -4), "negative q": (dict(q=-1), -4), "q >= 2^31": (dict(q=1 << 31, ldv=1 << 31), -4),
		"lda < d": (dict(lda=3), -5), "ldb < d": (dict(ldb=3), -5), "d < 1": (dict(d=0), -6), "negative d": (dict(d=-2), -6),
		"d = 17": (wide, -6), "d = 20": (dict(d=20, lda=20, ldb=20, ldo=231, ldc=64 * 231), -6),
		"t < 1": (dict(t=0), -10), "negative t": (dict(t=-4), -10), "too many row blocks": (dict(t=65536 * 16), -10),
		"too many row blocks x groups": (dict(t=65535 * 16 // 3 + 16), -10),
		"ldv < q": (dict(ldv=63), -13), "ldo < 1 + d + d (d + 1) / 2": (dict(ldo=14), -22), "ldo of stpy_kmv_dx": (dict(ldo=5, ldc=64 * 5), -22),
		"ldc < n * ldo": (dict(ldc=64 * 15 - 1), -23), "ldc < n * padded ldo": (dict(ldo=17), -23),
		"nan kappa": (dict(kappa=float("nan")), -11), "inf kappa": (dict(kappa=float("inf")), -11),
	}
	for what, (kw, code) in refused.items():
		before = _leave_another_message(lib)
		rc = call(**kw)
		assert rc == code, (what, rc)
		msg = lib.stpy_last_error_string()
		assert msg and b"stpy_kmv_dxx" in msg and msg != before, (what, msg)
	# d = 16 is served: with everything else in order the first thing d = 17 trips over is d itself
	assert call(d=16, lda=16, ldb=16, ldo=153, ldc=64 * 153, work=N) == -20
	# the empty output: 0 without looking at a pointer
	assert lib.stpy_kmv_dxx(0, 0, N, 0, 4, N, 64, 4, 4, N, N, 1.0, N, 64, 3, N, 0, 15, N, 0, N) == 0
	assert lib.stpy_kmv_dxx(3, 1, N, 0, 4, N, 0, 4, 4, N, N, 1.0, N, 0, 3, N, 0, 15, N, 0, N) == 0


def test_kmv_dxx_workspace_query_is_monotone():
	"""Positive everywhere and non-decreasing in n, q and t (stpy_kmv_dx's is not: it drops to nothing once the chip is full); room for at least
	two pieces where few queries meet many points, and bounded where the chip is full."""
	from stpy_amd import _lib as L
	lib = L.load()
	sizes = (1, 2, 5, 63, 64, 65, 256, 257, 1000, 4099, 16320, 16321, 65536, 1 << 20, (1 << 31) - 1)
	for dtype in (0, 1):
		esz = 4 if dtype else 8
		for d in (1, 3, 8, 16):
			for t in (1, 16, 70):
				for q in (1, 300, 1000, 1 << 20):
					last = 0
					for n in sizes:
						b = lib.stpy_kmv_dxx_workspace_bytes(dtype, n, q, d, t)
						assert b > 0 and b >= last, (n, q, d, t, b, last)
						last = b
				for n in (1, 5, 64, 1000, 1 << 20):
					last = 0
					for q in (0,) + sizes:
						b = lib.stpy_kmv_dxx_workspace_bytes(dtype, n, q, d, t)
						assert b > 0 and b >= last, (n, q, d, t, b, last)
						last = b
			for n in (1, 64, 1000):
				for q in (300, 1000, 1 << 20):
					last = 0
					for t in (1, 2, 15, 16, 17, 63, 64, 65, 70, 1000, 1 << 16):
						b = lib.stpy_kmv_dxx_workspace_bytes(dtype, n, q, d, t)
						assert b > 0 and b >= last, (n, q, d, t, b, last)
						last = b
			assert lib.stpy_kmv_dxx_workspace_bytes(dtype, 1 << 20, 1 << 20, d, 64) <= (1 << 28)               # never more than the fill threshold's worth
		assert lib.stpy_kmv_dxx_workspace_bytes(dtype, 5, 1000, 3, 5) >= 2 * 5 * 5 * XO.ncol(3) * esz          # at least two pieces at 1000 points
		assert lib.stpy_kmv_dxx_workspace_bytes(dtype, 5, 200, 3, 5) <= 4096                                # q <= 256 is never cut
		assert lib.stpy_kmv_dxx_workspace_bytes(dtype, 64, 1 << 20, 16, 1) >= 57 * 64 * XO.ncol(16) * esz   # 9 groups: ceil(512 / 9) pieces


# --------------------------------------------------------------------------------------------- 2. kernel resources
def test_kmv_dxx_kernel_resources(tmp_path):
	"""kmvdxx.hip compiles alone; every kernel of stpy_kmv_dxx: no scratch, no VGPR spills, at most 64 KiB of LDS.  Eight kernels: the main kernel
	with 4, 8 and 16 coordinates in registers and the adding second launch, in both types."""
	out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-comment", "-c", os.path.join(CSRC, "kmvdxx.hip"),
						  "-o", str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True).stderr
	blocks = [b for b in re.split(r"remark: Function Name: ", out)[1:] if "kmvxx" in b.split()[0]]
	assert sum("kmvxx_kernel" in b.split()[0] for b in blocks) == 6
	assert sum("kmvxx_reduce_kernel" in b.split()[0] for b in blocks) == 2
	assert len(blocks) == 8
	for b in blocks:
		name = b.split()[0]
		assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, name
		assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, name
		assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) <= 65536, name


# --------------------------------------------------------------------------------------------- 3. the oracle
def _inputs(n, q, d, t, seed, coincide=False):
	rng = np.random.RandomState(seed)
	a, b = rng.uniform(-1, 1, size=(n, d)), rng.uniform(-1, 1, size=(q, d))
	if coincide:
		a[:min(n, q) // 2] = b[:min(n, q) // 2]                         # rho == 0
	il = rng.uniform(0.5, 3.0, size=(d,)) / np.sqrt(d)
	return a, b, il, rng.standard_normal((t, q))


@pytest.mark.parametrize("kind", XO.HESSIAN_KINDS)
def test_oracle_hessian_is_the_central_difference_of_its_gradient_and_the_gradient_of_its_value(kind):
	"""In longdouble, with a step of 1e-6: the truncation error h^2 / 6 |f'''| and the rounding 1e-19 / h are both far below the tolerances."""
	d = 3
	a, b, il, V = _inputs(7, 40, d, 2, 5)
	h = np.longdouble(1e-6)
	out = XO.kmv_dxx_dense(kind, a, b, il, V, kappa=0.7)[0]
	Hfull = XO.full_hessian(out[:, :, d + 1:], d)
	assert np.array_equal(Hfull, np.swapaxes(Hfull, -1, -2))
	for l in range(d):
		ap, am = a.astype(np.longdouble), a.astype(np.longdouble)
		ap[:, l] += h
		am[:, l] -= h
		op, om = XO.kmv_dxx_dense(kind, ap, b, il, V, kappa=0.7)[0], XO.kmv_dxx_dense(kind, am, b, il, V, kappa=0.7)[0]
		fd_grad = ((op[:, :, d] - om[:, :, d]) / (2 * h)).astype(np.float64)
		assert np.allclose(out[:, :, l].astype(np.float64), fd_grad, rtol=1e-8, atol=1e-9), (kind, l)
		for k in range(d):
			fd_hess = ((op[:, :, k] - om[:, :, k]) / (2 * h)).astype(np.float64)
			assert np.allclose(Hfull[:, :, k, l].astype(np.float64), fd_hess, rtol=1e-8, atol=1e-8), (kind, k, l)
	# cols: the same numbers from a wider array; the refused kinds are refused by the oracle as well
	wide_a, wide_b = np.zeros((7, 8)), np.zeros((40, 8))
	wide_a[:, [6, 1, 3]], wide_b[:, [6, 1, 3]] = a, b
	assert np.array_equal(XO.kmv_dxx_dense(kind, wide_a, wide_b, il, V, cols=[6, 1, 3])[0], XO.kmv_dxx_dense(kind, a, b, il, V)[0])
	for bad in ("matern12", "matern32"):
		with pytest.raises(ValueError):
			XO.kmv_dxx_dense(bad, a, b, il, V)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("kind", XO.HESSIAN_KINDS)
def test_kmv_dxx_bound_holds_for_a_working_precision_emulation(kind, dtype):
	"""The subtract-first evaluation in the working dtype stays within kmv_dxx_oracle.kmv_dxx_bound, on plain and on coinciding points, and a
	coinciding pair alone gives exactly kappa chi(0) il_k^2 on the diagonal and 0 elsewhere."""
	eps = KO.eps_of(dtype)
	for (n, q, d, t, co) in ((5, 65, 1, 2, False), (33, 129, 3, 3, True), (17, 200, 8, 2, False), (9, 64, 16, 1, True), (4, 1, 5, 1, False)):
		a, b, il, V = (v.astype(dtype).astype(np.float64) for v in _inputs(n, q, d, t, 13 * n + q + d, co))
		truth, S0, S1, SK, SH = XO.kmv_dxx_dense(kind, a, b, il, V, kappa=1.3)
		bound = XO.kmv_dxx_bound(q, d, eps, S0, S1, SK, SH)
		got = XO.kmv_dxx_emulated(kind, a, b, il, V, dtype, kappa=1.3)
		assert got.shape == (t, n, XO.ncol(d)) and np.all(np.isfinite(got.astype(np.float64)))
		err = np.abs(got.astype(np.longdouble) - truth).astype(np.float64)
		ratio = err / bound
		print("%s %s n=%d q=%d d=%d: largest error / bound: first block %.3f, Hessian %.3f" % (kind, np.dtype(dtype).name, n, q, d, ratio[:, :, :d + 1].max(), ratio[:, :, d + 1:].max()))
		assert np.all(err <= bound), (kind, n, q, d, float(ratio.max()))
	x = np.array([[0.25, -0.5, 0.75]])
	il = np.array([1.5, 0.75, 2.0])
	out = XO.kmv_dxx_dense(kind, x, x, il, np.ones((1, 1)), kappa=2.0)[0][0, 0].astype(np.float64)
	chi0 = {"se": -1.0, "matern52": -5.0 / 3.0}[kind]
	assert np.all(out[:3] == 0) and out[3] == 2.0
	assert np.allclose(XO.full_hessian(out[4:], 3), np.diag(2.0 * chi0 * il * il), rtol=1e-15, atol=0)


# --------------------------------------------------------------------------------------------- 4. the condition on the test points
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("idx", [0, 1, 2, 3], ids=KO.PCG_IDS[:4])
def test_derivative_test_points_keep_the_variance_above_its_bound(idx, dtype_name):
	"""var >= 100 b_var at EVERY drawn test point of tests/test_gpu_iterative_derivs.py, for the dense oracle: the first-order propagation
	through 1 / (2 std) is then valid.  A statement about the inputs, checked here so that the GPU test needs no filter."""
	dt = np.float64 if dtype_name == "float64" else np.float32
	kind, n, d, gamma, r, cols = KO.PCG_CASES[idx]
	s, tol = KO.SETTINGS[dtype_name]
	x, y, xt = XO.test_points(idx, dt)
	o = XO.posterior_deriv_bounds(kind, x, y, xt, gamma, s, tol, KO.eps_of(dt), cols, hessian=False)
	print("%s %s: smallest var / b_var %.3g" % (KO.PCG_IDS[idx], dtype_name, (o["var"] / o["b_var"]).min()))
	assert xt.shape == (37, x.shape[1]) and np.all(o["ok"])
	assert np.all(o["var"] >= XO.VAR_MARGIN * o["b_var"])
	# and the points are not in the prior's flat far field: the derivatives the tests compare are not all tiny
	assert np.abs(o["dstd"]).max() > 0.1 and np.abs(o["dmu"]).max() > 0.1


def test_oracle_posterior_derivatives_are_central_differences():
	kind, n, d, gamma, r, cols = KO.PCG_CASES[0]
	x, y, xt = XO.test_points(0, np.float64, m_test=4)
	x, y = x[:150], y[:150]
	o = XO.posterior_deriv_bounds(kind, x, y, xt, gamma, 0.1, 1e-8, KO.eps_of(np.float64), cols)
	h = 1e-5
	for k in range(d):
		xp, xm = xt.copy(), xt.copy()
		xp[:, k] += h
		xm[:, k] -= h
		op = XO.posterior_deriv_bounds(kind, x, y, xp, gamma, 0.1, 1e-8, KO.eps_of(np.float64), cols)
		om = XO.posterior_deriv_bounds(kind, x, y, xm, gamma, 0.1, 1e-8, KO.eps_of(np.float64), cols)
		assert np.allclose(o["dmu"][:, k], (op["mu"] - om["mu"]) / (2 * h), rtol=1e-6, atol=1e-7)
		assert np.allclose(o["dstd"][:, k], (np.sqrt(op["var"]) - np.sqrt(om["var"])) / (2 * h), rtol=1e-6, atol=1e-7)
		assert np.allclose(o["H"][:, :, k], (op["dmu"] - om["dmu"]) / (2 * h), rtol=1e-6, atol=1e-6)


# --------------------------------------------------------------------------------------------- 5. the class, on the host
def test_iterative_derivative_methods_on_the_host(monkeypatch):
	import stpy_amd
	from stpy_amd import IterativeGaussianProcess, _lib

	def no_device(*a, **k):
		raise AssertionError("the device was touched")
	for name in ("device", "to_device", "load"):
		monkeypatch.setattr(_lib, name, no_device)
	assert "stpy_kmv_dxx" in _lib.SIGNATURES and "stpy_kmv_dxx_workspace_bytes" in _lib.SIGNATURES and callable(_lib.kmv_dxx)
	xt = torch.zeros(5, 2).double()
	gp = IterativeGaussianProcess(gamma=0.5, s=0.1, d=2)
	# not fitted: zeros of the right shapes
	dmu, dstd = gp.mean_std_grad(xt)
	assert dmu.shape == (5, 2) and dstd.shape == (5, 2) and not dmu.any() and not dstd.any()
	mu, g, H = gp.mean_value_grad_hessian(xt)
	assert mu.shape == (5, 1) and g.shape == (5, 2) and H.shape == (5, 2, 2) and not mu.any() and not g.any() and not H.any()
	g = gp.mean_gradient_hessian(xt)
	assert g.shape == (2,) and not g.any()
	g, H = gp.mean_gradient_hessian(xt, hessian=True)
	assert g.shape == (2,) and H.shape == (2, 2) and not g.any() and not H.any()
	assert gp.mean_std_grad(xt.float())[1].dtype == torch.float32
	# ucb_optimize needs bounds
	assert gp.bounds is None
	with pytest.raises(ValueError, match="bounds"):
		gp.ucb_optimize(4.0)
	with pytest.raises(ValueError, match="bounds"):
		gp.ucb_optimize(4.0, multistart=3, lcb=True)
	gpb = IterativeGaussianProcess(gamma=0.5, s=0.1, d=2, bounds=[(-1, 1), (-1, 1)])
	with pytest.raises(ValueError, match="multistart"):
		gpb.ucb_optimize(4.0, multistart=0)
	gpb.bounds = [(-1, 1)]
	with pytest.raises(ValueError, match="bounds"):
		gpb.ucb_optimize(4.0, multistart=2)
	# Matern 1/2 and 3/2 have no Hessian: the dense class's message, before the device; their first derivatives are served
	for nu, name in ((0.5, "Matern nu=0.5"), (1.5, "Matern nu=1.5")):
		m = IterativeGaussianProcess(gamma=0.5, s=0.1, d=2, kernel_name="matern", nu=nu)
		for fitted in (False, True):
			if fitted:
				m.x, m.y, m.n, m.fitted = torch.zeros(20, 2).double(), torch.zeros(20, 1).double(), 20, True
			with pytest.raises(NotImplementedError, match="Hessian of the %s term is not defined" % name):
				m.mean_value_grad_hessian(xt)
			with pytest.raises(NotImplementedError, match="singular at r = 0"):
				m.mean_gradient_hessian(xt, hessian=True)
	m = IterativeGaussianProcess(gamma=0.5, s=0.1, d=2, kernel_name="matern", nu=0.5)
	assert m.mean_gradient_hessian(xt).shape == (2,) and m.mean_std_grad(xt)[0].shape == (5, 2)
	IterativeGaussianProcess(gamma=0.5, s=0.1, d=2, kernel_name="matern", nu=2.5).mean_value_grad_hessian(xt)
	# more than 16 selected coordinates: refused on the host
	with pytest.raises(NotImplementedError, match="16"):
		IterativeGaussianProcess(gamma=0.5, s=0.1, d=17).mean_value_grad_hessian(torch.zeros(3, 17).double())
	# the old refusals stand, and the message points to the methods that serve the gradients
	gp.x, gp.y, gp.n, gp.fitted = torch.zeros(20, 2).double(), torch.zeros(20, 1).double(), 20, True
	rg = xt.clone().requires_grad_(True)
	for fn in (gp.mean, gp.mean_std, gp.ucb, gp.lcb, gp.mean_value_grad, gp.mean_value_grad_hessian, gp.mean_gradient_hessian):
		with pytest.raises(NotImplementedError, match="requires_grad") as info:
			fn(rg)
		assert "mean_std_grad" in str(info.value) and "further solves" not in str(info.value)
	doc = stpy_amd.continuous_processes.iterative_gp.__doc__
	assert "more solves per point" not in doc and "mean_std_grad" in doc
	for name in ("Hessians of pathwise samples", "warm-started solves", "Hessians beyond d = 16"):
		assert name in stpy_amd.continuous_processes.iterative_gp.__doc__
	with pytest.raises(NotImplementedError, match="Lanczos"):
		gp.log_marginal(None, None, 1.0)
	with pytest.raises(NotImplementedError, match="Lanczos"):
		gp.optimize_params()
	with pytest.raises(NotImplementedError, match="square root"):
		gp.sample(xt, size=2)
	with pytest.raises(NotImplementedError, match="Sigma"):
		gp.fit_gp(gp.x, gp.y, Sigma=torch.eye(20).double())
	from stpy_amd import KernelFunction
	k1, k2 = KernelFunction(kernel_name="squared_exponential", gamma=0.5, d=2), KernelFunction(kernel_name="squared_exponential", gamma=0.7, d=2)
	with pytest.raises(NotImplementedError):
		IterativeGaussianProcess(kernel=k1 + k2, s=0.1)
