"""
Matrix-free input gradients and pathwise samples, the parts that need no GPU: the error bound of stpy_kmv_dx against a working-precision
emulation, the dense oracle's gradient against central differences, the statistics of the oracle's pathwise draw (mean and variance for the
drawn basis, and that the variance test catches a missing noise draw), the argument checks of stpy_kmv_dx (every refusal comes before the
first HIP call, so placeholder pointers are safe), the kernels' resource usage, and the host refusals of the new methods.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import kmv_oracle as KO
from tests import pathwise_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stpy_amd", "csrc")
P, N = ctypes.c_void_p(0x1000), None          # a non-null pointer no refused call may dereference
BIG = 1 << 40


# --------------------------------------------------------------------------------------------- 1. the bound of stpy_kmv_dx
def _dx_inputs(n, q, d, t, seed, coincide=False):
	rng = np.random.RandomState(seed)
	a, b = rng.uniform(-1, 1, size=(n, d)), rng.uniform(-1, 1, size=(q, d))
	if coincide:
		a[:min(n, q) // 2] = b[:min(n, q) // 2]                         # rho == 0
	il = rng.uniform(0.5, 3.0, size=(d,)) / np.sqrt(d)
	return a, b, il, rng.standard_normal((t, q))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("kind", list(KO.KIND_CODE))
def test_kmv_dx_bound_holds_for_a_working_precision_emulation(kind, dtype):
	"""The subtract-first evaluation in the working dtype stays within pathwise_oracle.kmv_dx_bound, on plain and on coinciding points (the
	Matern 1/2 guard: no NaN, exactly the longdouble truth's zero contribution)."""
	eps = KO.eps_of(dtype)
	worst = 0.0
	for (n, q, d, t, co) in ((5, 65, 1, 2, False), (33, 129, 3, 3, True), (17, 200, 7, 2, False), (64, 64, 12, 1, True)):
		a, b, il, V = (v.astype(dtype).astype(np.float64) for v in _dx_inputs(n, q, d, t, 13 * n + q + d, co))
		truth, S0, S1, SK = PO.kmv_dx_dense(kind, a, b, il, V, kappa=1.3)
		bound = PO.kmv_dx_bound(q, d, eps, S0, S1, SK)
		got = PO.kmv_dx_emulated(kind, a, b, il, V, dtype, kappa=1.3)
		assert got.shape == (t, n, d + 1) and np.all(np.isfinite(got.astype(np.float64)))
		err = np.abs(got.astype(np.longdouble) - truth).astype(np.float64)
		ratio = float(np.max(err / bound))
		worst = max(worst, ratio)
		print("%s %s n=%d q=%d d=%d: largest error / bound %.3f" % (kind, np.dtype(dtype).name, n, q, d, ratio))
		assert ratio <= 1.0, (kind, n, q, d, ratio)
	print("%s %s: largest ratio %.3f" % (kind, np.dtype(dtype).name, worst))


def test_kmv_dx_dense_gradient_is_the_central_difference_of_its_value_column():
	a, b, il, V = _dx_inputs(9, 40, 3, 2, 5)
	for kind in KO.KIND_CODE:
		out = PO.kmv_dx_dense(kind, a, b, il, V, kappa=0.7)[0].astype(np.float64)
		K = PO.NO.kernel(kind, a, b, 1.0 / il, 0.7)
		assert np.allclose(out[:, :, 3], V @ K.T, rtol=1e-12)
		for k in range(3):
			h = 1e-6
			ap, am = a.copy(), a.copy()
			ap[:, k] += h
			am[:, k] -= h
			fd = (PO.kmv_dx_dense(kind, ap, b, il, V, kappa=0.7)[0][:, :, 3] - PO.kmv_dx_dense(kind, am, b, il, V, kappa=0.7)[0][:, :, 3]).astype(np.float64) / (2 * h)
			assert np.allclose(out[:, :, k], fd, rtol=1e-6, atol=1e-8), (kind, k)
	# cols: the same numbers from a wider array
	wide_a, wide_b = np.zeros((9, 8)), np.zeros((40, 8))
	wide_a[:, [6, 1, 3]], wide_b[:, [6, 1, 3]] = a, b
	assert np.array_equal(PO.kmv_dx_dense("se", wide_a, wide_b, il, V, cols=[6, 1, 3])[0], PO.kmv_dx_dense("se", a, b, il, V)[0])


def test_oracle_path_gradient_is_the_central_difference_of_the_path():
	for ci in (0, 2):
		kind, n, d, gamma, seed = PO.STAT_CASES[ci]
		x, y, xt, _ = PO.stat_problem(ci)
		dr = PO.make_draws(kind, 3, 64, n, d, 9)
		xt = xt[:4]
		o = PO.draw(kind, x, y, xt, gamma, PO.STAT_S, PO.STAT_KAPPA, dr)
		assert o["f"].shape == (4, 3) and o["g"].shape == (4, 3, d)
		for k in range(d):
			h = 1e-6
			xp, xm = xt.copy(), xt.copy()
			xp[:, k] += h
			xm[:, k] -= h
			fd = (PO.draw(kind, x, y, xp, gamma, PO.STAT_S, PO.STAT_KAPPA, dr)["f"] - PO.draw(kind, x, y, xm, gamma, PO.STAT_S, PO.STAT_KAPPA, dr)["f"]) / (2 * h)
			assert np.allclose(o["g"][:, :, k], fd, rtol=1e-5, atol=1e-6), (kind, k)


# --------------------------------------------------------------------------------------------- 2. statistics of the oracle's draw
@pytest.mark.parametrize("ci", range(len(PO.STAT_CASES)), ids=PO.STAT_IDS)
def test_oracle_draw_has_the_posterior_mean_and_the_variance_of_the_drawn_basis(ci):
	kind, n, d, gamma, seed = PO.STAT_CASES[ci]
	x, y, xt, dr = PO.stat_problem(ci)
	o = PO.draw(kind, x, y, xt, gamma, PO.STAT_S, PO.STAT_KAPPA, dr)
	mu, var_w = PO.moments(kind, x, y, xt, gamma, PO.STAT_S, PO.STAT_KAPPA, o["W"])
	# the mean is the exact posterior mean, whatever the basis
	mu_post = KO.posterior(kind, x, y, xt, gamma, PO.STAT_S, kappa=PO.STAT_KAPPA)[0][:, 0]
	assert np.allclose(mu, mu_post, rtol=1e-9, atol=1e-11)
	zm, zv = PO.statistics(o["f"], mu, var_w)
	print("%s: mean statistic %.2f, variance statistic %.2f (limits %.1f, %.1f)" % (PO.STAT_IDS[ci], zm.max(), zv.max(), PO.STAT_MEAN_Z, PO.STAT_VAR_Z))
	assert np.all(np.abs(o["f"].mean(axis=1) - mu) <= PO.STAT_MEAN_Z * np.sqrt(var_w / PO.STAT_SIZE))
	assert np.all(np.abs(o["f"].var(axis=1, ddof=1) / var_w - 1.0) <= PO.STAT_VAR_Z * np.sqrt(2.0 / (PO.STAT_SIZE - 1)))


def test_variance_statistic_catches_a_draw_without_the_noise_term():
	"""The squared-exponential case with eps left out (the reference's sample_matheron): the variance assertion FAILS."""
	kind, n, d, gamma, seed = PO.STAT_CASES[0]
	x, y, xt, dr = PO.stat_problem(0)
	o = PO.draw(kind, x, y, xt, gamma, PO.STAT_S, PO.STAT_KAPPA, dr, with_eps=False)
	mu, var_w = PO.moments(kind, x, y, xt, gamma, PO.STAT_S, PO.STAT_KAPPA, o["W"])
	zv = PO.statistics(o["f"], mu, var_w)[1]
	print("without eps: variance statistic %.2f" % zv.max())
	assert not np.all(np.abs(o["f"].var(axis=1, ddof=1) / var_w - 1.0) <= PO.STAT_VAR_Z * np.sqrt(2.0 / (PO.STAT_SIZE - 1)))


# --------------------------------------------------------------------------------------------- 3. argument checks
def _leave_another_message(lib):
	lib.stpy_lml_batch(0, 1, N, 1, 1, 1, N, N, 1, N, 1, N, 1.0, 1.0, N, 1, N, N, 2, N, N, 0, N)
	return lib.stpy_last_error_string()


def test_kmv_dx_argument_checks():
	from stpy_amd import _lib as L
	lib = L.load()

	def call(kind=0, dtype=0, a=P, n=64, lda=4, b=P, q=64, ldb=4, d=4, cols=N, inv_ls=P, kappa=1.0, Vt=P, ldv=64, t=3, out=P, ldc=64 * 5, ldo=5,
			 work=P, work_bytes=BIG):
		return lib.stpy_kmv_dx(kind, dtype, a, n, lda, b, q, ldb, d, cols, inv_ls, kappa, Vt, ldv, t, out, ldc, ldo, work, work_bytes, N)

	need = lib.stpy_kmv_dx_workspace_bytes(0, 64, 64, 4, 3)
	assert need > 0
	refused = {
		"unknown kind": (dict(kind=9), -1), "negative kind": (dict(kind=-1), -1), "LINEAR": (dict(kind=4), -1), "POLY": (dict(kind=5 | (2 << 8)), -1),
		"unknown dtype": (dict(dtype=7), -2), "negative dtype": (dict(dtype=-1), -2),
		"null a": (dict(a=N), -3), "null b": (dict(b=N), -3), "null inv_ls": (dict(inv_ls=N), -3), "null Vt": (dict(Vt=N), -3), "null out": (dict(out=N), -3),
		"null work": (dict(work=N), -20), "undersized work": (dict(work_bytes=need - 1), -20),
		"undersized work fp32": (dict(dtype=1, work_bytes=lib.stpy_kmv_dx_workspace_bytes(1, 64, 64, 4, 3) - 1), -20),
		"undersized work, cut range": (dict(n=5, q=2500, ldv=2500, ldc=25, work_bytes=lib.stpy_kmv_dx_workspace_bytes(0, 5, 2500, 4, 3) - 1), -20),
		"misaligned work": (dict(work=ctypes.c_void_p(0x1004)), -17),
		"negative n": (dict(n=-1), -4), "n >= 2^31": (dict(n=1 << 31, ldc=5 << 31), -4), "negative q": (dict(q=-1), -4), "q >= 2^31": (dict(q=1 << 31, ldv=1 << 31), -4),
		"lda < d": (dict(lda=3), -5), "ldb < d": (dict(ldb=3), -5), "d < 1": (dict(d=0), -6), "negative d": (dict(d=-2), -6),
		"t < 1": (dict(t=0), -10), "negative t": (dict(t=-4), -10), "too many row blocks": (dict(t=65536 * 16), -10),
		"too many row blocks x groups": (dict(d=20, lda=20, ldb=20, ldo=21, ldc=64 * 21, t=65535 * 16 // 3 + 16), -10),
		"ldv < q": (dict(ldv=63), -13), "ldo < d + 1": (dict(ldo=4), -22), "ldc < n * ldo": (dict(ldc=64 * 5 - 1), -23), "ldc < n * padded ldo": (dict(ldo=7), -23),
		"nan kappa": (dict(kappa=float("nan")), -11), "inf kappa": (dict(kappa=float("inf")), -11),
	}
	for what, (kw, code) in refused.items():
		before = _leave_another_message(lib)
		rc = call(**kw)
		assert rc == code, (what, rc)
		msg = lib.stpy_last_error_string()
		assert msg and b"stpy_kmv_dx" in msg and msg != before, (what, msg)
	# the empty output: 0 without looking at a pointer
	assert lib.stpy_kmv_dx(0, 0, N, 0, 4, N, 64, 4, 4, N, N, 1.0, N, 64, 3, N, 0, 5, N, 0, N) == 0
	assert lib.stpy_kmv_dx(3, 1, N, 0, 4, N, 0, 4, 4, N, N, 1.0, N, 0, 3, N, 0, 5, N, 0, N) == 0
	# the workspace: positive everywhere, and enough for one (t, n, d + 1) tile set per piece where the j range is cut (few queries, many points)
	for dtype in (0, 1):
		esz = 4 if dtype else 8
		for (n, q, d, t) in ((1, 1, 1, 1), (64, 64, 4, 3), (5, 2500, 3, 5), (25, 1 << 20, 8, 16), (1024, 1 << 18, 16, 1), (64, 1 << 20, 20, 33), (1 << 20, 1 << 20, 3, 64)):
			assert lib.stpy_kmv_dx_workspace_bytes(dtype, n, q, d, t) > 0
		assert lib.stpy_kmv_dx_workspace_bytes(dtype, 5, 2500, 3, 5) >= 2 * 5 * 5 * 4 * esz          # at least two pieces at 2500 points
		assert lib.stpy_kmv_dx_workspace_bytes(dtype, 25, 1 << 20, 8, 16) >= 512 * 16 * 25 * 9 * esz  # 512 pieces
		assert lib.stpy_kmv_dx_workspace_bytes(dtype, 1 << 20, 1 << 20, 3, 64) <= 4096               # the chip is full: no pieces


# --------------------------------------------------------------------------------------------- 4. kernel resources
def test_kmv_dx_kernel_resources(tmp_path):
	"""kmvdx.hip compiles alone; every kernel of stpy_kmv_dx: no scratch, no VGPR spills, at most 64 KiB of LDS."""
	out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-comment", "-c", os.path.join(CSRC, "kmvdx.hip"),
						  "-o", str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True).stderr
	blocks = [b for b in re.split(r"remark: Function Name: ", out)[1:] if "kmvx" in b.split()[0]]
	assert sum("kmvx_kernel" in b.split()[0] for b in blocks) == 8          # registers up to d = 4, 8 and 16, LDS rounds beyond, in both types
	assert sum("kmvx_reduce_kernel" in b.split()[0] for b in blocks) == 2
	assert len(blocks) == 10
	for b in blocks:
		name = b.split()[0]
		assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, name
		assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, name
		assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) <= 65536, name


# --------------------------------------------------------------------------------------------- 5. the new methods refuse on the host
def test_pathwise_python_refusals(monkeypatch):
	import stpy_amd
	from stpy_amd import IterativeGaussianProcess, _lib

	def no_device(*a, **k):
		raise AssertionError("the device was touched")
	for name in ("device", "to_device", "load"):
		monkeypatch.setattr(_lib, name, no_device)
	assert "PathwiseSamples" in stpy_amd.__all__
	x, y = torch.zeros(20, 2).double(), torch.zeros(20, 1).double()
	gp = IterativeGaussianProcess(gamma=0.5, s=0.1, d=2)
	# not fitted
	with pytest.raises(AttributeError, match="fit_gp"):
		gp.sample_paths(size=2, num_features=8)
	with pytest.raises(AttributeError, match="fit_gp"):
		gp.sample_and_optimize(size=2, multistart=3, num_features=8)
	mu, g = gp.mean_value_grad(torch.zeros(5, 2).double())
	assert mu.shape == (5, 1) and g.shape == (5, 2) and not mu.any() and not g.any()
	with pytest.raises(NotImplementedError, match="requires_grad"):
		gp.mean_value_grad(torch.zeros(5, 2).double().requires_grad_(True))
	# the checks that need the data's shape: an object that looks fitted, the device still out of reach
	for kw, matern in ((dict(gamma=0.5, s=0.1, d=2), False), (dict(gamma=0.5, s=0.1, d=2, kernel_name="matern", nu=2.5), True)):
		gp = IterativeGaussianProcess(**kw)
		gp.x, gp.y, gp.n, gp.fitted = x, y, 20, True
		for bad in (dict(size=0), dict(size=-3), dict(num_features=7), dict(num_features=0), dict(num_features=-2)):
			with pytest.raises(ValueError):
				gp.sample_paths(**dict(dict(size=2, num_features=8), **bad))
		good = {"z": np.zeros((4, 2)), "theta": np.zeros((2, 8)), "eps": np.zeros((2, 20))}
		if matern:
			good["u"] = np.ones(4)
		for key, shape in (("z", (4, 3)), ("z", (8, 2)), ("theta", (2, 7)), ("theta", (3, 8)), ("eps", (2, 19)), ("eps", (20, 2)), ("u", (5,))):
			if key == "u" and not matern:
				continue
			with pytest.raises(ValueError, match="draws"):
				gp.sample_paths(size=2, num_features=8, draws=dict(good, **{key: np.ones(shape)}))
		with pytest.raises(ValueError, match="draws"):
			gp.sample_paths(size=2, num_features=8, draws=dict(good, w=np.zeros(3)))
		if matern:
			with pytest.raises(ValueError, match="positive"):
				gp.sample_paths(size=2, num_features=8, draws=dict(good, u=np.zeros(4)))
		else:
			with pytest.raises(ValueError, match="Matern"):
				gp.sample_paths(size=2, num_features=8, draws=dict(good, u=np.ones(4)))
		with pytest.raises(ValueError):
			gp.sample_and_optimize(size=2, multistart=0, num_features=8)
		# the old refusals stand
		with pytest.raises(NotImplementedError, match="square root"):
			gp.sample(x, size=2)
