"""
The matrix-free route, the parts that need no GPU: the argument checks of stpy_kmv and stpy_pcg (every refusal comes before the first HIP
call, so placeholder pointers are safe), the workspace queries, the kernels' resource usage, the NumPy oracle's own PCG (it reaches the
tolerance it is asked for, and the preconditioner saves iterations, on every case the device is tested on), and the refusals of the class.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import kmv_oracle as KO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stpy_amd", "csrc")
P, N = ctypes.c_void_p(0x1000), None          # a non-null pointer no refused call may dereference
BIG = 1 << 40


def _leave_another_message(lib):
	lib.stpy_lml_batch(0, 1, N, 1, 1, 1, N, N, 1, N, 1, N, 1.0, 1.0, N, 1, N, N, 2, N, N, 0, N)
	return lib.stpy_last_error_string()


def _all_refused(lib, call, refused, name):
	for what, kw in refused.items():
		before = _leave_another_message(lib)
		rc = call(**kw)
		assert rc < 0, (what, rc)
		msg = lib.stpy_last_error_string()
		assert msg and name in msg and msg != before, (what, msg)


# --------------------------------------------------------------------------------------------- 1. argument checks
def test_kmv_argument_checks():
	from stpy_amd import _lib as L
	lib = L.load()

	def call(kind=0, dtype=0, a=P, n=64, lda=4, b=P, q=64, ldb=4, d=4, cols=N, inv_ls=P, kappa=1.0, diag_add=0.0, Vt=P, t=3, ldv=64, Yt=P, ldy=64,
			 work=P, work_bytes=BIG):
		return lib.stpy_kmv(kind, dtype, a, n, lda, b, q, ldb, d, cols, inv_ls, kappa, diag_add, Vt, t, ldv, Yt, ldy, work, work_bytes, N)

	need = lib.stpy_kmv_workspace_bytes(0, 64, 64, 4, 3)
	assert need > 0
	refused = {
		"unknown kind": dict(kind=9), "negative kind": dict(kind=-1), "LINEAR": dict(kind=4), "POLY": dict(kind=5 | (2 << 8)),
		"unknown dtype": dict(dtype=7), "negative dtype": dict(dtype=-1),
		"null a": dict(a=N), "null b": dict(b=N), "null inv_ls": dict(inv_ls=N), "null Vt": dict(Vt=N), "null Yt": dict(Yt=N),
		"null work": dict(work=N), "undersized work": dict(work_bytes=need - 1), "undersized work fp32": dict(dtype=1, work_bytes=lib.stpy_kmv_workspace_bytes(1, 64, 64, 4, 3) - 1),
		"negative n": dict(n=-1), "n >= 2^31": dict(n=1 << 31, ldy=1 << 31), "negative q": dict(q=-1), "q >= 2^31": dict(q=1 << 31, ldv=1 << 31),
		"lda < d": dict(lda=3), "ldb < d": dict(ldb=3), "d < 1": dict(d=0), "negative d": dict(d=-2), "t < 1": dict(t=0), "negative t": dict(t=-4),
		"ldv < q": dict(ldv=63), "ldy < n": dict(ldy=63),
		"diag_add with q != n": dict(diag_add=0.5, q=32), "nan kappa": dict(kappa=float("nan")), "inf kappa": dict(kappa=float("inf")),
		"nan diag_add": dict(diag_add=float("nan")), "inf diag_add": dict(diag_add=float("-inf")),
	}
	_all_refused(lib, call, refused, b"stpy_kmv")
	# the empty output: 0 without looking at a pointer
	assert lib.stpy_kmv(0, 0, N, 0, 4, N, 64, 4, 4, N, N, 1.0, 0.0, N, 3, 64, N, 0, N, 0, N) == 0
	assert lib.stpy_kmv(3, 1, N, 0, 4, N, 0, 4, 4, N, N, 1.0, 0.0, N, 3, 0, N, 0, N, 0, N) == 0
	# workspace query: positive, non-decreasing in n, q and t
	sizes = (1, 2, 63, 64, 65, 1000, 4099, 16320, 16321, 65536, 1 << 20, (1 << 31) - 1)
	for dtype in (0, 1):
		for t in (1, 16, 70):
			last = 0
			for n in sizes:
				b = lib.stpy_kmv_workspace_bytes(dtype, n, 1000, 3, t)
				assert b > 0 and b >= last, (n, b, last)
				last = b
			last = 0
			for q in sizes:
				b = lib.stpy_kmv_workspace_bytes(dtype, 1000, q, 3, t)
				assert b > 0 and b >= last, (q, b, last)
				last = b
		last = 0
		for t in (1, 2, 15, 16, 17, 63, 64, 65, 70, 1000):
			b = lib.stpy_kmv_workspace_bytes(dtype, 1000, 1000, 3, t)
			assert b > 0 and b >= last, (t, b, last)
			last = b


def test_pcg_argument_checks():
	from stpy_amd import _lib as L
	lib = L.load()

	def call(kind=0, dtype=0, x=P, n=64, ldx=4, d=4, cols=N, inv_ls=P, kappa=1.0, diag_add=0.01, Gt=P, ldgt=64, Gn=P, ldgn=8, r=8, Bt=P, ldb=64,
			 Xt=P, ldxt=64, t=3, tol=1e-8, iters=10, init=1, relres=P, bx=P, its=P, work=P, work_bytes=BIG):
		return lib.stpy_pcg(kind, dtype, x, n, ldx, d, cols, inv_ls, kappa, diag_add, Gt, ldgt, Gn, ldgn, r, Bt, ldb, Xt, ldxt, t, tol, iters, init,
							relres, bx, its, work, work_bytes, N)

	need = lib.stpy_pcg_workspace_bytes(0, 64, 4, 3, 8)
	assert need > 0
	refused = {
		"unknown kind": dict(kind=9), "negative kind": dict(kind=-1), "LINEAR": dict(kind=4), "POLY": dict(kind=5 | (2 << 8)),
		"unknown dtype": dict(dtype=7), "negative dtype": dict(dtype=-1),
		"null x": dict(x=N), "null inv_ls": dict(inv_ls=N), "null Bt": dict(Bt=N), "null Xt": dict(Xt=N), "null relres": dict(relres=N),
		"null bx": dict(bx=N), "null its": dict(its=N), "null work": dict(work=N), "undersized work": dict(work_bytes=need - 1),
		"undersized work fp32": dict(dtype=1, work_bytes=lib.stpy_pcg_workspace_bytes(1, 64, 4, 3, 8) - 1),
		"negative n": dict(n=-1), "n >= 2^31": dict(n=1 << 31, ldb=1 << 31, ldxt=1 << 31, ldgt=1 << 31),
		"ldx < d": dict(ldx=3), "d < 1": dict(d=0), "negative d": dict(d=-2), "t < 1": dict(t=0), "negative t": dict(t=-4),
		"nan kappa": dict(kappa=float("nan")), "inf diag_add": dict(diag_add=float("inf")),
		"negative tol": dict(tol=-1e-3), "nan tol": dict(tol=float("nan")), "inf tol": dict(tol=float("inf")),
		"iters < 0": dict(iters=-1), "r < 0": dict(r=-1), "r > 0 with null Gt": dict(Gt=N), "r > 0 with null Gn": dict(Gn=N),
		"ldgt < n": dict(ldgt=63), "ldgn < r": dict(ldgn=7), "ldb < n": dict(ldb=63), "ldxt < n": dict(ldxt=63),
	}
	_all_refused(lib, call, refused, b"stpy_pcg")
	assert lib.stpy_pcg(0, 0, N, 0, 4, 4, N, N, 1.0, 0.01, N, 0, N, 0, 0, N, 0, N, 0, 3, 1e-8, 10, 1, N, N, N, N, 0, N) == 0          # the empty problem
	for dtype in (0, 1):
		for fixed in (dict(t=3, r=8), dict(t=64, r=0)):
			last = 0
			for n in (1, 2, 64, 65, 1000, 4099, 65536, 1 << 20):
				b = lib.stpy_pcg_workspace_bytes(dtype, n, 3, fixed["t"], fixed["r"])
				assert b > 0 and b >= last, (n, b, last)
				last = b
		last = 0
		for t in (1, 2, 16, 17, 64, 65, 200):
			b = lib.stpy_pcg_workspace_bytes(dtype, 1000, 3, t, 16)
			assert b > 0 and b >= last, (t, b, last)
			last = b
		last = 0
		for r in (0, 1, 16, 256, 2048):
			b = lib.stpy_pcg_workspace_bytes(dtype, 1000, 3, 6, r)
			assert b > 0 and b >= last, (r, b, last)
			last = b
		# the state of a solve dominates: four vectors per column, and the partial sums of the product
		assert lib.stpy_pcg_workspace_bytes(dtype, 1 << 20, 3, 1, 0) >= 4 * (1 << 20) * (4 if dtype else 8) + lib.stpy_kmv_workspace_bytes(dtype, 1 << 20, 1 << 20, 3, 1)


# --------------------------------------------------------------------------------------------- 2. kernel resources
def test_kmv_kernel_resources(tmp_path):
	"""kmv.hip compiles alone; every kernel of the product and of the solver: no scratch, at most 64 KiB of LDS."""
	out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-comment", "-c", os.path.join(CSRC, "kmv.hip"),
						  "-o", str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True).stderr
	blocks = [b for b in re.split(r"remark: Function Name: ", out)[1:] if "kmv" in b.split()[0] or "pcg" in b.split()[0]]
	assert sum("kmv_kernel" in b.split()[0] for b in blocks) == 8          # registers up to d = 4, 8 and 16, LDS rounds beyond, in both types
	assert sum("kmv_reduce_kernel" in b.split()[0] for b in blocks) == 2
	assert sum("pcg_" in b.split()[0] for b in blocks) == 8                # init, step, dir, finish in both types
	for b in blocks:
		name = b.split()[0]
		assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, name
		assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, name
		assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) <= 65536, name


# --------------------------------------------------------------------------------------------- 3. the oracle's own PCG
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("idx", range(len(KO.PCG_CASES)), ids=KO.PCG_IDS)
def test_oracle_pcg_reaches_its_tolerance_and_the_preconditioner_helps(idx, dtype_name):
	o = KO.oracle_run(idx, dtype_name)
	assert np.all(o["its"] > 0) and np.all(o["its_plain"] > 0)
	assert o["true"].max() <= o["tol"] and o["true_plain"].max() <= o["tol"]          # TRUE relative residual, in float64
	assert o["its"].max() < o["its_plain"].max()
	assert np.all(o["its"] < o["its_plain"])
	# M^-1 = I - G G^T is s^2 (s^2 I + F F^T)^-1: symmetric positive definite with eigenvalues in (0, 1]
	G = o["G"].astype(np.float64)
	ev = np.linalg.eigvalsh(G.T @ G)
	assert ev.max() < 1.0 and ev.min() > 0.0


def test_oracle_pcg_freezes_zero_columns_and_flags_curvature():
	A = np.diag([2.0, 3.0, 5.0])
	B = np.array([[1.0, 0.0], [1.0, 0.0], [1.0, 0.0]])
	X, its, rel = KO.pcg(A, B, 1e-12, 10)
	assert its[1] == 0 and np.all(X[:, 1] == 0) and rel[1] == 0
	assert 0 < its[0] <= 3 and np.abs(A @ X[:, 0] - B[:, 0]).max() < 1e-12
	X, its, rel = KO.pcg(-A, B, 1e-12, 10)
	assert its[0] == -1 and np.all(X == 0) and rel[0] == 1


# --------------------------------------------------------------------------------------------- 4. the class refuses on the host
def test_iterative_gp_python_refusals(monkeypatch):
	import stpy_amd
	from stpy_amd import IterativeGaussianProcess, KernelFunction, _lib
	from stpy_amd.estimator import Estimator

	def no_device(*a, **k):
		raise AssertionError("the device was touched")
	for name in ("device", "to_device", "load"):
		monkeypatch.setattr(_lib, name, no_device)
	x, y = torch.zeros(20, 2).double(), torch.zeros(20, 1).double()
	unsupported = {
		"linear": KernelFunction(kernel_name="linear", d=2),
		"polynomial": KernelFunction(kernel_name="polynomial", d=2, power=2),
		"sum": KernelFunction(kernel_name="squared_exponential", gamma=0.5, d=2) + KernelFunction(kernel_name="matern", gamma=0.5, nu=1.5, d=2),
		"product": KernelFunction(kernel_name="squared_exponential", gamma=0.5, d=2) * KernelFunction(kernel_name="squared_exponential", gamma=0.2, d=2),
		"additive groups": KernelFunction(kernel_name="ard", ard_gamma=[0.5, 0.5], d=2, groups=[[0], [1]]),
		"full covariance": KernelFunction(kernel_name="full_covariance_se", d=2),
	}
	for what, k in unsupported.items():
		with pytest.raises(NotImplementedError):
			IterativeGaussianProcess(kernel=k)
	with pytest.raises(NotImplementedError):
		IterativeGaussianProcess(kernel_name="linear", d=2)
	for k in (KernelFunction(kernel_name="squared_exponential", gamma=0.5, d=2), KernelFunction(kernel_name="matern", gamma=0.3, nu=2.5, d=2),
			  KernelFunction(kernel_name="ard", ard_gamma=[0.5, 0.2], d=2), KernelFunction(kernel_name="ard_matern", ard_gamma=[0.5, 0.2], nu=0.5, d=2)):
		gp = IterativeGaussianProcess(kernel=k, s=0.1)
		assert isinstance(gp, Estimator) and gp.fitted is False and gp.A is None and gp.d == 2
		with pytest.raises(NotImplementedError, match="Sigma"):
			gp.fit_gp(x, y, Sigma=torch.eye(20).double())
		with pytest.raises(NotImplementedError, match="Lanczos"):
			gp.log_marginal(gp.kernel_object, {}, 1.0)
		with pytest.raises(NotImplementedError, match="Lanczos"):
			gp.optimize_params(type="bandwidth", restarts=2)
		with pytest.raises(NotImplementedError, match="square root"):
			gp.sample(x, size=2)
		xt = torch.zeros(5, 2).double().requires_grad_(True)
		for fn in (gp.mean, gp.mean_std, gp.mean_var, gp.ucb, gp.lcb):
			with pytest.raises(NotImplementedError, match="requires_grad"):
				fn(xt)
		assert gp.fitted is False and gp.cg_info["iterations"] == 0
	gp = IterativeGaussianProcess(gamma=0.4, s=0.2, kappa=1.5, kernel_name="matern", nu=2.5, d=3, precond_rank=32, tol=1e-6, maxiter=50, check_every=5, rhs_block=8)
	assert (gp.precond_rank, gp.maxiter, gp.check_every, gp.rhs_block) == (32, 50, 5, 8)
	assert gp._tol(torch.float64) == 1e-6 and IterativeGaussianProcess(d=2)._tol(torch.float64) == 1e-8 and IterativeGaussianProcess(d=2)._tol(torch.float32) == 1e-4
	for bad in (dict(precond_rank=-1), dict(precond_tol=-1.0), dict(maxiter=0), dict(check_every=0), dict(rhs_block=0), dict(tol=0.0), dict(tol=-1e-3)):
		with pytest.raises(ValueError):
			IterativeGaussianProcess(d=2, **bad)
	assert "IterativeGaussianProcess" in stpy_amd.__all__
