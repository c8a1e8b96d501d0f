"""
Pivoted partial Cholesky and Nystrom features, the parts that need no GPU: the argument checks of stpy_pchol (every refusal comes before
the first HIP call, so placeholder pointers are safe), the kernels' resource usage, the NumPy oracle's own invariants, the oracle
against the reference's NystromFeatures (golden N1), and the refusals of the Python class.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import nystrom_oracle as NO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stpy_amd", "csrc")


# --------------------------------------------------------------------------------------------- 1. argument checks
def test_pchol_argument_checks():
	from stpy_amd import _lib as L
	lib = L.load()
	P, N = ctypes.c_void_p(0x1000), None          # a non-null pointer no refused call may dereference
	big = 1 << 40

	def call(kind=0, dtype=0, x=P, n=64, ldx=4, d=4, cols=N, inv_ls=P, kappa=1.0, m=8, tol=0.0, Ft=P, ldf=64, dres=P, piv=P, rank=P, work=P,
			 work_bytes=big):
		return lib.stpy_pchol(kind, dtype, x, n, ldx, d, cols, inv_ls, kappa, m, tol, Ft, ldf, dres, piv, rank, work, work_bytes, N)

	refused = {
		"unknown kind": dict(kind=9), "negative kind": dict(kind=-1), "LINEAR": dict(kind=4), "POLY": dict(kind=5 | (2 << 8)),
		"unknown dtype": dict(dtype=7), "negative dtype": dict(dtype=-1),
		"null x": dict(x=N), "null inv_ls": dict(inv_ls=N), "null Ft": dict(Ft=N), "null dres": dict(dres=N), "null piv": dict(piv=N),
		"null rank": dict(rank=N), "null work": dict(work=N),
		"ldx < d": dict(ldx=3), "d < 1": dict(d=0), "negative d": dict(d=-2),
		"m < 1": dict(m=0), "negative m": dict(m=-3), "m > n": dict(m=65), "m above the cap": dict(n=20000, ldf=20000, m=8193),
		"ldf < n": dict(ldf=63),
		"negative tol": dict(tol=-1e-3), "nan tol": dict(tol=float("nan")), "inf tol": dict(tol=float("inf")),
		"n >= 2^31": dict(n=1 << 31, ldf=1 << 31), "negative n": dict(n=-1),
		"undersized workspace": dict(work_bytes=lib.stpy_pchol_workspace_bytes(0, 64, 4, 8) - 1),
		"undersized workspace fp32": dict(dtype=1, n=5000, ldf=5000, work_bytes=lib.stpy_pchol_workspace_bytes(1, 5000, 4, 8) - 1),
	}
	for what, kw in refused.items():
		lib.stpy_lml_batch(0, 1, N, 1, 1, 1, N, N, 1, N, 1, N, 1.0, 1.0, N, 1, N, N, 2, N, N, 0, N)          # (leaves some OTHER message behind)
		before = lib.stpy_last_error_string()
		rc = call(**kw)
		assert rc < 0, (what, rc)
		msg = lib.stpy_last_error_string()
		assert msg and b"stpy_pchol" in msg and msg != before, (what, msg)
	# the empty problem: 0 without looking at a pointer
	assert lib.stpy_pchol(0, 0, N, 0, 4, 4, N, N, 1.0, 8, 0.0, N, 0, N, N, N, N, 0, N) == 0
	assert lib.stpy_pchol(3, 1, N, 0, 4, 4, N, N, 1.0, 8, 0.0, N, 0, N, N, N, N, 0, N) == 0
	# workspace query: positive, non-decreasing in n and in m
	for dtype in (0, 1):
		last = 0
		for n in (1, 2, 127, 128, 129, 255, 256, 257, 1000, 4099, 65536, 1 << 20, (1 << 31) - 1):
			b = lib.stpy_pchol_workspace_bytes(dtype, n, 3, 1)
			assert b > 0 and b >= last, (n, b, last)
			last = b
		last = 0
		for m in (1, 2, 64, 1024, 1025, 8192):
			b = lib.stpy_pchol_workspace_bytes(dtype, 10000, 3, m)
			assert b > 0 and b >= last, (m, b, last)
			last = b


# --------------------------------------------------------------------------------------------- 2. kernel resources
def test_pchol_kernel_resources(tmp_path):
	"""Every kernel of the pivoted Cholesky: no scratch, at most 64 KiB of LDS."""
	out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-comment", "-c", os.path.join(CSRC, "pchol.hip"),
						  "-o", str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True).stderr
	blocks = [b for b in re.split(r"remark: Function Name: ", out)[1:] if "pchol" in b.split()[0]]
	assert len(blocks) >= 6          # init, step, tail in both types
	assert sum("pchol_step_kernel" in b.split()[0] for b in blocks) == 2
	for b in blocks:
		name = b.split()[0]
		assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, name
		assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) <= 65536, name


# --------------------------------------------------------------------------------------------- 3. the oracle's own invariants
@pytest.mark.parametrize("kind,n,d,gamma,m", [("se", 150, 2, 0.35, 20), ("matern52", 211, 2, 0.2, 33), ("matern12", 97, 3, 0.8, 40), ("matern32", 60, 1, 0.5, 9)])
def test_oracle_invariants(kind, n, d, gamma, m):
	x = np.random.RandomState(5).uniform(-1, 1, size=(n, d))
	K = NO.kernel(kind, x, x, gamma)
	assert np.array_equal(np.diag(K), np.ones(n))                       # coincident points: kappa exactly
	piv, Ft, dres, rank = NO.pivoted_cholesky(kind, x, gamma, m)
	assert rank == m and len(set(piv.tolist())) == m and piv[0] == 0
	assert np.abs(np.diag(K) - np.sum(Ft * Ft, axis=0) - dres).max() <= 1e-13          # diag(K) = colsumsq(F) + dres
	assert np.abs((Ft.T @ Ft)[piv] - K[piv]).max() <= 1e-12                            # F F^T reproduces K on the pivot rows
	assert np.all(dres[piv] == 0) and dres.min() >= -1e-13
	# greedy: every pivot carried the largest residual of its step
	tr = []
	NO.pivoted_cholesky(kind, x, gamma, m, trace=tr)
	assert all(a == b for a, b in tr)
	# a forced pivot list replays the same factor; a different list still satisfies the invariants
	_, Ft2, dres2, _ = NO.pivoted_cholesky(kind, x, gamma, m, pivots=piv)
	assert np.array_equal(Ft2, Ft) and np.array_equal(dres2, dres)
	forced = list(range(n - 1, n - 1 - m, -1))
	_, Ft3, dres3, r3 = NO.pivoted_cholesky(kind, x, gamma, m, pivots=forced)
	assert r3 == m and np.abs(np.diag(K) - np.sum(Ft3 * Ft3, axis=0) - dres3).max() <= 1e-13
	assert np.abs((Ft3.T @ Ft3)[forced] - K[forced]).max() <= 1e-12
	# float32 replay: float32 arrays, close to the float64 one
	_, Ft4, dres4, _ = NO.pivoted_cholesky(kind, x.astype(np.float32), gamma, m, pivots=piv, dtype=np.float32)
	assert Ft4.dtype == np.float32 and dres4.dtype == np.float32
	_, Ft5, _, _ = NO.pivoted_cholesky(kind, x.astype(np.float32).astype(np.float64), gamma, m, pivots=piv)
	assert np.abs(Ft4 - Ft5).max() < 1e-3


def test_oracle_stops_on_duplicates():
	rng = np.random.RandomState(8)
	x = np.repeat(rng.uniform(-1, 1, size=(10, 2)), 5, axis=0)[rng.permutation(50)]
	piv, Ft, dres, rank = NO.pivoted_cholesky("se", x, 0.5, 16, tol=1e-10)
	assert rank == 10 and np.all(piv[10:] == -1) and np.all(Ft[10:] == 0)
	assert len({tuple(x[p]) for p in piv[:10]}) == 10
	assert np.abs(dres).max() < 1e-12
	# Nystrom features on the pivots reproduce the kernel on all (duplicated) points
	Phi = NO.nystrom_features("se", x, piv[:10], x, 0.5)
	assert np.abs(Phi @ Phi.T - NO.kernel("se", x, x, 0.5)).max() < 1e-9


def test_oracle_matches_reference_golden():
	"""The oracle's Cholesky features against the reference's eigenvector features (NystromFeatures(approx="uniform"), golden N1): the
	feature Gram matrices and the ridge predictions do not see the rotation between the two."""
	g = np.load(os.path.join(ROOT, "tests", "golden", "N1_nystrom_uniform.npz"))
	gam, s, m = float(g["gamma"]), float(g["s"]), int(g["m"])
	assert len(set(g["C"].tolist())) == m
	Eq = NO.nystrom_features("se", g["x"], g["C"], g["xq"], gam, m=m)
	Ex = NO.nystrom_features("se", g["x"], g["C"], g["x"], gam, m=m)
	mu, std = NO.ridge(Ex, g["y"], Eq, s)
	assert np.abs(Eq @ Eq.T - g["gram_qq"]).max() <= 1e-10
	assert np.abs(Eq @ Ex.T - g["gram_qx"]).max() <= 1e-10
	assert np.abs(mu - g["mu"]).max() <= 1e-10 and np.abs(std - g["std"]).max() <= 1e-10


# --------------------------------------------------------------------------------------------- 4. the class refuses on the host
def test_nystrom_python_refusals(monkeypatch):
	import stpy_amd
	from stpy_amd import KernelFunction, NystromFeatures, pivoted_cholesky, _lib

	def no_device(*a, **k):
		raise AssertionError("the device was touched")
	for name in ("device", "to_device", "load"):
		monkeypatch.setattr(_lib, name, no_device)
	se = KernelFunction(kernel_name="squared_exponential", gamma=0.5, d=2)
	for approx in ("leverage", "online_leverage", "svd", "positive_svd", "cover"):
		with pytest.raises(NotImplementedError, match=approx):
			NystromFeatures(se, m=8, approx=approx)
	with pytest.raises(NotImplementedError):
		NystromFeatures(se, m=8, approx="no such thing")
	x = torch.zeros(20, 2).double()
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
			NystromFeatures(k, m=8, approx="pivoted")
		with pytest.raises(NotImplementedError):
			pivoted_cholesky(k, x, 4)
	# ... which the sampled routes accept (nothing is launched by the constructor), as the pivoted route accepts the stationary single terms
	NystromFeatures(unsupported["sum"], m=8, approx="uniform")
	for k in (se, KernelFunction(kernel_name="matern", gamma=0.3, nu=2.5, d=2), KernelFunction(kernel_name="ard", ard_gamma=[0.5, 0.2], d=2),
			  KernelFunction(kernel_name="ard_matern", ard_gamma=[0.5, 0.2], nu=0.5, d=2)):
		nys = NystromFeatures(k, m=8, approx="pivoted", tol=1e-6)
		assert nys.get_m() == 8 and nys.fit is False and nys.approx == "pivoted"
		with pytest.raises(AssertionError):
			nys.embed(x)
		with pytest.raises(NotImplementedError):
			nys._operands(torch.float64, 2)          # no input gradients through this embedding
	with pytest.raises(ValueError):
		NystromFeatures(se, m=8, approx="pivoted", tol=-1.0)
	assert "NystromFeatures" in stpy_amd.__all__ and "pivoted_cholesky" in stpy_amd.__all__
