"""
The local experts' spatial partition and routed prediction, the parts that need no GPU: partition="kdtree" of the package (torch, here on CPU
tensors) against the NumPy twin (tests/experts_route_oracle.py) and against the properties of the rule; routing ties on exactly representable
data; the work list (the package's torch version against the twin, and its invariants); the accuracy claim of the class docstring on the oracle
alone; the host refusals of the new constructor argument and of the new C entry points (every refusal comes before the first HIP call, so
placeholder pointers are safe); the resources of the new kernels.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import experts_oracle as XO
from tests import experts_route_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stpy_amd", "csrc")


def _package_kd(x, expert_size, inv_ls, cols=None):
	from stpy_amd.continuous_processes import local_experts as LE
	z = torch.from_numpy(RO.scaled(x, inv_ls, cols))
	return LE.partition_points(len(x), expert_size, "kdtree", z=z)


# --------------------------------------------------------------------------------------------- 1. the k-d partition
@pytest.mark.parametrize("n,size,d", [(XO.REF["N"], XO.REF["expert_size"], 3), (1000, 48, 2), (33, 34, 2), (34, 34, 2), (35, 34, 2), (700, 100, 5), (64, 1, 2)])
def test_kdtree_partition_rule(n, size, d):
	"""E not a power of two (REF: N = 167, size 34, E = 5; 21; 7), n below, equal to and one above expert_size, experts of one point"""
	rng = np.random.RandomState(n + d)
	x = rng.uniform(size=(n, d)) + 3.0
	inv_ls = 1.0 / np.array([0.4, 0.7, 0.3, 0.9, 0.5])[:d]
	splits = []
	order, sizes = RO.kd_partition(x, size, inv_ls, splits=splits)
	got, got_sizes = _package_kd(x, size, inv_ls)
	again, _ = _package_kd(x, size, inv_ls)
	assert got_sizes.tolist() == sizes == XO.balanced_sizes(n, size) and len(sizes) == -(-n // size)
	assert np.array_equal(got, order) and np.array_equal(got, again)          # the twin's order, deterministic
	assert sorted(got.tolist()) == list(range(n))                           # every point exactly once
	off = np.concatenate([[0], np.cumsum(sizes)])
	assert all(np.all(np.diff(got[off[e]:off[e + 1]]) > 0) for e in range(len(sizes)))          # ascending index within an expert
	z = RO.scaled(x, inv_ls)
	assert len(splits) == len(sizes) - 1
	for a, b, c, left, right in splits:          # every internal node: left <= right in the split coordinate, which has the largest spread
		pts = np.concatenate([left, right])
		spread = z[pts].max(axis=0) - z[pts].min(axis=0)
		assert z[left, c].max() <= z[right, c].min() and spread[c] == spread.max() and not np.any(spread[:c] == spread.max())
		assert len(left) == sum(sizes[a:a + (b - a + 1) // 2])


def test_kdtree_partition_reference_case_and_column_group():
	r = XO.reference_case()
	order, sizes = _package_kd(r["x"], XO.REF["expert_size"], r["inv_ls"])
	assert sizes.tolist() == [34, 34, 33, 33, 33]
	# a column group in an order of its own, the unread columns NaN: the partition of the group's columns
	wide = np.full((len(r["x"]), 5), np.nan)
	wide[:, [3, 0, 2]] = r["x"]
	il = 1.0 / np.array([0.4, 0.7, 0.3])
	o1, _ = _package_kd(wide, 34, il, cols=[3, 0, 2])
	o2, _ = RO.kd_partition(r["x"], 34, il)
	assert np.array_equal(o1, o2) and not np.array_equal(o1, order)          # (other lengthscales: another tree)


def test_kdtree_partition_of_identical_points():
	"""all points identical: every spread is zero (coordinate 0), every key ties, the original index decides: balanced contiguous pieces"""
	x = np.tile(np.array([[0.3, 1.7, -2.0]]), (167, 1))
	order, sizes = _package_kd(x, 34, np.ones(3))
	assert sizes.tolist() == [34, 34, 33, 33, 33] and np.array_equal(order, np.arange(167))
	# duplicates among distinct points: still balanced, still the twin
	x = np.repeat(np.random.RandomState(0).uniform(size=(20, 2)), 9, axis=0)
	order, sizes = _package_kd(x, 25, np.ones(2))
	assert sizes.tolist() == XO.balanced_sizes(180, 25) and np.array_equal(order, RO.kd_partition(x, 25, np.ones(2))[0])


def test_partition_strings_still_refused():
	import stpy_amd
	from stpy_amd.continuous_processes import local_experts as LE
	for name in ("kmeans", "tree", "kd", ""):
		with pytest.raises(ValueError):
			LE.partition_points(10, 3, name)
		with pytest.raises(ValueError):
			stpy_amd.LocalExpertsGaussianProcess(d=2, partition=name)
	with pytest.raises(ValueError, match="scaled coordinates"):
		LE.partition_points(10, 3, "kdtree")
	stpy_amd.LocalExpertsGaussianProcess(d=2, partition="kdtree")


# --------------------------------------------------------------------------------------------- 2. routing ties
def test_routing_ties_go_to_the_lower_id():
	# centroids on the integer grid, test points on it and midway: every distance is exact
	cent = np.array([[0.0, 0.0], [2.0, 0.0], [0.0, 2.0], [2.0, 2.0], [2.0, 2.0], [np.inf, np.inf]])          # 3 and 4: identical; 5: no rows
	xt = np.array([[1.0, 1.0], [1.0, 0.0], [2.0, 2.0], [2.0, 1.0], [0.0, 0.0]])
	il = np.ones(2)
	assert RO.route(cent, xt, il, 1).ravel().tolist() == [0, 0, 3, 1, 0]
	assert RO.route(cent, xt, il, 2).tolist() == [[0, 1], [0, 1], [3, 4], [1, 3], [0, 1]]
	assert RO.route(cent, xt, il, 3).tolist() == [[0, 1, 2], [0, 1, 2], [1, 3, 4], [1, 3, 4], [0, 1, 2]]
	sel = RO.route(cent, xt, il, 6)
	assert np.all(sel == np.arange(6)[None, :])          # k = E: everyone, the expert without rows too
	assert RO.route(cent, xt, il, 5).max() == 4          # ... which comes last
	for k in range(1, 7):
		assert np.all(np.diff(RO.route(cent, xt, il, k), axis=1) > 0)
	# two experts with identical points have identical centroids: the lower id wins
	xs = np.concatenate([np.arange(8.0).reshape(4, 2), np.arange(8.0).reshape(4, 2), 10 + np.arange(8.0).reshape(4, 2)])
	c = RO.centroids(xs, [4, 4, 0, 4], il)
	assert np.array_equal(c[0], c[1]) and np.all(np.isinf(c[2])) and np.array_equal(c[0], [3.0, 4.0])
	assert RO.route(c, np.array([[3.0, 4.0], [13.0, 14.0]]), il, 1).ravel().tolist() == [0, 3]
	assert RO.smallest_gap(c, np.array([[3.0, 4.0]]), il, 1) == 0.0 and RO.smallest_gap(c, np.array([[3.0, 4.0]]), il, 4) == np.inf


# --------------------------------------------------------------------------------------------- 3. the work list
@pytest.mark.parametrize("M,k,E", [(97, 3, 14), (65, 5, 5), (1, 1, 4), (40, 1, 3), (33, 2, 70)])
def test_work_list(M, k, E):
	from stpy_amd import _lib as L
	rng = np.random.RandomState(M + k)
	sel = np.sort(np.array([rng.choice(E, size=k, replace=False) for _ in range(M)]), axis=1)
	if (M, k) == (40, 1):
		sel[:] = 1          # one expert takes every point: full tiles and a partial one, the others none
	wexp, wpair = RO.work_list(sel, E)
	T = RO.tile_bound(E, M, k)
	assert L.experts_route_tiles(E, M, k) == T and len(wexp) == T and len(wpair) == 32 * T
	got_e, got_p = L.experts_work_list(torch.from_numpy(sel.astype(np.int32)), E)
	assert got_e.dtype == got_p.dtype == torch.int32 and np.array_equal(got_e.numpy(), wexp) and np.array_equal(got_p.numpy(), wpair)
	pairs = wpair[wpair >= 0]
	assert sorted(pairs.tolist()) == list(range(M * k))                    # every pair exactly once
	used = int(np.sum(wexp >= 0))
	assert used <= T and np.all(wexp[used:] == -1) and np.all(wpair[32 * used:] == -1)
	assert used == sum(-(-int(np.sum(sel == e)) // 32) for e in range(E))
	last = {}
	for w in range(used):
		p = wpair[32 * w:32 * w + 32]
		p = p[p >= 0]
		assert len(p) and np.all(sel.reshape(-1)[p] == wexp[w])               # a tile holds a single expert
		t = p // k
		assert np.all(np.diff(t) > 0) and t[0] > last.get(wexp[w], -1)         # test index ascending within an expert, across its tiles too
		last[wexp[w]] = t[-1]
	assert np.all(np.diff(wexp[:used]) >= 0)


# --------------------------------------------------------------------------------------------- 4. accuracy (the table of the class docstring)
@pytest.mark.parametrize("case", RO.ACCURACY, ids=lambda c: "N%d_d%d" % (c["N"], c["d"]))
def test_routing_is_accurate_only_on_a_spatial_partition(case):
	"""On the k-d partition the 4 nearest experts give the RMSE of all E (measured: 1.005, 1.010, 1.003); on a random partition the same
	truncation costs a factor (measured against kd, k = 4: 1.95, 1.97, 1.74)"""
	r = RO.accuracy_case(case)
	print(case, r, r["kd_k4"] / r["kd_all"], r["random_k4"] / r["kd_k4"])
	assert r["kd_k4"] <= 1.05 * r["kd_all"]
	assert r["random_k4"] >= 1.5 * r["kd_k4"]


# --------------------------------------------------------------------------------------------- 5. host refusals
@pytest.fixture
def no_device(monkeypatch):
	from stpy_amd import _lib

	def boom(*a, **k):
		raise AssertionError("the device was touched")
	for name in ("device", "to_device", "load"):
		monkeypatch.setattr(_lib, name, boom)
	return _lib


def test_constructor_argument(no_device):
	import stpy_amd
	for bad in (0, -1, 2.0, "4", True):
		with pytest.raises(ValueError, match="predict_experts"):
			stpy_amd.LocalExpertsGaussianProcess(d=2, predict_experts=bad)
	gp = stpy_amd.LocalExpertsGaussianProcess(d=2, predict_experts=4, partition="kdtree")
	assert gp.experts_info == {"E": 0, "sizes": [], "launches": 0, "factor_bytes": 0, "partition": "kdtree", "predict_experts": 4}
	assert stpy_amd.LocalExpertsGaussianProcess(d=2, predict_experts=1000).experts_info["partition"] == "random"
	assert set(stpy_amd.LocalExpertsGaussianProcess(d=2).experts_info) == {"E", "sizes", "launches", "factor_bytes"}          # the defaults: as before
	x = torch.rand(40, 2).double()
	mu, sd = gp.mean_std(x)          # unfitted: the prior
	assert torch.all(mu == 0) and torch.all(sd == 1)
	with pytest.raises(AttributeError):
		gp.route(x)
	with pytest.raises(ValueError, match="predict_experts=None"):
		stpy_amd.LocalExpertsGaussianProcess(d=2).route(x)
	# above the cap with more experts than the cap: refused at the fit, on the host, with the reason
	gp = stpy_amd.LocalExpertsGaussianProcess(d=2, predict_experts=17, expert_size=2)
	with pytest.raises(ValueError, match="at most 16"):
		gp.fit_gp(x, torch.rand(40, 1).double())
	assert gp.fitted is False


def test_route_argument_checks():
	from stpy_amd import _lib as L
	lib = L.load()
	P, N, Q = ctypes.c_void_p(0x1000), None, ctypes.c_void_p(0x1004)
	assert lib.stpy_experts_route_max_k() == 16
	big = 1 << 50

	def centroids(dtype=0, xs=P, n=100, ldx=4, d=4, cols=N, offsets=P, E=3, inv_ls=P, cent=P, ldc=4):
		return lib.stpy_experts_centroids(dtype, xs, n, ldx, d, cols, offsets, E, inv_ls, cent, ldc, N)

	def route(dtype=0, cent=P, ldc=4, E=20, d=4, cols=N, inv_ls=P, xt=P, M=70, ldt=4, k=4, sel=P):
		return lib.stpy_experts_route(dtype, cent, ldc, E, d, cols, inv_ls, xt, M, ldt, k, sel, N)

	def routed(kind=0, dtype=0, xs=P, n=100, ldx=4, d=4, cols=N, offsets=P, E=20, nmax=64, inv_ls=P, kappa=1.0, factor=P, fbytes=big, alpha=P, info=P,
			   xt=P, M=70, ldt=4, k=4, wexp=P, wpair=P, T=28, mu_s=P, var_s=P, ldm=70, work=P, wbytes=big):
		return lib.stpy_experts_predict_routed(kind, dtype, xs, n, ldx, d, cols, offsets, E, nmax, inv_ls, kappa, factor, fbytes, alpha, info, xt, M, ldt,
											   k, wexp, wpair, T, mu_s, var_s, ldm, work, wbytes, N)

	def routed_grad(kind=0, dtype=0, xs=P, n=100, ldx=4, d=4, cols=N, offsets=P, E=20, nmax=64, inv_ls=P, kappa=1.0, factor=P, fbytes=big, alpha=P, info=P,
					xt=P, M=70, ldt=4, k=4, wexp=P, wpair=P, T=28, mu_s=P, var_s=P, ldm=70, gmu_s=P, gvar_s=P, ldg=4, lde=280, work=P, wbytes=big):
		return lib.stpy_experts_predict_routed_grad(kind, dtype, xs, n, ldx, d, cols, offsets, E, nmax, inv_ls, kappa, factor, fbytes, alpha, info, xt, M,
													ldt, k, wexp, wpair, T, mu_s, var_s, ldm, gmu_s, gvar_s, ldg, lde, work, wbytes, N)

	wr, wg, fb = lib.stpy_experts_predict_routed_workspace_bytes(0, 64, 4, 28), lib.stpy_experts_predict_routed_grad_workspace_bytes(0, 64, 4, 28), lib.stpy_experts_factor_bytes(0, 64, 20)
	assert wr == 28 * 32 * 64 * 8 and wg == 2 * wr and lib.stpy_experts_predict_routed_workspace_bytes(0, 33, 4, 28) == wr
	assert lib.stpy_experts_predict_routed_workspace_bytes(1, 64, 4, 28) == 0 and lib.stpy_experts_predict_routed_workspace_bytes(0, 513, 4, 28) == 0
	assert lib.stpy_experts_predict_routed_workspace_bytes(0, 64, 4, 0) == 0
	assert lib.stpy_experts_predict_routed_workspace_bytes(0, 64, 4, 28) < lib.stpy_experts_predict_routed_workspace_bytes(0, 64, 4, 29)
	kk = {"k = 0": dict(k=0), "k negative": dict(k=-1), "k above the cap": dict(k=17), "k above E": dict(E=3, k=4), "M k at 2^31": dict(M=1 << 30, k=2)}
	predict = dict(kk, **{"unknown kind": dict(kind=9), "fp32": dict(dtype=1), "nmax above the cap": dict(nmax=513), "ldx < d": dict(ldx=3), "d < 1": dict(d=0),
				   "null xs": dict(xs=N), "null offsets": dict(offsets=N), "null inv_ls": dict(inv_ls=N), "null factor": dict(factor=N), "null alpha": dict(alpha=N),
				   "null info": dict(info=N), "null xt": dict(xt=N), "null wexp": dict(wexp=N), "null wpair": dict(wpair=N), "null mu_s": dict(mu_s=N),
				   "null var_s": dict(var_s=N), "null work": dict(work=N), "ldt < d": dict(ldt=3), "ldm < M": dict(ldm=69), "negative M": dict(M=-1),
				   "negative T": dict(T=-1), "T at 2^31": dict(T=1 << 31), "kappa 0": dict(kappa=0.0), "kappa nan": dict(kappa=float("nan")),
				   "small factor": dict(fbytes=fb - 1), "misaligned work": dict(work=Q), "misaligned mu_s": dict(mu_s=Q), "E out of range": dict(E=1 << 31)})
	cases = [("stpy_experts_centroids", centroids, {"fp32": dict(dtype=1), "d < 1": dict(d=0), "ldx < d": dict(ldx=3), "ldc < d": dict(ldc=3), "null xs": dict(xs=N),
			  "null offsets": dict(offsets=N), "null inv_ls": dict(inv_ls=N), "null cent": dict(cent=N), "misaligned cent": dict(cent=Q), "negative E": dict(E=-1)}),
			 ("stpy_experts_route", route, dict(kk, **{"fp32": dict(dtype=1), "d < 1": dict(d=0), "ldc < d": dict(ldc=3), "ldt < d": dict(ldt=3), "null cent": dict(cent=N),
			  "null inv_ls": dict(inv_ls=N), "null xt": dict(xt=N), "null sel": dict(sel=N), "misaligned xt": dict(xt=Q), "negative M": dict(M=-1)})),
			 ("stpy_experts_predict_routed", routed, dict(predict, **{"small workspace": dict(wbytes=wr - 1)})),
			 ("stpy_experts_predict_routed_grad", routed_grad, dict(predict, **{"small workspace": dict(wbytes=wg - 1), "null gmu_s": dict(gmu_s=N),
			  "null gvar_s": dict(gvar_s=N), "ldg < d": dict(ldg=3), "lde < M ldg": dict(lde=279), "misaligned gvar_s": dict(gvar_s=Q)}))]
	for name, call, refused in cases:
		for what, kw in refused.items():
			lib.stpy_lml_batch(0, 1, N, 1, 1, 1, N, N, 1, N, 1, N, 1.0, 1.0, N, 1, N, N, 2, N, N, 0, N)          # (leaves some OTHER message behind)
			before = lib.stpy_last_error_string()
			rc = call(**kw)
			assert rc < 0, (name, what, rc)
			msg = lib.stpy_last_error_string()
			assert msg and name.encode() in msg and msg != before, (name, what, msg)
	assert route(k=0) == routed(k=17) == routed_grad(E=3, k=4) == -23 and routed(ldm=69) == -13 and routed(wbytes=wr - 1) == -20 and routed(dtype=1) == -2
	# the empty problems: 0 without looking at a pointer
	assert centroids(E=0, xs=N, cent=N) == 0 and route(E=0, cent=N) == 0 and route(M=0, xt=N, sel=N) == 0
	for call in (routed, routed_grad):
		assert call(E=0, xs=N, work=N) == 0 and call(M=0, xt=N, mu_s=N) == 0 and call(n=0, xs=N) == 0 and call(T=0, wexp=N, wpair=N, work=N) == 0


# --------------------------------------------------------------------------------------------- 6. kernel resources
def test_route_kernel_resources(tmp_path):
	"""The four new kernels: no scratch -- the routing kernel's candidate lists and the routed tiles' tables included -- and the LDS and occupancy
	figures of the kernels they stand beside"""
	out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-comment", "-c", os.path.join(CSRC, "experts.hip"),
						  "-o", str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True).stderr
	blocks = {b.split()[0]: b for b in re.split(r"remark: Function Name: ", out)[1:]}
	for kernel in ("experts_predict_routed_kernel", "experts_predict_routed_grad_kernel", "experts_centroids_kernel", "experts_route_kernel"):
		b = [v for name, v in blocks.items() if kernel in name]
		assert len(b) == 1, (kernel, sorted(blocks))
		assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b[0]).group(1)) == 0, kernel
		assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b[0]).group(1)) <= 40960, kernel
		assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b[0]).group(1)) >= 2, kernel
