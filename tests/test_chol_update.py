"""
Rank-k Cholesky update / downdate: stpy_chol_update (csrc/cholupdate.hip) and KernelizedFeatures.add_data_point(iterative=True)
built on it.  The checkers are written here: the column-by-column rotation algorithm in NumPy, carried out in the call's dtype, and
numpy.linalg.cholesky of the updated matrix.  The updated factor must leave exactly the layout stpy_potrf leaves (inverse diagonal
blocks included), so every consumer runs on it unchanged.
"""
import inspect
import os

import numpy as np
import pytest
import torch

from tests.conftest import ROOT, rel_err

IB = 128


# ---------------------------------------------------------------- CPU: the interface exists
def test_header_declares_chol_update():
	with open(os.path.join(ROOT, "include", "stpy_hip.h")) as f:
		h = " ".join(f.read().split())
	assert "int64_t stpy_chol_update_workspace_bytes(int dtype, int64_t n, int64_t k);" in h
	assert ("int stpy_chol_update(int dtype, int64_t n, int64_t k, int sign, void* L, int64_t ldl, void* winv, int64_t winv_elems, "
			"void* W, int64_t ldw, void* work, int64_t work_bytes, int32_t* info_dev, void* stream);") in h


def test_signatures_list_chol_update():
	"""One ctypes entry per prototype argument: 14 for stpy_chol_update as the header declares it (dtype, n, k, sign, L, ldl, winv,
	winv_elems, W, ldw, work, work_bytes, info_dev, stream), 3 for the workspace query."""
	from stpy_amd import _lib
	assert _lib.SIGNATURES["stpy_chol_update_workspace_bytes"] == (_lib._i64, [_lib._i32, _lib._i64, _lib._i64])
	res, args = _lib.SIGNATURES["stpy_chol_update"]
	assert res is _lib._i32 and len(args) == 14
	assert args[:4] == [_lib._i32, _lib._i64, _lib._i64, _lib._i32] and args[-2:] == [_lib._vp, _lib._vp]
	assert "sign" in inspect.signature(_lib.chol_update).parameters


def test_add_data_point_accepts_iterative():
	from stpy_amd.continuous_processes.kernelized_features import KernelizedFeatures
	p = inspect.signature(KernelizedFeatures.add_data_point).parameters
	assert "iterative" in p and p["iterative"].default is False
	assert inspect.signature(KernelizedFeatures.add_data).parameters["iterative"].default is False


# ---------------------------------------------------------------- checkers (NumPy)
def np_rotate(L, W, sign, dtype):
	"""The column-by-column rotation algorithm in ``dtype``: returns (L', 0), or (None, j + 1) at the first pivot that is not positive."""
	L = np.tril(L).astype(dtype).copy()
	W = np.array(W, dtype=dtype, copy=True)
	n, k = W.shape
	sg = dtype(sign)
	for j in range(n):
		for r in range(k):
			a, w = L[j, j], W[j, r]
			d = a * a + sg * w * w
			if not (d > 0 and np.isfinite(d)):
				return None, j + 1
			b = np.sqrt(d)
			c, s = b / a, w / a
			L[j, j] = b
			if j + 1 < n:
				L[j + 1:, j] = (L[j + 1:, j] + sg * s * W[j + 1:, r]) / c
				W[j + 1:, r] = c * W[j + 1:, r] - s * L[j + 1:, j]
	return L, 0


def residual(Lnew, target):
	"""||L' L'^T - target||_F / ||target||_F in fp64."""
	Ln = np.tril(np.asarray(Lnew, dtype=np.float64))
	return np.linalg.norm(Ln @ Ln.T - target) / np.linalg.norm(target)


def residual_bound(L, W, sign, dtype):
	"""8 x the larger of: the residual of the NumPy rotation checker in ``dtype``, the residual of numpy.linalg.cholesky of the
	target rounded to ``dtype``.  The target is formed in fp64 from the dtype-rounded inputs."""
	L64, W64 = np.tril(L).astype(np.float64), np.asarray(W, dtype=np.float64)
	target = L64 @ L64.T + sign * (W64 @ W64.T)
	Lrot, bad = np_rotate(L, W, sign, dtype)
	assert bad == 0
	r_rot = residual(Lrot, target)
	r_chol = residual(np.linalg.cholesky(target.astype(dtype)), target)
	return target, 8.0 * max(r_rot, r_chol), (r_rot, r_chol)


def first_bad_minor(A):
	"""1-based order of the first leading minor of the symmetric matrix A that is not positive (0: none)."""
	A = np.array(A, dtype=np.float64, copy=True)
	for j in range(A.shape[0]):
		if not A[j, j] > 0:
			return j + 1
		A[j + 1:, j] /= np.sqrt(A[j, j])
		A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
	return 0


# ---------------------------------------------------------------- data: V = Phi^T Phi + c I from seeded random features
NS = [1, 127, 128, 129, 389, 640]
KS = [1, 2, 7, 128, 129]
ROWS, KMAX, GAMMA, RIDGE = 600, 129, 0.3, 0.01
_CACHE = {}


def features(x, Wf, b):
	"""sqrt(2 / m) cos(<W_j, x> + b_j), (n, m)."""
	return np.sqrt(2.0 / Wf.shape[0]) * np.cos(x @ Wf.T + b.reshape(1, -1))


def problem(n):
	"""(fp64 factor of V (n x n), the features of KMAX further points as W (n x KMAX))."""
	if n not in _CACHE:
		rng = np.random.RandomState(100 + n)
		Wf, b = rng.normal(size=(n, 2)) / GAMMA, 2 * np.pi * rng.uniform(size=n)
		Phi = features(rng.uniform(-1, 1, size=(ROWS, 2)), Wf, b)
		V = Phi.T @ Phi + RIDGE * np.eye(n)
		_CACHE[n] = (np.linalg.cholesky(V), features(rng.uniform(-1, 1, size=(KMAX, 2)), Wf, b).T.copy())
	return _CACHE[n]


def np_dtype(dtype):
	return np.float64 if dtype == torch.float64 else np.float32


def on_device(L, dtype, fill=3.0):
	"""Lower triangle of L on the device in ``dtype``, the strict upper triangle filled with ``fill`` (it is never read)."""
	n = L.shape[0]
	A = torch.from_numpy(np.tril(L)).to(dtype) + torch.triu(torch.full((n, n), fill, dtype=dtype), 1)
	return A.cuda().contiguous()


def run_update(A, W, sign, winv=None):
	"""stpy_chol_update through the typed wrapper on copies; returns (L', winv', info)."""
	from stpy_amd import _lib
	A = A.clone()
	if winv is None:
		winv = torch.full((_lib.potrf_winv_elems(A.shape[0]),), 5.0, dtype=A.dtype, device=A.device)
	else:
		winv = winv.clone()
	info = _lib.chol_update(A, winv, W.clone(), sign)
	torch.cuda.synchronize()
	return A, winv, int(info.item())


def winv_reference(L, n):
	"""The inverse 128 x 128 diagonal blocks of the fp64 factor L in the layout stpy_potrf leaves (identity border on a ragged tile)."""
	nt = -(-n // IB)
	out = np.zeros((nt, IB, IB))
	for c in range(nt):
		nb = min(IB, n - c * IB)
		blk = np.eye(IB)
		blk[:nb, :nb] = np.tril(L[c * IB:c * IB + nb, c * IB:c * IB + nb])
		out[c] = np.linalg.inv(blk)
	return out.reshape(-1)


# ---------------------------------------------------------------- GPU, C ABI level
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_gpu_update_then_downdate(gpu_device, n, k, dtype):
	"""sign = +1: residual against L L^T + W W^T; consumers on (L', winv'); then sign = -1 with the same W returns to the original
	matrix -- both under the residual rule of the module header; the strict upper triangle keeps its fill."""
	from stpy_amd import _lib
	nd = np_dtype(dtype)
	L0, Wall = problem(n)
	L0r, Wr = np.tril(L0).astype(nd), Wall[:, :k].astype(nd)
	A = on_device(L0r, dtype)
	Wd = torch.from_numpy(Wr).cuda().contiguous()
	# ---- update
	target, bound, parts = residual_bound(L0r, Wr, +1, nd)
	A1, winv1, info = run_update(A, Wd, +1)
	assert info == 0
	L1 = A1.cpu().numpy()
	res = residual(L1, target)
	print("n=%d k=%d %s update: residual %.3e  bound %.3e  (rotation %.3e, cholesky %.3e)" % ((n, k, nd.__name__, res, bound) + parts))
	assert res <= bound
	assert np.all(np.diag(L1) > 0)
	assert np.array_equal(np.triu(L1, 1), np.triu(np.full((n, n), 3.0, dtype=nd), 1))
	# ---- consumers: both vector solves and the log-determinant on (L', winv') against NumPy on the fp64 target
	Lref = np.linalg.cholesky(target)
	y = np.random.RandomState(n + k).normal(size=n)
	want = [np.linalg.solve(Lref, y), np.linalg.solve(Lref.T, y), np.sum(np.log(np.diag(Lref)))]
	yd = torch.from_numpy(y).to(dtype).cuda()

	def consumers(Lc, wc):
		return [_lib.trsv(Lc, wc, yd, trans=0).cpu().numpy(), _lib.trsv(Lc, wc, yd, trans=1).cpu().numpy(), float(_lib.logdet_quad(Lc)[0].item())]
	got = consumers(A1, winv1)
	_lib.check_async("stpy_trsv on the updated factor")
	if dtype == torch.float64:
		tols = [1e-8] * 3
		assert rel_err(winv1.cpu().numpy(), winv_reference(Lref, n)) < 1e-8
	else:
		# 4 x what stpy_potrf of the same matrix in fp32 shows against the same NumPy values
		P = torch.from_numpy(np.tril(target)).to(dtype).cuda().contiguous()
		wp, pinfo = _lib.potrf(P)
		assert int(pinfo.item()) == 0
		tols = [4.0 * rel_err(g, w) for g, w in zip(consumers(P, wp), want)]
	for name, g, w, tol in zip(("trsv", "trsv trans", "logdet"), got, want, tols):
		err = rel_err(g, w)
		print("   %s: err %.3e  tol %.3e" % (name, err, tol))
		assert err <= tol, name
	# ---- downdate back
	target2, bound2, parts2 = residual_bound(L1, Wr, -1, nd)
	A2, winv2, info2 = run_update(A1, Wd, -1, winv1)
	assert info2 == 0
	res2 = residual(A2.cpu().numpy(), target2)
	print("n=%d k=%d %s downdate: residual %.3e  bound %.3e  (rotation %.3e, cholesky %.3e)" % ((n, k, nd.__name__, res2, bound2) + parts2))
	assert res2 <= bound2
	assert np.all(np.diag(A2.cpu().numpy()) > 0)
	if dtype == torch.float64:
		assert rel_err(winv2.cpu().numpy(), winv_reference(np.linalg.cholesky(target2), n)) < 1e-8


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("j", [5, 385])
def test_gpu_indefinite_downdate_is_reported(gpu_device, j, dtype):
	"""W = 2 x column j of L (first / last tile of n = 389): the downdated matrix is indefinite from leading minor j + 1 on."""
	nd = np_dtype(dtype)
	L0 = np.tril(problem(389)[0]).astype(nd)
	Wr = (2 * L0[:, j:j + 1]).copy()
	L64, W64 = L0.astype(np.float64), Wr.astype(np.float64)
	bad = first_bad_minor(L64 @ L64.T - W64 @ W64.T)
	assert bad == j + 1
	_, _, info = run_update(on_device(L0, dtype), torch.from_numpy(Wr).cuda(), -1)
	print("j=%d: info %d, first non-positive leading minor %d" % (j, info, bad))
	assert 1 <= info <= bad


@pytest.mark.gpu
def test_gpu_refusals_and_empty_update(gpu_device):
	from stpy_amd import _lib
	lib = _lib.load()
	n, k = 389, 3
	L0, Wall = problem(n)
	A = on_device(L0, torch.float64)
	before = A.clone()
	W = torch.from_numpy(Wall[:, :k].copy()).cuda()
	winv = torch.zeros((_lib.potrf_winv_elems(n),), dtype=torch.float64, device="cuda")
	need = int(lib.stpy_chol_update_workspace_bytes(_lib.F64, n, k))
	assert need > 0 and int(lib.stpy_chol_update_workspace_bytes(_lib.F64, n, 0)) == 0
	work = torch.empty((need,), dtype=torch.uint8, device="cuda")
	info = torch.zeros((1,), dtype=torch.int32, device="cuda")

	def call(k_, winv_elems, work_bytes):
		return lib.stpy_chol_update(_lib.F64, n, k_, 1, _lib.ptr(A), n, _lib.ptr(winv), winv_elems, _lib.ptr(W), k, _lib.ptr(work), work_bytes,
									_lib.ptr(info), _lib.stream_ptr())
	assert call(k, winv.numel(), need - 1) == -20
	assert call(k, winv.numel() - 1, need) == -21
	assert call(0, winv.numel(), need) == 0
	torch.cuda.synchronize()
	assert torch.equal(A, before)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("sign", [1, -1])
def test_gpu_update_is_reproducible(gpu_device, sign, dtype):
	"""Two runs on identical inputs: bit-identical L' and winv' (ragged order, two chunks of W)."""
	nd = np_dtype(dtype)
	L0, Wall = problem(389)
	A, Wd = on_device(L0.astype(nd), dtype), torch.from_numpy(Wall[:, :40].astype(nd)).cuda().contiguous()
	if sign < 0:          # (a downdate that stays positive definite: it takes out what an update put in)
		A, _, i0 = run_update(A, Wd, +1)
		assert i0 == 0
	a1, w1, i1 = run_update(A, Wd, sign)
	a2, w2, i2 = run_update(A, Wd, sign)
	assert i1 == 0 and i2 == 0
	assert torch.equal(a1, a2) and torch.equal(w1, w2)


# ---------------------------------------------------------------- GPU, estimator level
M_FEAT, N_INIT, N_TEST = 389, 300, 64


def phase_embedding(seed=3):
	"""Random features sqrt(2 / m) cos(<W_j, x> + b_j) in the (n, m) orientation, so that the feature count may be odd."""
	import stpy_amd.embeddings.embedding as E
	from stpy_amd import _lib

	class PhaseFeatures(E.RFFEmbedding):
		def __init__(self, m, **kw):
			super().__init__(m=m + m % 2, **kw)
			self.m = m
			self.b = torch.from_numpy(2 * np.pi * np.random.uniform(size=m))

		def _operands(self, dtype, d):
			Wd, _, fs, scale = super()._operands(dtype, d)
			return Wd, _lib.to_device(self.b, dtype), fs, scale

	np.random.seed(seed)
	return PhaseFeatures(M_FEAT, gamma=GAMMA, d=2)


def kf_data(extra):
	rng = np.random.RandomState(17)
	n = N_INIT + extra
	x = rng.uniform(-1, 1, size=(n, 2))
	y = np.sin(3 * x[:, :1]) * np.cos(2 * x[:, 1:]) + 0.05 * rng.normal(size=(n, 1))
	return x, y, rng.uniform(-1, 1, size=(N_TEST, 2))


S_NOISE, LAM = 0.1, 1.0


def make_kf(emb, x, y, dtype=torch.float64, primal=True):
	from stpy_amd.continuous_processes.kernelized_features import KernelizedFeatures
	KF = KernelizedFeatures(embedding=emb, m=emb.get_m(), s=S_NOISE, lam=LAM, d=2, primal=primal)
	KF.fit_gp(torch.from_numpy(x).to(dtype), torch.from_numpy(y).to(dtype))
	return KF


def oracle_mean_std(emb, x, y, xt):
	from oracle import gp_oracle as O
	Wf, b = emb.W.numpy()[:M_FEAT], emb.b.numpy()
	_, invV, theta = O.kernelized_features_fit(features(x, Wf, b), y, S_NOISE, LAM)
	return O.kernelized_features_mean_std(features(xt, Wf, b), invV, theta, S_NOISE)


@pytest.fixture
def counters(monkeypatch):
	"""Call counters on the typed wrappers _lib.potrf / _lib.potri."""
	from stpy_amd import _lib
	count = {"potrf": 0, "potri": 0}

	def counting(name):
		inner = getattr(_lib, name)

		def wrapper(*a, **kw):
			count[name] += 1
			return inner(*a, **kw)
		return wrapper
	for name in count:
		monkeypatch.setattr(_lib, name, counting(name))
	return count


def t64(a):
	return a.detach().double().cpu().numpy()


@pytest.mark.gpu
def test_gpu_single_point_adds_never_refactor(gpu_device, counters):
	x, y, xt = kf_data(20)
	emb = phase_embedding()
	KF = make_kf(emb, x[:N_INIT], y[:N_INIT])
	xtt = torch.from_numpy(xt)
	KF.mean_std(xtt)
	after_fit = dict(counters)
	for i in range(N_INIT, N_INIT + 20):
		KF.add_data_point(torch.from_numpy(x[i:i + 1]), torch.from_numpy(y[i:i + 1]), iterative=True)
		mu, std = KF.mean_std(xtt)
		mu_o, std_o = oracle_mean_std(emb, x[:i + 1], y[:i + 1], xt)
		assert rel_err(t64(mu), mu_o) < 1e-8 and rel_err(t64(std), std_o) < 1e-8, i
	assert counters["potrf"] == after_fit["potrf"], "an iterative single-point add refactored"
	assert KF.n == N_INIT + 20 and KF.x.shape[0] == N_INIT + 20
	fresh = make_kf(emb, x, y)
	mu_f, std_f = fresh.mean_std(xtt)
	assert rel_err(t64(mu), t64(mu_f)) < 1e-8 and rel_err(t64(std), t64(std_f)) < 1e-8
	# V_acc and Phi^T y stayed exact: V and theta of the updated object are those of the fresh fit
	assert rel_err(t64(KF.V), t64(fresh.V)) < 1e-12
	assert rel_err(t64(KF.theta_mean()), t64(fresh.theta_mean())) < 1e-8


@pytest.mark.gpu
def test_gpu_batches_and_refit_routes(gpu_device, counters):
	x, y, xt = kf_data(12)
	emb = phase_embedding()
	xtt = torch.from_numpy(xt)
	tx, ty = lambda a, b: torch.from_numpy(x[a:b]), lambda a, b: torch.from_numpy(y[a:b])

	def agree(KF, rows):
		mu, std = KF.mean_std(xtt)
		mu_o, std_o = oracle_mean_std(emb, x[:rows], y[:rows], xt)
		mu_f, std_f = make_kf(emb, x[:rows], y[:rows]).mean_std(xtt)
		assert rel_err(t64(mu), mu_o) < 1e-8 and rel_err(t64(std), std_o) < 1e-8
		assert rel_err(t64(mu), t64(mu_f)) < 1e-8 and rel_err(t64(std), t64(std_f)) < 1e-8

	# one batch of 5 rows: one update, no factorisation
	KF = make_kf(emb, x[:N_INIT], y[:N_INIT])
	c0 = counters["potrf"]
	KF.add_data_point(tx(N_INIT, N_INIT + 5), ty(N_INIT, N_INIT + 5), iterative=True)
	KF.precompute()
	assert counters["potrf"] == c0
	agree(KF, N_INIT + 5)
	# two queued entries, both iterative: still one update
	c0 = counters["potrf"]
	KF.add_data_point(tx(N_INIT + 5, N_INIT + 7), ty(N_INIT + 5, N_INIT + 7), iterative=True)
	KF.add_data_point(tx(N_INIT + 7, N_INIT + 8), ty(N_INIT + 7, N_INIT + 8), iterative=True)
	KF.precompute()
	assert counters["potrf"] == c0
	agree(KF, N_INIT + 8)
	# a batch wider than update_max_rank refits
	KF.update_max_rank = 3
	c0 = counters["potrf"]
	KF.add_data_point(tx(N_INIT + 8, N_INIT + 12), ty(N_INIT + 8, N_INIT + 12), iterative=True)
	KF.precompute()
	assert counters["potrf"] == c0 + 1
	agree(KF, N_INIT + 12)
	# one entry queued without the flag: the whole batch refits, and the entry keeps the [x, y] form
	KF2 = make_kf(emb, x[:N_INIT], y[:N_INIT])
	KF2.add_data_point(tx(N_INIT, N_INIT + 1), ty(N_INIT, N_INIT + 1), iterative=True)
	KF2.add_data_point(tx(N_INIT + 1, N_INIT + 2), ty(N_INIT + 1, N_INIT + 2))
	assert len(KF2.to_add[1]) == 2
	c0 = counters["potrf"]
	KF2.precompute()
	assert counters["potrf"] == c0 + 1
	agree(KF2, N_INIT + 2)
	# a changed noise level refits
	KF3 = make_kf(emb, x[:N_INIT], y[:N_INIT])
	KF3.s = 2 * S_NOISE
	KF3.add_data_point(tx(N_INIT, N_INIT + 1), ty(N_INIT, N_INIT + 1), iterative=True)
	c0 = counters["potrf"]
	KF3.precompute()
	assert counters["potrf"] == c0 + 1


@pytest.mark.gpu
def test_gpu_dual_form_refits(gpu_device, counters):
	"""primal=False with fewer rows than features: the flag is accepted and the dual refit runs, results as without it."""
	x, y, xt = kf_data(3)
	emb = phase_embedding()
	xtt = torch.from_numpy(xt)
	out = []
	for flag in (True, False):
		KF = make_kf(emb, x[:N_INIT], y[:N_INIT], primal=False)
		assert KF.dual
		c0 = counters["potrf"]
		KF.add_data_point(torch.from_numpy(x[N_INIT:]), torch.from_numpy(y[N_INIT:]), iterative=flag)
		out.append(KF.mean_std(xtt))
		assert counters["potrf"] == c0 + 1
	assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.gpu
def test_gpu_sampler_factor_follows_the_update(gpu_device, counters):
	x2, y2, _ = kf_data(3)
	x, y = x2[:N_INIT + 1], y2[:N_INIT + 1]
	emb = phase_embedding()
	KF = make_kf(emb, x[:N_INIT], y[:N_INIT])
	torch.manual_seed(5)
	first = KF.sample_theta()
	# the factor of V^-1 is kept: a second draw with the same seed is the same draw, without another factorisation
	c0 = dict(counters)
	torch.manual_seed(5)
	assert torch.equal(KF.sample_theta(), first)
	KF.add_data_point(torch.from_numpy(x[N_INIT:]), torch.from_numpy(y[N_INIT:]), iterative=True)
	torch.manual_seed(6)
	th = KF.sample_theta(size=3)
	assert counters == c0, "a draw after an iterative add factored or inverted again"
	fresh = make_kf(emb, x, y)
	torch.manual_seed(6)
	th_f = fresh.sample_theta(size=3)
	assert th.shape == (M_FEAT, 3)
	assert rel_err(t64(th), t64(th_f)) < 1e-8
	# a batch of two rows drops the kept factor; the next draw recomputes it and still agrees
	KF.add_data_point(torch.from_numpy(x2[N_INIT + 1:]), torch.from_numpy(y2[N_INIT + 1:]), iterative=True)
	torch.manual_seed(7)
	th2 = KF.sample_theta()
	torch.manual_seed(7)
	assert rel_err(t64(th2), t64(make_kf(emb, x2, y2).sample_theta())) < 1e-8


@pytest.mark.gpu
def test_gpu_default_add_is_unchanged(gpu_device, counters):
	"""No flag: the queued points are folded in by a refactorisation, bit for bit the same on two objects."""
	x, y, xt = kf_data(4)
	emb = phase_embedding()
	xtt = torch.from_numpy(xt)
	out = []
	for _ in range(2):
		KF = make_kf(emb, x[:N_INIT], y[:N_INIT])
		c0 = counters["potrf"]
		for i in range(N_INIT, N_INIT + 4):
			KF.add_data_point(torch.from_numpy(x[i:i + 1]), torch.from_numpy(y[i:i + 1]))
			assert KF.to_add and len(KF.to_add[-1]) == 2
			mu, std = KF.mean_std(xtt)
		assert counters["potrf"] == c0 + 4
		torch.manual_seed(2)
		out.append((mu, std, KF.sample_theta()))
	for a, b in zip(*out):
		assert torch.equal(a, b)
	mu_o, std_o = oracle_mean_std(emb, x, y, xt)
	assert rel_err(t64(out[0][0]), mu_o) < 1e-8 and rel_err(t64(out[0][1]), std_o) < 1e-8


@pytest.mark.gpu
def test_gpu_input_gradients_after_update(gpu_device):
	"""mean_std through a test tensor with requires_grad, before and after an iterative add: the inverse kept for the gradient of
	sigma belongs to the old factor and must have been dropped."""
	x, y, xt = kf_data(1)
	emb = phase_embedding()

	def grads(KF):
		z = torch.from_numpy(xt[:8]).clone().requires_grad_(True)
		mu, std = KF.mean_std(z)
		(mu.sum() + 2.0 * std.sum()).backward()
		return t64(z.grad)
	KF = make_kf(emb, x[:N_INIT], y[:N_INIT])
	g_old = grads(KF)
	KF.add_data_point(torch.from_numpy(x[N_INIT:]), torch.from_numpy(y[N_INIT:]), iterative=True)
	g_new = grads(KF)
	g_fresh = grads(make_kf(emb, x, y))
	assert rel_err(g_new, g_fresh) < 1e-8
	assert rel_err(g_old, g_fresh) > 1e-6          # (the added point does move the gradient: the comparison above is not vacuous)


@pytest.mark.gpu
def test_gpu_single_point_adds_fp32(gpu_device, counters):
	"""The 20-add loop in fp32: within 4 x the deviation of the fp32 refit path from the fp64 oracle on the same data."""
	x, y, xt = kf_data(20)
	emb = phase_embedding()
	xtt = torch.from_numpy(xt).float()
	KF = make_kf(emb, x[:N_INIT], y[:N_INIT], dtype=torch.float32)
	c0 = counters["potrf"]
	for i in range(N_INIT, N_INIT + 20):
		KF.add_data_point(torch.from_numpy(x[i:i + 1]).float(), torch.from_numpy(y[i:i + 1]).float(), iterative=True)
		mu, std = KF.mean_std(xtt)
	assert counters["potrf"] == c0
	assert mu.dtype == torch.float32
	mu_r, std_r = make_kf(emb, x, y, dtype=torch.float32).mean_std(xtt)
	mu_o, std_o = oracle_mean_std(emb, x, y, xt)
	for name, got, refit, want in (("mu", mu, mu_r, mu_o), ("std", std, std_r, std_o)):
		e_upd, e_refit = rel_err(t64(got), want), rel_err(t64(refit), want)
		print("fp32 %s: update path %.3e, refit path %.3e" % (name, e_upd, e_refit))
		assert e_upd <= 4.0 * e_refit, name
