"""
Batched evidence (stpy_lml_batch / optimize_params(parallel=True)), the parts that need no GPU: the argument checks of the C entry
point (every refusal comes before the first HIP call, so placeholder pointers are safe), the kernel's resource usage, and the
lockstep / stacked restart drivers of Estimator.optimize_params_general on an estimator whose evidence is the NumPy oracle.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.linalg
import torch

from oracle import gp_oracle as O
from stpy_amd.estimator import Estimator, Euclidean

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stpy_amd", "csrc")


# --------------------------------------------------------------------------------------------- 1. argument checks
def test_lml_batch_argument_checks():
	from stpy_amd import _lib as L
	lib = L.load()
	P, N = ctypes.c_void_p(0x1000), None          # a non-null pointer no refused call may dereference
	cap = lib.stpy_lml_batch_max_n()
	assert cap >= 512
	big = 1 << 40

	def call(kind=0, dtype=0, x=P, n=64, ldx=4, d=4, cols=N, y=P, batch=3, inv_ls=P, ldi=4, noise=P, pidx=P, np_=1, value=P, grad=P, ldg=2,
			 info=P, work=P, work_bytes=big):
		return lib.stpy_lml_batch(kind, dtype, x, n, ldx, d, cols, y, batch, inv_ls, ldi, noise, 1.0, 1.0, pidx, np_, value, grad, ldg, info,
								  work, work_bytes, N)

	refused = {
		"null x": dict(x=N), "null y": dict(y=N), "null inv_ls": dict(inv_ls=N), "null noise": dict(noise=N), "null pidx": dict(pidx=N),
		"null value": dict(value=N), "null grad": dict(grad=N), "null info": dict(info=N), "null work": dict(work=N),
		"n above the cap": dict(n=cap + 1),
		"ldx < d": dict(ldx=3), "ldi < d": dict(ldi=3), "ldg < np + 1": dict(np_=2, ldg=2),
		"d < 1": dict(d=0, ldx=1, ldi=1), "np < 1": dict(np_=0),
		"unknown kind": dict(kind=9), "negative kind": dict(kind=-1), "LINEAR": dict(kind=4), "POLY": dict(kind=5 | (2 << 8)),
		"undersized workspace": dict(work_bytes=lib.stpy_lml_batch_workspace_bytes(0, 64, 4, 3) - 1),
		"fp32": dict(dtype=1), "unknown dtype": dict(dtype=7),
	}
	for what, kw in refused.items():
		lib.stpy_lml_batch(0, 1, N, 1, 1, 1, N, N, 1, N, 1, N, 1.0, 1.0, N, 1, N, N, 2, N, N, 0, N)          # (leaves some OTHER message behind)
		before = lib.stpy_last_error_string()
		rc = call(**kw)
		assert rc < 0, (what, rc)
		msg = lib.stpy_last_error_string()
		assert msg and b"stpy_lml_batch" in msg and (what == "fp32" or msg != before), (what, msg)
	# the two empty problems: 0 without looking at a pointer
	assert lib.stpy_lml_batch(0, 0, N, 0, 4, 4, N, N, 3, N, 4, N, 1.0, 1.0, N, 1, N, N, 2, N, N, 0, N) == 0
	assert lib.stpy_lml_batch(0, 0, N, 64, 4, 4, N, N, 0, N, 4, N, 1.0, 1.0, N, 1, N, N, 2, N, N, 0, N) == 0
	# workspace query: positive, non-decreasing in n and in batch
	last = 0
	for n in (1, 2, 31, 32, 33, 100, 128, 300, 511, 512, cap):
		b = lib.stpy_lml_batch_workspace_bytes(0, n, 4, 5)
		assert b > 0 and b >= last, (n, b, last)
		last = b
	last = 0
	for batch in (1, 2, 7, 8, 64, 300):
		b = lib.stpy_lml_batch_workspace_bytes(0, 200, 4, batch)
		assert b > 0 and b >= last, (batch, b, last)
		last = b


# --------------------------------------------------------------------------------------------- 2. kernel resources
def test_lml_batch_kernel_resources(tmp_path):
	"""Every kernel of the batched evidence: no scratch, at most 64 KiB of LDS and registers for two waves per SIMD (two candidates share a CU)."""
	out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-comment", "-c", os.path.join(CSRC, "reduce.hip"),
						  "-o", str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True).stderr
	blocks = [b for b in re.split(r"remark: Function Name: ", out)[1:] if "lml_batch" in b.split()[0]]
	assert len(blocks) >= 1
	for b in blocks:
		name = b.split()[0]
		assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, name
		assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) <= 65536, name
		assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)) >= 2, name


# --------------------------------------------------------------------------------------------- 3. driver logic on an oracle-backed estimator
N_PTS, DIM, S0 = 40, 2, 0.1


def _data():
	rng = np.random.RandomState(3)
	x = rng.uniform(-1, 1, size=(N_PTS, DIM))
	y = np.sin(3 * x[:, :1]) * np.cos(2 * x[:, 1:2]) + 0.1 * rng.normal(size=(N_PTS, 1))
	return x, y


def _oracle(x, y, gamma, s, weight):
	"""(value, d/dgamma, d/ds) of the SE evidence from the NumPy oracle; LinAlgError when the matrix is not positive definite"""
	spec = [("squared_exponential", {"gamma": float(gamma), "kappa": 1.0}, "-")]
	try:
		v, g, gs = O.log_marginal_grad(x, y, spec, float(s), None, weight)
	except (np.linalg.LinAlgError, scipy.linalg.LinAlgError, ValueError) as e:
		raise torch.linalg.LinAlgError(str(e))
	v = float(v[0, 0])
	if not np.isfinite(v):
		raise torch.linalg.LinAlgError("not finite")
	return v, float(g[0]["gamma"][0]), float(gs)


class _Stub:
	def __init__(self):
		self.params_dict = {'0': {'gamma': 1.0, 'kappa': 1.0, 'group': list(range(DIM))}}


class _OracleFn(torch.autograd.Function):
	@staticmethod
	def forward(ctx, est, weight, gamma, s):
		v, ctx.gg, ctx.gs = _oracle(est.x, est.y, float(gamma.reshape(-1)[0]), float(s.reshape(-1)[0]), weight)
		ctx.shapes = (gamma.shape, s.shape)
		return torch.full((1, 1), v, dtype=torch.float64)

	@staticmethod
	def backward(ctx, gout):
		sc = float(gout.reshape(-1)[0])
		return None, None, torch.full(ctx.shapes[0], sc * ctx.gg, dtype=torch.float64), torch.full(ctx.shapes[1], sc * ctx.gs, dtype=torch.float64)


class OracleEstimator(Estimator):
	"""log_marginal and log_marginal_batch from the CPU oracle (SE, fixed data): what the restart drivers see of an estimator"""

	def __init__(self):
		self.x, self.y = _data()
		self.s = S0
		self.kernel_object = _Stub()
		self.batch_calls = []
		self.evals = 0

	def ucb(self, x):
		return None

	def lcb(self, x):
		return None

	def fit_gp(self, x, y):
		return None

	def log_marginal(self, kernel, X, weight):
		self.evals += 1
		gamma = torch.as_tensor(X['0']['gamma']).double()
		s = self.s if torch.is_tensor(self.s) else torch.tensor([float(self.s)], dtype=torch.float64)
		return _OracleFn.apply(self, weight, gamma, s.double())

	def log_marginal_batch(self, kernel, Xs, weight, s=None):
		self.lml_batch_path = "device"          # (what a batched evaluator reports)
		self.batch_calls.append(len(Xs))
		vals, grads = [], []
		for b, X in enumerate(Xs):
			gam = torch.as_tensor(X['0']['gamma']).double()
			try:
				v, gg, gs = _oracle(self.x, self.y, float(gam.reshape(-1)[0]), float(self.s if s is None else s[b]), weight)
			except torch.linalg.LinAlgError:
				v, gg, gs = float("inf"), 0.0, 0.0
			vals.append(v)
			g = {'0': {'gamma': torch.full(gam.shape, gg, dtype=torch.float64)}}
			if s is not None:
				g['likelihood'] = {'sigma': torch.tensor([gs], dtype=torch.float64)}
			grads.append(g)
		return torch.tensor(vals, dtype=torch.float64), grads


def _init(k):
	return torch.rand(k).double() * 1.5 + 0.3


def _run(parallel, optimizer, seed=11, params=None, **kw):
	np.random.seed(seed)
	torch.manual_seed(seed)
	est = OracleEstimator()
	params = params or {'0': {'gamma': (_init, Euclidean(1), kw.pop("bounds", None))}}
	assert est.optimize_params_general(params=params, optimizer=optimizer, parallel=parallel, **kw) is True
	return est, (np.random.get_state(), torch.get_rng_state())


def _same_rng(a, b):
	return a[0][0] == b[0][0] and np.array_equal(a[0][1], b[0][1]) and a[0][2:] == b[0][2:] and torch.equal(a[1], b[1])


def test_lockstep_descent_matches_serial():
	ser, rng_s = _run(False, "pymanopt", restarts=4, maxiter=6)
	par, rng_p = _run(True, "pymanopt", restarts=4, maxiter=6)
	ts, tp = ser.optimization_trace, par.optimization_trace
	assert len(tp["params"]) == len(ts["params"]) == 4
	for a, b in zip(tp["params"], ts["params"]):
		assert np.allclose(a, b, rtol=1e-12, atol=0), (a, b)
	assert np.allclose(tp["values"], ts["values"], rtol=1e-12, atol=0)
	assert tp["best"] == ts["best"]
	assert tp["batched"] is True and ts["batched"] is False
	assert par.batch_calls and max(par.batch_calls) == 4 and ser.batch_calls == []          # all restarts in one call, fewer as they finish
	assert par.evals == 0 and ser.evals > 0
	assert float(par.kernel_object.params_dict['0']['gamma']) == float(ser.kernel_object.params_dict['0']['gamma'])
	assert _same_rng(rng_s, rng_p)
	# random starts (no init function): the manifold's random_point() draws, same count and order
	par2, rng_p2 = _run(True, "pymanopt", restarts=3, maxiter=2, params={'0': {'gamma': (None, Euclidean(1), None)}})
	ser2, rng_s2 = _run(False, "pymanopt", restarts=3, maxiter=2, params={'0': {'gamma': (None, Euclidean(1), None)}})
	assert _same_rng(rng_s2, rng_p2)
	for a, b in zip(par2.optimization_trace["params"], ser2.optimization_trace["params"]):
		assert np.allclose(a, b, rtol=1e-12, atol=0)


def test_lockstep_descent_with_noise_and_regularizer():
	"""the noise std as a second variable, a regulariser evaluated per candidate on the host; self.s restored"""
	reg = lambda xt: 0.01 * torch.sum(1.0 / xt)
	mk = lambda: {'0': {'gamma': (_init, Euclidean(1), None)}, 'likelihood': {'sigma': ((lambda k: S0), Euclidean(1), None)}}
	ser, _ = _run(False, "pymanopt", restarts=3, maxiter=4, params=mk(), regularizer_func=reg)
	par, _ = _run(True, "pymanopt", restarts=3, maxiter=4, params=mk(), regularizer_func=reg)
	for a, b in zip(par.optimization_trace["params"], ser.optimization_trace["params"]):
		assert np.allclose(a, b, rtol=1e-12, atol=0), (a, b)
	assert np.allclose(par.optimization_trace["values"], ser.optimization_trace["values"], rtol=1e-12, atol=0)
	assert float(par.s) == float(ser.s)
	# ... and it was the batch method that carried the parallel run: all three restarts in one call, no serial evaluation
	assert par.optimization_trace["batched"] is True and ser.optimization_trace["batched"] is False
	assert par.batch_calls and max(par.batch_calls) == 3 and ser.batch_calls == []
	assert par.evals == 0 and ser.evals > 0


def test_stacked_lbfgs_reaches_stationary_points():
	bounds, mg = [(0.05, 3.0)], 1e-4
	ser, rng_s = _run(False, "pytorch-minimize", restarts=4, bounds=bounds, mingradnorm=mg)
	par, rng_p = _run(True, "pytorch-minimize", restarts=4, bounds=bounds, mingradnorm=mg)
	assert _same_rng(rng_s, rng_p)
	x, y = _data()
	tp, ts = par.optimization_trace, ser.optimization_trace
	assert len(tp["params"]) == 4 and tp["batched"] is True
	for p, v in zip(tp["params"], tp["values"]):
		f, g, _ = _oracle(x, y, p[0], S0, 1.0)
		assert abs(f - v) <= 1e-12 * abs(f)                     # each restart's own value, not the sum
		pg = g                                                  # gradient projected onto the box
		if (p[0] <= bounds[0][0] and g > 0) or (p[0] >= bounds[0][1] and g < 0):
			pg = 0.0
		assert abs(pg) <= mg, (p, g)
	# two mingradnorm-stationary points of one basin differ by at most 2 mg^2 / h in value, h the curvature there
	xb = float(ts["params"][ts["best"]][0])
	e = 1e-4
	h = (_oracle(x, y, xb + e, S0, 1.0)[0] - 2 * _oracle(x, y, xb, S0, 1.0)[0] + _oracle(x, y, xb - e, S0, 1.0)[0]) / e ** 2
	assert h > 0
	margin = 2 * mg ** 2 / h
	print("curvature", h, "margin", margin, "serial best", min(ts["values"]), "parallel best", min(tp["values"]))
	assert min(tp["values"]) <= min(ts["values"]) + margin
	assert max(par.batch_calls) == 4 and par.evals == 0


def test_one_bad_start_does_not_void_the_rest():
	"""a start whose matrix is not positive definite (NaN lengthscale: the oracle's Cholesky fails) is reported inf by the batch method;
	the lockstep driver drops it, finishes the others and picks the best of the rest"""
	def mk():
		count = [0]

		def init(k):
			count[0] += 1
			v = _init(k)
			return v * float("nan") if count[0] == 2 else v
		return {'0': {'gamma': (init, Euclidean(1), None)}}
	par, _ = _run(True, "pymanopt", restarts=4, maxiter=5, params=mk())
	ser, _ = _run(False, "pymanopt", restarts=4, maxiter=5, params=mk())
	tp, ts = par.optimization_trace, ser.optimization_trace
	assert np.isinf(tp["values"][1]) and tp["best"] != 1 and np.isfinite(tp["values"][tp["best"]])
	keep = [0, 2, 3]
	assert np.allclose([tp["values"][i] for i in keep], [ts["values"][i] for i in keep], rtol=1e-12, atol=0)
	assert tp["best"] == ts["best"] == int(np.argmin([tp["values"][i] if i in keep else np.inf for i in range(4)]))
	assert par.batch_calls[0] == 4 and par.batch_calls[1] == 3          # the bad start is gone after the first round
	assert float(par.s) == S0


def test_serial_batch_method_of_the_base_class():
	"""Estimator.log_marginal_batch: the candidates one after another through log_marginal + autograd, same structure"""
	est = OracleEstimator()
	x, y = _data()
	Xs = [{'0': {'gamma': torch.tensor([g], dtype=torch.float64)}} for g in (0.4, 0.9, float("nan"))]
	vals, grads = Estimator.log_marginal_batch(est, est.kernel_object, Xs, 0.5, s=[0.1, 0.2, 0.1])
	assert est.lml_batch_path == "serial" and est.s == S0 and tuple(vals.shape) == (3,)
	for b, (g, s) in enumerate(((0.4, 0.1), (0.9, 0.2))):
		f, gg, gs = _oracle(x, y, g, s, 0.5)
		assert float(vals[b]) == f and float(grads[b]['0']['gamma']) == gg and float(grads[b]['likelihood']['sigma']) == gs
		assert tuple(grads[b]['0']['gamma'].shape) == (1,)
	assert np.isinf(float(vals[2])) and float(grads[2]['0']['gamma']) == 0.0 and float(grads[2]['likelihood']['sigma']) == 0.0
	vals, grads = Estimator.log_marginal_batch(est, est.kernel_object, Xs[:2], 1.0)
	assert 'likelihood' not in grads[0] and float(vals[0]) == _oracle(x, y, 0.4, S0, 1.0)[0]
