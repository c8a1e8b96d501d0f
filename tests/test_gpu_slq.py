"""
The stochastic evidence on the device: stpy_pcg_lanczos against stpy_pcg and against the dense quadrature of tests/slq_oracle.py, and
IterativeGaussianProcess.log_marginal_estimate / optimize_params_estimate against the oracle's estimate on the same probes.

Tolerances of the estimate (float64; the class solves to tol = 1e-8, the reference is the oracle solved to 1e-12; delta = 2 tol is the TRUE
relative residual the device's solve may leave, as in tests/test_gpu_pcg.py), derived as kmv_oracle.posterior_bounds derives its own:
  y^T alpha     alpha~ = alpha + A^-1 e, |e| <= delta |y|:  |y^T (alpha~ - alpha)| = |alpha^T e| <= |alpha| delta |y|;
  q_c           the Gauss quadrature of 1 / (x + tau) errs by r(tau)^T (B + tau)^-1 r(tau) with |r(tau)| <= |r(0)| for the shifted solves, and
                log x = int_0^inf [1 / (1 + tau) - 1 / (x + tau)] dtau, so |q_c - dense| <= |r|^2 log(cond B) (1 + o(1)) <= delta^2 |z_c|^2 log(cond B):
                1e-12 here, far below what the recurrence's rounding leaves.  The tolerance is the one stated for the coefficients themselves,
                1e-6 max|q|; an indexing error moves q by O(|q|);
  a_c = u_c^T dA v_c   u~ = u + A^-1 e, |e| <= delta |z_c|:  |a~_c - a_c| <= delta |z_c| |A^-1 dA v_c|;  alpha^T dA alpha: 2 delta |y| |A^-1 dA alpha|;
  tr~ = mean(a) + beta (E b - mean b), beta = cov(a, b) / var(b):  |d beta| <= sqrt(t / (t - 1)) max|da| / sd(b), so
                |d tr~| <= max_c |da_c| (1 + sqrt(t / (t - 1)) |E b - mean b| / sd(b));
  everything else (the factor, the probes, the derivative sums) differs by rounding, eps x cond(A) ~ 1e-10 relative: 1e-9 |reference| is added.
"""
import numpy as np
import pytest
import torch

from tests import kmv_oracle as KO
from tests import slq_oracle as SO
from tests.test_gpu_pcg import Solver
from tests.test_slq_cpu import T_PROBES, f32_deviation, grid_minimum

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
CASES = (0, 3, 4)
IDS = [KO.PCG_IDS[i] for i in CASES]


class LanczosSolver(Solver):
	"""tests/test_gpu_pcg.Solver through stpy_pcg_lanczos: the same operands, plus coef (t, cap, 2) prefilled with a sentinel, and rz0."""

	def __init__(self, *a, cap=64, **kw):
		super().__init__(*a, **kw)
		t = self.Bt.shape[0]
		self.coef = torch.full((t, cap, 2), SENTINEL, dtype=torch.float64, device=self.x.device)
		self.rz0 = torch.full((t,), SENTINEL, dtype=torch.float64, device=self.x.device)

	def run(self, iters):
		self.L.pcg_lanczos(self.kind, self.x, self.inv_ls, self.Bt, self.Xt, self.work, self.out, self.coef, self.rz0, cols=self.cols, kappa=1.0,
						   diag_add=self.diag_add, Gt=self.Gt, Gn=self.Gn, tol=self.tol, iters=iters, init=not self.started)
		self.started = True
		torch.cuda.synchronize()
		return self

	def get(self):
		return dict(super().get(), coef=self.coef.cpu().numpy(), rz0=self.rz0.cpu().numpy())


def _solvers(idx, dtype_name, **kw):
	kind, n, d, gamma, r, cols = KO.PCG_CASES[idx]
	o = KO.oracle_run(idx, dtype_name)
	args = (kind, o["x"], gamma, o["B64"], dtype_name, o["s"] ** 2)
	return args, dict(G=o["G"], cols=cols, tol=o["tol"], **kw)


# --------------------------------------------------------------------------------------------- stpy_pcg_lanczos
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("idx", [0, 2], ids=[KO.PCG_IDS[0], KO.PCG_IDS[2]])
def test_pcg_lanczos_solves_with_the_bits_of_pcg_and_leaves_unused_slots(idx, dtype_name):
	args, kw = _solvers(idx, dtype_name)
	a = Solver(*args, **kw).solve().get()
	b = LanczosSolver(*args, cap=1000, **kw).solve().get()
	for k in ("X", "relres", "bx", "its"):
		assert np.array_equal(a[k], b[k]), k
	for c, m in enumerate(b["its"]):
		assert m > 0
		assert np.all(b["coef"][c, m:] == SENTINEL)                       # slots at and beyond its[c]
		assert b["coef"][c, m - 1, 1] == SENTINEL                         # the column converged on iteration m: no ratio after it
		assert np.all(b["coef"][c, :m, 0] > 0) and np.all(b["coef"][c, :m - 1, 1] > 0)
	assert np.all(b["rz0"] > 0)


def test_pcg_lanczos_zero_column_and_cap():
	"""A zero column writes nothing at all; iterations beyond cap write nothing (and nothing out of bounds: the next column's slots stay)."""
	kind, n, d, gamma, r, cols = KO.PCG_CASES[3]
	o = KO.oracle_run(3, "float64")
	B = np.stack([o["B64"][:, 0], np.zeros(n), o["B64"][:, 1]], axis=1)
	s = LanczosSolver(kind, o["x"], gamma, B, "float64", o["s"] ** 2, tol=0.0, cap=4).run(9).get()
	assert list(s["its"]) == [9, 0, 9]
	assert np.all(s["coef"][1] == SENTINEL) and s["rz0"][1] == SENTINEL
	assert np.all(s["coef"][[0, 2]] != SENTINEL)


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_pcg_lanczos_blocks_give_the_coefficients_of_one_long_call(dtype_name):
	args, kw = _solvers(5, dtype_name)
	kw["tol"] = 0.0                                                       # nothing freezes: 50 iterations everywhere
	one = LanczosSolver(*args, cap=50, **kw).run(50).get()
	s = LanczosSolver(*args, cap=50, pad=3, **kw)
	for _ in range(5):
		s.run(10)
	five = s.get()
	for k in ("X", "relres", "bx", "its", "coef", "rz0"):
		assert np.array_equal(one[k], five[k]), k
	assert np.all(one["its"] == 50) and np.all(one["coef"] != SENTINEL)


@pytest.mark.parametrize("idx", CASES, ids=IDS)
def test_quadrature_from_device_coefficients(idx):
	"""q_c from the device's coefficients of the oracle's probes (the oracle's G) against the dense form, float64: 1e-6 relative to max|q|."""
	e, (kind, x, y, gamma, s, r, cols, W, tol) = SO.case_estimate(idx, T_PROBES)
	got = LanczosSolver(kind, x, gamma, e["Z"], "float64", s * s, G=e["G"], cols=cols, tol=tol, cap=300).solve().get()
	assert np.all(got["its"] > 0) and np.all(got["relres"] <= tol)
	q = SO.q_from_coef(got["coef"], got["its"], got["rz0"], s)
	qd = SO.q_dense(e["A"], e["G"], e["Z"], s)
	rel = np.abs(q - qd).max() / np.abs(qd).max()
	print("%s: device q against the dense form %.2e (relative to max|q|), iterations %d" % (KO.PCG_IDS[idx], rel, got["its"].max()))
	assert rel <= 1e-6


# --------------------------------------------------------------------------------------------- log_marginal_estimate
ARD = dict(kind="se", n=400, d=3, gamma=np.array([0.3, 0.5, 0.8]), r=40, seed=4242)


def _problem(name):
	"""(kind, x, y, gamma, r, cols) of PCG case ``name`` or of the ARD case."""
	if name == "ard":
		rng = np.random.RandomState(ARD["seed"])
		x = rng.uniform(-1, 1, size=(ARD["n"], ARD["d"]))
		y = (np.sin(3.0 * x @ rng.uniform(-1, 1, size=(3,))) + 0.1 * rng.standard_normal(ARD["n"])).reshape(-1, 1)
		return ARD["kind"], x, y, ARD["gamma"], ARD["r"], None
	kind, n, d, gamma, r, cols = KO.PCG_CASES[name]
	x, y, _ = KO.case_data(name)
	return kind, x, y, gamma, r, cols


def _gp(kind, d, gamma, s, r, **kw):
	from stpy_amd import IterativeGaussianProcess, KernelFunction
	if np.ndim(gamma) > 0:
		return IterativeGaussianProcess(kernel=KernelFunction(kernel_name="ard", ard_gamma=torch.from_numpy(np.asarray(gamma)), d=d), s=s, precond_rank=r, **kw)
	return IterativeGaussianProcess(kernel_name="squared_exponential", gamma=gamma, s=s, d=d, precond_rank=r, **kw)


_REF = {}


def _reference(name):
	"""The oracle's estimate solved to 1e-12 on probes from RandomState(100 + case), and the tolerances of the module docstring."""
	if name not in _REF:
		kind, x, y, gamma, r, cols = _problem(name)
		s, tol = KO.SETTINGS["float64"]
		n, t = x.shape[0], T_PROBES
		W = SO.probes(n, r, t, 100 + (7 if name == "ard" else name))
		e = SO.estimate(kind, x, y, gamma, s, r, W, 1e-12, cols=cols)
		delta = 2 * tol
		A, alpha, ynorm = e["A"], e["alpha"], np.linalg.norm(y)
		znorm = np.linalg.norm(e["Z"], axis=0)
		crowd = np.sqrt(t / (t - 1.0))
		tol_q = 1e-6 * np.abs(e["q"]).max()
		tol_val = 0.5 * np.linalg.norm(alpha) * delta * ynorm + 0.5 * tol_q + 1e-9 * abs(e["value"])

		def tol_trace(D, a_ref, b, Eb):
			da = max(delta * znorm[c] * np.linalg.norm(np.linalg.solve(A, D @ e["V"][:, c])) for c in range(t))
			return da * (1 + crowd * abs(Eb - b.mean()) / b.std(ddof=1))
		G = e["G"]
		tol_g = []
		for D in e["dK"]:
			b = np.array([e["V"][:, c] @ D @ e["V"][:, c] for c in range(t)]) / (s * s)
			tt = tol_trace(D, None, b, -np.sum(G * (D @ G)) / (s * s))
			tol_g.append(0.5 * 2 * delta * ynorm * np.linalg.norm(np.linalg.solve(A, D @ alpha)) + 0.5 * tt)
		bs = 2 * s * np.sum(e["V"] * e["V"], axis=0) / (s * s)
		tol_s = 0.5 * 2 * delta * ynorm * np.linalg.norm(np.linalg.solve(A, 2 * s * alpha)) + 0.5 * tol_trace(2 * s * np.eye(n), None, bs, 2 * s * (n - np.sum(G * G)) / (s * s))
		gam = np.ones(len(e["dK"])) * gamma if np.ndim(gamma) else np.array([gamma])
		g_ref = e["grad_loggamma"] / gam
		_REF[name] = dict(e=e, W=W, s=s, tol_q=tol_q, tol_val=tol_val, g_ref=g_ref, tol_g=np.array(tol_g) / gam + 1e-9 * np.abs(g_ref),
						  tol_s=tol_s + 1e-9 * abs(e["grad_s"]), problem=(kind, x, y, gamma, r, cols))
	return _REF[name]


def _device_estimate(name, dtype=torch.float64, s=None, W=None):
	ref = _reference(name) if dtype == torch.float64 else None
	kind, x, y, gamma, r, cols = _problem(name)
	if dtype == torch.float32:
		x, y, _ = KO.case_data(name, np.float32)                          # the float32-rounded problem the oracle's float32 run solves
	s = ref["s"] if s is None else s
	gp = _gp(kind, x.shape[1], gamma, torch.tensor([s], dtype=torch.float64, requires_grad=True), r)
	gp.x, gp.y = torch.from_numpy(x).to(dtype), torch.from_numpy(y).to(dtype)
	pname = "ard_gamma" if np.ndim(gamma) else "gamma"
	g = torch.tensor(np.ones(1) * gamma if not np.ndim(gamma) else gamma, dtype=torch.float64, requires_grad=True)
	f = gp.log_marginal_estimate(gp.kernel_object, {"0": {pname: g}}, 1.0, probes=torch.from_numpy(ref["W"] if W is None else W))
	f.backward()
	return gp, f, g.grad.numpy().copy(), float(gp.s.grad.reshape(-1)[0])


@pytest.mark.parametrize("name", [0, 3, "ard"], ids=[KO.PCG_IDS[0], KO.PCG_IDS[3], "se-ard-n400"])
def test_estimate_against_the_oracle_on_the_same_probes(name):
	ref = _reference(name)
	e = ref["e"]
	gp, f, g, gs = _device_estimate(name)
	info = gp.evidence_info
	assert set(info) >= {"value", "stderr", "logdet", "logdet_stderr", "grad_stderr", "probes", "iterations", "rank", "kmv_launches"}
	assert tuple(f.shape) == (1, 1) and not f.is_cuda and float(f.detach()) == info["value"]
	assert info["rank"] == e["rank"] and info["probes"] == T_PROBES and info["kmv_launches"] >= info["iterations"] + 1
	print("%s: |value - oracle| %.2e (tol %.2e), q %.2e (%.2e), d/dgamma %s (%s), d/ds %.2e (%.2e); stderr %.3f / %.3f" % (
		name, abs(info["value"] - e["value"]), ref["tol_val"], np.abs(info["q"] - e["q"]).max(), ref["tol_q"], np.abs(g - ref["g_ref"]), ref["tol_g"],
		abs(gs - e["grad_s"]), ref["tol_s"], info["stderr"], e["stderr"]))
	assert np.all(np.abs(info["q"] - e["q"]) <= ref["tol_q"])
	assert abs(info["logdet"] - e["logdet"]) <= ref["tol_q"] + 1e-9 * abs(e["logdet"])
	assert abs(info["value"] - e["value"]) <= ref["tol_val"]
	assert np.all(np.abs(g - ref["g_ref"]) <= ref["tol_g"])
	assert abs(gs - e["grad_s"]) <= ref["tol_s"]
	# the reported standard errors are those of the same samples
	assert abs(info["stderr"] - e["stderr"]) <= 1e-6 * e["stderr"] + ref["tol_q"]
	gam = np.ones(len(g)) * ref["problem"][3]
	assert np.allclose(info["grad_stderr"]["ard_gamma" if name == "ard" else "gamma"], e["grad_loggamma_stderr"] / gam, rtol=1e-4)
	assert np.allclose(info["grad_stderr"]["sigma"], e["grad_s_stderr"], rtol=1e-4)


def test_estimate_float32_against_the_float64_oracle():
	"""Case 4 in float32 (s = 0.3, tol = 1e-4) against the float64 oracle solved to 1e-8: at most 10x what the oracle's own float32 restatement
	deviates (slq_oracle.F32_RESTATEMENT_DEVIATION)."""
	dev, e64 = f32_deviation()
	kind, n, d, gamma, r, cols = KO.PCG_CASES[4]
	s, _ = KO.SETTINGS["float32"]
	gp, f, g, gs = _device_estimate(4, dtype=torch.float32, s=s, W=SO.probes(n, r, T_PROBES, 104))
	assert f.dtype == torch.float32
	got = (abs(gp.evidence_info["value"] - e64["value"]) / abs(e64["value"]), abs(g[0] * gamma - e64["grad_loggamma"][0]) / abs(e64["grad_loggamma"][0]),
		   abs(gs - e64["grad_s"]) / abs(e64["grad_s"]))
	print("float32 device against the float64 oracle: value %.3e, d/dgamma %.3e, d/ds %.3e; the oracle's own float32: %.3e, %.3e, %.3e" % (got + dev))
	for a, const in zip(got, SO.F32_RESTATEMENT_DEVIATION):
		assert a <= 10 * const


def test_estimate_leaves_the_fit_alone_and_repeats_its_bits():
	kind, x, y, gamma, r, cols = _problem(4)
	xt, yt = torch.from_numpy(x), torch.from_numpy(y)
	gp = _gp(kind, 2, gamma, 0.1, r, num_probes=6, probe_seed=5)
	gp.fit_gp(xt, yt)
	mu = gp.mean(xt[:7]).clone()
	before = (gp._alpha.clone(), gp._Gt.clone(), gp._Gn.clone(), dict(gp.cg_info), mu)
	a = gp.log_marginal_estimate()
	b = gp.log_marginal_estimate(gp.kernel_object, {"0": {"gamma": torch.tensor([0.3], dtype=torch.float64)}}, 1.0)
	c = gp.log_marginal_estimate()
	assert gp.evidence_info["probes"] == 6 and gp.evidence_info["grad_stderr"] is None
	assert float(a) == float(c) and float(a) != float(b)                  # the same seed, the same bits; another gamma, another value
	other = _gp(kind, 2, gamma, 0.1, r, num_probes=6, probe_seed=5)
	other.x, other.y = xt, yt                                             # data without a fit is enough
	assert float(other.log_marginal_estimate()) == float(a) and other.fitted is False
	assert torch.equal(gp._alpha, before[0]) and torch.equal(gp._Gt, before[1]) and torch.equal(gp._Gn, before[2]) and gp.cg_info == before[3]
	assert torch.equal(gp.mean(xt[:7]), before[4]) and gp.fitted and gp.cg_info["kmv_launches"] == before[3]["kmv_launches"] + 1
	with pytest.raises(NotImplementedError, match="Lanczos"):
		gp.log_marginal(gp.kernel_object, {}, 1.0)


def test_optimize_params_estimate_meets_the_oracle_runs_criterion():
	"""Case 3 from gamma = 0.5 with 16 probes: the end point's exact dense objective is below the start's and not above the exact objective's
	minimum over the grid of tests/test_slq_cpu.py by more than 4 standard errors of the estimate there."""
	kind, x, y, gamma, r, cols = _problem(3)
	s, _ = KO.SETTINGS["float64"]
	gp = _gp(kind, 1, 0.5, s, r, num_probes=T_PROBES, probe_seed=3)
	xt, yt = torch.from_numpy(x), torch.from_numpy(y)
	gp.fit_gp(xt, yt)
	assert gp.optimize_params_estimate(type="bandwidth", restarts=1, optimizer="pytorch-minimize", init_func=lambda k: torch.tensor([0.5]), bounds=[(0.01, 1.0)]) is True
	g_end = float(torch.as_tensor(gp.kernel_object.params_dict["0"]["gamma"]).reshape(-1)[0])
	gp.log_marginal_estimate()
	stderr = gp.evidence_info["stderr"]
	f_end, f_start, f_grid = SO.exact(kind, x, y, g_end, s)["value"], SO.exact(kind, x, y, 0.5, s)["value"], grid_minimum()
	print("device run: gamma %.5f, exact objective %.6f (start %.6f, grid minimum %.6f), stderr there %.2e" % (g_end, f_end, f_start, f_grid, stderr))
	assert gp.fitted and 0.01 <= g_end <= 1.0
	assert f_end < f_start
	assert f_end <= f_grid + 4 * stderr
