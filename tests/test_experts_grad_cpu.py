"""
Input gradients of the local experts, the parts that need no GPU: the NumPy oracle (tests/experts_grad_oracle.py) against central differences of
tests/experts_oracle.py and against its own restatement in extended precision, the distance of the GPU tests' cases from the combination's clamp,
the host side of LocalExpertsGaussianProcess.mean_std_grad / ucb_optimize with the device out of reach, the argument checks of the two new C entry
points (every refusal comes before the first HIP call, so placeholder pointers are safe), and the resource usage of the new kernels.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import experts_grad_oracle as GO
from tests import experts_oracle as XO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stpy_amd", "csrc")
MODES = (XO.POE, XO.GPOE, XO.BCM, XO.RBCM)


def _rel(got, want):
	want = np.asarray(want, dtype=np.float64)
	return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want))) / float(np.max(np.abs(want)))


# --------------------------------------------------------------------------------------------- 1. the oracle against central differences
@pytest.mark.parametrize("kind", XO.KINDS)
def test_oracle_is_the_central_difference(kind):
	"""h = 1e-5: truncation h^2 f''' / 6 near 1e-10 f''' and rounding eps |f| / h near 1e-11 |f|, both inside the 1e-6 of the largest gradient
	entry asked for.  The 45 free test points of the reference case: none coincides with a training point (Matern 1/2 has its kink there)."""
	r = XO.reference_case()
	kappa, il, h = r["kappa"], r["inv_ls"], 1e-5
	xt = r["xt"][XO.REF["M_train"]:]
	assert not any(np.any(np.all(r["xs"] == t, axis=1)) for t in xt)
	M, d = xt.shape
	orc = XO.experts(kind, r["xs"], r["ys"], r["sizes"], il, r["s"], kappa, xt=xt)
	assert XO.n_clamped(orc["var_e"], kappa) == 0
	gmu_e, gvar_e = GO.experts_grad(kind, r["xs"], orc, il, kappa, xt)
	# every test point moved by +h and -h along every axis: one oracle prediction of 2 M d points
	moved = np.repeat(xt[None, :, :], 2 * d, axis=0)
	for m in range(d):
		moved[2 * m, :, m] += h
		moved[2 * m + 1, :, m] -= h
	o2 = XO.experts(kind, r["xs"], r["ys"], r["sizes"], il, r["s"], kappa, xt=moved.reshape(-1, d))
	E = len(r["sizes"])
	mu2, var2 = o2["mu_e"].reshape(E, 2 * d, M), o2["var_e"].reshape(E, 2 * d, M)
	assert XO.n_clamped(o2["var_e"], kappa) == 0
	fd = lambda a: np.stack([(a[..., 2 * m, :] - a[..., 2 * m + 1, :]) / (2 * h) for m in range(d)], axis=-1)
	err = dict(gmu_e=_rel(gmu_e, fd(mu2)), gvar_e=_rel(gvar_e, fd(var2)))
	for mode in MODES:
		mu, var, dmu, dstd = GO.combine_grad(mode, orc["mu_e"], orc["var_e"], gmu_e, gvar_e, kappa)
		m0, v0 = XO.combine(mode, orc["mu_e"], orc["var_e"], kappa)
		assert np.array_equal(mu, m0) and np.array_equal(var, v0)
		c = [XO.combine(mode, mu2[:, j], var2[:, j], kappa) for j in range(2 * d)]
		err["dmu mode %d" % mode] = _rel(dmu, fd(np.array([a for a, _ in c])))
		err["dstd mode %d" % mode] = _rel(dstd, fd(np.sqrt(np.array([b for _, b in c]))))
	print("kind", kind, err)
	assert all(v <= 1e-6 for v in err.values()), err


# --------------------------------------------------------------------------------------------- 2. float64 against extended precision
def _against_extended(kind, xs, ys, sizes, il, s, kappa, xt):
	"""largest error of the float64 oracle against the extended one, each relative to the largest entry of the array: per-expert gradients and the
	combined ones under the four modes"""
	orc = XO.experts(kind, xs, ys, sizes, il, s, kappa, xt=xt)
	assert XO.n_clamped(orc["var_e"], kappa) == 0
	gmu_e, gvar_e = GO.experts_grad(kind, xs, orc, il, kappa, xt)
	off = orc["offsets"]
	x = [GO.expert_grad_extended(kind, xs[off[e]:off[e + 1]], ys[off[e]:off[e + 1]], il, s, kappa, xt) for e in range(len(sizes))]
	gmu_x, gvar_x = np.array([f["gmu"] for f in x]), np.array([f["gvar"] for f in x])
	mu_x, var_x = np.array([f["mu"] for f in x]), np.array([f["var"] for f in x])
	relx = lambda a, b: float(np.max(np.abs(np.asarray(a - b, dtype=np.float64))) / np.max(np.abs(np.asarray(b, dtype=np.float64))))          # (the difference is taken in the extended type)
	err = dict(gmu_e=relx(gmu_e, gmu_x), gvar_e=relx(gvar_e, gvar_x))
	for mode in MODES:
		_, _, dmu, dstd = GO.combine_grad(mode, orc["mu_e"], orc["var_e"], gmu_e, gvar_e, kappa)
		_, _, dmu_x, dstd_x = GO.combine_grad(mode, mu_x, var_x, gmu_x, gvar_x, kappa, extended=True)
		err["dmu mode %d" % mode], err["dstd mode %d" % mode] = relx(dmu, dmu_x), relx(dstd, dstd_x)
	return err


@pytest.mark.parametrize("kind", XO.KINDS)
def test_reference_case_oracle_against_extended_precision(kind):
	"""all 65 test points, the 20 training points among them (Matern 1/2: the zero convention on both sides): 1e-10, two orders inside the GPU
	tests' 1e-8"""
	r = XO.reference_case()
	err = _against_extended(kind, r["xs"], r["ys"], r["sizes"], r["inv_ls"], r["s"], r["kappa"], r["xt"])
	print("kind", kind, err)
	assert all(v <= 1e-10 for v in err.values()), err


@pytest.mark.parametrize("kind", XO.KINDS)
def test_border_case_oracle_against_extended_precision(kind):
	"""the mixed-size case (experts of 1 .. 512 points), all 97 test points (27 training points, the far one): the solves with K_e^-1 that the
	variance gradient adds are as well conditioned as those of the prediction (cond(K_e) <= 2e4 on this case)"""
	c = XO.border_case()
	err = _against_extended(kind, c["xs"], c["ys"], c["sizes"], c["inv_ls"], c["s"], c["kappa"], c["xt"])
	print("kind", kind, err)
	assert all(v <= 1e-10 for v in err.values()), err


# --------------------------------------------------------------------------------------------- 3. the clamp
def test_gpu_cases_stay_clear_of_the_clamp():
	"""no expert variance is clamped on the cases whose combined gradients the GPU tests compare with this oracle: the reference case, the border
	case (all 97 test points, the far one included: var_e == kappa there is the tie on which the clamp is inactive); the class-level GPU tests
	assert the same of their own case"""
	r, c = XO.reference_case(), XO.border_case()
	for kind in XO.KINDS:
		o = XO.experts(kind, r["xs"], r["ys"], r["sizes"], r["inv_ls"], r["s"], r["kappa"], xt=r["xt"])
		assert XO.n_clamped(o["var_e"], r["kappa"]) == 0 and o["var_e"].min() > 1e-3 * r["kappa"]
		o = XO.experts(kind, c["xs"], c["ys"], c["sizes"], c["inv_ls"], c["s"], c["kappa"], xt=c["xt"])
		assert XO.n_clamped(o["var_e"], c["kappa"]) == 0 and o["var_e"].min() > 1e-3 * c["kappa"]


def test_clamp_rule_of_the_oracle():
	"""dv = 0 where the clamp is active, gvar_e on the ties; an active clamp leaves the expert's mean gradient in play"""
	kappa = 1.3
	var_e = np.array([[0.0, -1.0, kappa, 2 * kappa, 0.4, kappa * 2.0 ** -52, kappa * 2.0 ** -53]])
	mu_e = np.full((1, 7), 0.7)
	gmu_e, gvar_e = np.full((1, 7, 2), 0.3), np.full((1, 7, 2), -0.2)
	for mode in MODES:
		mu, var, dmu, dstd = GO.combine_grad(mode, mu_e, var_e, gmu_e, gvar_e, kappa)
		m0, v0 = XO.combine(mode, mu_e, var_e, kappa)
		assert np.array_equal(mu, m0) and np.array_equal(var, v0)
		assert np.all(dstd[[0, 1, 3, 6]] == 0.0) and np.all(dstd[[4, 5]] != 0.0)
		assert np.all(np.isfinite(dmu)) and np.all(np.isfinite(dstd))
	# PoE with one expert is the expert: d std = gvar / (2 sqrt(var)), d mu = gmu
	_, _, dmu, dstd = GO.combine_grad(XO.POE, mu_e, var_e, gmu_e, gvar_e, kappa)
	assert np.allclose(dmu[4], 0.3, rtol=1e-14, atol=0) and np.allclose(dstd[4], -0.2 / (2 * np.sqrt(0.4)), rtol=1e-14, atol=0)
	assert np.allclose(dstd[2], -0.2 / (2 * np.sqrt(kappa)), rtol=1e-14, atol=0)          # (the tie at kappa: inactive)


def test_synthetic_combine_case_is_well_conditioned():
	"""the case of the GPU test of stpy_experts_combine_grad: every way past the clamp is in it, and the float64 oracle agrees with the extended one
	to 1e-13 ENTRY BY ENTRY (zeros exactly), a tenth of what the GPU test asks of the device"""
	c = GO.synthetic_combine_case()
	S, kappa, ve = GO.SYNTH, GO.SYNTH["kappa"], c["var_e"]
	assert ve.shape == (S["E"], S["M"]) and c["gvar_e"].shape == (S["E"], S["M"], S["d"]) == (5, 50, 3)
	assert np.any((ve > 0) & (ve < kappa * 2.0 ** -52)) and np.any(ve < 0) and np.any(ve == 0) and np.any(ve == kappa) and np.any(ve > kappa)
	assert XO.n_clamped(ve, kappa) == 21 and not np.any(ve == kappa * 2.0 ** -52)
	worst = 0.0
	for mode in MODES:
		a = GO.combine_grad(mode, c["mu_e"], ve, c["gmu_e"], c["gvar_e"], kappa)
		b = GO.combine_grad(mode, c["mu_e"], ve, c["gmu_e"], c["gvar_e"], kappa, extended=True)
		m0, v0 = XO.combine(mode, c["mu_e"], ve, kappa)
		assert np.array_equal(a[0], m0) and np.array_equal(a[1], v0)
		for x, y in zip(a, b):
			y64, dif = np.asarray(y, dtype=np.float64), np.abs(np.asarray(x - y, dtype=np.float64))
			assert np.all(np.isfinite(x)) and np.all(x[y64 == 0] == 0)
			worst = max(worst, float(np.max(dif[y64 != 0] / np.abs(y64[y64 != 0]))))
	print("synthetic combine case: worst entrywise error of the float64 oracle", worst)
	assert worst <= 1e-13


# --------------------------------------------------------------------------------------------- 4. host behaviour without the device
@pytest.fixture
def no_device(monkeypatch):
	from stpy_amd import _lib

	def boom(*a, **k):
		raise AssertionError("the device was touched")
	for name in ("device", "to_device", "load"):
		monkeypatch.setattr(_lib, name, boom)
	return _lib


def test_gradient_surface_without_the_device(no_device):
	import stpy_amd
	bounds = [(0.0, 1.0), (-1.0, 2.0), (3.0, 4.0)]
	gp = stpy_amd.LocalExpertsGaussianProcess(gamma=0.4, s=0.1, kappa=1.3, d=3, expert_size=34, bounds=bounds)
	assert gp.bounds == bounds and stpy_amd.LocalExpertsGaussianProcess(d=3).bounds is None
	import inspect
	assert list(inspect.signature(stpy_amd.LocalExpertsGaussianProcess.__init__).parameters)[-1] == "bounds"
	x = torch.rand(40, 3).double()
	dmu, dstd = gp.mean_std_grad(x)          # unfitted: the prior is flat
	assert tuple(dmu.shape) == tuple(dstd.shape) == (40, 3) and torch.all(dmu == 0) and torch.all(dstd == 0)
	dmu, dstd = gp.mean_std_grad(x.clone().requires_grad_(True))          # (the contract of GaussianProcess.mean_std_grad: the tensor is detached)
	assert tuple(dmu.shape) == (40, 3) and not dmu.requires_grad
	with pytest.raises(NotImplementedError, match="fit"):          # not fitted comes before the bounds
		gp.ucb_optimize(2.0)
	with pytest.raises(NotImplementedError, match="fit"):
		stpy_amd.LocalExpertsGaussianProcess(d=3).ucb_optimize(2.0, multistart=3, lcb=True)
	with pytest.raises(NotImplementedError, match="requires_grad") as info:
		gp.mean_std(x.clone().requires_grad_(True))
	assert "mean_std_grad" in str(info.value)
	with pytest.raises(AttributeError):
		gp.expert_mean_var_grad(x)
	# a fitted object's bounds are checked on the host: none, or the wrong number of them
	gp.fitted = True
	gp.bounds = None
	with pytest.raises(ValueError, match="bounds"):
		gp.ucb_optimize(2.0)
	gp.bounds = bounds[:2]
	with pytest.raises(ValueError, match="bounds"):
		gp.ucb_optimize(2.0)
	# the gradient path's chunk rule: E * chunk * (2 + 2 d) elements under the budget; the prediction's rule is untouched
	from stpy_amd.continuous_processes import local_experts as LE
	gp._sizes = np.full(1000, 34)
	step = LE.PREDICT_BUDGET // (1000 * 8)
	assert gp._grad_chunks(300, 3) == [(a, min(a + step, 300)) for a in range(0, 300, step)] and step == 131
	assert gp._chunks(300) == [(0, 300)]
	gp.max_size = 7
	assert gp._grad_chunks(15, 3) == [(0, 7), (7, 14), (14, 15)]


# --------------------------------------------------------------------------------------------- 5. argument checks of the C ABI
def test_gradient_argument_checks():
	from stpy_amd import _lib as L
	lib = L.load()
	P, N = ctypes.c_void_p(0x1000), None          # a non-null, 16-byte aligned pointer no refused call may dereference
	Q = ctypes.c_void_p(0x1004)                    # ... and a misaligned one
	big = 1 << 50

	def predict(kind=0, dtype=0, xs=P, n=100, ldx=4, d=4, cols=N, offsets=P, E=3, nmax=64, inv_ls=P, kappa=1.0, factor=P, fbytes=big, alpha=P, info=P,
				xt=P, M=70, ldt=4, mu_e=P, var_e=P, ldm=70, gmu_e=P, gvar_e=P, ldg=4, lde=280, work=P, wbytes=big):
		return lib.stpy_experts_predict_grad(kind, dtype, xs, n, ldx, d, cols, offsets, E, nmax, inv_ls, kappa, factor, fbytes, alpha, info, xt, M, ldt,
											 mu_e, var_e, ldm, gmu_e, gvar_e, ldg, lde, work, wbytes, N)

	def combine(mode=3, E=3, M=70, d=4, mu_e=P, var_e=P, ldm=70, gmu_e=P, gvar_e=P, ldg=4, lde=280, kappa=1.0, mu=P, var=P, dmu=P, dstd=P, ldo=4):
		return lib.stpy_experts_combine_grad(mode, E, M, d, mu_e, var_e, ldm, gmu_e, gvar_e, ldg, lde, kappa, mu, var, dmu, dstd, ldo, N)

	wgrad, wpred, fb = lib.stpy_experts_predict_grad_workspace_bytes(0, 64, 4, 3, 70), lib.stpy_experts_predict_workspace_bytes(0, 64, 4, 3, 70), lib.stpy_experts_factor_bytes(0, 64, 3)
	assert wgrad == 2 * wpred == 2 * 3 * 3 * 32 * 64 * 8          # two slices of 32 NPM doubles per expert and tile
	assert lib.stpy_experts_predict_grad_workspace_bytes(1, 64, 4, 3, 70) == 0 and lib.stpy_experts_predict_grad_workspace_bytes(0, 513, 4, 3, 70) == 0
	refused = [
		(predict, "stpy_experts_predict_grad", {
			"unknown kind": (dict(kind=9), -1), "LINEAR": (dict(kind=4), -1), "fp32": (dict(dtype=1), -2), "nmax above the cap": (dict(nmax=513), -4),
			"ldx < d": (dict(ldx=3), -5), "ldt < d": (dict(ldt=3), -5), "d < 1": (dict(d=0), -6), "E out of range": (dict(E=1 << 31), -9),
			"negative M": (dict(M=-1), -9), "kappa 0": (dict(kappa=0.0), -11), "kappa nan": (dict(kappa=float("nan")), -11), "ldm < M": (dict(ldm=69), -13),
			"ldg < d": (dict(ldg=3), -19), "lde < M ldg": (dict(lde=279), -19), "small workspace": (dict(wbytes=wgrad - 1), -20),
			"the prediction's workspace": (dict(wbytes=wpred), -20), "small factor": (dict(fbytes=fb - 1), -22),
			"misaligned work": (dict(work=Q), -21), "misaligned factor": (dict(factor=Q), -21), "misaligned xt": (dict(xt=Q), -21),
			"misaligned gmu_e": (dict(gmu_e=Q), -21), "misaligned gvar_e": (dict(gvar_e=Q), -21),
			**{"null " + k: ({k: N}, -3) for k in ("xs", "offsets", "inv_ls", "factor", "alpha", "info", "xt", "mu_e", "var_e", "gmu_e", "gvar_e", "work")}}),
		(combine, "stpy_experts_combine_grad", {
			"mode 4": (dict(mode=4), -10), "mode -1": (dict(mode=-1), -10), "negative E": (dict(E=-1), -9), "d < 1": (dict(d=0), -6),
			"ldm < M": (dict(ldm=69), -13), "ldg < d": (dict(ldg=3), -19), "lde < M ldg": (dict(lde=279), -19), "ldo < d": (dict(ldo=3), -19),
			"kappa 0": (dict(kappa=0.0), -11), "kappa inf": (dict(kappa=float("inf")), -11), "misaligned dstd": (dict(dstd=Q), -21),
			"misaligned gvar_e": (dict(gvar_e=Q), -21),
			**{"null " + k: ({k: N}, -3) for k in ("mu_e", "var_e", "gmu_e", "gvar_e", "mu", "var", "dmu", "dstd")}})]
	for call, name, cases in refused:
		for what, (kw, code) in cases.items():
			lib.stpy_lml_batch(0, 1, N, 1, 1, 1, N, N, 1, N, 1, N, 1.0, 1.0, N, 1, N, N, 2, N, N, 0, N)          # (leaves some OTHER message behind)
			before = lib.stpy_last_error_string()
			rc = call(**kw)
			assert rc == code, (name, what, rc)
			msg = lib.stpy_last_error_string()
			assert msg and name.encode() in msg and msg != before, (name, what, msg)
	# the empty problems: 0 without looking at a pointer
	assert predict(E=0, xs=N, work=N) == 0 and predict(M=0, xt=N, gmu_e=N) == 0 and predict(n=0, xs=N) == 0
	assert combine(E=0, mu_e=N) == 0 and combine(M=0, dmu=N) == 0


# --------------------------------------------------------------------------------------------- 6. kernel resources
def test_gradient_kernel_resources(tmp_path):
	"""experts_predict_grad_kernel keeps two waves per SIMD and uses no more scratch than experts_predict_kernel in the same compile (none); the
	combination's gradient kernel has no scratch either"""
	out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-comment", "-c", os.path.join(CSRC, "experts.hip"),
						  "-o", str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True).stderr
	blocks = {b.split()[0]: b for b in re.split(r"remark: Function Name: ", out)[1:]}
	find = lambda key: next(b for name, b in blocks.items() if key in name)
	num = lambda b, what: int(re.search(re.escape(what) + r": (\d+)", b).group(1))
	grad, pred, comb = find("experts_predict_grad_kernel"), find("experts_predict_kernel"), find("experts_combine_grad_kernel")
	print({k: (num(b, "VGPRs"), num(b, "ScratchSize [bytes/lane]"), num(b, "Occupancy [waves/SIMD]"), num(b, "LDS Size [bytes/block]"))
		   for k, b in (("predict_grad", grad), ("predict", pred), ("combine_grad", comb))})
	assert num(grad, "Occupancy [waves/SIMD]") >= 2
	assert num(grad, "ScratchSize [bytes/lane]") <= num(pred, "ScratchSize [bytes/lane]")
	assert num(comb, "ScratchSize [bytes/lane]") == 0 and num(comb, "Occupancy [waves/SIMD]") >= 2
