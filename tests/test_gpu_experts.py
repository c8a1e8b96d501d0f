"""
Local GP experts on the device: stpy_experts_fit / _predict / _combine against the NumPy oracle (tests/experts_oracle.py), the properties the
class relies on (an expert's outputs do not depend on the batch around it; a failing expert is reported and leaves the others alone), and
LocalExpertsGaussianProcess against the dense class where the two coincide (one expert, PoE).

Tolerance 1e-8, as in the rest of the C-ABI suite: relative to kappa for variances, to max |mu| for means, to the largest entry for alpha and the
gradient rows.  tests/test_experts_cpu.py shows that on the reference case no expert variance comes near the clamp (min var_e / kappa > 1e-3) and
the float64 oracle itself is five orders inside the tolerance.

The second half runs the kernels where their index arithmetic changes: XO.border_case() puts experts of 1, 31 .. 33, 63 .. 65, 96, 97, 128, 129, 200,
511 and 512 points into ONE batch under nmax = 512 (one block, one round of 64 rows and its border, half a last round, the cap; every expert but
the last with a row stride NP_e below NPM), fits it with every kind and a gradient and predicts at M = 97 .. 1; one variant passes wide rows with
cols, a strided xt and strided outputs.  Then the promises of the header as properties -- predictions independent of position, batch and nmax;
the last of 300 experts as the expert alone; info = -1 / -2 and an empty expert between untouched neighbours -- and the class against the oracle:
three partitions (an explicit one with sizes 512, 0, 97, 1, 90), the four combinations, A, chunked expert_mean_var, ARD on a column group, the
summed evidence with its gradient, log_marginal_batch.  The oracle on that case is within 1e-10 of an extended-precision restatement
(tests/test_experts_cpu.py), nothing is clamped on it, and the border tests print the worst device error per group of quantities.
"""
import numpy as np
import pytest
import torch

from tests import experts_oracle as XO

pytestmark = pytest.mark.gpu

TOL = 1e-8


@pytest.fixture(scope="module")
def S(gpu_device):
	import stpy_amd
	return stpy_amd


@pytest.fixture(scope="module")
def ref():
	return XO.reference_case()


def _dev(a, dev, dtype=None):
	return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype=dtype))).to(dev)


def _fit(dev, kind, xs, ys, sizes, inv_ls, s, kappa, weight=1.0, pidx=None, n_params=0, cols=None, nmax=None, offsets=None):
	"""one stpy_experts_fit call through the typed wrapper; NumPy results plus the device buffers a prediction needs.  xs: a NumPy array or a device
	tensor (which may be a strided view); offsets: the int32 array to pass in place of the running sums of sizes (sizes[e] must still be expert
	e's row count where it is valid: _V reads it)"""
	from stpy_amd import _lib as L
	E, N = len(sizes), xs.shape[0]
	nmax = int(max(sizes)) if nmax is None else nmax
	st = dict(xs=xs if torch.is_tensor(xs) else _dev(xs, dev), ys=_dev(ys, dev), nmax=nmax,
			  offsets=_dev(np.concatenate([[0], np.cumsum(sizes)]) if offsets is None else offsets, dev, np.int32),
			  inv_ls=_dev(inv_ls, dev), cols=None if cols is None else _dev(cols, dev, np.int32), kind=kind, kappa=kappa, sizes=list(sizes))
	st["factor"] = L.experts_factor(nmax, E, st["xs"])
	st["alpha"] = torch.full((N,), float("nan"), dtype=torch.float64, device=dev)
	value, grad, total, info, _ = L.experts_fit(kind, st["xs"], st["ys"], st["offsets"], nmax, st["inv_ls"], _dev(np.array([s]), dev), kappa, weight,
												st["factor"], st["alpha"], pidx=None if pidx is None else _dev(pidx, dev, np.int32), n_params=n_params, cols=st["cols"])
	torch.cuda.synchronize()
	st["info"] = info
	st.update(value_h=value.cpu().numpy(), grad_h=None if grad is None else grad.cpu().numpy(), total_h=total.cpu().numpy(), info_h=info.cpu().numpy(),
			  alpha_h=st["alpha"].cpu().numpy(), factor_h=st["factor"].cpu().numpy().view(np.float64))
	return st


def _V(st, e):
	n, npm = st["sizes"][e], -(-st["nmax"] // 32) * 32
	NP = -(-n // 32) * 32
	# (upper triangular; only the block diagonal and the blocks just below it are written below the diagonal, as zeros)
	return np.triu(st["factor_h"][e * npm * npm:e * npm * npm + NP * NP].reshape(NP, NP)[:n, :n])


def _predict(dev, st, xt, modes=(0, 1, 2, 3), pad=0):
	"""one stpy_experts_predict call and one stpy_experts_combine call per mode.  xt: a NumPy array or a device tensor (which may be a strided
	view); pad > 0: mu_e / var_e are the [:, :M] views of NaN-filled (E, M + pad) buffers, and the padding is checked to be NaN still"""
	from stpy_amd import _lib as L
	E, M = len(st["sizes"]), xt.shape[0]
	xt_d = xt if torch.is_tensor(xt) else _dev(xt, dev)
	mu_full = torch.full((E, M + pad), float("nan"), dtype=torch.float64, device=dev)
	var_full = torch.full((E, M + pad), float("nan"), dtype=torch.float64, device=dev)
	mu_e, var_e = mu_full[:, :M], var_full[:, :M]
	L.experts_predict(st["kind"], st["xs"], st["offsets"], st["nmax"], st["inv_ls"], st["kappa"], st["factor"], st["alpha"], st["info"], xt_d, mu_e, var_e, cols=st["cols"])
	out = {}
	for mode in modes:
		mu = torch.full((M,), float("nan"), dtype=torch.float64, device=dev)
		var = torch.full((M,), float("nan"), dtype=torch.float64, device=dev)
		L.experts_combine(mode, mu_e, var_e, st["kappa"], mu, var)
		out[mode] = (mu.cpu().numpy(), var.cpu().numpy())
	torch.cuda.synchronize()
	assert bool(torch.isnan(mu_full[:, M:]).all()) and bool(torch.isnan(var_full[:, M:]).all())
	return mu_e.cpu().numpy(), var_e.cpu().numpy(), out


WORST = {}          # the largest error seen per group of quantities, for the summaries the border tests print


def _close(got, want, scale=None, tol=TOL, what="", group=None):
	scale = float(np.max(np.abs(want))) if scale is None else scale
	err = float(np.max(np.abs(np.asarray(got) - np.asarray(want)))) / (scale if scale > 0 else 1.0)
	print(what, "error", err)
	if group is not None:
		WORST[group] = max(WORST.get(group, 0.0), err)
	assert err <= tol, (what, err)


def _check_fit(st, orc, kappa, with_grad, what, worst=False):
	"""worst: also record the errors in WORST, by group"""
	g = (lambda name: name) if worst else (lambda name: None)
	assert not st["info_h"].any(), st["info_h"]
	_close(st["alpha_h"], orc["alpha"], what=what + " alpha", group=g("alpha"))
	_close(st["value_h"], orc["value"], what=what + " value", group=g("value"))
	_close(st["total_h"][:1], orc["total"][:1], what=what + " total value", group=g("value"))
	if with_grad:
		for e in range(len(st["sizes"])):
			_close(st["grad_h"][e], orc["grad"][e], what=what + " grad of expert %d" % e, group=g("gradient"))
		_close(st["total_h"], orc["total"], scale=float(np.max(np.abs(orc["total"][1:]))), what=what + " total", group=g("gradient"))
	for e, f in enumerate(orc["fits"]):
		V = _V(st, e)          # L^-T, upper triangular: V V^T = K_e^-1
		_close(V @ V.T @ f["K"], np.eye(V.shape[0]), scale=1.0, what=what + " V V^T K of expert %d" % e, group=g("V V^T K - I"))


BORDER_SIZES = [1, 31, 32, 33, 64, 65]


@pytest.mark.parametrize("kind", ["se", "matern12", "matern32", "matern52", "ard"])
def test_fit_against_oracle(S, gpu_device, ref, kind):
	ard = kind == "ard"
	k = XO.SE if ard else {"se": 0, "matern12": 1, "matern32": 2, "matern52": 3}[kind]
	d = XO.REF["d"]
	if ard:          # a lengthscale and a slot per coordinate, the coordinates picked out of wider rows by cols
		cols = [3, 0, 2]
		inv_ls, pidx, npar = 1.0 / np.array([0.4, 0.7, 0.3]), [0, 1, 2], 3
		widen = lambda x: np.concatenate([x[:, 1:2], 7.0 + x[:, :1], x[:, 2:3], x[:, :1], -x[:, :1]], axis=1)
	else:
		cols, inv_ls, pidx, npar = None, ref["inv_ls"], [0] * d, 1
		widen = lambda x: x
	xs = widen(ref["xs"])          # (ard: column 3 = x0, column 0 = x1, column 2 = x2)
	weight = 0.5 if ard else 1.0
	st = _fit(gpu_device, k, xs, ref["ys"], ref["sizes"], inv_ls, ref["s"], ref["kappa"], weight, pidx, npar, cols)
	orc = XO.experts(k, xs, ref["ys"], ref["sizes"], inv_ls, ref["s"], ref["kappa"], weight, pidx, npar, cols)
	_check_fit(st, orc, ref["kappa"], True, kind + " reference")
	# the same without a gradient: the same bits for what both write
	st0 = _fit(gpu_device, k, xs, ref["ys"], ref["sizes"], inv_ls, ref["s"], ref["kappa"], weight, None, 0, cols)
	assert st0["grad_h"] is None and st0["total_h"].shape == (1,)
	for key in ("alpha_h", "value_h", "info_h"):
		assert np.array_equal(st0[key], st[key]), key
	assert all(np.array_equal(_V(st0, e), _V(st, e)) for e in range(len(ref["sizes"])))
	assert st0["total_h"][0] == st["total_h"][0]
	# the 32-block border and the one-point expert, in one call
	n = sum(BORDER_SIZES)
	rng = np.random.RandomState(11)
	xb = widen(rng.uniform(0, 1, size=(n, d)) + 1.5)
	yb = np.sin(3 * xb[:, 0]) + 0.1 * rng.normal(size=n)
	stb = _fit(gpu_device, k, xb, yb, BORDER_SIZES, inv_ls, ref["s"], ref["kappa"], weight, pidx, npar, cols)
	orb = XO.experts(k, xb, yb, BORDER_SIZES, inv_ls, ref["s"], ref["kappa"], weight, pidx, npar, cols)
	_check_fit(stb, orb, ref["kappa"], True, kind + " border sizes")


def test_position_independence(S, gpu_device):
	rng = np.random.RandomState(3)
	d = 4
	blocks = {name: (rng.uniform(-1, 1, size=(n, d)), rng.normal(size=n)) for name, n in (("A", 70), ("B", 33), ("C", 128))}
	inv_ls, pidx = 1.0 / np.array([0.5, 0.8, 0.4, 1.1]), [0, 1, 2, 3]

	def run(names):
		xs, ys = np.concatenate([blocks[k][0] for k in names]), np.concatenate([blocks[k][1] for k in names])
		sizes = [blocks[k][0].shape[0] for k in names]
		st = _fit(gpu_device, XO.MATERN52, xs, ys, sizes, inv_ls, 0.2, 1.1, 0.7, pidx, 4, nmax=128)
		off = np.concatenate([[0], np.cumsum(sizes)])
		return {k: (st["alpha_h"][off[i]:off[i + 1]], st["value_h"][i], st["grad_h"][i], _V(st, i)) for i, k in enumerate(names)}, st

	abc, st1 = run("ABC")
	ca, _ = run("CA")
	for k in "AC":
		for a, b in zip(abc[k], ca[k]):
			assert np.array_equal(a, b), k
	_, st2 = run("ABC")
	for key in ("alpha_h", "value_h", "grad_h", "total_h"):
		assert np.array_equal(st1[key], st2[key]), key
	assert all(np.array_equal(_V(st1, e), _V(st2, e)) for e in range(3))


def test_one_expert_is_the_dense_gp(S, gpu_device):
	from stpy_amd import _lib as L
	n, d, s, kappa, ls = 200, 3, 0.15, 1.3, 0.6
	rng = np.random.RandomState(7)
	x = rng.uniform(-1, 1, size=(n, d))
	y = np.sin(3 * x[:, 0]) + 0.5 * np.cos(2 * x[:, 2]) + 0.1 * rng.normal(size=n)
	inv_ls = np.full(d, 1.0 / ls)
	st = _fit(gpu_device, XO.SE, x, y, [n], inv_ls, s, kappa, 1.0, [0] * d, 1)
	value, grad, info, _ = L.lml_batch(XO.SE, st["xs"], st["ys"], _dev(inv_ls.reshape(1, d), gpu_device), _dev(np.array([s]), gpu_device),
									   _dev([0] * d, gpu_device, np.int32), 1, kappa, 1.0)
	# (the two kernels are shells around ONE body, lb_fit of csrc/lb_block.h: the same bits)
	assert np.array_equal(st["value_h"], value.cpu().numpy()), (st["value_h"], value.cpu().numpy())
	assert np.array_equal(st["grad_h"], grad.cpu().numpy()), (st["grad_h"], grad.cpu().numpy())
	assert int(info.cpu()[0]) == 0
	# ... and on a second 64-row round, the remainder of the four-wide lengthscale pass, a slot per coordinate and a weight
	n2, d2, rng2 = 97, 5, np.random.RandomState(8)
	x2 = rng2.uniform(-1, 1, size=(n2, d2))
	y2 = np.sin(3 * x2[:, 0]) + 0.5 * np.cos(2 * x2[:, 4]) + 0.1 * rng2.normal(size=n2)
	inv_ls2 = 1.0 / rng2.uniform(0.5, 0.9, size=d2)
	st2 = _fit(gpu_device, XO.MATERN52, x2, y2, [n2], inv_ls2, s, kappa, 0.7, list(range(d2)), d2)
	value2, grad2, info2, _ = L.lml_batch(XO.MATERN52, st2["xs"], st2["ys"], _dev(inv_ls2.reshape(1, d2), gpu_device), _dev(np.array([s]), gpu_device),
										  _dev(list(range(d2)), gpu_device, np.int32), d2, kappa, 0.7)
	assert int(info2.cpu()[0]) == 0 and not st2["info_h"].any()
	assert np.all(np.isfinite(st2["grad_h"])) and np.all(st2["grad_h"] != 0.0)
	assert np.array_equal(st2["value_h"], value2.cpu().numpy()), (st2["value_h"], value2.cpu().numpy())
	assert np.array_equal(st2["grad_h"], grad2.cpu().numpy()), (st2["grad_h"], grad2.cpu().numpy())
	# the class: one expert under PoE is the exact GP
	xt = rng.uniform(-1.2, 1.2, size=(37, d))
	xT, yT, xtT = torch.from_numpy(x), torch.from_numpy(y).reshape(-1, 1), torch.from_numpy(xt)
	le = S.LocalExpertsGaussianProcess(gamma=ls, s=s, kappa=kappa, d=d, expert_size=n, combine="poe")
	le.fit_gp(xT, yT)
	gp = S.GaussianProcess(gamma=ls, s=s, kappa=kappa, d=d)
	gp.fit_gp(xT, yT)
	assert le.experts_info["E"] == 1 and le.experts_info["sizes"] == [n]
	mu, sd = le.mean_std(xtT)
	mu0, sd0 = gp.mean_std(xtT)
	_close(mu.numpy(), mu0.numpy(), what="mean against GaussianProcess")
	_close(sd.numpy() ** 2, sd0.numpy() ** 2, scale=kappa, what="variance against GaussianProcess")
	# evidence and its gradients (value 1e-8, gradient 1e-7: the tolerances of the dense class's own gradient tests)
	for est in (le, gp):
		est.s = torch.tensor([s], dtype=torch.float64, requires_grad=True)
	res = []
	for est in (le, gp):
		g = torch.tensor([ls], dtype=torch.float64, requires_grad=True)
		f = est.log_marginal(est.kernel_object, {'0': {'gamma': g, 'kappa': kappa, 'group': list(range(d))}}, 0.8)
		assert tuple(f.shape) == (1, 1)
		f.backward()
		res.append((float(f.detach()), float(g.grad), float(est.s.grad)))
		est.s.grad = None
	print("evidence", res)
	assert abs(res[0][0] - res[1][0]) <= 1e-8 * abs(res[1][0])
	assert abs(res[0][1] - res[1][1]) <= 1e-7 * abs(res[1][1]) and abs(res[0][2] - res[1][2]) <= 1e-7 * abs(res[1][2])


@pytest.mark.parametrize("kind", [XO.SE, XO.MATERN12, XO.MATERN32, XO.MATERN52])
def test_predict_and_combine_against_oracle(S, gpu_device, ref, kind):
	xs, ys = ref["xs"].copy(), ref["ys"].copy()
	if kind == XO.MATERN12:          # a duplicated training point inside expert 1 (r = 0 exactly: the kernel's kink)
		xs[ref["sizes"][0] + 5] = xs[ref["sizes"][0] + 2]
	st = _fit(gpu_device, kind, xs, ys, ref["sizes"], ref["inv_ls"], ref["s"], ref["kappa"])
	xt_all = ref["xt"].copy()
	xt_all[:XO.REF["M_train"]] = xs[[int(np.argmin(np.sum((ref["xs"] - t) ** 2, axis=1))) for t in ref["xt"][:XO.REF["M_train"]]]]
	if kind == XO.MATERN12:
		xt_all[XO.REF["M_train"]] = xs[ref["sizes"][0] + 5]          # ... and a test point on it
	orc = XO.experts(kind, xs, ys, ref["sizes"], ref["inv_ls"], ref["s"], ref["kappa"], xt=xt_all)
	assert XO.n_clamped(orc["var_e"], ref["kappa"]) == 0
	full = None
	for M in (65, 63, 1):
		mu_e, var_e, comb = _predict(gpu_device, st, xt_all[:M])
		_close(mu_e, orc["mu_e"][:, :M], scale=float(np.max(np.abs(orc["mu_e"]))), what="mu_e M=%d" % M)
		_close(var_e, orc["var_e"][:, :M], scale=ref["kappa"], what="var_e M=%d" % M)
		for mode in range(4):
			mu, var = XO.combine(mode, orc["mu_e"][:, :M], orc["var_e"][:, :M], ref["kappa"])
			_close(comb[mode][0], mu, scale=float(np.max(np.abs(orc["mu_e"]))), what="mode %d mean M=%d" % (mode, M))
			_close(comb[mode][1], var, scale=ref["kappa"], what="mode %d variance M=%d" % (mode, M))
		if full is None:
			full = (mu_e, var_e)
		else:          # a test point's result does not depend on the tile it sits in
			assert np.array_equal(mu_e, full[0][:, :M]) and np.array_equal(var_e, full[1][:, :M])
	# the combination's clamp on the device: variances outside [kappa 2^-52, kappa]
	from stpy_amd import _lib as L
	ve = np.array([[0.0, 1e-300, 2.0 * ref["kappa"], 0.3], [0.5, 0.2, -1.0, ref["kappa"]]])
	me = np.array([[1.0, -2.0, 0.5, 0.1], [0.3, 0.4, -0.7, 2.0]])
	for mode in range(4):
		mu = torch.empty(4, dtype=torch.float64, device=gpu_device)
		var = torch.empty(4, dtype=torch.float64, device=gpu_device)
		L.experts_combine(mode, _dev(me, gpu_device), _dev(ve, gpu_device), ref["kappa"], mu, var)
		m0, v0 = XO.combine(mode, me, ve, ref["kappa"])
		assert np.allclose(mu.cpu().numpy(), m0, rtol=1e-12, atol=0) and np.allclose(var.cpu().numpy(), v0, rtol=1e-12, atol=0), mode
		assert np.all(np.isfinite(var.cpu().numpy())) and (mode < 2 or np.all(var.cpu().numpy() <= ref["kappa"] * (1 + 1e-12)))


def test_failing_expert(S, gpu_device, ref):
	sizes = [40, 20, 33]
	rng = np.random.RandomState(2)
	xs = rng.uniform(0, 1, size=(sum(sizes), 3))
	ys = rng.normal(size=sum(sizes))
	# expert 1: its first two points coincide, no noise, kappa = 1: the second pivot is fma(-1, 1, 1) = 0 exactly, whatever the rounding elsewhere
	xs[40 + 1] = xs[40 + 0]
	bad = _fit(gpu_device, XO.SE, xs, ys, sizes, ref["inv_ls"], 0.0, 1.0, 1.0, [0, 0, 0], 1)
	keep = np.r_[0:40, 60:93]
	good = _fit(gpu_device, XO.SE, xs[keep], ys[keep], [40, 33], ref["inv_ls"], 0.0, 1.0, 1.0, [0, 0, 0], 1, nmax=40)
	assert bad["info_h"].tolist() == [0, 2, 0], bad["info_h"]
	assert np.isinf(bad["value_h"][1]) and bad["value_h"][1] > 0 and np.all(bad["grad_h"][1] == 0.0) and np.all(bad["alpha_h"][40:60] == 0.0)
	assert np.isinf(bad["total_h"][0])
	for e_bad, e_good, rows_bad, rows_good in ((0, 0, slice(0, 40), slice(0, 40)), (2, 1, slice(60, 93), slice(40, 73))):
		assert bad["value_h"][e_bad] == good["value_h"][e_good] and np.array_equal(bad["grad_h"][e_bad], good["grad_h"][e_good])
		assert np.array_equal(bad["alpha_h"][rows_bad], good["alpha_h"][rows_good]) and np.array_equal(_V(bad, e_bad), _V(good, e_good))
	# its prediction is the prior; the others predict as without it
	xt = rng.uniform(0, 1, size=(5, 3))
	mu_b, var_b, _ = _predict(gpu_device, bad, xt, modes=())
	mu_g, var_g, _ = _predict(gpu_device, good, xt, modes=())
	assert np.all(mu_b[1] == 0.0) and np.all(var_b[1] == 1.0)
	assert np.array_equal(mu_b[[0, 2]], mu_g) and np.array_equal(var_b[[0, 2]], var_g)
	# the class names the expert and stays unfitted
	ids = torch.from_numpy(np.repeat([0, 1, 2], sizes))
	le = S.LocalExpertsGaussianProcess(gamma=0.4, s=0.0, d=3, partition=ids)
	with pytest.raises(torch.linalg.LinAlgError, match="expert 1"):
		le.fit_gp(torch.from_numpy(xs), torch.from_numpy(ys).reshape(-1, 1))
	assert le.fitted is False


def test_class_level(S, gpu_device):
	n, d = 300, 2
	rng = np.random.RandomState(4)
	x = torch.from_numpy(rng.uniform(-1, 1, size=(n, d)))
	y = torch.sin(3 * x[:, :1]) * torch.cos(2 * x[:, 1:2]) + 0.1 * torch.from_numpy(rng.normal(size=(n, 1)))
	xt = torch.from_numpy(rng.uniform(-1, 1, size=(50, d)))
	le = S.LocalExpertsGaussianProcess(gamma=0.7, s=0.2, d=d, expert_size=64)
	le.fit_gp(x, y)
	info = le.experts_info
	assert info["E"] == 5 and info["sizes"] == [60] * 5 and info["launches"] == 2 and info["factor_bytes"] == 5 * 64 * 64 * 8
	mu, sd = le.mean_std(xt)
	assert tuple(mu.shape) == tuple(sd.shape) == (50, 1) and not mu.is_cuda
	le.max_size = 16          # four chunks: the bits of one
	mu2, sd2 = le.mean_std(xt)
	assert torch.equal(mu, mu2) and torch.equal(sd, sd2)
	mu_e, var_e = le.expert_mean_var(xt)
	assert tuple(mu_e.shape) == tuple(var_e.shape) == (5, 50)
	m0, v0 = XO.combine(XO.RBCM, mu_e.numpy(), var_e.numpy(), 1.0)
	assert np.allclose(mu.numpy().ravel(), m0, rtol=1e-12, atol=1e-14) and np.allclose(sd.numpy().ravel() ** 2, v0, rtol=1e-12, atol=0)
	with pytest.raises(NotImplementedError):
		le.mean_std(xt.clone().requires_grad_(True))
	start = float(le.log_marginal(le.kernel_object, {}, 1.0))
	np.random.seed(0)
	torch.manual_seed(0)
	assert le.optimize_params(type="bandwidth+noise", restarts=2, maxiter=20) is True
	assert le.fitted is True
	end = float(le.log_marginal(le.kernel_object, {}, 1.0))
	print("factorised evidence", start, "->", end, "gamma", le.kernel_object.params_dict['0']['gamma'], "s", le.s)
	assert end <= start
	mu3, sd3 = le.mean_std(xt)
	assert torch.all(torch.isfinite(mu3)) and torch.all(sd3 > 0)


# --------------------------------------------------------------------------------------------- every block size up to the cap, in one batch
# XO.border_case(): experts of 1, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 200, 511 and 512 points under nmax = 512, so that all but the last have a
# row stride NP_e below NPM; tests/test_experts_cpu.py holds the float64 oracle to 1e-10 of an extended-precision restatement on it.
_BORDER = {}


def _border(dev, kind):
	"""the case, its oracle (weight 0.7, a slot per coordinate, the 97 test points) and its device fit with a gradient: once per kind, read only"""
	if kind not in _BORDER:
		c, d = XO.border_case(), XO.BORDER["d"]
		orc = XO.experts(kind, c["xs"], c["ys"], c["sizes"], c["inv_ls"], c["s"], c["kappa"], 0.7, list(range(d)), d, xt=c["xt"])
		st = _fit(dev, kind, c["xs"], c["ys"], c["sizes"], c["inv_ls"], c["s"], c["kappa"], 0.7, list(range(d)), d)
		_BORDER[kind] = (c, orc, st)
	return _BORDER[kind]


def _same_fit(a, b, experts_a, experts_b, rows_a, rows_b, grad=True):
	"""experts experts_a of fit a and experts_b of fit b (their alpha rows: rows_a, rows_b) carry the same bits"""
	for ea, eb, ra, rb in zip(experts_a, experts_b, rows_a, rows_b):
		assert a["value_h"][ea] == b["value_h"][eb] and a["info_h"][ea] == b["info_h"][eb] == 0, (ea, eb)
		assert np.array_equal(a["alpha_h"][ra], b["alpha_h"][rb]) and np.array_equal(_V(a, ea), _V(b, eb)), (ea, eb)
		assert not grad or np.array_equal(a["grad_h"][ea], b["grad_h"][eb]), (ea, eb)


@pytest.mark.parametrize("kind", XO.KINDS)
def test_border_fit_against_oracle(S, gpu_device, kind):
	c, orc, st = _border(gpu_device, kind)
	assert st["nmax"] == 512 and st["grad_h"].shape == (14, 6)
	WORST.clear()
	_check_fit(st, orc, c["kappa"], True, "kind %d border case" % kind, worst=True)
	print("worst fit errors, kind %d:" % kind, dict(WORST))
	# the same without a gradient: the same bits for what both write
	st0 = _fit(gpu_device, kind, c["xs"], c["ys"], c["sizes"], c["inv_ls"], c["s"], c["kappa"], 0.7)
	assert st0["grad_h"] is None and st0["total_h"].shape == (1,) and st0["total_h"][0] == st["total_h"][0]
	off = c["offsets"]
	rows = [slice(off[e], off[e + 1]) for e in range(14)]
	_same_fit(st0, st, range(14), range(14), rows, rows, grad=False)


@pytest.mark.parametrize("kind", XO.KINDS)
def test_border_predict_against_oracle(S, gpu_device, kind):
	c, orc, st = _border(gpu_device, kind)
	kappa = c["kappa"]
	assert XO.n_clamped(orc["var_e"], kappa) == 0
	mscale = float(np.max(np.abs(orc["mu_e"])))
	WORST.clear()
	full = None
	for M in (97, 65, 64, 33, 32, 31, 1):
		mu_e, var_e, comb = _predict(gpu_device, st, c["xt"][:M])
		_close(mu_e, orc["mu_e"][:, :M], scale=mscale, what="mu_e M=%d" % M, group="mu_e")
		_close(var_e, orc["var_e"][:, :M], scale=kappa, what="var_e M=%d" % M, group="var_e")
		for mode in range(4):
			mu, var = XO.combine(mode, orc["mu_e"][:, :M], orc["var_e"][:, :M], kappa)
			_close(comb[mode][0], mu, scale=mscale, what="mode %d mean M=%d" % (mode, M), group="combined")
			_close(comb[mode][1], var, scale=kappa, what="mode %d variance M=%d" % (mode, M), group="combined")
		if full is None:
			full = (mu_e, var_e, comb)
		else:          # a test point's bits do not depend on M
			assert np.array_equal(mu_e, full[0][:, :M]) and np.array_equal(var_e, full[1][:, :M])
			assert all(np.array_equal(comb[mode][i], full[2][mode][i][:M]) for mode in range(4) for i in range(2))
	print("worst prediction errors, kind %d:" % kind, dict(WORST))
	# the last test point is 40 units from the data along every axis: every expert returns the prior
	assert np.all(np.abs(full[0][:, -1]) < 1e-30) and np.all(full[1][:, -1] == kappa)


def test_border_layout_variant(S, gpu_device):
	"""xs and xt as rows of width 8 of which cols picks (and permutes) five, NaN in the others; xt a row- and column-sliced view of a wider buffer
	(ldt = 11); mu_e / var_e views of wider buffers (ldm = M + 5): the bits of the dense layout, and nothing written beside the views"""
	kind = XO.MATERN52
	c, orc, st = _border(gpu_device, kind)
	d, cols = XO.BORDER["d"], [6, 1, 4, 0, 3]

	def wide(a):
		out = np.full((a.shape[0], 8), np.nan)
		out[:, cols] = a
		return out
	stw = _fit(gpu_device, kind, wide(c["xs"]), c["ys"], c["sizes"], c["inv_ls"], c["s"], c["kappa"], 0.7, list(range(d)), d, cols=cols)
	assert stw["xs"].stride(0) == 8 and np.array_equal(stw["total_h"], st["total_h"])
	off = c["offsets"]
	rows = [slice(off[e], off[e + 1]) for e in range(14)]
	_same_fit(stw, st, range(14), range(14), rows, rows)
	for M in (97, 33, 1):
		buf = torch.full((M + 3, 11), float("nan"), dtype=torch.float64, device=gpu_device)
		xt = buf[2:2 + M, 1:9]
		xt.copy_(_dev(wide(c["xt"][:M]), gpu_device))
		assert xt.stride(0) == 11
		mu_w, var_w, comb_w = _predict(gpu_device, stw, xt, pad=5)
		mu_d, var_d, comb_d = _predict(gpu_device, st, c["xt"][:M])
		assert np.array_equal(mu_w, mu_d) and np.array_equal(var_w, var_d) and not np.isnan(mu_w).any() and not np.isnan(var_w).any()
		assert all(np.array_equal(comb_w[mode][i], comb_d[mode][i]) for mode in range(4) for i in range(2))
		_close(mu_w, orc["mu_e"][:, :M], scale=float(np.max(np.abs(orc["mu_e"]))), what="wide layout mu_e M=%d" % M)
		_close(var_w, orc["var_e"][:, :M], scale=c["kappa"], what="wide layout var_e M=%d" % M)


# --------------------------------------------------------------------------------------------- the header's promises
def test_predict_position_and_slice_independence(S, gpu_device):
	"""an expert's predictions carry the same bits wherever it sits in whatever batch, whatever nmax sizes the slices, and in a repeated call"""
	rng = np.random.RandomState(13)
	d, kind = 4, XO.MATERN32
	blocks = {name: (rng.uniform(-1, 1, size=(n, d)), rng.normal(size=n)) for name, n in (("A", 70), ("B", 33), ("C", 128), ("D", 512))}
	inv_ls = 1.0 / np.array([0.5, 0.8, 0.4, 1.1])
	xt = np.concatenate([blocks["A"][0][[0, 69]], blocks["C"][0][[0, 127]], rng.uniform(-1.2, 1.2, size=(40, d))])

	def run(names, nmax):
		xs, ys = np.concatenate([blocks[k][0] for k in names]), np.concatenate([blocks[k][1] for k in names])
		sizes = [blocks[k][0].shape[0] for k in names]
		st = _fit(gpu_device, kind, xs, ys, sizes, inv_ls, 0.2, 1.1, nmax=nmax)
		assert not st["info_h"].any()
		mu_e, var_e, _ = _predict(gpu_device, st, xt, modes=())
		mu_2, var_2, _ = _predict(gpu_device, st, xt, modes=())
		assert np.array_equal(mu_e, mu_2) and np.array_equal(var_e, var_2) and np.all(np.isfinite(mu_e)) and np.all(var_e > 0)
		off = np.concatenate([[0], np.cumsum(sizes)])
		return {k: (mu_e[i], var_e[i], st["alpha_h"][off[i]:off[i + 1]], st["value_h"][i], _V(st, i)) for i, k in enumerate(names)}

	abc, ca, adc = run("ABC", 128), run("CA", 128), run("ADC", 512)
	for k in "AC":
		for other in (ca, adc):
			for a, b in zip(abc[k], other[k]):
				assert np.array_equal(a, b), k
	# ... and they are the right ones
	for k in "ACD":
		f = XO.expert_fit(kind, blocks[k][0], blocks[k][1], inv_ls, 0.2, 1.1)
		mu, var = XO.expert_predict(kind, blocks[k][0], f, inv_ls, 1.1, xt)
		_close(adc[k][0], mu, what="block %s mean" % k)
		_close(adc[k][1], var, scale=1.1, what="block %s variance" % k)


def test_last_of_300_experts_is_the_expert_alone(S, gpu_device):
	"""E = 300 experts of 33 points and two tiles of test points (300 fit workgroups, 600 prediction workgroups, more than the CUs of the device):
	the last expert's factor, alpha and predictions are the bits of the same expert fitted and predicted alone"""
	E, n, d, M = 300, 33, 3, 33
	rng = np.random.RandomState(19)
	xs, ys = rng.uniform(0, 1, size=(E * n, d)), rng.normal(size=E * n)
	xt = np.concatenate([xs[[(E - 1) * n, E * n - 1, 0]], rng.uniform(0, 1, size=(M - 3, d))])
	inv_ls = np.full(d, 2.5)
	st = _fit(gpu_device, XO.SE, xs, ys, [n] * E, inv_ls, 0.1, 1.3)
	one = _fit(gpu_device, XO.SE, xs[(E - 1) * n:], ys[(E - 1) * n:], [n], inv_ls, 0.1, 1.3)
	assert not st["info_h"].any() and not one["info_h"].any()
	_same_fit(st, one, [E - 1], [0], [slice((E - 1) * n, E * n)], [slice(0, n)], grad=False)
	mu_e, var_e, _ = _predict(gpu_device, st, xt, modes=())
	mu_1, var_1, _ = _predict(gpu_device, one, xt, modes=())
	assert np.array_equal(mu_e[E - 1], mu_1[0]) and np.array_equal(var_e[E - 1], var_1[0])
	for e in (0, 150, E - 1):
		x, y = xs[e * n:(e + 1) * n], ys[e * n:(e + 1) * n]
		mu, var = XO.expert_predict(XO.SE, x, XO.expert_fit(XO.SE, x, y, inv_ls, 0.1, 1.3), inv_ls, 1.3, xt)
		_close(mu_e[e], mu, what="expert %d of 300 mean" % e)
		_close(var_e[e], var, scale=1.3, what="expert %d of 300 variance" % e)


def test_refused_and_empty_experts(S, gpu_device):
	"""info = -1 (more rows than nmax), info = -2 (decreasing offsets) and an empty expert, each between good neighbours that come out as in a
	batch without it.  Neither offender is the last expert and every offset lies in [0, N]: the slices behind the offender are there."""
	rng = np.random.RandomState(29)
	d, kappa, s = 3, 1.3, 0.1
	inv_ls = np.full(d, 2.5)
	xt = rng.uniform(0, 1, size=(7, d))

	def data(n):
		return rng.uniform(0, 1, size=(n, d)), rng.normal(size=n)

	def fit(x, y, sizes, **kw):
		return _fit(gpu_device, XO.SE, x, y, sizes, inv_ls, s, kappa, 1.0, [0] * d, 1, **kw)

	def rows(sizes):
		off = np.concatenate([[0], np.cumsum(sizes)])
		return [slice(off[e], off[e + 1]) for e in range(len(sizes))]

	def offender(st, e, info, alpha_rows):
		assert st["info_h"][e] == info and np.isinf(st["value_h"][e]) and st["value_h"][e] > 0 and np.all(st["grad_h"][e] == 0.0)
		assert np.isinf(st["total_h"][0]) and st["total_h"][0] > 0
		if alpha_rows is not None:
			assert np.all(st["alpha_h"][alpha_rows] == 0.0)

	# 1. a middle expert of 40 rows under nmax = 32
	sizes = [20, 40, 32, 5, 17, 32]
	x, y = data(sum(sizes))
	keep = np.r_[0:20, 60:sum(sizes)]
	bad, good = fit(x, y, sizes, nmax=32), fit(x[keep], y[keep], sizes[:1] + sizes[2:], nmax=32)
	assert bad["info_h"].tolist() == [0, -1, 0, 0, 0, 0] and not good["info_h"].any()
	offender(bad, 1, -1, slice(20, 60))
	_same_fit(bad, good, [0, 2, 3, 4, 5], range(5), [r for e, r in enumerate(rows(sizes)) if e != 1], rows(sizes[:1] + sizes[2:]))
	assert np.array_equal(bad["total_h"][1:], good["total_h"][1:])          # (its gradient row is zero)
	mu_b, var_b, _ = _predict(gpu_device, bad, xt, modes=())
	mu_g, var_g, _ = _predict(gpu_device, good, xt, modes=())
	assert np.all(mu_b[1] == 0.0) and np.all(var_b[1] == kappa)
	assert np.array_equal(mu_b[[0, 2, 3, 4, 5]], mu_g) and np.array_equal(var_b[[0, 2, 3, 4, 5]], var_g)

	# 2. offsets 40, 73, 0, 33, 40: expert 1 runs from 73 back to 0; experts 0, 2, 3 own the rows 40 .. 73, 0 .. 33, 33 .. 40
	x, y = data(73)
	bad = fit(x, y, [33, 0, 33, 7], offsets=np.array([40, 73, 0, 33, 40]))
	good = fit(x, y, [33, 7, 33])
	assert bad["info_h"].tolist() == [0, -2, 0, 0] and not good["info_h"].any()
	offender(bad, 1, -2, None)
	assert np.array_equal(bad["alpha_h"], good["alpha_h"]) and not np.isnan(bad["alpha_h"]).any()          # (alpha is indexed by row: the same array)
	for eb, eg in ((0, 2), (2, 0), (3, 1)):
		assert bad["value_h"][eb] == good["value_h"][eg] and np.array_equal(bad["grad_h"][eb], good["grad_h"][eg]) and np.array_equal(_V(bad, eb), _V(good, eg))
	mu_b, var_b, _ = _predict(gpu_device, bad, xt, modes=())
	mu_g, var_g, _ = _predict(gpu_device, good, xt, modes=())
	assert np.all(mu_b[1] == 0.0) and np.all(var_b[1] == kappa)
	assert np.array_equal(mu_b[[2, 3, 0]], mu_g) and np.array_equal(var_b[[2, 3, 0]], var_g)

	# 3. an empty expert: no evidence, no gradient, the prior
	sizes = [33, 0, 20]
	x, y = data(53)
	hole, good = fit(x, y, sizes), fit(x, y, [33, 20])
	assert hole["info_h"].tolist() == [0, 0, 0] and hole["value_h"][1] == 0.0 and np.all(hole["grad_h"][1] == 0.0)
	assert np.array_equal(hole["alpha_h"], good["alpha_h"]) and np.array_equal(hole["total_h"], good["total_h"])
	_same_fit(hole, good, [0, 2], [0, 1], [slice(0, 33), slice(33, 53)], [slice(0, 33), slice(33, 53)])
	mu_h, var_h, comb_h = _predict(gpu_device, hole, xt)
	mu_g, var_g, comb_g = _predict(gpu_device, good, xt)
	assert np.all(mu_h[1] == 0.0) and np.all(var_h[1] == kappa)
	assert np.array_equal(mu_h[[0, 2]], mu_g) and np.array_equal(var_h[[0, 2]], var_g)
	orc = XO.experts(XO.SE, x, y, sizes, inv_ls, s, kappa, xt=xt)
	for mode in range(4):          # (the prior of the empty expert counts in gPoE's 1 / E and in BCM's (1 - E) / kappa: not the committee of two)
		mu, var = XO.combine(mode, orc["mu_e"], orc["var_e"], kappa)
		_close(comb_h[mode][0], mu, scale=float(np.max(np.abs(orc["mu_e"]))), what="empty expert, mode %d mean" % mode)
		_close(comb_h[mode][1], var, scale=kappa, what="empty expert, mode %d variance" % mode)


# --------------------------------------------------------------------------------------------- the class against the oracle
CLASS = dict(N=700, d=3, M=50, s=0.1, kappa=1.3, ls=0.4, expert_size=200, shift=(0.5, -0.25, 2.0), id_sizes=[512, 0, 97, 1, 90])
_CLASS = {}


def _class_case():
	"""x (700, 3), y as in the reference case, 50 test points (three of them training points), and an explicit assignment with sizes 512, 0, 97, 1, 90"""
	if not _CLASS:
		C = CLASS
		rng = np.random.RandomState(23)
		x = rng.uniform(0.0, 1.0, size=(C["N"], C["d"])) + np.array(C["shift"])
		y = np.sin(4.0 * x[:, 0]) * np.cos(3.0 * x[:, 1]) + 0.5 * x[:, 2] + 0.1 * rng.normal(size=C["N"])
		xt = np.concatenate([x[[0, 5, C["N"] - 1]], rng.uniform(-0.2, 1.2, size=(C["M"] - 3, C["d"])) + np.array(C["shift"])])
		ids = rng.permutation(np.repeat(np.arange(len(C["id_sizes"])), C["id_sizes"]))
		_CLASS.update(x=x, y=y, xt=xt, ids=ids)
	return _CLASS


def _check_class(le, orc, order, sizes, xt, kappa, what):
	"""partition bookkeeping, A, expert_mean_var (chunked into strided outputs and not) and mean_std under the four combinations"""
	N = len(order)
	assert le.experts_info["sizes"] == list(sizes) and np.array_equal(le.offsets_, np.concatenate([[0], np.cumsum(sizes)]))
	assignment = np.empty(N, dtype=np.int64)
	assignment[order] = np.repeat(np.arange(len(sizes)), sizes)
	assert np.array_equal(le.assignment_, assignment)
	alpha = np.empty(N)
	alpha[order] = orc["alpha"]
	assert tuple(le.A.shape) == (N, 1)
	_close(le.A.numpy().ravel(), alpha, what=what + " A")
	xt_t = torch.from_numpy(xt)
	mscale = float(np.max(np.abs(orc["mu_e"])))
	le.max_size = 10000
	mu_e, var_e = le.expert_mean_var(xt_t)
	le.max_size = 16          # four chunks, written into column slices of the (E, M) results
	mu_c, var_c = le.expert_mean_var(xt_t)
	assert torch.equal(mu_e, mu_c) and torch.equal(var_e, var_c)
	_close(mu_e.numpy(), orc["mu_e"], scale=mscale, what=what + " mu_e")
	_close(var_e.numpy(), orc["var_e"], scale=kappa, what=what + " var_e")
	for name, mode in (("poe", XO.POE), ("gpoe", XO.GPOE), ("bcm", XO.BCM), ("rbcm", XO.RBCM)):
		le.combine = name
		mu, sd = le.mean_std(xt_t)
		m0, v0 = XO.combine(mode, orc["mu_e"], orc["var_e"], kappa)
		assert tuple(mu.shape) == tuple(sd.shape) == (len(xt), 1)
		_close(mu.numpy().ravel(), m0, scale=mscale, what="%s %s mean" % (what, name))
		_close(sd.numpy().ravel() ** 2, v0, scale=kappa, what="%s %s variance" % (what, name))


@pytest.mark.parametrize("part", ["ids", "random", "contiguous"])
def test_class_against_oracle(S, gpu_device, part):
	c, C = _class_case(), CLASS
	given = c["ids"] if part == "ids" else part
	le = S.LocalExpertsGaussianProcess(gamma=C["ls"], s=C["s"], kappa=C["kappa"], d=C["d"], expert_size=C["expert_size"],
									   partition=torch.from_numpy(c["ids"]) if part == "ids" else part, partition_seed=0)
	le.fit_gp(torch.from_numpy(c["x"]), torch.from_numpy(c["y"]).reshape(-1, 1))
	order, sizes = XO.partition(C["N"], C["expert_size"], given, 0)
	assert sizes == (C["id_sizes"] if part == "ids" else [175] * 4)
	assert part != "contiguous" or np.array_equal(order, np.arange(C["N"]))
	orc = XO.experts(XO.SE, c["x"][order], c["y"][order], sizes, np.full(C["d"], 1.0 / C["ls"]), C["s"], C["kappa"], xt=c["xt"])
	_check_class(le, orc, order, sizes, c["xt"], C["kappa"], part)


def test_class_ard_on_a_column_group(S, gpu_device):
	"""an ARD kernel on three of five columns (the other two NaN), in an order of its own: predictions, A and the evidence with its gradient"""
	c, C = _class_case(), CLASS
	group = [3, 0, 2]
	ag = np.array([0.7, 9.0, 0.3, 0.4, 9.0])          # (entries 1 and 4 belong to the columns the kernel does not read)

	def wide(a):
		out = np.full((a.shape[0], 5), np.nan)
		out[:, group] = a
		return out
	kernel = S.KernelFunction(kernel_name="ard", ard_gamma=torch.from_numpy(ag), kappa=C["kappa"], d=5, group=group)
	le = S.LocalExpertsGaussianProcess(kernel=kernel, s=C["s"], expert_size=C["expert_size"], partition="random", partition_seed=3)
	le.fit_gp(torch.from_numpy(wide(c["x"])), torch.from_numpy(c["y"]).reshape(-1, 1))
	order, sizes = XO.partition(C["N"], C["expert_size"], "random", 3)
	orc = XO.experts(XO.SE, c["x"][order], c["y"][order], sizes, 1.0 / ag[group], C["s"], C["kappa"], 0.8, group, 5, xt=c["xt"])
	_check_class(le, orc, order, sizes, wide(c["xt"]), C["kappa"], "ard group")
	le.s = torch.tensor([C["s"]], dtype=torch.float64, requires_grad=True)
	g = torch.from_numpy(ag).clone().requires_grad_(True)
	f = le.log_marginal(le.kernel_object, {'0': {'ard_gamma': g}}, 0.8)
	f.backward()
	assert tuple(f.shape) == (1, 1) and abs(float(f.detach()) - orc["total"][0]) <= 1e-8 * abs(orc["total"][0])
	assert g.grad[1] == 0.0 and g.grad[4] == 0.0
	_close(np.concatenate([g.grad.numpy(), le.s.grad.numpy()]), orc["total"][1:], tol=1e-7, what="ard group evidence gradient")


@pytest.mark.parametrize("name", ["squared_exponential", "ard", "matern"])
def test_class_evidence_against_oracle(S, gpu_device, name):
	"""log_marginal and its autograd gradient (lengthscales and the noise std) of a committee with the cap, an empty expert and a one-point expert
	against the oracle's summed evidence: value 1e-8, gradient 1e-7 of its largest entry (the dense class's own tolerances); log_marginal_batch
	against log_marginal"""
	c, C = _class_case(), CLASS
	d, w = C["d"], 0.8
	if name == "ard":
		ls, pname, pidx, npar = np.array([0.4, 0.7, 0.3]), "ard_gamma", [0, 1, 2], 3
		kernel = S.KernelFunction(kernel_name="ard", ard_gamma=torch.from_numpy(ls), kappa=C["kappa"], d=d)
	else:
		ls, pname, pidx, npar = np.array([C["ls"]]), "gamma", [0] * d, 1
		kernel = S.KernelFunction(kernel_name=name, gamma=C["ls"], nu=1.5, kappa=C["kappa"], d=d)
	kind = XO.MATERN32 if name == "matern" else XO.SE
	le = S.LocalExpertsGaussianProcess(kernel=kernel, s=C["s"], partition=torch.from_numpy(c["ids"]))
	le.fit_gp(torch.from_numpy(c["x"]), torch.from_numpy(c["y"]).reshape(-1, 1))
	mu0, sd0 = le.mean_std(torch.from_numpy(c["xt"]))
	order, sizes = XO.partition(C["N"], 0, c["ids"])
	xs, ys = c["x"][order], c["y"][order]

	def oracle(scale, s):
		return XO.experts(kind, xs, ys, sizes, 1.0 / (scale * ls if name == "ard" else np.full(d, scale * ls[0])), s, C["kappa"], w, pidx, npar)["total"]

	def one(scale, s):
		le.s = torch.tensor([s], dtype=torch.float64, requires_grad=True)
		g = torch.from_numpy(scale * ls).clone().requires_grad_(True)
		f = le.log_marginal(le.kernel_object, {'0': {pname: g}}, w)
		f.backward()
		return float(f.detach()), g.grad.numpy().copy(), le.s.grad.numpy().copy()

	cands = [(1.0, 0.1), (0.75, 0.15), (1.5, 0.2)]
	single = [one(*cand) for cand in cands]
	for cand, (f, gl, gs) in zip(cands, single):
		tot = oracle(*cand)
		print(name, cand, "evidence", f, tot[0], "gradient", gl, gs, tot[1:])
		assert abs(f - tot[0]) <= 1e-8 * abs(tot[0])
		_close(np.concatenate([gl, gs]), tot[1:], tol=1e-7, what="%s evidence gradient at %s" % (name, cand))
	le.s = C["s"]
	values, grads = le.log_marginal_batch(le.kernel_object, [{'0': {pname: torch.from_numpy(sc * ls)}} for sc, _ in cands], w, s=[s for _, s in cands])
	assert le.lml_batch_path == "device"
	for b, (f, gl, gs) in enumerate(single):          # the same launches: the same bits
		assert float(values[b]) == f and np.array_equal(grads[b]['0'][pname].numpy(), gl) and np.array_equal(grads[b]['likelihood']['sigma'].numpy(), gs)
	# the resident factor is the fit's still
	mu1, sd1 = le.mean_std(torch.from_numpy(c["xt"]))
	assert torch.equal(mu0, mu1) and torch.equal(sd0, sd1)


def test_class_evidence_batch_with_a_failing_candidate(S, gpu_device):
	"""kappa = 1, two coincident points in one expert: at s = 0 that expert's second pivot is fma(-1, 1, 1) = 0 exactly.  The candidate gets +inf and
	zero gradients; its neighbours in the batch are what they are without it"""
	rng = np.random.RandomState(31)
	x = rng.uniform(0, 1, size=(200, 3))
	x[1] = x[0]
	y = rng.normal(size=(200, 1))
	le = S.LocalExpertsGaussianProcess(gamma=0.4, s=0.1, kappa=1.0, d=3, expert_size=64, partition="contiguous")
	le.fit_gp(torch.from_numpy(x), torch.from_numpy(y))
	X = lambda v: {'0': {'gamma': torch.tensor([v], dtype=torch.float64)}}
	values, grads = le.log_marginal_batch(le.kernel_object, [X(0.4), X(0.4), X(0.5)], 1.0, s=[0.1, 0.0, 0.2])
	values2, grads2 = le.log_marginal_batch(le.kernel_object, [X(0.4), X(0.5)], 1.0, s=[0.1, 0.2])
	assert np.isinf(float(values[1])) and float(values[1]) > 0
	assert torch.all(grads[1]['0']['gamma'] == 0.0) and torch.all(grads[1]['likelihood']['sigma'] == 0.0)
	for b, b2 in ((0, 0), (2, 1)):
		assert np.isfinite(float(values[b])) and float(values[b]) == float(values2[b2])
		assert torch.equal(grads[b]['0']['gamma'], grads2[b2]['0']['gamma']) and torch.equal(grads[b]['likelihood']['sigma'], grads2[b2]['likelihood']['sigma'])
		assert float(grads[b]['0']['gamma'].abs().max()) > 0 and float(grads[b]['likelihood']['sigma'].abs().max()) > 0
