"""
Local GP experts on the device: stpy_experts_fit / _predict / _combine against the NumPy oracle (tests/experts_oracle.py), the properties the
class relies on (an expert's outputs do not depend on the batch around it; a failing expert is reported and leaves the others alone), and
LocalExpertsGaussianProcess against the dense class where the two coincide (one expert, PoE).

Tolerance 1e-8, as in the rest of the C-ABI suite: relative to kappa for variances, to max |mu| for means, to the largest entry for alpha and the
gradient rows.  tests/test_experts_cpu.py shows that on the reference case no expert variance comes near the clamp (min var_e / kappa > 1e-3) and
the float64 oracle itself is five orders inside the tolerance.
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


def _fit(dev, kind, xs, ys, sizes, inv_ls, s, kappa, weight=1.0, pidx=None, n_params=0, cols=None, nmax=None):
	"""one stpy_experts_fit call through the typed wrapper; NumPy results plus the device buffers a prediction needs"""
	from stpy_amd import _lib as L
	E, N = len(sizes), xs.shape[0]
	nmax = int(max(sizes)) if nmax is None else nmax
	st = dict(xs=_dev(xs, dev), ys=_dev(ys, dev), offsets=_dev(np.concatenate([[0], np.cumsum(sizes)]), dev, np.int32), nmax=nmax,
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


def _predict(dev, st, xt, modes=(0, 1, 2, 3)):
	from stpy_amd import _lib as L
	E, M = len(st["sizes"]), xt.shape[0]
	xt_d = _dev(xt, dev)
	mu_e = torch.full((E, M), float("nan"), dtype=torch.float64, device=dev)
	var_e = torch.full((E, M), float("nan"), dtype=torch.float64, device=dev)
	L.experts_predict(st["kind"], st["xs"], st["offsets"], st["nmax"], st["inv_ls"], st["kappa"], st["factor"], st["alpha"], st["info"], xt_d, mu_e, var_e, cols=st["cols"])
	out = {}
	for mode in modes:
		mu = torch.full((M,), float("nan"), dtype=torch.float64, device=dev)
		var = torch.full((M,), float("nan"), dtype=torch.float64, device=dev)
		L.experts_combine(mode, mu_e, var_e, st["kappa"], mu, var)
		out[mode] = (mu.cpu().numpy(), var.cpu().numpy())
	torch.cuda.synchronize()
	return mu_e.cpu().numpy(), var_e.cpu().numpy(), out


def _close(got, want, scale=None, tol=TOL, what=""):
	scale = float(np.max(np.abs(want))) if scale is None else scale
	err = float(np.max(np.abs(np.asarray(got) - np.asarray(want)))) / (scale if scale > 0 else 1.0)
	print(what, "error", err)
	assert err <= tol, (what, err)


def _check_fit(st, orc, kappa, with_grad, what):
	assert not st["info_h"].any(), st["info_h"]
	_close(st["alpha_h"], orc["alpha"], what=what + " alpha")
	_close(st["value_h"], orc["value"], what=what + " value")
	_close(st["total_h"][:1], orc["total"][:1], what=what + " total value")
	if with_grad:
		for e in range(len(st["sizes"])):
			_close(st["grad_h"][e], orc["grad"][e], what=what + " grad of expert %d" % e)
		_close(st["total_h"], orc["total"], scale=float(np.max(np.abs(orc["total"][1:]))), what=what + " total")
	for e, f in enumerate(orc["fits"]):
		V = _V(st, e)          # L^-T, upper triangular: V V^T = K_e^-1
		_close(V @ V.T @ f["K"], np.eye(V.shape[0]), scale=1.0, what=what + " V V^T K of expert %d" % e)


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
