"""
The local experts' routed prediction on the device: stpy_experts_centroids / _route / _predict_routed / _predict_routed_grad and
LocalExpertsGaussianProcess(partition="kdtree", predict_experts=k) against the NumPy twin (tests/experts_route_oracle.py) and against the
unrouted kernels, whose bits a routed slot must carry.

Shapes: XO.reference_case() under the k-d partition (E = 5: 34, 34, 33, 33, 33; M = 65; k = 1, 2, 3, 5) and XO.border_case() (experts of 1 .. 512
points, M = 97; k = 3, 8, 14: experts without a test point, partial tiles, several tiles per expert), then the edges: an expert with exactly 32
and one with exactly 33 routed points, M = 1 and 0, a failed expert that is selected, ARD on a column group, ucb_optimize, two calls.

Tolerances: 1e-12 relative for the centroids (a sum of n_e <= 512 terms of one sign: n_e eps = 1e-13), bit equality for the routed slots against
the unrouted entries and for k = E against the unrouted object, TOL = 1e-8 with the scales of tests/test_gpu_experts*.py for the combined results
against the oracle.  The selection is compared after the oracle alone has shown that no test point's k-th and (k + 1)-th distance are closer
than 1e-9 relative (the device may contract a multiply-add the twin does not).
"""
import numpy as np
import pytest
import torch

from tests import experts_grad_oracle as GO
from tests import experts_oracle as XO
from tests import experts_route_oracle as RO
from tests.test_gpu_experts import CLASS, _border, _class_case, _close, _dev, _fit, _predict
from tests.test_gpu_experts_grad import _border_grad, _predict_grad

pytestmark = pytest.mark.gpu

TOL = 1e-8
MODES = (XO.POE, XO.GPOE, XO.BCM, XO.RBCM)
NAMES = {"poe": XO.POE, "gpoe": XO.GPOE, "bcm": XO.BCM, "rbcm": XO.RBCM}
NAN = float("nan")


@pytest.fixture(scope="module")
def S(gpu_device):
	import stpy_amd
	return stpy_amd


_KD = {}


def _kd_ref():
	"""the reference case gathered by the k-d partition (the oracle's): once, read only"""
	if not _KD:
		r = XO.reference_case()
		order, sizes = RO.kd_partition(r["x"], XO.REF["expert_size"], r["inv_ls"])
		_KD.update(r, order=order, sizes=sizes, xs=r["x"][order], ys=r["y"][order])
	return _KD


def _routed(dev, st, xt, k, grad=False):
	"""centroids, route, work list and one routed prediction (with gradients: the gradient kernel) through the typed wrappers, every output the
	leading view of a NaN-filled buffer.  Returns dict(cent, sel, wexp, wpair, mu_s, var_s[, gmu_s, gvar_s]) as NumPy arrays plus the device slots"""
	from stpy_amd import _lib as L
	E, M, d = len(st["sizes"]), xt.shape[0], int(st["inv_ls"].numel())
	xt_d = _dev(xt, dev)
	cent = L.experts_centroids(st["xs"], st["offsets"], st["inv_ls"], cols=st["cols"])
	sel = L.experts_route(cent, st["inv_ls"], xt_d, k, cols=st["cols"])
	wexp, wpair = L.experts_work_list(sel, E)
	full = lambda *shape: torch.full(shape, NAN, dtype=torch.float64, device=dev)
	mu_f, var_f = full(k, M + 3), full(k, M + 3)
	mu_s, var_s = mu_f[:, :M], var_f[:, :M]
	out = {}
	if grad:
		gmu_f, gvar_f = full(k, M + 3, d + 2), full(k, M + 3, d + 2)
		gmu_s, gvar_s = gmu_f[:, :M, :d], gvar_f[:, :M, :d]
		L.experts_predict_routed_grad(st["kind"], st["xs"], st["offsets"], st["nmax"], st["inv_ls"], st["kappa"], st["factor"], st["alpha"], st["info"], xt_d,
									  wexp, wpair, mu_s, var_s, gmu_s, gvar_s, cols=st["cols"])
		out.update(gmu_s=gmu_s.cpu().numpy(), gvar_s=gvar_s.cpu().numpy(), dev_g=(gmu_s, gvar_s))
		pads = [gmu_f[:, M:], gmu_f[:, :, d:], gvar_f[:, M:], gvar_f[:, :, d:]]
	else:
		L.experts_predict_routed(st["kind"], st["xs"], st["offsets"], st["nmax"], st["inv_ls"], st["kappa"], st["factor"], st["alpha"], st["info"], xt_d,
								 wexp, wpair, mu_s, var_s, cols=st["cols"])
		pads = []
	torch.cuda.synchronize()
	for pad in pads + [mu_f[:, M:], var_f[:, M:]]:          # nothing beside the views
		assert bool(torch.isnan(pad).all())
	out.update(cent=cent.cpu().numpy(), sel=sel.cpu().numpy(), wexp=wexp.cpu().numpy(), wpair=wpair.cpu().numpy(), mu_s=mu_s.cpu().numpy(),
			   var_s=var_s.cpu().numpy(), dev=(mu_s, var_s))
	return out


def _combined(dev, got, kappa, M, d, grad):
	"""{mode: (mu, var[, dmu, dstd])} from the routed slots by the UNCHANGED combination kernels (E := k)"""
	from stpy_amd import _lib as L
	res = {}
	for mode in MODES:
		mu, var = torch.full((M,), NAN, dtype=torch.float64, device=dev), torch.full((M,), NAN, dtype=torch.float64, device=dev)
		if grad:
			dmu, dstd = torch.full((M, d), NAN, dtype=torch.float64, device=dev), torch.full((M, d), NAN, dtype=torch.float64, device=dev)
			L.experts_combine_grad(mode, got["dev"][0], got["dev"][1], got["dev_g"][0], got["dev_g"][1], kappa, mu, var, dmu, dstd)
			res[mode] = tuple(t.cpu().numpy() for t in (mu, var, dmu, dstd))
		else:
			L.experts_combine(mode, got["dev"][0], got["dev"][1], kappa, mu, var)
			res[mode] = (mu.cpu().numpy(), var.cpu().numpy())
	return res


def _check_routed(dev, st, orc, g_orc, xt, k, kappa, what, unrouted, min_gap=1e-9):
	"""every comparison of a routed prediction at the test points xt with k experts.  unrouted: (mu_e, var_e, gmu_e, gvar_e) of the all-experts
	kernels on the device (NumPy), whose entries the routed slots must carry bit for bit"""
	E, M, d = len(st["sizes"]), xt.shape[0], int(st["inv_ls"].numel())
	inv_ls, cols = st["inv_ls"].cpu().numpy(), None if st["cols"] is None else st["cols"].cpu().numpy().tolist()
	cent_o = RO.centroids(st["xs"].cpu().numpy(), st["sizes"], inv_ls, cols)
	gap = RO.smallest_gap(cent_o, xt, inv_ls, k, cols)
	print(what, "k", k, "smallest relative gap between the k-th and the next distance", gap)
	assert gap > min_gap          # (on the oracle alone: no point is left out of the comparison below)
	sel_o = RO.route(cent_o, xt, inv_ls, k, cols)
	mu_e, var_e, gmu_e, gvar_e = unrouted
	for grad in (False, True):
		got = _routed(dev, st, xt, k, grad)
		fin = np.isfinite(cent_o)
		assert np.array_equal(np.isinf(got["cent"]), ~fin) and np.all(got["cent"][~fin] > 0)
		assert np.all(np.abs(got["cent"][fin] - cent_o[fin]) <= 1e-12 * np.abs(cent_o[fin])), what
		assert np.array_equal(got["sel"], sel_o), what
		wexp_o, wpair_o = RO.work_list(sel_o, E)
		assert np.array_equal(got["wexp"], wexp_o) and np.array_equal(got["wpair"], wpair_o)
		# the bit contract: slot (j, t) is entry (sel[t, j], t) of the unrouted kernels
		assert np.array_equal(got["mu_s"], RO.gather(sel_o, mu_e)) and np.array_equal(got["var_s"], RO.gather(sel_o, var_e)), (what, k, grad)
		if grad:
			assert np.array_equal(got["gmu_s"], RO.gather(sel_o, gmu_e)) and np.array_equal(got["gvar_s"], RO.gather(sel_o, gvar_e)), (what, k)
		comb = _combined(dev, got, kappa, M, d, grad)
		for mode in MODES:
			if grad:
				mu_o, var_o, dmu_o, dstd_o = RO.routed_combine_grad(mode, sel_o, orc["mu_e"], orc["var_e"], g_orc[0], g_orc[1], kappa)
				_close(comb[mode][2], dmu_o, what="%s k %d mode %d dmu" % (what, k, mode))
				_close(comb[mode][3], dstd_o, what="%s k %d mode %d dstd" % (what, k, mode))
			else:
				mu_o, var_o = RO.routed_combine(mode, sel_o, orc["mu_e"], orc["var_e"], kappa)
			_close(comb[mode][0], mu_o, scale=float(np.max(np.abs(orc["mu_e"]))), what="%s k %d mode %d mean" % (what, k, mode))
			_close(comb[mode][1], var_o, scale=kappa, what="%s k %d mode %d variance" % (what, k, mode))
	return sel_o


# --------------------------------------------------------------------------------------------- the reference case under the k-d partition
@pytest.mark.parametrize("kind", XO.KINDS)
def test_reference_case_kernels(S, gpu_device, kind):
	r = _kd_ref()
	assert r["sizes"] == [34, 34, 33, 33, 33]
	st = _fit(gpu_device, kind, r["xs"], r["ys"], r["sizes"], r["inv_ls"], r["s"], r["kappa"])
	orc = XO.experts(kind, r["xs"], r["ys"], r["sizes"], r["inv_ls"], r["s"], r["kappa"], xt=r["xt"])
	g_orc = GO.experts_grad(kind, r["xs"], orc, r["inv_ls"], r["kappa"], r["xt"])
	unrouted = _predict_grad(gpu_device, st, r["xt"], modes=())[:4]
	plain = _predict(gpu_device, st, r["xt"], modes=())
	assert np.array_equal(unrouted[0], plain[0]) and np.array_equal(unrouted[1], plain[1])
	for k in (1, 2, 3, 5):
		_check_routed(gpu_device, st, orc, g_orc, r["xt"], k, r["kappa"], "kd reference kind %d" % kind, unrouted)


@pytest.mark.parametrize("name,nu,kind", [("squared_exponential", 1.5, XO.SE), ("matern", 0.5, XO.MATERN12), ("matern", 1.5, XO.MATERN32), ("matern", 2.5, XO.MATERN52)])
def test_reference_case_class(S, gpu_device, name, nu, kind):
	"""the class on the reference case: the partition of the twin, route, mean_std and mean_std_grad under the four combinations, launch counts,
	and k = E bit for bit the object without routing"""
	r = _kd_ref()
	x, y, xt = torch.from_numpy(r["x"]), torch.from_numpy(r["y"]).reshape(-1, 1), torch.from_numpy(r["xt"])
	make = lambda k: S.LocalExpertsGaussianProcess(gamma=XO.REF["ls"], s=r["s"], kappa=r["kappa"], d=XO.REF["d"], kernel_name=name, nu=nu,
												   expert_size=XO.REF["expert_size"], partition="kdtree", predict_experts=k)
	orc = XO.experts(kind, r["xs"], r["ys"], r["sizes"], r["inv_ls"], r["s"], r["kappa"], xt=r["xt"])
	g_orc = GO.experts_grad(kind, r["xs"], orc, r["inv_ls"], r["kappa"], r["xt"])
	cent_o = RO.centroids(r["xs"], r["sizes"], r["inv_ls"])
	plain = make(None)
	plain.fit_gp(x, y)
	assert plain.launches == 2 and np.array_equal(plain._order, r["order"]) and plain.experts_info["sizes"] == r["sizes"]
	assert plain.experts_info["partition"] == "kdtree" and plain.experts_info["predict_experts"] is None
	assignment = np.empty(len(r["order"]), dtype=np.int64)
	assignment[r["order"]] = np.repeat(np.arange(5), r["sizes"])
	assert np.array_equal(plain.assignment_, assignment) and np.array_equal(plain.offsets_, np.concatenate([[0], np.cumsum(r["sizes"])]))
	for k in (1, 2, 3, 5, 9):
		le = make(k)
		le.fit_gp(x, y)
		kk = min(k, 5)          # above E: clamps to E
		assert le.launches == 3 and le.experts_info["predict_experts"] == k and np.array_equal(le._order, r["order"])
		sel_o = RO.route(cent_o, r["xt"], r["inv_ls"], kk)
		sel = le.route(xt)
		assert sel.dtype == torch.int64 and tuple(sel.shape) == (65, kk) and not sel.is_cuda and np.array_equal(sel.numpy(), sel_o)
		assert le.launches == 4
		for cname, mode in NAMES.items():
			le.combine = plain.combine = cname
			before = le.launches
			mu, sd = le.mean_std(xt)
			assert le.launches - before == 3
			dmu, dstd = le.mean_std_grad(xt)
			assert le.launches - before == 6
			mu_o, var_o, dmu_o, dstd_o = RO.routed_combine_grad(mode, sel_o, orc["mu_e"], orc["var_e"], g_orc[0], g_orc[1], r["kappa"])
			what = "class %s k %d %s" % (name, k, cname)
			_close(mu.numpy().ravel(), mu_o, scale=float(np.max(np.abs(orc["mu_e"]))), what=what + " mean")
			_close(sd.numpy().ravel() ** 2, var_o, scale=r["kappa"], what=what + " variance")
			_close(dmu.numpy(), dmu_o, what=what + " dmu")
			_close(dstd.numpy(), dstd_o, what=what + " dstd")
			if kk == 5:          # every expert selected: the unrouted object, bit for bit
				mu_p, sd_p = plain.mean_std(xt)
				dmu_p, dstd_p = plain.mean_std_grad(xt)
				assert torch.equal(mu, mu_p) and torch.equal(sd, sd_p) and torch.equal(dmu, dmu_p) and torch.equal(dstd, dstd_p), what
		if k == 2:          # chunks, one point, no point, and the same call again
			le.combine = "rbcm"
			mu, sd = le.mean_std(xt)
			dmu, dstd = le.mean_std_grad(xt)
			le.max_size = 16
			before = le.launches
			mu_c, sd_c = le.mean_std(xt)
			assert le.launches - before == 3 * 5 and torch.equal(mu, mu_c) and torch.equal(sd, sd_c)
			dmu_c, dstd_c = le.mean_std_grad(xt)
			assert torch.equal(dmu, dmu_c) and torch.equal(dstd, dstd_c) and torch.equal(le.route(xt), sel)
			le.max_size = 10000
			mu_1, sd_1 = le.mean_std(xt[7:8])
			dmu_1, dstd_1 = le.mean_std_grad(xt[7:8])
			assert torch.equal(mu_1, mu[7:8]) and torch.equal(sd_1, sd[7:8]) and torch.equal(dmu_1, dmu[7:8]) and torch.equal(dstd_1, dstd[7:8])
			mu_0, sd_0 = le.mean_std(xt[:0])
			dmu_0, dstd_0 = le.mean_std_grad(xt[:0])
			assert tuple(mu_0.shape) == tuple(sd_0.shape) == (0, 1) and tuple(dmu_0.shape) == tuple(dstd_0.shape) == (0, 3) and tuple(le.route(xt[:0]).shape) == (0, 2)
			mu_e, var_e = le.expert_mean_var(xt)          # the diagnostics stay all-experts
			assert tuple(mu_e.shape) == (5, 65)
			_close(mu_e.numpy(), orc["mu_e"], what="class expert_mean_var")


# --------------------------------------------------------------------------------------------- every block size, given ids
@pytest.mark.parametrize("kind", XO.KINDS)
def test_border_case(S, gpu_device, kind):
	"""experts of 1 .. 512 points, M = 97; at k = 3 the experts receive 23, 44, 49, 6, 25, 29, 18, 27, 10, 0, 34, 15, 0, 11 points: none, partial
	tiles, several tiles"""
	c, orc, st, g_orc = _border_grad(gpu_device, kind)
	unrouted = _predict_grad(gpu_device, st, c["xt"], modes=())[:4]
	for k in (3, 8, 14):
		sel = _check_routed(gpu_device, st, orc, g_orc, c["xt"], k, c["kappa"], "border kind %d" % kind, unrouted)
		if k == 3:
			assert np.bincount(sel.ravel(), minlength=14).tolist() == [23, 44, 49, 6, 25, 29, 18, 27, 10, 0, 34, 15, 0, 11]


# --------------------------------------------------------------------------------------------- the edges
def test_full_tile_and_one_more(S, gpu_device):
	"""two clusters far apart, k = 1: one expert is asked by exactly 32 test points (one full tile), the other by 33 (a full tile and one column)"""
	rng = np.random.RandomState(9)
	sizes, d = [40, 50], 3
	xs = np.concatenate([rng.uniform(0, 1, size=(40, d)), 10.0 + rng.uniform(0, 1, size=(50, d))])
	ys = np.sin(3 * xs[:, 0]) + 0.1 * rng.normal(size=90)
	xt = np.concatenate([rng.uniform(0, 1, size=(32, d)), 10.0 + rng.uniform(0, 1, size=(33, d))])[rng.permutation(65)]
	inv_ls = np.full(d, 2.0)
	st = _fit(gpu_device, XO.MATERN52, xs, ys, sizes, inv_ls, 0.1, 1.3)
	orc = XO.experts(XO.MATERN52, xs, ys, sizes, inv_ls, 0.1, 1.3, xt=xt)
	g_orc = GO.experts_grad(XO.MATERN52, xs, orc, inv_ls, 1.3, xt)
	unrouted = _predict_grad(gpu_device, st, xt, modes=())[:4]
	sel = _check_routed(gpu_device, st, orc, g_orc, xt, 1, 1.3, "32 and 33", unrouted)
	assert np.bincount(sel.ravel()).tolist() == [32, 33]
	wexp, _ = RO.work_list(sel, 2)
	assert wexp.tolist() == [0, 1, 1] + [-1] * (RO.tile_bound(2, 65, 1) - 3)
	_check_routed(gpu_device, st, orc, g_orc, xt[:1], 1, 1.3, "M = 1", tuple(a[:, :1] for a in unrouted))
	from stpy_amd import _lib as L
	assert tuple(L.experts_route(_dev(RO.centroids(xs, sizes, inv_ls), gpu_device), st["inv_ls"], _dev(xt[:0], gpu_device), 1).shape) == (0, 1)


def test_failing_expert_that_is_selected(S, gpu_device):
	"""the construction of test_failing_expert (tests/test_gpu_experts.py): expert 1 fails at its second pivot.  Where it is selected its slot
	holds the prior, flat; the other slots carry the bits of the fit without it"""
	sizes = [40, 20, 33]
	rng = np.random.RandomState(2)
	xs = rng.uniform(0, 1, size=(sum(sizes), 3))
	ys = rng.normal(size=sum(sizes))
	xs[40 + 1] = xs[40 + 0]
	inv_ls = np.full(3, 2.5)
	bad = _fit(gpu_device, XO.SE, xs, ys, sizes, inv_ls, 0.0, 1.0)
	keep = np.r_[0:40, 60:93]
	good = _fit(gpu_device, XO.SE, xs[keep], ys[keep], [40, 33], inv_ls, 0.0, 1.0, nmax=40)
	assert bad["info_h"].tolist() == [0, 2, 0]
	xt = rng.uniform(0, 1, size=(37, 3))
	g = _predict_grad(gpu_device, good, xt, modes=())[:4]
	for k in (1, 2, 3):
		got = _routed(gpu_device, bad, xt, k, grad=True)
		sel = got["sel"]
		assert np.array_equal(sel, RO.route(RO.centroids(xs, sizes, inv_ls), xt, inv_ls, k)) and np.any(sel == 1)
		for j in range(k):
			for e_bad, e_good in ((0, 0), (2, 1)):
				t = np.nonzero(sel[:, j] == e_bad)[0]
				for name, ref in zip(("mu_s", "var_s", "gmu_s", "gvar_s"), g):
					assert np.array_equal(got[name][j, t], ref[e_good, t]), (k, j, name)
			t = np.nonzero(sel[:, j] == 1)[0]
			assert np.all(got["mu_s"][j, t] == 0.0) and np.all(got["var_s"][j, t] == 1.0) and np.all(got["gmu_s"][j, t] == 0.0) and np.all(got["gvar_s"][j, t] == 0.0)


def test_class_ard_on_a_column_group(S, gpu_device):
	"""an ARD kernel on three of five columns (the other two NaN), in an order of its own: the k-d partition in the group's scaled coordinates,
	route and the routed prediction with its gradients, placed into the wide columns"""
	c, C = _class_case(), CLASS
	group = [3, 0, 2]
	ag = np.array([0.7, 9.0, 0.3, 0.4, 9.0])

	def wide(a):
		out = np.full((a.shape[0], 5), np.nan)
		out[:, group] = a
		return out
	il = 1.0 / ag[group]
	kernel = S.KernelFunction(kernel_name="ard", ard_gamma=torch.from_numpy(ag), kappa=C["kappa"], d=5, group=group)
	le = S.LocalExpertsGaussianProcess(kernel=kernel, s=C["s"], expert_size=C["expert_size"], partition="kdtree", predict_experts=2)
	le.fit_gp(torch.from_numpy(wide(c["x"])), torch.from_numpy(c["y"]).reshape(-1, 1))
	order, sizes = RO.kd_partition(c["x"], C["expert_size"], il)
	assert sizes == [175] * 4 and np.array_equal(le._order, order)
	xs, ys = c["x"][order], c["y"][order]
	orc = XO.experts(XO.SE, xs, ys, sizes, il, C["s"], C["kappa"], xt=c["xt"])
	g_orc = GO.experts_grad(XO.SE, xs, orc, il, C["kappa"], c["xt"])
	cent_o = RO.centroids(xs, sizes, il)
	assert RO.smallest_gap(cent_o, c["xt"], il, 2) > 1e-9
	sel_o = RO.route(cent_o, c["xt"], il, 2)
	xt = torch.from_numpy(wide(c["xt"]))
	assert np.array_equal(le.route(xt).numpy(), sel_o)
	mu, sd = le.mean_std(xt)
	dmu, dstd = le.mean_std_grad(xt)
	mu_o, var_o, dmu_o, dstd_o = RO.routed_combine_grad(XO.RBCM, sel_o, orc["mu_e"], orc["var_e"], g_orc[0], g_orc[1], C["kappa"])
	_close(mu.numpy().ravel(), mu_o, scale=float(np.max(np.abs(orc["mu_e"]))), what="ard group mean")
	_close(sd.numpy().ravel() ** 2, var_o, scale=C["kappa"], what="ard group variance")
	assert tuple(dmu.shape) == (C["M"], 5) and torch.all(dmu[:, [1, 4]] == 0) and torch.all(dstd[:, [1, 4]] == 0)
	_close(dmu.numpy()[:, group], dmu_o, what="ard group dmu")
	_close(dstd.numpy()[:, group], dstd_o, what="ard group dstd")


def test_ucb_optimize_routed(S, gpu_device):
	"""the reference case under the bounding box of its data, eight starts, k = 2: no worse than any start, the acquisition mean_std gives at
	the solution, three launches per evaluation (route, routed prediction, combination), the same bits under the same seed"""
	r = _kd_ref()
	lo, hi = r["x"].min(axis=0), r["x"].max(axis=0)
	le = S.LocalExpertsGaussianProcess(gamma=XO.REF["ls"], s=r["s"], kappa=r["kappa"], d=XO.REF["d"], expert_size=XO.REF["expert_size"], partition="kdtree",
									   predict_experts=2, bounds=[(float(a), float(b)) for a, b in zip(lo, hi)])
	le.fit_gp(torch.from_numpy(r["x"]), torch.from_numpy(r["y"]).reshape(-1, 1))
	runs = []
	for _ in range(2):
		np.random.seed(11)
		before = le.launches
		sol, val = le.ucb_optimize(4.0, multistart=8)
		info = le.optimize_info
		assert np.all(sol.numpy() >= lo) and np.all(sol.numpy() <= hi)
		assert info["start_values"].shape == (8,) and np.all(float(val) >= info["start_values"])
		assert info["launches"] == le.launches - before == 3 * info["evaluations"]
		mu, sd = le.mean_std(sol.reshape(1, -1))
		acq = float(mu) + 2.0 * float(sd)
		print("routed ucb: solution", sol.numpy(), "value", float(val), "acquisition from mean_std", acq, "evaluations", info["evaluations"])
		assert abs(float(val) - acq) <= 1e-10 * abs(acq)
		mu, sd = le.mean_std(torch.from_numpy(info["starts"]))
		assert np.allclose(info["start_values"], (mu + 2.0 * sd).numpy().ravel(), rtol=1e-12, atol=0)
		runs.append((sol, val))
	assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_two_calls_are_bit_identical(S, gpu_device):
	c, orc, st = _border(gpu_device, XO.SE)
	a, b = _routed(gpu_device, st, c["xt"], 8, grad=True), _routed(gpu_device, st, c["xt"], 8, grad=True)
	for key in ("cent", "sel", "wexp", "wpair", "mu_s", "var_s", "gmu_s", "gvar_s"):
		assert np.array_equal(a[key], b[key]), key
